// pvnet_bf16_pack.h -- "K9 in bf16": the round-to-nearest-even that makes bf16 of float32 and the layout of the bf16 weight buffer that
// pvnet_bf16_trunk_kernel (pvnet_bf16_kernel.hip) streams.  Plain C++ that also compiles as device code: the host packs with these functions
// (gmk_pvnet_set_precision), one small kernel runs the SAME functions on the device (gmk_train_export), so both give the same bits.
//
// The bf16 buffer is derived from the handle's float32 buffers (pvnet_pack.h: d_w1, d_w2, d_w3, d_wh), which are pure gathers of the
// weights: every bf16 element is the rounding of one float of those buffers, or zero.  Segments, in elements (all A operands of
// v_mfma_f32_32x32x16_bf16: lane l = (row r = l & 31, half h = l >> 5) holds A[r][k = 8 h + e] in element e of its eight):
//   layer 1  [5 steps][64 lanes][8]            k-step s, half h = tap 2 s + h (the tenth tap: zeros), element e = input channel e (6, 7: zeros)
//   layer 2  [2 cout tiles][18 steps][64][8]   step = tap * 2 + channel group; element e = input channel 16 group + 8 h + e
//   layer 3  [4 cout tiles][36 steps][64][8]   step = tap * 4 + channel group
//   heads    [4 waves][2 steps][64][8]         row r = head row (0..3 policy, 4..5 value, above: zeros); the k of step s, half h, element e is
//                                              layer-3 channel 32 wave + 16 s + 8 (e >> 2) + 4 h + (e & 3): the order in which an accumulator
//                                              tile's registers 8 s .. 8 s + 7 hold its rows (cdna_hip_programming.md, "An accumulator tile as the
//                                              next MFMA's operand")
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define GMK_BF16_HD __host__ __device__
#else
#define GMK_BF16_HD
#endif

namespace gmk {
namespace bf16pack {

constexpr int kQ1 = 0, kQ1Size = 5 * 512;
constexpr int kQ2 = kQ1 + kQ1Size, kQ2Size = 2 * 18 * 512;
constexpr int kQ3 = kQ2 + kQ2Size, kQ3Size = 4 * 36 * 512;
constexpr int kQh = kQ3 + kQ3Size, kQhSize = 4 * 2 * 512;
constexpr int kElements = kQh + kQhSize;           // 98 816 bf16 = 193 KB

// float32 -> bf16, round to nearest, ties to even; NaN -> the quiet NaN 0x7FC0; values that round past the largest bf16 -> Inf
GMK_BF16_HD inline uint16_t rne_bits(uint32_t u) {
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0;
    return static_cast<uint16_t>((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
inline uint16_t rne(float f) { uint32_t u; std::memcpy(&u, &f, 4); return rne_bits(u); }
inline float widen(uint16_t b) { const uint32_t u = static_cast<uint32_t>(b) << 16; float f; std::memcpy(&f, &u, 4); return f; }

// where pack_layer (pvnet_pack.h) puts w[co][ci][tap] of a layer with `cin` input channels
GMK_BF16_HD inline int f32_layer_index(int cin, int co, int ci, int tap) {
    const int CP = cin >= 16 ? 8 : cin / 2, chunks = cin / 2 / CP, groups = (chunks * 9 * CP + 3) / 4;
    const int tile = co / 32, lane = (co & 31) + 32 * (ci & 1), chunk = ci / (2 * CP), cp = (ci % (2 * CP)) / 2;
    const int kp = (chunk * 9 + tap) * CP + cp;
    return ((tile * groups + kp / 4) * 64 + lane) * 4 + (kp & 3);
}
// where pack_heads puts head row j (0..3 policy, 4..5 value) of layer-3 channel c: its per-channel block behind the 4x4x1 operands
GMK_BF16_HD inline int f32_head_index(int j, int c) { return 4 * 32 * 64 + ((c / 32) * 6 + j) * 32 + (c % 32); }

// element i of the bf16 buffer: which float32 buffer (0 = d_w1, 1 = d_w2, 2 = d_w3, 3 = d_wh) and which float of it; -1: a zero
GMK_BF16_HD inline int source(int i, int& buffer) {
    if (i < kQ2) {
        const int s = i / 512, lane = (i / 8) & 63, e = i & 7, tap = 2 * s + (lane >> 5);
        buffer = 0;
        return e < 6 && tap < 9 ? f32_layer_index(6, lane & 31, e, tap) : -1;
    }
    if (i < kQh) {
        const bool l3 = i >= kQ3;
        const int cin = l3 ? 64 : 32, per_tap = cin / 16, k = i - (l3 ? kQ3 : kQ2);
        const int tile = k / (9 * per_tap * 512), step = (k / 512) % (9 * per_tap), lane = (k / 8) & 63, e = k & 7;
        buffer = l3 ? 2 : 1;
        return f32_layer_index(cin, 32 * tile + (lane & 31), 16 * (step % per_tap) + 8 * (lane >> 5) + e, step / per_tap);
    }
    const int k = i - kQh, wave = k / 1024, s = (k / 512) & 1, lane = (k / 8) & 63, e = k & 7, j = lane & 31;
    buffer = 3;
    return j < 6 ? f32_head_index(j, 32 * wave + 16 * s + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3)) : -1;
}

// the host's packer: q[kElements] from the four float32 buffers as gmk_pvnet_create filled them
inline void pack(const float* w1, const float* w2, const float* w3, const float* wh, uint16_t* q) {
    const float* src[4] = {w1, w2, w3, wh};
    for (int i = 0; i < kElements; ++i) {
        int b = 0;
        const int at = source(i, b);
        q[i] = at < 0 ? 0 : rne(src[b][at]);
    }
}

}  // namespace bf16pack
}  // namespace gmk
