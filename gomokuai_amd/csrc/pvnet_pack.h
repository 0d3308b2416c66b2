// pvnet_pack.h -- the host-side packers of K9's device buffers and the gmk_pvnet handle (host code only, plain C++).
//
// gmk_pvnet_create / gmk_pvnet_set_dense (pvnet_kernel.hip) run these on the weights; the trainer (train_kernel.hip, train_host.h) runs the
// SAME functions once on arrays that hold `index + 1` to learn where every packed float comes from, so the layouts are stated once, here.
// Every packer is a pure gather with zero padding: an output float is one input float or 0.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace gmk {
namespace pvpack {

constexpr int kPix = 225;
constexpr int kHeadRows = 6;                       // 4 policy + 2 value channels
constexpr int kDenseBody = 12, kDenseBodies = 19, kPolicySteps = 225;       // pvnet_dense_kernel's walk (pvnet_kernel.hip)
constexpr int kBiasFloats = 32 + 64 + 128 + 8;     // b1 | b2 | b3 | b_policy_conv [4] | b_value_conv [2] | 2 pad
constexpr int kHeadFloats = 4 * 32 * 64 + 4 * kHeadRows * 32;
constexpr int kDenseBlockFloats = 256 + 64 + 64;   // policy biases [256] | hidden biases [64] | output weights [64]
constexpr size_t kDenseWeightFloats = static_cast<size_t>(4) * (kDenseBodies + 1) * kDenseBody * 5 * 64;

// The order in which a layer's k-pairs are walked (and packed): chunks of 2 * CP input channels; inside a chunk the nine taps; inside a tap
// ("step") the chunk's CP channel pairs.
inline void step_chunk_tap(int step, int& chunk, int& tap) { chunk = step / 9; tap = step - 9 * chunk; }

// A operands of one layer in lane order, four consecutive k-pairs of a lane side by side: [cout tile][k-pair / 4][64 lanes][4]; k-pair order as
// conv_tiles() walks it (layer 1's 27 k-pairs: seven groups, the last one padded)
inline void pack_layer(const float* w /* [cout][cin][3][3] */, int cin, int cout, std::vector<float>& out) {
    const int CP = cin >= 16 ? 8 : cin / 2, chunks = cin / 2 / CP, steps = chunks * 9, kps = steps * CP, groups = (kps + 3) / 4;
    out.assign((static_cast<size_t>(cout / 32) * groups + 2 * CP / 4 + 1) * 256, 0.0f);      // + the two steps conv_tiles() fetches past the last tile's end
    for (int tile = 0; tile < cout / 32; ++tile)
        for (int step = 0; step < steps; ++step) {
            int chunk, tap;
            step_chunk_tap(step, chunk, tap);
            for (int cp = 0; cp < CP; ++cp) {
                const int kp = step * CP + cp;
                for (int lane = 0; lane < 64; ++lane) {
                    const int co = tile * 32 + (lane & 31), ci = chunk * 2 * CP + 2 * cp + (lane >> 5);
                    out[((static_cast<size_t>(tile) * groups + kp / 4) * 64 + lane) * 4 + (kp & 3)] = w[(static_cast<size_t>(co) * cin + ci) * 9 + tap];
                }
            }
        }
}

// The 1x1 heads: [4 waves][16 registers policy, 16 registers value][64 lanes] A operands of the 4x4x1 form, then [4 waves][6 rows][32 channels]
// for the corner pixel.  wp [4][128], wv [2][128].
inline void pack_heads(const float* wp, const float* wv, std::vector<float>& ph) {
    ph.assign(kHeadFloats, 0.0f);
    for (int wave = 0; wave < 4; ++wave)                         // 4x4x1 A operands: lane l carries row l % 4 of its block, for the channel that accumulator
        for (int r = 0; r < 16; ++r)                             // register r of wave `wave` holds on that lane half
            for (int lane = 0; lane < 64; ++lane) {
                const int c = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), j = lane & 3;
                ph[(wave * 32 + r) * 64 + lane] = wp[j * 128 + c];
                ph[(wave * 32 + 16 + r) * 64 + lane] = j < 2 ? wv[j * 128 + c] : 0.0f;
            }
    for (int wave = 0; wave < 4; ++wave)                         // ... and per channel for the corner pixel
        for (int j = 0; j < kHeadRows; ++j)
            for (int c = 0; c < 32; ++c) ph[4 * 32 * 64 + (wave * kHeadRows + j) * 32 + c] = j < 4 ? wp[j * 128 + 32 * wave + c] : wv[(j - 4) * 128 + 32 * wave + c];
}

inline void pack_bias(const float* b1, const float* b2, const float* b3, const float* bp, const float* bv, std::vector<float>& bias) {
    bias.assign(kBiasFloats, 0.0f);
    std::memcpy(&bias[0], b1, 32 * 4); std::memcpy(&bias[32], b2, 64 * 4); std::memcpy(&bias[96], b3, 128 * 4);
    std::memcpy(&bias[224], bp, 4 * 4); std::memcpy(&bias[228], bv, 2 * 4);
}

// B operands of v_mfma_f32_16x16x4_f32 in lane order: lane l carries W[output = 16 tile + (l & 15)][k = 4 step + (l >> 4)]; per wave and body
// the nine steps' four policy tiles and hidden tile side by side (zeros: the 16th policy tile, k >= 450 of the hidden layer, the pad body);
// and the block policy biases [256] | hidden biases [64] | output weights [64]
inline void pack_dense(const float* w_policy, const float* b_policy, const float* w_hidden, const float* b_hidden, const float* w_out,
                       std::vector<float>& wp, std::vector<float>& dense) {
    wp.assign(kDenseWeightFloats, 0.0f);
    dense.assign(kDenseBlockFloats, 0.0f);
    for (int wave = 0; wave < 4; ++wave)
        for (int step = 0; step < kPolicySteps; ++step)
            for (int q = 0; q < 5; ++q)
                for (int lane = 0; lane < 64; ++lane) {
                    const int k = 4 * step + (lane >> 4), body = step / kDenseBody, g = (step % kDenseBody) / 4;
                    float v = 0.0f;
                    if (q < 4) { const int o = 16 * (wave + 4 * q) + (lane & 15); if (o < kPix) v = w_policy[static_cast<size_t>(o) * 900 + k]; }
                    else if (k < 450) v = w_hidden[static_cast<size_t>(16 * wave + (lane & 15)) * 450 + k];
                    wp[((((static_cast<size_t>(wave) * (kDenseBodies + 1) + body) * 5 + q) * 3 + g) * 64 + lane) * 4 + (step & 3)] = v;
                }
    std::memcpy(&dense[0], b_policy, kPix * 4); std::memcpy(&dense[256], b_hidden, 64 * 4); std::memcpy(&dense[320], w_out, 64 * 4);
}

}  // namespace pvpack
}  // namespace gmk

// The handle itself is declared here, next to the packers that define what its buffers hold, because two translation units fill them:
// pvnet_kernel.hip (create / set_dense, from host arrays) and train_kernel.hip (gmk_train_export, on the device).
struct gmk_pvnet {
    float *d_w1 = nullptr, *d_w2 = nullptr, *d_w3 = nullptr, *d_wh = nullptr, *d_b = nullptr;
    bool attr_set = false;
    // the dense layers (gmk_pvnet_set_dense): packed weights, biases (policy [256] | hidden [64] | output weights [64]), the output bias, and the
    // head activations between the two kernels of gmk_pvnet_evaluate ([capacity][900 + 450], grown on demand)
    float *d_wp = nullptr, *d_dense = nullptr, *d_flat = nullptr;
    float b_out = 0.0f;
    bool has_dense = false, dense_attr_set = false;
    int flat_capacity = 0;
    // "K9 in bf16" (gmk_pvnet_set_precision): the bf16 weight buffer derived from d_w1 .. d_wh (pvnet_bf16_pack.h), allocated at the first
    // switch to GMK_PVNET_BF16 and kept; `precision` picks the trunk kernel
    int precision = 0;                               // GMK_PVNET_F32
    unsigned short* d_q = nullptr;
    bool bf16_attr_set = false;
    // "K22" (gmk_pvnet_evaluate_sym, pvnet_sym_kernel.hip): expanded states, their outputs and the picks, [sym_capacity] rows, grown on demand
    float* d_sym = nullptr;
    int sym_capacity = 0;
};

namespace gmk {
// pvnet_bf16_kernel.hip: the bf16 trunk in place of pvnet_trunk_kernel, and d_q refreshed from d_w1 .. d_wh by one kernel on `stream`
int pvnet_bf16_launch(gmk_pvnet* net, const float* d_states, int n, float* d_pflat, float* d_vflat, void* stream);
int pvnet_bf16_refresh(gmk_pvnet* net, void* stream);
// pvnet_sym_kernel.hip: gives d_sym back
void pvnet_sym_release(gmk_pvnet* net);
}  // namespace gmk
