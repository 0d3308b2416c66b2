// train_host.h -- the host-side bookkeeping of the trainer (K11, train_kernel.hip): the parameter block's layout, the scratch sizing, the
// argument checks and the repack index table.  Plain C++ with no HIP in it, so that tools/train_host_check.cpp can run it under the
// address and undefined-behaviour sanitizers on a machine without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/gomoku_hip.h"
#include "pvnet_pack.h"

namespace gmk {
namespace train {

// ---- the parameter block: sixteen tensors side by side, in THIS order (the order of d_grads, of the moments and of gmk_train_get_block) ----
//   0 w1 [32][6][3][3]     1 b1 [32]     2 w2 [64][32][3][3]    3 b2 [64]     4 w3 [128][64][3][3]   5 b3 [128]
//   6 w_policy_conv [4][128]   7 w_value_conv [2][128]   8 b_policy_conv [4]   9 b_value_conv [2]      (the two 1x1 heads are one GEMM: N = 6)
//  10 w_policy [225][900]  11 b_policy [225]  12 w_hidden [64][450]  13 b_hidden [64]  14 w_out [64]  15 b_out [1]
constexpr int kTensors = 16;
constexpr int kSizes[kTensors] = {32 * 54, 32, 64 * 288, 64, 128 * 576, 128, 4 * 128, 2 * 128, 4, 2, 225 * 900, 225, 64 * 450, 64, 64, 1};
constexpr bool kIsWeight[kTensors] = {true, false, true, false, true, false, true, true, false, false, true, false, true, false, true, false};
// gmk_train_create / gmk_train_params / gmk_train_set_params take the arrays in the order of gmk_pvnet_create followed by gmk_pvnet_set_dense:
// w1 b1 w2 b2 w3 b3 w_policy_conv b_policy_conv w_value_conv b_value_conv w_policy b_policy w_hidden b_hidden w_out b_out; argument i is tensor
constexpr int kArgTensor[kTensors] = {0, 1, 2, 3, 4, 5, 6, 8, 7, 9, 10, 11, 12, 13, 14, 15};
constexpr int offset_of(int t) { int o = 0; for (int i = 0; i < t; ++i) o += kSizes[i]; return o; }
constexpr int kParams = offset_of(kTensors);
enum { W1, B1, W2, B2, W3, B3, WPC, WVC, BPC, BVC, WPD, BPD, WHID, BHID, WOUT, BOUT };

constexpr int kPix = 225;
constexpr int kSlabPos = 32;                       // positions whose im2col columns are held at once (layer 3: 32 x 225 x 576 floats = 16.6 MB)
constexpr int kKSlabPos = 8;                       // positions (x 225 rows) per split-K slab of a weight gradient
constexpr int kKSlabRows = kKSlabPos * kPix;
constexpr int kMaxBatchLimit = 4096;               // 225 x 4096 rows: every index of a whole-batch matrix stays far below 2^31

struct Scratch {                                   // all in floats
    size_t act1, act2, act3, pflat, vflat, logits, hidden, probs, value, dlogits, dz, dhid, dh6, dact3, dact2, dact1, col, splitk, partial, total;
};

inline int k_slabs(int n) { return (n + kKSlabPos - 1) / kKSlabPos; }

// what a trainer for batches of up to max_batch positions holds besides the four parameter-sized blocks
inline Scratch scratch_floats(int max_batch) {
    Scratch s{};
    const size_t n = static_cast<size_t>(max_batch), rows = n * kPix, slab_rows = static_cast<size_t>(max_batch < kSlabPos ? max_batch : kSlabPos) * kPix;
    s.act1 = rows * 32; s.act2 = rows * 64; s.act3 = rows * 128;
    s.pflat = n * 900; s.vflat = n * 450; s.logits = n * kPix; s.hidden = n * 64; s.probs = n * kPix; s.value = n;
    s.dlogits = n * kPix; s.dz = n; s.dhid = n * 64; s.dh6 = rows * 6;
    s.dact3 = rows * 128; s.dact2 = rows * 64; s.dact1 = rows * 32;
    s.col = slab_rows * 576;
    s.splitk = static_cast<size_t>(k_slabs(max_batch)) * (128 * 576);     // the largest weight gradient, one copy per K slab
    s.partial = n * 4;
    s.total = s.act1 + s.act2 + s.act3 + s.pflat + s.vflat + s.logits + s.hidden + s.probs + s.value + s.dlogits + s.dz + s.dhid + s.dh6 + s.dact3 +
              s.dact2 + s.dact1 + s.col + s.splitk + s.partial;
    return s;
}

inline bool valid_max_batch(long long max_batch) { return max_batch >= 1 && max_batch <= kMaxBatchLimit; }
// a batch call: n within the trainer's capacity, the pointers it needs present and 4-byte aligned
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool valid_batch(int n, int max_batch, const void* const* required, int n_required, const void* const* optional, int n_optional) {
    if (n < 1 || n > max_batch) return false;
    for (int i = 0; i < n_required; ++i) if (!required[i] || !aligned4(required[i])) return false;
    for (int i = 0; i < n_optional; ++i) if (optional[i] && !aligned4(optional[i])) return false;
    return true;
}

// ---- the kernel-level entries (gmk_train_kernel_*): the caller chooses strides and extents, so every index is worked out here, in int64, before
// anything is launched.  Each check returns nullptr if the call fits and the name of the first field at fault otherwise.
constexpr int64_t kStrideLimit = int64_t(1) << 31;     // strides and dimensions below 2^31: every product of two of them fits an int64
constexpr int64_t kGridYZLimit = 65535;                // blocks along y (rows / 128) and z (k slabs) of one launch
inline bool stride_ok(int64_t s) { return s >= 0 && s < kStrideLimit; }
inline bool required_ptr(const void* p) { return p && aligned4(p); }

inline const char* gemm_fits(const gmk_train_gemm_desc& d) {
    if (d.M < 1) return "M";
    if (d.N < 1) return "N";
    if (d.K < 1) return "K";
    if ((static_cast<int64_t>(d.M) + 127) / 128 > kGridYZLimit) return "M";
    if (!required_ptr(d.A)) return "A";
    if (!required_ptr(d.B)) return "B";
    if (!stride_ok(d.sam)) return "sam";
    if (!stride_ok(d.sak)) return "sak";
    if (!stride_ok(d.sbk)) return "sbk";
    if (!stride_ok(d.sbn)) return "sbn";
    const int64_t M = d.M, N = d.N, K = d.K;
    if ((M - 1) * d.sam + (K - 1) * d.sak >= d.a_floats) return "a_floats";
    if ((K - 1) * d.sbk + (N - 1) * d.sbn >= d.b_floats) return "b_floats";
    if (d.kslab < 1) return "kslab";
    if (d.nz < 1 || d.nz > kGridYZLimit) return "nz";
    const int64_t span = static_cast<int64_t>(d.nz) * d.kslab;
    if (span < K || span >= kStrideLimit) return "nz";
    // the optional operands are held to their extents in both forms, though the split-K form does not read them
    if (d.bias && (!aligned4(d.bias) || N - 1 >= d.bias_floats)) return "bias";
    if (d.mask) {
        if (!aligned4(d.mask)) return "mask";
        if (!stride_ok(d.ldm)) return "ldm";
        if ((M - 1) * d.ldm + (N - 1) >= d.mask_floats) return "mask_floats";
    }
    if (d.relu != 0 && d.relu != 1) return "relu";
    if (d.part) {                                      // split-K: nz slabs, each with at least one k
        if (!aligned4(d.part)) return "part";
        if ((static_cast<int64_t>(d.nz) - 1) * d.kslab >= K) return "nz";
        if (d.z0 < 0) return "z0";
        if (d.part_floats < M * N || static_cast<int64_t>(d.z0) + d.nz > d.part_floats / (M * N)) return "part_floats";
        return nullptr;
    }
    if (d.nz != 1) return "nz";                        // direct: one slab that holds every k
    if (d.kslab < K) return "kslab";
    if (d.nsplit < 0) return "nsplit";
    if (d.cq < 1) return "cq";
    const int64_t nc = d.nsplit < N ? d.nsplit : N;    // columns 0 .. nc - 1 go to C, the rest to C2
    if (nc > 0) {
        if (!required_ptr(d.C)) return "C";
        if (!stride_ok(d.ldc)) return "ldc";
        int64_t row = nc;                              // one row's extent under the store map
        if (d.cq < nc) {
            if (!stride_ok(d.cs) || d.cs < d.cq) return "cs";          // groups of cq columns, cs apart: they must not overlap
            row = ((nc - 1) / d.cq) * d.cs + (nc - 1) % d.cq + 1;
        }
        if (d.ldc < row) return "ldc";
        if ((M - 1) * d.ldc + row > d.c_floats) return "c_floats";
    }
    if (nc < N) {
        if (!required_ptr(d.C2)) return "C2";
        if (!stride_ok(d.ldc2) || d.ldc2 < N - nc) return "ldc2";
        if ((M - 1) * d.ldc2 + (N - nc) > d.c2_floats) return "c2_floats";
    }
    return nullptr;
}

inline const char* reduce_fits(const void* part, int nz, int64_t mn, const void* out) {
    if (!required_ptr(part)) return "part";
    if (!required_ptr(out)) return "out";
    if (nz < 1) return "nz";
    if (mn < 1 || mn >= kStrideLimit) return "mn";     // nz * mn fits an int64, (mn + 255) / 256 a grid
    return nullptr;
}

// npos positions of C channels: 225 npos rows of 9 C columns, all of it below 2^31 floats
inline const char* conv_fits(int C, int npos) {
    if (C < 1) return "C";
    if (npos < 1) return "npos";
    if (static_cast<int64_t>(C) * npos > (kStrideLimit - 1) / (9 * kPix)) return "npos";
    return nullptr;
}
inline const char* im2col_fits(const void* in, int64_t in_floats, int64_t sb, int64_t sp, int64_t sc, int C, int npos, const void* col) {
    if (const char* bad = conv_fits(C, npos)) return bad;
    if (!required_ptr(in)) return "in";
    if (!required_ptr(col)) return "col";
    if (!stride_ok(sb)) return "sb";
    if (!stride_ok(sp)) return "sp";
    if (!stride_ok(sc)) return "sc";
    if ((npos - int64_t(1)) * sb + (kPix - 1) * sp + (C - int64_t(1)) * sc >= in_floats) return "in_floats";
    return nullptr;
}
inline const char* col2im_fits(const void* dcol, int C, int npos, const void* mask, const void* out) {
    if (const char* bad = conv_fits(C, npos)) return bad;
    if (!required_ptr(dcol)) return "dcol";
    if (!required_ptr(mask)) return "mask";
    if (!required_ptr(out)) return "out";
    return nullptr;
}

// ---- the repack table: for every float of a gmk_pvnet's seven device buffers, 1 + the index of the parameter it holds, or 0 for a zero ----
// Segments in the order d_w1, d_w2, d_w3, d_wh, d_b, d_wp, d_dense; seg[i] .. seg[i + 1] is buffer i's part of the table.
constexpr int kRepackBuffers = 7;
inline bool build_repack_table(std::vector<int32_t>& table, size_t (&seg)[kRepackBuffers + 1]) {
    std::vector<float> ids(kParams);
    for (int i = 0; i < kParams; ++i) ids[i] = static_cast<float>(i + 1);                       // exact: kParams < 2^24
    static_assert(kParams < (1 << 24), "parameter indices must be exact in float32");
    auto at = [&](int t) { return ids.data() + offset_of(t); };
    std::vector<float> out[kRepackBuffers];
    pvpack::pack_layer(at(W1), 6, 32, out[0]);
    pvpack::pack_layer(at(W2), 32, 64, out[1]);
    pvpack::pack_layer(at(W3), 64, 128, out[2]);
    pvpack::pack_heads(at(WPC), at(WVC), out[3]);
    pvpack::pack_bias(at(B1), at(B2), at(B3), at(BPC), at(BVC), out[4]);
    pvpack::pack_dense(at(WPD), at(BPD), at(WHID), at(BHID), at(WOUT), out[5], out[6]);
    table.clear();
    seg[0] = 0;
    for (int b = 0; b < kRepackBuffers; ++b) {
        for (float v : out[b]) {
            const int32_t id = static_cast<int32_t>(v);
            if (id < 0 || id > kParams || static_cast<float>(id) != v) return false;           // a packer that is not a pure gather
            table.push_back(id);
        }
        seg[b + 1] = table.size();
    }
    return true;
}

// TF1's Adam (tf.train.AdamOptimizer): the step size of step t >= 1
inline double adam_lr_t(double lr, long long t);

}  // namespace train
}  // namespace gmk

#include <cmath>
inline double gmk::train::adam_lr_t(double lr, long long t) {
    return lr * std::sqrt(1.0 - std::pow(0.999, static_cast<double>(t))) / (1.0 - std::pow(0.9, static_cast<double>(t)));
}
