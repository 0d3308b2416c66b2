// train_host.h -- the host-side bookkeeping of the trainer (K11, train_kernel.hip): the parameter block's layout, the scratch sizing, the
// argument checks and the repack index table.  Plain C++ with no HIP in it, so that tools/train_host_check.cpp can run it under the
// address and undefined-behaviour sanitizers on a machine without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

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
