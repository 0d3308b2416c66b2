// train_host_check.cpp -- the trainer's host-side bookkeeping (gomokuai_amd/csrc/train_host.h, pvnet_pack.h) as a stand-alone program, for a
// run under the address and undefined-behaviour sanitizers on a machine without a GPU:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined tools/train_host_check.cpp -o tools/bin/train_host_check && tools/bin/train_host_check
// It builds the repack index table from the packers, checks that every parameter reaches every buffer it should, walks the scratch sizing
// and the argument checks over their edge cases, and exits non-zero on the first thing that is wrong.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gomokuai_amd/csrc/train_host.h"

using namespace gmk::train;

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "train_host_check: %s failed (line %d)\n", #cond, __LINE__); return 1; } } while (0)

int main() {
    REQUIRE(kParams == 326540);
    for (int a = 0, seen = 0; a < kTensors; ++a) { seen |= 1 << kArgTensor[a]; if (a == kTensors - 1) REQUIRE(seen == 0xFFFF); }

    // ---- the index table ----
    std::vector<int32_t> table;
    size_t seg[kRepackBuffers + 1];
    REQUIRE(build_repack_table(table, seg));
    REQUIRE(seg[kRepackBuffers] == table.size());
    REQUIRE(seg[4] - seg[3] == static_cast<size_t>(gmk::pvpack::kHeadFloats) && seg[5] - seg[4] == static_cast<size_t>(gmk::pvpack::kBiasFloats));
    REQUIRE(seg[6] - seg[5] == gmk::pvpack::kDenseWeightFloats && seg[7] - seg[6] == static_cast<size_t>(gmk::pvpack::kDenseBlockFloats));
    std::vector<int> uses(kParams + 1, 0);
    for (int32_t id : table) { REQUIRE(id >= 0 && id <= kParams); ++uses[id]; }
    for (int t = 0; t < kTensors; ++t)                               // every parameter but b_out (a host scalar of the handle) is packed somewhere
        for (int i = 0; i < kSizes[t]; ++i) REQUIRE((uses[offset_of(t) + i + 1] > 0) == (t != BOUT));
    // applying the table to real values gives what the packers give
    std::vector<float> params(kParams);
    for (int i = 0; i < kParams; ++i) params[i] = static_cast<float>((i * 2654435761u) >> 8) * 1e-6f - 8.0f;
    std::vector<float> direct[kRepackBuffers];
    auto at = [&](int t) { return params.data() + offset_of(t); };
    gmk::pvpack::pack_layer(at(W1), 6, 32, direct[0]);
    gmk::pvpack::pack_layer(at(W2), 32, 64, direct[1]);
    gmk::pvpack::pack_layer(at(W3), 64, 128, direct[2]);
    gmk::pvpack::pack_heads(at(WPC), at(WVC), direct[3]);
    gmk::pvpack::pack_bias(at(B1), at(B2), at(B3), at(BPC), at(BVC), direct[4]);
    gmk::pvpack::pack_dense(at(WPD), at(BPD), at(WHID), at(BHID), at(WOUT), direct[5], direct[6]);
    for (int b = 0; b < kRepackBuffers; ++b) {
        REQUIRE(direct[b].size() == seg[b + 1] - seg[b]);
        for (size_t i = 0; i < direct[b].size(); ++i) {
            const int32_t id = table[seg[b] + i];
            REQUIRE((id ? params[id - 1] : 0.0f) == direct[b][i]);
        }
    }

    // ---- scratch sizing ----
    for (int mb : {1, 2, 7, 8, 9, 31, 32, 33, 130, 512, kMaxBatchLimit}) {
        const Scratch s = scratch_floats(mb);
        REQUIRE(s.col == static_cast<size_t>(mb < kSlabPos ? mb : kSlabPos) * kPix * 576);
        REQUIRE(s.splitk == static_cast<size_t>((mb + 7) / 8) * 128 * 576);
        // the k slabs of all position slabs of a batch of n <= mb fit the split-K buffer, as do the column sums of 225 n rows
        for (int n = 1; n <= mb; n += (mb > 64 ? 37 : 1)) {
            int z = 0;
            for (int pos0 = 0; pos0 < n; pos0 += kSlabPos) { const int ns = (n - pos0 < kSlabPos ? n - pos0 : kSlabPos); z += (ns * kPix + kKSlabRows - 1) / kKSlabRows; }
            REQUIRE(z <= k_slabs(mb) && (n * kPix + kKSlabRows - 1) / kKSlabRows <= k_slabs(mb));
        }
        REQUIRE(s.total > s.act1 + s.act2 + s.act3 && s.total * 4 < (static_cast<size_t>(1) << 36));
    }
    REQUIRE(!valid_max_batch(0) && !valid_max_batch(-1) && valid_max_batch(1) && valid_max_batch(kMaxBatchLimit) && !valid_max_batch(kMaxBatchLimit + 1LL));

    // ---- argument checks ----
    alignas(8) char buf[16];
    const void* good[2] = {buf, buf + 4};
    const void* null_in[2] = {buf, nullptr};
    const void* odd[2] = {buf, buf + 2};
    REQUIRE(valid_batch(1, 4, good, 2, nullptr, 0) && valid_batch(4, 4, good, 2, null_in, 2));
    REQUIRE(!valid_batch(0, 4, good, 2, nullptr, 0) && !valid_batch(5, 4, good, 2, nullptr, 0) && !valid_batch(-3, 4, good, 2, nullptr, 0));
    REQUIRE(!valid_batch(1, 4, null_in, 2, nullptr, 0) && !valid_batch(1, 4, odd, 2, nullptr, 0) && !valid_batch(1, 4, good, 2, odd, 2));

    // ---- Adam's step size ----
    REQUIRE(std::fabs(adam_lr_t(0.1, 1) - 0.1 * std::sqrt(0.001) / 0.1) < 1e-15);
    std::printf("train_host_check: ok (%zu table entries, %d parameters)\n", table.size(), kParams);
    return 0;
}
