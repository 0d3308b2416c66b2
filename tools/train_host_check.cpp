// train_host_check.cpp -- the trainer's host-side bookkeeping (gomokuai_amd/csrc/train_host.h, pvnet_pack.h) as a stand-alone program, for a
// run under the address and undefined-behaviour sanitizers on a machine without a GPU:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined tools/train_host_check.cpp -o tools/bin/train_host_check && tools/bin/train_host_check
// It builds the repack index table from the packers, checks that every parameter reaches every buffer it should, walks the scratch sizing,
// the argument checks and the kernel-level entries' addressing checks (gemm_fits ...) over their edge cases, and exits non-zero on the first thing that is wrong.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

    // ---- the kernel-level entries' addressing checks (gemm_fits and its kin): every buffer is 4 floats that nothing dereferences ----
    {
        alignas(16) static float mem[4];
        auto refused = [](const gmk_train_gemm_desc& d, const char* field) { const char* bad = gemm_fits(d); return bad && std::strcmp(bad, field) == 0; };
        // a 5 x 7 x 3 direct GEMM with every optional buffer, each extent exactly its largest index + 1
        gmk_train_gemm_desc ok{};
        ok.A = mem; ok.sam = 4; ok.sak = 1; ok.a_floats = 4 * 4 + 2 + 1;
        ok.B = mem; ok.sbk = 1; ok.sbn = 3; ok.b_floats = 2 + 6 * 3 + 1;
        ok.M = 5; ok.N = 7; ok.K = 3; ok.kslab = 3; ok.nz = 1; ok.z0 = 0;
        ok.C = mem; ok.ldc = 9; ok.cq = INT_MAX; ok.cs = 0; ok.c_floats = 4 * 9 + 7;
        ok.nsplit = INT_MAX; ok.C2 = nullptr;
        ok.bias = mem; ok.bias_floats = 7; ok.relu = 1; ok.mask = mem; ok.ldm = 8; ok.mask_floats = 4 * 8 + 7;
        REQUIRE(gemm_fits(ok) == nullptr);
        gmk_train_gemm_desc d;
        // the largest index exactly at the extent passes (above); one beyond it is refused, buffer by buffer
        d = ok; d.a_floats -= 1; REQUIRE(refused(d, "a_floats"));
        d = ok; d.b_floats -= 1; REQUIRE(refused(d, "b_floats"));
        d = ok; d.c_floats -= 1; REQUIRE(refused(d, "c_floats"));
        d = ok; d.bias_floats -= 1; REQUIRE(refused(d, "bias"));
        d = ok; d.mask_floats -= 1; REQUIRE(refused(d, "mask_floats"));
        d = ok; d.a_floats = 0; REQUIRE(refused(d, "a_floats"));
        d = ok; d.a_floats = -1; REQUIRE(refused(d, "a_floats"));
        // null and misaligned pointers; the optional ones may be null
        d = ok; d.A = nullptr; REQUIRE(refused(d, "A"));
        d = ok; d.B = nullptr; REQUIRE(refused(d, "B"));
        d = ok; d.C = nullptr; REQUIRE(refused(d, "C"));
        d = ok; d.A = reinterpret_cast<const float*>(reinterpret_cast<const char*>(mem) + 2); REQUIRE(refused(d, "A"));
        d = ok; d.B = reinterpret_cast<const float*>(reinterpret_cast<const char*>(mem) + 1); REQUIRE(refused(d, "B"));
        d = ok; d.C = reinterpret_cast<float*>(reinterpret_cast<char*>(mem) + 2); REQUIRE(refused(d, "C"));
        d = ok; d.bias = reinterpret_cast<const float*>(reinterpret_cast<const char*>(mem) + 2); REQUIRE(refused(d, "bias"));
        d = ok; d.mask = reinterpret_cast<const float*>(reinterpret_cast<const char*>(mem) + 3); REQUIRE(refused(d, "mask"));
        d = ok; d.bias = nullptr; d.mask = nullptr; d.bias_floats = d.mask_floats = 0; REQUIRE(gemm_fits(d) == nullptr);
        // strides: negative is refused, 0 is a stride like any other (the extent shrinks with it), 2^31 is too large
        d = ok; d.sam = -1; REQUIRE(refused(d, "sam"));
        d = ok; d.sak = -1; REQUIRE(refused(d, "sak"));
        d = ok; d.sbk = -1; REQUIRE(refused(d, "sbk"));
        d = ok; d.sbn = -1; REQUIRE(refused(d, "sbn"));
        d = ok; d.ldm = -1; REQUIRE(refused(d, "ldm"));
        d = ok; d.ldc = -9; REQUIRE(refused(d, "ldc"));
        d = ok; d.sam = kStrideLimit; REQUIRE(refused(d, "sam"));
        d = ok; d.sam = 0; d.sak = 0; d.a_floats = 1; REQUIRE(gemm_fits(d) == nullptr);
        d.a_floats = 0; REQUIRE(refused(d, "a_floats"));
        d = ok; d.sbn = 0; d.b_floats = 3; REQUIRE(gemm_fits(d) == nullptr);
        d.b_floats = 2; REQUIRE(refused(d, "b_floats"));
        d = ok; d.ldm = 0; d.mask_floats = 7; REQUIRE(gemm_fits(d) == nullptr);
        // shapes
        d = ok; d.M = 0; REQUIRE(refused(d, "M"));
        d = ok; d.N = 0; REQUIRE(refused(d, "N"));
        d = ok; d.K = 0; REQUIRE(refused(d, "K"));
        d = ok; d.M = -5; REQUIRE(refused(d, "M"));
        d = ok; d.M = 128 * 65535 + 1; REQUIRE(refused(d, "M"));
        d = ok; d.relu = 2; REQUIRE(refused(d, "relu"));
        // the direct form: one slab that holds every k
        d = ok; d.kslab = 0; REQUIRE(refused(d, "kslab"));
        d = ok; d.kslab = 2; REQUIRE(refused(d, "nz"));                           // nz * kslab < K
        d = ok; d.kslab = 2; d.nz = 2; REQUIRE(refused(d, "nz"));                 // covers K, but a direct launch of two slabs would store twice
        d = ok; d.kslab = 3; d.nz = 2; REQUIRE(refused(d, "nz"));
        d = ok; d.nz = 0; REQUIRE(refused(d, "nz"));
        d = ok; d.kslab = INT_MAX; REQUIRE(gemm_fits(d) == nullptr);
        // int64 products that wrap in int32: 70 000 rows of stride 70 000 end at 4 899 930 000 + 2
        d = ok; d.M = 70000; d.sam = 70000; d.a_floats = 69999LL * 70000 + 2 + 1; d.ldc = 70000; d.c_floats = 69999LL * 70000 + 7;
        d.ldm = 70000; d.mask_floats = 69999LL * 70000 + 7;
        REQUIRE(gemm_fits(d) == nullptr);
        d.a_floats -= 1; REQUIRE(refused(d, "a_floats")); d.a_floats += 1;
        d.c_floats -= 1; REQUIRE(refused(d, "c_floats")); d.c_floats += 1;
        d.mask_floats -= 1; REQUIRE(refused(d, "mask_floats")); d.mask_floats += 1;
        d.a_floats = static_cast<int32_t>(static_cast<uint32_t>(69999LL * 70000 + 3)); REQUIRE(refused(d, "a_floats"));      // what int32 would have made of it
        d = ok; d.M = 1; d.K = INT_MAX; d.kslab = INT_MAX; d.sak = kStrideLimit - 1; d.a_floats = (INT_MAX - 1LL) * (kStrideLimit - 1) + 1;
        d.sbk = 0; d.b_floats = 6 * 3 + 1; d.c_floats = 7; d.mask_floats = 7;
        REQUIRE(gemm_fits(d) == nullptr);
        d.a_floats -= 1; REQUIRE(refused(d, "a_floats"));
        // the store map: groups of cq columns cs apart, rows ldc apart, columns from nsplit on in C2
        d = ok; d.cq = 0; REQUIRE(refused(d, "cq"));
        d = ok; d.cq = 2; d.cs = 1; REQUIRE(refused(d, "cs"));                    // groups overlap
        d = ok; d.cq = 2; d.cs = -2; REQUIRE(refused(d, "cs"));
        d = ok; d.cq = 2; d.cs = 2; REQUIRE(gemm_fits(d) == nullptr);             // 7 columns in groups of 2, 2 apart: a row is 7 floats
        d = ok; d.cq = 2; d.cs = 3; d.ldc = 10; d.c_floats = 4 * 10 + 10; REQUIRE(gemm_fits(d) == nullptr);       // 3 * 3 + 0 + 1 = 10 floats
        d.ldc = 9; REQUIRE(refused(d, "ldc"));
        d.ldc = 10; d.c_floats -= 1; REQUIRE(refused(d, "c_floats"));
        d = ok; d.ldc = 6; REQUIRE(refused(d, "ldc"));                            // rows overlap
        d = ok; d.ldc = 7; d.c_floats = 4 * 7 + 7; REQUIRE(gemm_fits(d) == nullptr);
        d = ok; d.nsplit = 4; REQUIRE(refused(d, "C2"));                          // a split needs its second output
        d = ok; d.nsplit = -1; REQUIRE(refused(d, "nsplit"));
        d = ok; d.nsplit = 4; d.ldc = 4; d.c_floats = 4 * 4 + 4; d.C2 = mem; d.ldc2 = 3; d.c2_floats = 4 * 3 + 3; REQUIRE(gemm_fits(d) == nullptr);
        d.ldc2 = 2; REQUIRE(refused(d, "ldc2"));
        d.ldc2 = 3; d.c2_floats -= 1; REQUIRE(refused(d, "c2_floats")); d.c2_floats += 1;
        d.ldc = 3; REQUIRE(refused(d, "ldc"));
        d.ldc = 4; d.nsplit = 7; REQUIRE(refused(d, "ldc"));                      // nsplit = N: all seven columns in C again, rows of 4 overlap
        d.nsplit = 0; d.C = nullptr; d.c_floats = 0; d.ldc2 = 7; d.c2_floats = 4 * 7 + 7; REQUIRE(gemm_fits(d) == nullptr);      // everything to C2
        d.c2_floats -= 1; REQUIRE(refused(d, "c2_floats"));
        // the split-K form: exactly ceil(K / kslab) slabs, all of them inside part
        gmk_train_gemm_desc sp = ok;
        sp.C = nullptr; sp.c_floats = 0; sp.K = 7; sp.kslab = 3; sp.nz = 3; sp.z0 = 2; sp.part = mem; sp.part_floats = 5 * 5 * 7;
        sp.a_floats = 4 * 4 + 6 + 1; sp.b_floats = 6 + 6 * 3 + 1;
        REQUIRE(gemm_fits(sp) == nullptr);
        d = sp; d.part_floats -= 1; REQUIRE(refused(d, "part_floats"));
        d = sp; d.part_floats = 0; REQUIRE(refused(d, "part_floats"));
        d = sp; d.nz = 2; REQUIRE(refused(d, "nz"));                              // k = 6 dropped
        d = sp; d.nz = 4; d.part_floats += 5 * 7; REQUIRE(refused(d, "nz"));      // a fourth slab would hold no k
        d = sp; d.z0 = -1; REQUIRE(refused(d, "z0"));
        d = sp; d.kslab = 0; REQUIRE(refused(d, "kslab"));
        d = sp; d.part = reinterpret_cast<float*>(reinterpret_cast<char*>(mem) + 2); REQUIRE(refused(d, "part"));
        d = sp; d.sak = 0; d.sbk = 0; d.nz = 65536; d.kslab = 1; d.K = 65536; REQUIRE(refused(d, "nz"));
        d = sp; d.M = 1; d.N = 1; d.sbn = 0; d.K = INT_MAX; d.sak = 0; d.sbk = 0; d.kslab = 1 << 30; d.nz = 2; REQUIRE(refused(d, "nz"));      // nz * kslab = 2^31
        d = sp; d.z0 = INT_MAX; d.part_floats = INT64_MAX; REQUIRE(gemm_fits(d) == nullptr);      // z0 + nz is an int64 sum
        d = sp; d.bias_floats = 6; REQUIRE(refused(d, "bias"));                   // named buffers are held to their extents in this form too

        // the reduction, im2col and col2im
        REQUIRE(reduce_fits(mem, 1, 1, mem) == nullptr && reduce_fits(mem, 33, kStrideLimit - 1, mem) == nullptr);
        REQUIRE(reduce_fits(nullptr, 1, 1, mem) && reduce_fits(mem, 1, 1, nullptr) && reduce_fits(mem, 0, 1, mem) && reduce_fits(mem, 1, 0, mem));
        REQUIRE(reduce_fits(mem, 1, kStrideLimit, mem) && reduce_fits(reinterpret_cast<char*>(mem) + 2, 1, 1, mem));
        // channels-last, 3 positions of 5 channels: the largest index is 2 * 1125 + 224 * 5 + 4
        REQUIRE(im2col_fits(mem, 3 * 1125, 1125, 5, 1, 5, 3, mem) == nullptr);
        REQUIRE(std::strcmp(im2col_fits(mem, 3 * 1125 - 1, 1125, 5, 1, 5, 3, mem), "in_floats") == 0);
        REQUIRE(im2col_fits(mem, 3 * 1125, 1125, 1, 225, 5, 3, mem) == nullptr && im2col_fits(mem, 3 * 1125 - 1, 1125, 1, 225, 5, 3, mem));      // planes
        REQUIRE(im2col_fits(mem, 1, 0, 0, 0, 5, 3, mem) == nullptr && im2col_fits(mem, 0, 0, 0, 0, 5, 3, mem));                                // stride 0
        REQUIRE(im2col_fits(mem, 3 * 1125, -1, 5, 1, 5, 3, mem) && im2col_fits(mem, 3 * 1125, 1125, -5, 1, 5, 3, mem) && im2col_fits(mem, 3 * 1125, 1125, 5, -1, 5, 3, mem));
        REQUIRE(im2col_fits(nullptr, 3 * 1125, 1125, 5, 1, 5, 3, mem) && im2col_fits(mem, 3 * 1125, 1125, 5, 1, 5, 3, nullptr));
        REQUIRE(im2col_fits(mem, 3 * 1125, 1125, 5, 1, 0, 3, mem) && im2col_fits(mem, 3 * 1125, 1125, 5, 1, 5, 0, mem));
        REQUIRE(im2col_fits(mem, INT64_MAX, kStrideLimit - 1, kStrideLimit - 1, kStrideLimit - 1, 1, 1000000, mem) == nullptr);                 // int64 products
        REQUIRE(std::strcmp(im2col_fits(mem, INT64_MAX, 0, 0, 0, 2048, 1024, mem), "npos") == 0);                                              // 2025 * 2^21 floats of columns
        REQUIRE(col2im_fits(mem, 5, 3, mem, mem) == nullptr && col2im_fits(mem, 0, 3, mem, mem) && col2im_fits(mem, 5, 0, mem, mem));
        REQUIRE(col2im_fits(nullptr, 5, 3, mem, mem) && col2im_fits(mem, 5, 3, nullptr, mem) && col2im_fits(mem, 5, 3, mem, nullptr));
        REQUIRE(col2im_fits(mem, 5, 3, reinterpret_cast<char*>(mem) + 2, mem) && col2im_fits(mem, 1 << 20, 3, mem, mem));
    }

    // ---- Adam's step size ----
    REQUIRE(std::fabs(adam_lr_t(0.1, 1) - 0.1 * std::sqrt(0.001) / 0.1) < 1e-15);
    std::printf("train_host_check: ok (%zu table entries, %d parameters)\n", table.size(), kParams);
    return 0;
}
