// ensemble_merge.h -- the arithmetic of K13's merge of root tables (ensemble_kernel.hip), one text for the device kernels and for
// gmk_ensemble_merge_host.  A replica's (visits n, value q) at a cell enters the ensemble's sums as the integer pair
//     n   and   llrint(double(n) * double(q) * 2^24),
// so every sum is an integer sum -- the same bits in any order, with atomics or with a tree -- and the merged value is
//     float(double(S) / 2^24 / double(N)).
// double(n) * double(q) is exact (24 x 24 bits), the scaling is exact, llrint rounds to nearest even once; the division's operands are a
// rounded int64 and an exact count.  Nothing here may be contracted into an fma (the library is built with -ffp-contract=off).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GMK_ENS_HD __host__ __device__
#else
#define GMK_ENS_HD
#endif

namespace gmk {
namespace ensemble {

constexpr int kMaxGroup = 4096;                      // replicas per ensemble
constexpr uint32_t kCountLimit = 1u << 24;           // a replica's counts stay below this: |S| < 4096 * 2^24 * 2^24 = 2^60
constexpr double kScale = 16777216.0;                // 2^24
enum : int32_t { kStatusMismatch = 1, kStatusRange = 2, kStatusSaturated = 4 };

GMK_ENS_HD inline int64_t term(uint32_t n, float q) {
    const double product = static_cast<double>(n) * static_cast<double>(q);
    const double scaled = product * kScale;
    return static_cast<int64_t>(llrint(scaled));
}

GMK_ENS_HD inline float mean(int64_t s, uint64_t n) {
    if (n == 0) return 0.0f;
    const double unscaled = static_cast<double>(s) / kScale;
    return static_cast<float>(unscaled / static_cast<double>(n));
}

// the uint32 a sum of up to 4096 counts below 2^24 is reported as
GMK_ENS_HD inline uint32_t saturate(uint64_t n) { return n > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(n); }

}  // namespace ensemble
}  // namespace gmk
