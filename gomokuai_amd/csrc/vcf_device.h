// vcf_device.h -- what K14 (vcf_kernel.hip) and K15 (vcf_defend_kernel.hip) share: the board of one position as one ROW per lane, sixteen lanes
// per position, and the geometry of fours on it.  Vertical and diagonal neighbours are the rows y-4 .. y+4 of a plane, fetched with DPP row
// shifts, which stay inside a 16-lane row and deliver zero from outside it -- exactly a board edge.  Device code only; no state.
#pragma once
#include "capi_common.h"

namespace gmk::vcf {

constexpr int kCells = 225;
constexpr uint32_t kRowMask = 0x7FFFu;
constexpr int kLevels = GMK_VCF_MAX_DEPTH;                  // pushes stop at depth 29 (a push needs depth + 3 <= limit <= 32)

enum : int { kIdle = 0, kInit = 1, kRun = 2 };

// rows[4 + k] = the plane's row y + k for k = -4 .. 4, zero where that row is off the board (DPP row shifts never leave the 16-lane group).
template <int K>
__device__ __forceinline__ uint32_t row_from_below(uint32_t v) {      // lane i <- lane i + K
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x100 + K, 0xF, 0xF, true));
}
template <int K>
__device__ __forceinline__ uint32_t row_from_above(uint32_t v) {      // lane i <- lane i - K
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x110 + K, 0xF, 0xF, true));
}
__device__ __forceinline__ void gather_rows(uint32_t v, uint32_t (&rows)[9]) {
    rows[4] = v;
    rows[5] = row_from_below<1>(v); rows[6] = row_from_below<2>(v); rows[7] = row_from_below<3>(v); rows[8] = row_from_below<4>(v);
    rows[3] = row_from_above<1>(v); rows[2] = row_from_above<2>(v); rows[1] = row_from_above<3>(v); rows[0] = row_from_above<4>(v);
}

__device__ __forceinline__ uint32_t shifted(uint32_t v, int k) { return k >= 0 ? v >> k : v << -k; }

// The plane's value k steps along direction D from every cell of this row: 0 horizontal, 1 vertical, 2 and 3 the diagonals.
template <int D>
__device__ __forceinline__ uint32_t along(const uint32_t (&rows)[9], int k) {
    if (D == 0) return shifted(rows[4], k);
    if (D == 1) return rows[4 + k];
    if (D == 2) return shifted(rows[4 + k], k);
    return shifted(rows[4 - k], k);
}

// Cells at which one more stone of the plane makes a run of five or more: the stones adjacent on both sides add up to four.
template <int D>
__device__ __forceinline__ uint32_t completing_dir(const uint32_t (&s)[9]) {
    const uint32_t l1 = along<D>(s, -1), l2 = l1 & along<D>(s, -2), l3 = l2 & along<D>(s, -3), l4 = l3 & along<D>(s, -4);
    const uint32_t r1 = along<D>(s, 1), r2 = r1 & along<D>(s, 2), r3 = r2 & along<D>(s, 3), r4 = r3 & along<D>(s, 4);
    return l4 | (l3 & r1) | (l2 & r2) | (l1 & r3) | r4;
}
__device__ __forceinline__ uint32_t completing(const uint32_t (&s)[9], uint32_t empty) {
    return empty & (completing_dir<0>(s) | completing_dir<1>(s) | completing_dir<2>(s) | completing_dir<3>(s));
}

// Runs of five or more that already stand.
template <int D>
__device__ __forceinline__ uint32_t five_dir(const uint32_t (&s)[9]) {
    return s[4] & along<D>(s, 1) & along<D>(s, 2) & along<D>(s, 3) & along<D>(s, 4);
}
__device__ __forceinline__ uint32_t five(const uint32_t (&s)[9]) { return five_dir<0>(s) | five_dir<1>(s) | five_dir<2>(s) | five_dir<3>(s); }

// Four-making cells: a five-window through the cell whose other four cells are free (attacker or empty, on the board) and hold at least three
// attacker stones.  a = attacker rows, f = free rows.
__device__ __forceinline__ uint32_t three_of(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (a & b & (c | d)) | (c & d & (a | b)); }
template <int D>
__device__ __forceinline__ uint32_t four_making_dir(const uint32_t (&a)[9], const uint32_t (&f)[9]) {
    uint32_t A[9], F[9];
#pragma unroll
    for (int k = -4; k <= 4; ++k) {
        if (k == 0) continue;
        A[4 + k] = along<D>(a, k);
        F[4 + k] = along<D>(f, k);
    }
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {                                    // the cell is the window's j-th
        const int o0 = -j + (0 >= j ? 1 : 0), o1 = -j + 1 + (1 >= j ? 1 : 0), o2 = -j + 2 + (2 >= j ? 1 : 0), o3 = -j + 3 + (3 >= j ? 1 : 0);
        any |= F[4 + o0] & F[4 + o1] & F[4 + o2] & F[4 + o3] & three_of(A[4 + o0], A[4 + o1], A[4 + o2], A[4 + o3]);
    }
    return any;
}
__device__ __forceinline__ uint32_t four_making(const uint32_t (&a)[9], const uint32_t (&f)[9], uint32_t empty) {
    return empty & (four_making_dir<0>(a, f) | four_making_dir<1>(a, f) | four_making_dir<2>(a, f) | four_making_dir<3>(a, f));
}

// One bit per row of this lane's group.
__device__ __forceinline__ uint32_t group_rows(bool p, int gbase) { return static_cast<uint32_t>(__ballot(p) >> gbase) & 0xFFFFu; }

// The lowest cell of a plane, or -1; the cell is taken out of `v`.
__device__ __forceinline__ int take_lowest(uint32_t& v, int y, int gbase) {
    const uint32_t rows = group_rows(v != 0, gbase);
    const int row = rows ? __builtin_ctz(rows) : 0;
    const uint32_t bits = static_cast<uint32_t>(__shfl(static_cast<int>(v), gbase + row));
    const int x = bits ? __builtin_ctz(bits) : 0;
    if (y == row) v &= ~(1u << x);
    return rows ? row * 15 + x : -1;
}

}  // namespace gmk::vcf
