// records_access.h -- where a game's moves, visit rows and winner live, and the numbering of the eight board symmetries.
// Shared by K4 + K5 (records_kernel.hip) and the replay buffer (replay_kernel.hip): a body is written once over an accessor; the two
// instantiations are the fixed-stride arrays gmk_mcts_advance writes and the wire form of selfplay.pack_records (records_wire.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace gmk {

// index permutation of network/data_helper.py:36-55: out[j] = in[perm(j)] for np.rot90(a, k) then optional np.fliplr
// (constexpr, and callable on the host, for the tables pvnet_sym_kernel.hip builds at compile time; include/gomoku_symmetry.h is the C statement)
constexpr __host__ __device__ __forceinline__ int augment_source(int j, int k, bool flip) {
    int r = j / 15, c = j % 15;
    if (flip) c = 14 - c;                     // fliplr(b)[r][c] = b[r][14 - c]
    for (int i = 0; i < k; ++i) {             // rot90(a)[r][c] = a[c][14 - r]
        const int nr = c, nc = 14 - r;
        r = nr; c = nc;
    }
    return r * 15 + c;
}

// inverse of augment_source for symmetry a = 2k + flip: the output cell that shows source cell c
constexpr __host__ __device__ __forceinline__ int augment_target(int c, int a) {
    int r = c / 15, x = c % 15;
    for (int i = 0; i < (a >> 1); ++i) {       // rot90 undone: (r, x) <- (14 - x, r)
        const int nr = 14 - x, nx = r;
        r = nr; x = nx;
    }
    if (a & 1) x = 14 - x;
    return r * 15 + x;
}

struct StrideRecords {
    const uint8_t* moves;
    const uint16_t* visits;
    const int8_t* winner;
    struct Row {
        const uint16_t* p;
        __device__ __forceinline__ uint16_t operator[](int c) const { return p[c]; }
    };
    __device__ __forceinline__ const uint8_t* moves_of(int g) const { return moves + static_cast<size_t>(g) * 225; }
    __device__ __forceinline__ Row visit_row(int g, int t) const { return Row{visits + (static_cast<size_t>(g) * 225 + static_cast<size_t>(t)) * 225}; }
    __device__ __forceinline__ int8_t winner_of(int g) const { return winner[g]; }
};

// The wire form: lens int32[n] | winner int8[n] | moves uint8[T] | visits uint16[T][225], T = offsets[n].  Move t of game g is byte
// 5n + offsets[g] + t; its visit row starts at byte 5n + T + 450 (offsets[g] + t), which is odd whenever 5n + T is: a count is read as
// its two bytes, never as an unaligned 16-bit load.
struct PackedRecords {
    const uint8_t* buf;
    const int64_t* offsets;
    int n;
    struct Row {
        const uint8_t* p;
        __device__ __forceinline__ uint16_t operator[](int c) const {
            return static_cast<uint16_t>(p[2 * c] | (p[2 * c + 1] << 8));
        }
    };
    __device__ __forceinline__ const uint8_t* moves_of(int g) const { return buf + 5 * static_cast<size_t>(n) + offsets[g]; }
    __device__ __forceinline__ Row visit_row(int g, int t) const {
        return Row{buf + 5 * static_cast<size_t>(n) + static_cast<size_t>(offsets[n]) + 450 * static_cast<size_t>(offsets[g] + t)};
    }
    __device__ __forceinline__ int8_t winner_of(int g) const { return static_cast<int8_t>(buf[4 * static_cast<size_t>(n) + g]); }
};

}  // namespace gmk
