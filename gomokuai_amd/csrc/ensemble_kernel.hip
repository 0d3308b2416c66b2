// ensemble_kernel.hip -- K13: root-parallel tree ensembles.  The n_games of a K3 or K6 / K8 handle are read as n_games / group ensembles of
// `group` consecutive games, the replicas of ONE position searched with their own arenas and random streams; this file merges the replicas'
// root tables into one table per ensemble, on the device, without touching a search kernel.
//
// The merge (ensemble_merge.h) is a sum of integers -- visit counts, and visits * value in 2^-24 fixed point -- so its result is the same
// bits whatever the launch geometry or the order in which the replicas arrive:
//   1. the handle's accumulator (uint64 visits and int64 value sums per cell, the root's pair, a status word per ensemble) is cleared;
//   2. gather: one wavefront per REPLICA reads its root and the root's children (lane l takes children l, l + 64, ...) and adds them into
//      its ensemble's accumulator with 64-bit integer atomics; it also compares its position with replica 0's of its ensemble;
//   3. finish: one wavefront per ENSEMBLE takes the first maximum of the summed visits in cell order (MCTS::stepForward's rule,
//      core/lib/src/MCTS.cpp:129-134), divides, and writes the outputs; the cell goes to every replica's slot of d_cells_per_game.
// No step walks the replicas one after another: 4 096 dependent HBM reads would rival the search they follow.
#include <cstring>
#include <vector>

#include "capi_common.h"
#include "ensemble_merge.h"
#include "mcts_tree.h"
#include "trad_tree.h"

namespace {

using namespace gmk::ensemble;
using gmk::mcts::GameHeader;
using gmk::tree::TradArena;
using gmk::tree::TradHeader;
using gmk::tree::kStatusIdleSlot;

constexpr int kCells = 225;

struct Accumulator {                                 // one per ensemble
    unsigned long long visits[kCells];
    unsigned long long sums[kCells];                 // int64, two's complement
    unsigned long long root_visits, root_sum;
    uint32_t status, pad;
};

struct Outputs {
    uint32_t* visits;
    float* values;
    int16_t* cells;
    int16_t* cells_per_game;
    uint32_t* root_visits;
    float* root_value;
    int32_t* status;
};

// what one lane holds of a root: its children l, l + 64, l + 128, l + 192 (cell, visits, value bits); cell 255 = none
struct LaneChildren {
    uint32_t cell[4], n[4], q[4];
};

// One wavefront adds a replica's root (N, V) and children into its ensemble's sums.  A replica with a count of 2^24 or more adds nothing and
// flags the ensemble (the sums then stay inside int64 whatever the other replicas hold).
__device__ __forceinline__ void add_replica(Accumulator& acc, const LaneChildren& ch, uint32_t root_n, uint32_t root_q, int lane) {
    bool bad = root_n >= kCountLimit;
#pragma unroll
    for (int k = 0; k < 4; ++k) bad |= ch.cell[k] < static_cast<uint32_t>(kCells) && ch.n[k] >= kCountLimit;
    if (__any(bad)) {
        if (lane == 0) atomicOr(&acc.status, static_cast<uint32_t>(kStatusRange));
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (ch.cell[k] >= static_cast<uint32_t>(kCells) || ch.n[k] == 0u) continue;        // (a term of an unvisited child is zero)
        atomicAdd(&acc.visits[ch.cell[k]], static_cast<unsigned long long>(ch.n[k]));
        atomicAdd(&acc.sums[ch.cell[k]], static_cast<unsigned long long>(term(ch.n[k], __uint_as_float(ch.q[k]))));
    }
    if (lane == 0 && root_n != 0u) {
        atomicAdd(&acc.root_visits, static_cast<unsigned long long>(root_n));
        atomicAdd(&acc.root_sum, static_cast<unsigned long long>(term(root_n, __uint_as_float(root_q))));
    }
}

// K3: the position is the header's sixteen row words (the player to move follows from the stones), the root's children are the empty
// cells in ascending order.  A finished game (status bit 0) adds nothing.
__global__ __launch_bounds__(64)
void ensemble_gather_mcts_kernel(const GameHeader* __restrict__ headers, const uint2* __restrict__ stats, const uint32_t* __restrict__ link,
                                 size_t cap, size_t arena_stride, int n_games, int group, Accumulator* __restrict__ acc) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n_games) return;
    const int e = g / group;
    const GameHeader& hdr = headers[g];
    const GameHeader& first_hdr = headers[e * group];
    const bool same = lane >= 16 || hdr.rows[lane] == first_hdr.rows[lane];
    if (!__all(same)) {
        if (lane == 0) atomicOr(&acc[e].status, static_cast<uint32_t>(kStatusMismatch));
        return;
    }
    if (hdr.status & 1u) return;
    const size_t base = static_cast<size_t>(g) * cap + (hdr.arena ? arena_stride : 0);
    const uint32_t root = hdr.root;
    if (root >= cap) return;
    const uint32_t first = link[base + root] >> 8;
    uint32_t n_child = first ? 225u - min(hdr.stones, 225u) : 0u;
    if (static_cast<size_t>(first) + n_child > cap) n_child = 0u;
    LaneChildren ch;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = lane + 64 * k;
        ch.cell[k] = 255u; ch.n[k] = 0u; ch.q[k] = 0u;
        if (i < n_child) {
            const uint2 st = stats[base + first + i];
            ch.cell[k] = link[base + first + i] & 0xFFu; ch.n[k] = st.x; ch.q[k] = st.y;
        }
    }
    const uint2 rs = stats[base + root];
    add_replica(acc[e], ch, rs.x, rs.y, lane);
}

// the stones of a move list (black first, alternating) as sixteen row words black | white << 16, by one wavefront
__device__ __forceinline__ void rows_of(const uint8_t* mv, int len, uint32_t* rows, int lane) {
    for (int i = lane; i < min(len, kCells); i += 64) {
        const uint32_t cell = mv[i];
        if (cell < static_cast<uint32_t>(kCells)) atomicOr(&rows[cell / 15u], 1u << (cell % 15u + 16u * (i & 1)));
    }
}

// K6 / K8: the position is the game's move list (the same stones in another order are the same position; equal stones mean an equal
// number of moves, so the same player to move), the root is node 0 and names its children.  An idle slot (status bit 4) adds nothing,
// nor does a game that was positioned and never searched (fresh == 1: its arena still holds the tree of an earlier position).
__global__ __launch_bounds__(64)
void ensemble_gather_trad_kernel(TradArena a, const TradHeader* __restrict__ hdrs, const uint8_t* __restrict__ moves, const int32_t* __restrict__ lens,
                                 int cap, int n_games, int group, Accumulator* __restrict__ acc) {
    __shared__ uint32_t s_rows[2][16];
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= n_games) return;
    const int e = g / group, g0 = e * group;
    if (lane < 32) s_rows[lane >> 4][lane & 15] = 0u;
    __syncthreads();
    rows_of(moves + static_cast<size_t>(g) * kCells, lens[g], s_rows[0], lane);
    rows_of(moves + static_cast<size_t>(g0) * kCells, lens[g0], s_rows[1], lane);
    __syncthreads();
    const bool same = lane >= 16 || s_rows[0][lane] == s_rows[1][lane];
    if (!__all(same)) {
        if (lane == 0) atomicOr(&acc[e].status, static_cast<uint32_t>(kStatusMismatch));
        return;
    }
    const TradHeader& hdr = hdrs[g];
    if ((hdr.status & kStatusIdleSlot) || hdr.fresh == 1u) return;
    const size_t base = static_cast<size_t>(g) * cap;
    const uint32_t lk = a.link[base], first = lk & 0xFFFFFFu;
    uint32_t n_child = min(lk >> 24, 225u);
    if (first + n_child > static_cast<uint32_t>(cap)) n_child = 0u;
    LaneChildren ch;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = lane + 64 * k;
        ch.cell[k] = 255u; ch.n[k] = 0u; ch.q[k] = 0u;
        if (i < n_child) {
            const uint2 st = a.stat[base + first + i];
            ch.cell[k] = a.info[base + first + i].x >> 24; ch.n[k] = st.x; ch.q[k] = st.y;
        }
    }
    const uint2 rs = a.stat[base];
    add_replica(acc[e], ch, rs.x, rs.y, lane);
}

// One wavefront per ensemble: the first maximum of the summed visits in ascending cell order, the values, the outputs.
__global__ __launch_bounds__(64)
void ensemble_finish_kernel(const Accumulator* __restrict__ acc, int n_ensembles, int group, Outputs out) {
    const int e = blockIdx.x, lane = threadIdx.x;
    if (e >= n_ensembles) return;
    const Accumulator& a = acc[e];
    int32_t status = static_cast<int32_t>(a.status);
    const bool refused = (status & kStatusMismatch) != 0;
    unsigned long long key = 0ull;                   // visits << 8 | 255 - cell: the largest key is the first maximum
    bool saturated = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c >= kCells) continue;
        const unsigned long long n = refused ? 0ull : a.visits[c];
        const long long s = refused ? 0ll : static_cast<long long>(a.sums[c]);
        saturated |= n > 0xFFFFFFFFull;
        if (out.visits) out.visits[static_cast<size_t>(e) * kCells + c] = saturate(n);
        if (out.values) out.values[static_cast<size_t>(e) * kCells + c] = mean(s, n);
        if (n) key = max(key, (n << 8) | static_cast<unsigned long long>(255 - c));
    }
    for (int s = 32; s > 0; s >>= 1) key = max(key, static_cast<unsigned long long>(__shfl_xor(key, s)));
    const unsigned long long root_n = refused ? 0ull : a.root_visits;
    saturated |= root_n > 0xFFFFFFFFull;
    if (__any(saturated)) status |= kStatusSaturated;
    const int16_t cell = key ? static_cast<int16_t>(255 - static_cast<int>(key & 0xFFull)) : static_cast<int16_t>(-1);
    if (lane == 0) {
        if (out.cells) out.cells[e] = cell;
        if (out.root_visits) out.root_visits[e] = saturate(root_n);
        if (out.root_value) out.root_value[e] = mean(refused ? 0ll : static_cast<long long>(a.root_sum), root_n);
        if (out.status) out.status[e] = status;
    }
    if (out.cells_per_game)
        for (int r = lane; r < group; r += 64) out.cells_per_game[static_cast<size_t>(e) * group + r] = cell;
}

bool group_ok(int group, int n_games) { return group >= 1 && group <= kMaxGroup && n_games % group == 0; }

// the handle's accumulator, large enough for n_ensembles, cleared on `stream`
int clear_accumulator(void** d_ensemble, int* capacity, int n_ensembles, hipStream_t stream, const char* name) {
    if (*capacity < n_ensembles) {
        (void)gmk::device_free(*d_ensemble);
        *d_ensemble = nullptr; *capacity = 0;
        Accumulator* p = nullptr;
        if (gmk::device_malloc(&p, static_cast<size_t>(n_ensembles) * sizeof(Accumulator)) != hipSuccess) {
            (void)hipGetLastError();
            gmk::set_error("%s: hipMalloc of %d accumulators failed", name, n_ensembles);
            return GMK_ERR_HIP;
        }
        *d_ensemble = p; *capacity = n_ensembles;
    }
    GMK_HIP_CHECK(hipMemsetAsync(*d_ensemble, 0, static_cast<size_t>(n_ensembles) * sizeof(Accumulator), stream));
    return GMK_OK;
}

int finish(void* d_ensemble, int n_ensembles, int group, const Outputs& out, hipStream_t stream) {
    hipLaunchKernelGGL(ensemble_finish_kernel, dim3(n_ensembles), dim3(64), 0, stream, static_cast<const Accumulator*>(d_ensemble), n_ensembles, group, out);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

}  // namespace

extern "C" int gmk_mcts_ensemble_merge(gmk_mcts* m, int group, uint32_t* d_visits, float* d_values, int16_t* d_cells, int16_t* d_cells_per_game,
                                       uint32_t* d_root_visits, float* d_root_value, int32_t* d_status, void* stream) {
    if (!m || !group_ok(group, m->n_games)) { gmk::set_error("gmk_mcts_ensemble_merge: bad arguments (1 <= group <= 4096, and group divides the handle's games)"); return GMK_ERR_ARG; }
    if (!m->rooted) { gmk::set_error("gmk_mcts_ensemble_merge: gmk_mcts_set_roots has not been called"); return GMK_ERR_STATE; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_ensembles = m->n_games / group;
    if (const int rc = clear_accumulator(&m->d_ensemble, &m->ensemble_capacity, n_ensembles, s, "gmk_mcts_ensemble_merge"); rc != GMK_OK) return rc;
    hipLaunchKernelGGL(ensemble_gather_mcts_kernel, dim3(m->n_games), dim3(64), 0, s, m->d_headers, m->d_stats, m->d_link, static_cast<size_t>(m->node_capacity),
                       m->arena_stride(), m->n_games, group, static_cast<Accumulator*>(m->d_ensemble));
    GMK_HIP_CHECK(hipGetLastError());
    return finish(m->d_ensemble, n_ensembles, group, Outputs{d_visits, d_values, d_cells, d_cells_per_game, d_root_visits, d_root_value, d_status}, s);
}

extern "C" int gmk_trad_ensemble_merge(gmk_trad* t, int group, uint32_t* d_visits, float* d_values, int16_t* d_cells, int16_t* d_cells_per_game,
                                       uint32_t* d_root_visits, float* d_root_value, int32_t* d_status, void* stream) {
    if (!t || !group_ok(group, t->n_games)) { gmk::set_error("gmk_trad_ensemble_merge: bad arguments (1 <= group <= 4096, and group divides the handle's games)"); return GMK_ERR_ARG; }
    if (!t->positioned) { gmk::set_error("gmk_trad_ensemble_merge: gmk_trad_set_positions has not been called"); return GMK_ERR_STATE; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_ensembles = t->n_games / group;
    if (const int rc = clear_accumulator(&t->d_ensemble, &t->ensemble_capacity, n_ensembles, s, "gmk_trad_ensemble_merge"); rc != GMK_OK) return rc;
    hipLaunchKernelGGL(ensemble_gather_trad_kernel, dim3(t->n_games), dim3(64), 0, s, t->a, t->d_hdr, t->d_moves, t->d_lens, t->cap, t->n_games, group,
                       static_cast<Accumulator*>(t->d_ensemble));
    GMK_HIP_CHECK(hipGetLastError());
    return finish(t->d_ensemble, n_ensembles, group, Outputs{d_visits, d_values, d_cells, d_cells_per_game, d_root_visits, d_root_value, d_status}, s);
}

// The same merge on host arrays (the arithmetic of ensemble_merge.h, the rules of the kernels above); needs no device and no gmk_init.
extern "C" int gmk_ensemble_merge_host(int n_ensembles, int group, const uint32_t* h_visits, const float* h_values, const uint32_t* h_root_visits,
                                       const float* h_root_values, uint32_t* out_visits, float* out_values, int16_t* out_cells,
                                       uint32_t* out_root_visits, float* out_root_value, int32_t* out_status) {
    if (n_ensembles < 0 || group < 1 || group > kMaxGroup || !h_visits || !h_values) {
        gmk::set_error("gmk_ensemble_merge_host: bad arguments (1 <= group <= 4096)");
        return GMK_ERR_ARG;
    }
    std::vector<uint64_t> visits(kCells);
    std::vector<int64_t> sums(kCells);
    for (int e = 0; e < n_ensembles; ++e) {
        std::fill(visits.begin(), visits.end(), 0); std::fill(sums.begin(), sums.end(), 0);
        uint64_t root_n = 0; int64_t root_s = 0; int32_t status = 0;
        for (int r = 0; r < group; ++r) {
            const size_t g = static_cast<size_t>(e) * group + r;
            const uint32_t* n = h_visits + g * kCells;
            const float* q = h_values + g * kCells;
            const uint32_t rn = h_root_visits ? h_root_visits[g] : 0u;
            bool bad = rn >= kCountLimit;
            for (int c = 0; c < kCells; ++c) bad |= n[c] >= kCountLimit;
            if (bad) { status |= kStatusRange; continue; }
            for (int c = 0; c < kCells; ++c) { visits[c] += n[c]; sums[c] += term(n[c], q[c]); }
            root_n += rn; root_s += term(rn, h_root_values ? h_root_values[g] : 0.0f);
        }
        int cell = -1; uint64_t most = 0;
        for (int c = 0; c < kCells; ++c) {
            if (visits[c] > most) { most = visits[c]; cell = c; }
            if (visits[c] > 0xFFFFFFFFull) status |= kStatusSaturated;
            if (out_visits) out_visits[static_cast<size_t>(e) * kCells + c] = saturate(visits[c]);
            if (out_values) out_values[static_cast<size_t>(e) * kCells + c] = mean(sums[c], visits[c]);
        }
        if (root_n > 0xFFFFFFFFull) status |= kStatusSaturated;
        if (out_cells) out_cells[e] = static_cast<int16_t>(cell);
        if (out_root_visits) out_root_visits[e] = saturate(root_n);
        if (out_root_value) out_root_value[e] = mean(root_s, root_n);
        if (out_status) out_status[e] = status;
    }
    return GMK_OK;
}
