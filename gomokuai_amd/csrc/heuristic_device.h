// heuristic_device.h -- device functions of the hand-written pattern heuristic (core/lib/include/algorithms/Heuristic.hpp:16-45, 94-161):
// the per-cell float vectors of one wavefront, their one summation order, Heuristic::DensityWeight and Heuristic::DecisiveFilter over an
// evaluator state in LDS (evalstate_device.h).  Shared by K6 (trad_kernel.hip: hybridSimulate inside the playout loop) and K10
// (pattern_kernel.hip: the heuristic on its own), which therefore compile the same text.
#pragma once
#include "evalstate_device.h"
#include "noise_device.h"

namespace gmk::evs {

using gmk::noise::tree_sum;                      // the one summation order of the float reductions (noise_device.h; oracle/go_trad.c: sum225)

struct Cells {                                   // a per-cell float vector: lane l holds cells l + 64 j
    float v[4];
};

__device__ __forceinline__ float sum225(const Cells& x, int lane) {
    float p = x.v[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) if (lane + 64 * j < kCells) p += x.v[j];
    return tree_sum(p);
}

// MatrixBase::normalized() / normalize() (Eigen 3.3+: a zero vector stays as it is)
__device__ __forceinline__ void normalize225(Cells& x, int lane) {
    Cells sq;
#pragma unroll
    for (int j = 0; j < 4; ++j) sq.v[j] = x.v[j] * x.v[j];
    const float z = sum225(sq, lane);
    if (z > 0.0f) {
        const float n = sqrtf(z);
#pragma unroll
        for (int j = 0; j < 4; ++j) x.v[j] = x.v[j] / n;
    }
}

// Heuristic::DensityWeight (Heuristic.hpp:39-45)
__device__ __forceinline__ Cells density_weight(const uint32_t* st, int black, int lane) {
    const uint32_t* packed = st + oDensity + black * kCells;      // count | weight << 16
    Cells out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = min(lane + 64 * j, kCells - 1);
        const uint32_t w = packed[q];
        const float N = static_cast<float>(max(density_count(w), 0)), W = static_cast<float>(max(density_weight_of(w), 0));
        out.v[j] = (3.0f * W) / (1.0f + 2.0f * N);
    }
    normalize225(out, lane);
    return out;
}

// Heuristic::DecisiveFilter (Heuristic.hpp:94-161).  Candidates are (pattern, player is black): pattern < 9 a
// Pattern::Type, otherwise 9 + Compound::Type.  All lanes walk the same automaton; the mask is per cell.
__device__ __forceinline__ void decisive_filter(const uint32_t* st, int cur_black, Cells& probs, int lane) {
    enum { S4, SL3, STo44, STo43, STo33, SEnd };
    // AutomataTable[anti][state] (Heuristic.hpp:103-107) as immediates: next state in nibble anti * 6 + state, next "anti" in
    // bit anti * 6 + state (a table in memory would cost a dependent scalar load per step)
    //   anti 0: {_4,1} {To44,0} {L3,1} {To43,1} {To33,1} {End,0}     anti 1: {L3,0} {To44,1} {To43,0} {To33,0} {End,0} {End,1}
    constexpr unsigned long long kNextNibbles = 0x554321543120ull;
    constexpr uint32_t kAntiBits = 0x89Du;
    int state = S4, anti = 0;
    // the totals the automaton looks at: pattern types 4..7 and the three compound types (one round of LDS reads)
    uint32_t totals[12];
#pragma unroll
    for (int i = 0; i < 8; ++i) totals[i] = i >= 4 ? st[oPdist + pdist_index(225, i)] : 0u;
#pragma unroll
    for (int i = 0; i < 3; ++i) totals[9 + i] = st[oCdist + 225 * 3 + i];
    totals[8] = 0u;
    while (state != SEnd) {
        const uint32_t black = anti ? cur_black ^ 1 : cur_black;
        // the std::deque as 16-bit entries of one register: pattern | black << 8, entry k at bits 16 k
        uint64_t cands;
        int n, head = 0;
        if (state == S4) { cands = (7u | black << 8) | (static_cast<uint64_t>(6u | black << 8) << 16); n = 2; }           // LiveFour, DeadFour
        else if (state == SL3) { cands = 5u | black << 8; n = 1; }                                                       // LiveThree
        else { cands = static_cast<uint32_t>(9 + (STo33 - state)) | black << 8; n = 1; }
        for (; head < n; ++head) {
            const uint32_t pattern = (cands >> (16 * head)) & 0xFFu, pb = (cands >> (16 * head + 8)) & 1u;
            uint32_t total = 0;                                  // totals[pattern], without a dynamically indexed array
#pragma unroll
            for (int i = 4; i < 12; ++i) total = pattern == static_cast<uint32_t>(i) ? totals[i] : total;
            if ((total >> (16 * pb)) & 0xFFFFu) {
                if (anti && state != S4) { cands |= static_cast<uint64_t>(4u | (pb ^ 1u) << 8) << (16 * n); ++n; }       // the own DeadThree counts when answering
                break;
            }
        }
        if (head < n) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = min(lane + 64 * j, kCells - 1);
                bool keep = false;
                for (int k = head; k < n; ++k) {
                    const uint32_t pattern = (cands >> (16 * k)) & 0xFFu, pb = (cands >> (16 * k + 8)) & 1u;
                    const uint32_t field = pattern < 9 ? st[oPdist + pdist_index(q, static_cast<int>(pattern))] : st[oCdist + q * 3 + pattern - 9];
                    keep |= ((field >> (8 * group2(pb, cur_black))) & 0xFFu) != 0u;
                }
                if (!keep) probs.v[j] = 0.0f;
            }
            normalize225(probs, lane);
            state = SEnd;
        } else {
            const int at = anti * 6 + state;
            state = static_cast<int>((kNextNibbles >> (4 * at)) & 15u);
            anti = static_cast<int>((kAntiBits >> at) & 1u);
        }
    }
}

}  // namespace gmk::evs
