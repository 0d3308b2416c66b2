// pattern_kernel.hip -- K10: the hand-written pattern heuristic on its own, per position and for whole greedy games.
//
// Heuristic::EvaluationProbs, DecisiveFilter and EvaluationValue (core/lib/include/algorithms/Heuristic.hpp:16-45, 94-161) as their three users
// call them: TraditionalPolicy::hybridSimulate and PatternEvalAgent::getAction (filter = 1), and Heuristic::MaxEvaluatedRollout (:61-83, filter = 0),
// which plays a game out by taking the largest probability at every ply.  The heuristic reads the evaluator's per-cell flag words, which depend
// on the order the moves were played in: a position is a move LIST, replayed on a fresh evaluator with K2's update
// (evalstate_device.h), and the heuristic's device functions are K6's (heuristic_device.h), so the numbers are K6's bit for bit.
// Mapping: one wavefront per position / game, the evaluator state (16.0 KB) in LDS, nine wavefronts per workgroup = one workgroup per CU
// (9 x 16.3 KB + 14.4 KB of tables of the 160 KB; K6 fits eight because a search also keeps its path there).  Lists are 0 .. 225 moves long
// and games end when they end, so the work is not dealt out by index: a wavefront takes the next item from a counter when it has finished
// one, as K6's persistent loop hands out games.  A whole game is ONE pass of that loop: probabilities, filter, value, first-maximum argmax,
// applyMove, again -- nothing is replayed and the host does nothing between plies.
#include <algorithm>
#include <atomic>
#include <mutex>

#include "../../include/gomoku_pattern_states.h"
#include "evalstate_device.h"
#include "heuristic_device.h"
#include "host_staging.h"

namespace {

using namespace gmk::evs;

constexpr int kWaves = 9;
constexpr int kThreads = 64 * kWaves;
constexpr int kPerWave = (kStateWords + kScratchWords + 3) & ~3;
static_assert(kWaves * kPerWave + 2224 + 1248 + gmk::kPrefixWords <= 160 * 256, "LDS of a workgroup (production tables: 2 224 + 1 248 words)");

enum : uint32_t { kOver = 1u, kEvaluatorError = 2u, kIllegal = 4u, kStalled = 8u };      // status bits (include/gomoku_hip.h)

struct PatternParams {
    uint8_t* moves;                              // [n][stride]; the policy form only reads it
    int32_t* lens;
    int stride, n, filter, max_moves;
    float* probs;                                // policy form: [n][225], [n], [n]
    float* value;
    int32_t* best;
    int8_t* winner;                              // play form: [n], [n][225]
    float* values;
    int32_t* status;
    uint32_t* counter;                           // the next item nobody has taken yet (zero at launch)
    const uint32_t* g_trans;
    const uint32_t* g_records;
    int trans_words, record_words;
};

struct Verdict {                                 // what the heuristic says at one position, for the player to move
    Cells probs;
    float value;
    int best;
};

// EvaluationProbs (+ DecisiveFilter) and EvaluationValue on the live evaluator, as K6's simulate stage states them (trad_kernel.hip), and
// probs.maxCoeff(&best): the FIRST maximum in cell order
__device__ __forceinline__ Verdict evaluate(const Ctx& c, int filter) {
    const int lane = c.lane;
    const int32_t* meta = reinterpret_cast<const int32_t*>(c.st + oMeta);
    const int cur_black = meta[1] > 0;
    Verdict out;
    Cells& probs = out.probs;
    const Cells dw_self = density_weight(c.st, cur_black, lane), dw_rival = density_weight(c.st, cur_black ^ 1, lane);
    const int32_t* scores = reinterpret_cast<const int32_t*>(c.st + oScores);
    Cells prod_self, prod_rival;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = min(lane + 64 * j, kCells - 1);
        const float self_worthy = static_cast<float>(scores[group2(cur_black, cur_black) * kCells + q]) * dw_self.v[j];
        const float rival_anti = static_cast<float>(scores[group2(cur_black ^ 1, cur_black) * kCells + q]) * dw_rival.v[j];
        probs.v[j] = 0.6f * self_worthy + 0.4f * rival_anti;                   // EvaluationProbs (Heuristic.hpp:16-28)
        prod_self.v[j] = self_worthy;
        prod_rival.v[j] = static_cast<float>(scores[group2(cur_black ^ 1, cur_black ^ 1) * kCells + q]) * dw_rival.v[j];
    }
    if (meta[0] != 0) {
        normalize225(probs, lane);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) probs.v[j] = (lane + 64 * j == 7 * 15 + 7) ? 1.0f : 0.0f;
    }
    if (filter) decisive_filter(c.st, cur_black, probs, lane);
    const float self_sum = sum225(prod_self, lane), rival_sum = sum225(prod_rival, lane);
    out.value = static_cast<float>(tanh((1.2 * self_sum - rival_sum) / 500.0f));           // EvaluationValue (:33-37)
    // the lane's own first maximum (its cells ascend with j), then a reduce on (value, lowest cell)
    float bv = probs.v[0];
    int bi = lane;
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (lane + 64 * j < kCells && probs.v[j] > bv) { bv = probs.v[j]; bi = lane + 64 * j; }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
        const float ov = __shfl_xor(bv, sft);
        const int oi = __shfl_xor(bi, sft);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    out.best = bi;
    return out;
}

// kPlay = false: gmk_pattern_policy (replay the list, one verdict); true: gmk_pattern_play (replay the opening, then verdict and applyMove of its
// best cell until the game ends).  One loop serves both, so that the evaluator's update and the heuristic exist once per kernel.
template <bool kPlay>
__global__ __launch_bounds__(kThreads)
void pattern_kernel(PatternParams prm) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    // layout: [trans][records, then the four-symbol prefix table: record_words counts both][wavefronts: kWaves * kPerWave]
    for (int i = threadIdx.x; i < prm.trans_words + prm.record_words; i += kThreads)
        lds[i] = i < prm.trans_words ? prm.g_trans[i] : prm.g_records[i - prm.trans_words];
    __syncthreads();                                            // tables staged; the wavefronts of a block never wait for each other again
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* base = lds + prm.trans_words + prm.record_words + wave * kPerWave;
    const Ctx c{base, base + kStateWords, reinterpret_cast<const char*>(lds), reinterpret_cast<const uint4*>(lds + prm.trans_words),
                reinterpret_cast<const char*>(lds + prm.trans_words + prm.record_words - gmk::kPrefixWords), lane};
    int32_t* meta = reinterpret_cast<int32_t*>(c.st + oMeta);
    const uint8_t* record = reinterpret_cast<const uint8_t*>(c.st + oRecord);

    for (;;) {
        uint32_t taken = 0;
        if (lane == 0) taken = atomicAdd(prm.counter, 1u);
        taken = __builtin_amdgcn_readfirstlane(taken);
        if (taken >= static_cast<uint32_t>(prm.n)) break;
        const size_t item = taken;
        uint8_t* row = prm.moves + item * static_cast<size_t>(prm.stride);
        const int len0 = prm.lens[item];
        uint32_t status = 0;
        Verdict now;
#pragma unroll
        for (int j = 0; j < 4; ++j) now.probs.v[j] = 0.0f;
        now.value = 0.0f;
        now.best = -1;
        float seen[4] = {0.0f, 0.0f, 0.0f, 0.0f};              // kPlay: lane l holds the values of the plies l + 64 j
        reset_state(c);
        if (len0 < 0 || len0 > kCells) {
            status = kIllegal;
        } else {
            int ply = 0, added = 0, chunk = 255;               // the list 64 moves at a time, one per lane, handed out with v_readlane (as K2 does)
            for (;;) {
                int mv;
                if (ply < len0) {
                    if ((ply & 63) == 0) chunk = ply + lane < len0 ? row[ply + lane] : 255;
                    mv = __builtin_amdgcn_readlane(chunk, ply & 63);
                    // Evaluator::applyMove would ignore these (Pattern.cpp:310-313); a list that holds one is not a position
                    if (mv >= kCells || meta[1] == 0 || ((c.st[oLines + mv / 15] >> (2 * (mv % 15))) & 3u) != 3u) { status |= kIllegal; break; }
                } else {
                    // Evaluator::checkGameEnd (Pattern.cpp:344-354)
                    bool ended = meta[1] == 0;
                    if (!ended && meta[0] == kCells) {
                        if (lane == 0) { meta[1] = 0; meta[2] = 0; }
                        wave_phase_fence();
                        ended = true;
                    }
                    if (ended) { status |= kOver; break; }
                    if (kPlay && prm.max_moves > 0 && added >= prm.max_moves) break;
                    now = evaluate(c, prm.filter);
                    if (!kPlay) break;
                    mv = now.best;
                    // MaxEvaluatedRollout would ask again for ever (Heuristic.hpp:65-68): the game stops where it stands
                    if (((c.st[oLines + mv / 15] >> (2 * (mv % 15))) & 3u) != 3u) { status |= kStalled; break; }
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (lane == (ply & 63) && j == (ply >> 6)) seen[j] = now.value;
                    ++added;
                }
                evaluator_step(c, mv);                          // the one place where moves are applied
                wave_phase_fence();
                ++ply;
            }
        }
        if (meta[3] != 0) status |= kEvaluatorError;
        if (kPlay) {
            const bool legal = !(status & kIllegal);           // an illegal opening stays as it was given
            const int len = meta[0];
            if (legal) for (int i = len0 + lane; i < len; i += 64) row[i] = record[i];
            if (prm.values) {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (lane + 64 * j < kCells) prm.values[item * kCells + lane + 64 * j] = legal ? seen[j] : 0.0f;
            }
            if (lane == 0) {
                if (legal) prm.lens[item] = len;
                if (prm.winner) prm.winner[item] = static_cast<int8_t>((legal && (status & kOver)) ? meta[2] : 0);
                if (prm.status) prm.status[item] = static_cast<int32_t>(status);
            }
        } else {
            const bool live = !(status & (kOver | kIllegal));  // otherwise the zero verdict
            if (prm.probs) {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (lane + 64 * j < kCells) prm.probs[item * kCells + lane + 64 * j] = live ? now.probs.v[j] : 0.0f;
            }
            if (lane == 0) {
                if (prm.value) prm.value[item] = live ? now.value : 0.0f;
                if (prm.best) prm.best[item] = live ? now.best : -1;
                if (prm.status) prm.status[item] = static_cast<int32_t>(status);
            }
        }
        wave_phase_fence();                                     // the record was read above: the next item's reset comes after
    }
}

// K23: the same verdict for a row of network planes, float32 [6][225] (Board.encoded_states, K7's leaf batch).  The row's canonical move list
// (include/gomoku_pattern_states.h) is never written anywhere: four ballots per plane give the stone sets as scalar masks, the header's check
// and walk run on them, and every cell the walk hands out goes to the update the list form feeds.  Its own loop around evaluate() and
// evaluator_step(), so that the two instantiations above stay the code they were.
struct StatesParams {
    const float* states;                         // [n][6][225]
    int n, filter, norm;
    float* value;                                // [n]
    float* probs;                                // [n][225]
    int32_t* status;                             // [n] or nullptr
    uint32_t* counter;
    const uint32_t* g_trans;
    const uint32_t* g_records;
    int trans_words, record_words;
};

__global__ __launch_bounds__(kThreads)
void pattern_states_kernel(StatesParams prm) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    for (int i = threadIdx.x; i < prm.trans_words + prm.record_words; i += kThreads)
        lds[i] = i < prm.trans_words ? prm.g_trans[i] : prm.g_records[i - prm.trans_words];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* base = lds + prm.trans_words + prm.record_words + wave * kPerWave;
    const Ctx c{base, base + kStateWords, reinterpret_cast<const char*>(lds), reinterpret_cast<const uint4*>(lds + prm.trans_words),
                reinterpret_cast<const char*>(lds + prm.trans_words + prm.record_words - gmk::kPrefixWords), lane};
    int32_t* meta = reinterpret_cast<int32_t*>(c.st + oMeta);

    for (;;) {
        uint32_t taken = 0;
        if (lane == 0) taken = atomicAdd(prm.counter, 1u);
        taken = __builtin_amdgcn_readfirstlane(taken);
        if (taken >= static_cast<uint32_t>(prm.n)) break;
        const size_t item = taken;
        const float* s = prm.states + item * static_cast<size_t>(GMK_PATTERN_PLANES * kCells);
        // front: lane l holds the cells l + 64 j of planes 0, 1, 3 and 4; one ballot per plane and j
        gmk_pattern_masks m;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = lane + 64 * j;
            const bool in = q < kCells;
            const float f0 = in ? s[q] : 0.0f, f1 = in ? s[kCells + q] : 0.0f, f3 = in ? s[3 * kCells + q] : 0.0f, f4 = in ? s[4 * kCells + q] : 0.0f;
            m.own[j] = __ballot(gmk_pattern_is_set(f0));
            m.opp[j] = __ballot(gmk_pattern_is_set(f1));
            m.last[j] = __ballot(gmk_pattern_is_set(f3));
            m.last2[j] = __ballot(gmk_pattern_is_set(f4));
        }
        m.black_to_move = __builtin_amdgcn_readfirstlane(static_cast<int>(gmk_pattern_is_set(s[5 * kCells])));
        uint32_t status = static_cast<uint32_t>(gmk_pattern_check(&m));
        Verdict now;
#pragma unroll
        for (int j = 0; j < 4; ++j) now.probs.v[j] = 0.0f;
        now.value = 0.0f;
        now.best = -1;
        reset_state(c);
        if (status == 0u) {
            gmk_pattern_walk w;
            gmk_pattern_walk_begin(&m, &w);
            int ply = 0;
            for (;;) {
                int mv;
                if (ply < w.plies) {
                    mv = gmk_pattern_walk_next(&w, ply);
                    // as the list form: a move after the end is not a position (the cell is empty and below 225 by construction)
                    if (meta[1] == 0 || ((c.st[oLines + mv / 15] >> (2 * (mv % 15))) & 3u) != 3u) { status |= kIllegal; break; }
                } else {
                    bool ended = meta[1] == 0;                  // Evaluator::checkGameEnd (Pattern.cpp:344-354)
                    if (!ended && meta[0] == kCells) {
                        if (lane == 0) { meta[1] = 0; meta[2] = 0; }
                        wave_phase_fence();
                        ended = true;
                    }
                    if (ended) status |= kOver; else now = evaluate(c, prm.filter);
                    break;
                }
                evaluator_step(c, mv);                          // the one place where moves are applied
                wave_phase_fence();
                ++ply;
            }
            if (meta[3] != 0) status |= kEvaluatorError;
        }
        // back: the prior, the value and the status of the row
        const bool live = !(status & (kOver | kIllegal));
        Cells out;
#pragma unroll
        for (int j = 0; j < 4; ++j) out.v[j] = live ? now.probs.v[j] : 0.0f;
        if (live && prm.norm == GMK_PATTERN_NORM_SUM) {
            double p = static_cast<double>(out.v[0]);           // gmk_gumbel_sum225, as gumbel_row adds it up (az_kernel.hip)
#pragma unroll
            for (int j = 1; j < 4; ++j) if (lane + 64 * j < kCells) p += static_cast<double>(out.v[j]);
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) {
                const double other = __shfl_down(p, off, 16);
                p = p + (((lane & 15) + off < 16) ? other : 0.0);
            }
            const double sum = (__shfl(p, 0) + __shfl(p, 16)) + (__shfl(p, 32) + __shfl(p, 48));
            if (sum == 0.0) {
                // the uniform fallback; every stone of the row is on the evaluator's board by now, so the empty cells are read there
                const int empty = kCells - meta[0];
                const float u = (status == 0u && empty > 0) ? static_cast<float>(1.0 / static_cast<double>(empty)) : 0.0f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int q = min(lane + 64 * j, kCells - 1);
                    out.v[j] = ((c.st[oLines + q / 15] >> (2 * (q % 15))) & 3u) == 3u ? u : 0.0f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) out.v[j] = static_cast<float>(static_cast<double>(out.v[j]) / sum);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) if (lane + 64 * j < kCells) prm.probs[item * kCells + lane + 64 * j] = out.v[j];
        if (lane == 0) {
            prm.value[item] = live ? now.value : 0.0f;
            if (prm.status) prm.status[item] = static_cast<int32_t>(status);
        }
        wave_phase_fence();
    }
}

// The work counters: every launch takes the next word of a small ring and clears it on its stream, so launches on different streams (and
// launches queued behind each other) never share one.  256 launches would have to be in flight at once for two of them to meet.
constexpr unsigned kCounterRing = 256;
std::mutex g_ring_mutex;
uint32_t* g_ring = nullptr;
std::atomic<unsigned> g_ring_next{0};

int next_counter(hipStream_t stream, uint32_t** out) {
    {
        std::lock_guard<std::mutex> lock(g_ring_mutex);
        if (!g_ring) GMK_HIP_CHECK(hipMalloc(&g_ring, kCounterRing * sizeof(uint32_t)));
    }
    uint32_t* slot = g_ring + g_ring_next.fetch_add(1u) % kCounterRing;
    GMK_HIP_CHECK(hipMemsetAsync(slot, 0, sizeof(uint32_t), stream));
    *out = slot;
    return GMK_OK;
}

template <bool kPlay>
int launch(PatternParams prm, hipStream_t stream) {
    const gmk::DeviceState& st = gmk::device_state();
    prm.g_trans = st.d_trans;
    prm.g_records = st.d_records;
    prm.trans_words = st.n_states * 4;
    prm.record_words = st.n_records * 4 + gmk::kPrefixWords;
    const size_t lds = static_cast<size_t>(kWaves * kPerWave + prm.trans_words + prm.record_words) * 4;
    if (lds > 160 * 1024) { gmk::set_error("K10: the pattern tables do not fit beside %d evaluator states in LDS", kWaves); return GMK_ERR_CAPACITY; }
    static bool attr_set = false;
    if (!attr_set) {
        GMK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pattern_kernel<kPlay>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    const int rc = next_counter(stream, &prm.counter);
    if (rc != GMK_OK) return rc;
    // one workgroup fills a CU's LDS: no more workgroups than CUs, and no more than the items need
    const int grid = std::max(1, std::min((prm.n + kWaves - 1) / kWaves, st.cu_count > 0 ? st.cu_count : 1));
    hipLaunchKernelGGL(pattern_kernel<kPlay>, dim3(grid), dim3(kThreads), lds, stream, prm);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

using gmk::misaligned;

}  // namespace

extern "C" int gmk_pattern_policy(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int filter,
                                  float* d_probs, float* d_value, int32_t* d_best, int32_t* d_status, void* stream) {
    GMK_NEED_INIT();
    if (n < 0 || (n > 0 && (!d_moves || !d_lens || stride <= 0 || misaligned(d_lens, 4) || misaligned(d_probs, 4) || misaligned(d_value, 4) ||
                            misaligned(d_best, 4) || misaligned(d_status, 4)))) {
        gmk::set_error("gmk_pattern_policy: bad arguments (n >= 0, stride > 0; d_lens and the outputs 4-byte aligned)");
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    PatternParams prm{};
    prm.moves = const_cast<uint8_t*>(d_moves);                   // (the policy kernel only reads it)
    prm.lens = const_cast<int32_t*>(d_lens);
    prm.stride = stride; prm.n = n; prm.filter = filter != 0; prm.max_moves = 0;
    prm.probs = d_probs; prm.value = d_value; prm.best = d_best; prm.status = d_status;
    return launch<false>(prm, static_cast<hipStream_t>(stream));
}

extern "C" int gmk_pattern_policy_host(const uint8_t* h_moves, int stride, const int32_t* h_lens, int n, int filter,
                                       float* h_probs, float* h_value, int32_t* h_best, int32_t* h_status) {
    GMK_NEED_INIT();
    if (n < 0 || (n > 0 && (!h_moves || !h_lens || stride <= 0))) { gmk::set_error("gmk_pattern_policy_host: bad arguments"); return GMK_ERR_ARG; }
    if (n == 0) return GMK_OK;
    // one device block: moves | lens | probs | value | best | status.  It is asked for at the size from which the library's pool keeps blocks
    // (16 MB) even when the batch is small, so that the next call gets it back without a trip to the driver.
    const size_t un = static_cast<size_t>(n);
    gmk::Staging st("gmk_pattern_policy_host", gmk::kPoolKeeps);
    uint8_t* d_moves;
    int32_t *d_lens, *d_best, *d_status;
    float *d_probs, *d_value;
    st.in(d_moves, h_moves, un * static_cast<size_t>(stride)); st.in(d_lens, h_lens, un);
    st.out(d_probs, h_probs, un * kCells); st.out(d_value, h_value, un); st.out(d_best, h_best, un); st.out(d_status, h_status, un);
    int rc = st.take();
    if (rc == GMK_OK) rc = gmk_pattern_policy(d_moves, stride, d_lens, n, filter, d_probs, d_value, d_best, d_status, nullptr);
    if (rc != GMK_OK) return rc;                                  // the device form's code and text, untouched
    GMK_STAGED(st, hipDeviceSynchronize());
    return st.download();
}

extern "C" int gmk_pattern_play(uint8_t* d_moves, int32_t* d_lens, int n, int filter, int max_moves,
                                int8_t* d_winner, float* d_values, int32_t* d_status, void* stream) {
    GMK_NEED_INIT();
    if (n < 0 || max_moves < 0 || (n > 0 && (!d_moves || !d_lens || misaligned(d_lens, 4) || misaligned(d_values, 4) || misaligned(d_status, 4)))) {
        gmk::set_error("gmk_pattern_play: bad arguments (n >= 0, max_moves >= 0; d_lens, d_values and d_status 4-byte aligned)");
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    PatternParams prm{};
    prm.moves = d_moves; prm.lens = d_lens;
    prm.stride = kCells; prm.n = n; prm.filter = filter != 0; prm.max_moves = max_moves;
    prm.winner = d_winner; prm.values = d_values; prm.status = d_status;
    return launch<true>(prm, static_cast<hipStream_t>(stream));
}

extern "C" int gmk_pattern_evaluate_states(const float* d_states, int n, int filter, int norm,
                                           float* d_value, float* d_probs, int32_t* d_status, void* stream) {
    if (n < 0 || (n > 0 && (!d_states || !d_value || !d_probs)) || (filter != 0 && filter != 1) ||
        (norm != GMK_PATTERN_NORM_L2 && norm != GMK_PATTERN_NORM_SUM) || misaligned(d_states, 4) || misaligned(d_value, 4) || misaligned(d_probs, 4) ||
        misaligned(d_status, 4)) {
        gmk::set_error("gmk_pattern_evaluate_states: bad arguments (n >= 0; d_states, d_value and d_probs set and 4-byte aligned; filter 0 or 1; "
                       "norm GMK_PATTERN_NORM_L2 or GMK_PATTERN_NORM_SUM)");
        return GMK_ERR_ARG;
    }
    GMK_NEED_INIT();
    if (n == 0) return GMK_OK;
    const gmk::DeviceState& st = gmk::device_state();
    StatesParams prm{};
    prm.states = d_states; prm.n = n; prm.filter = filter; prm.norm = norm;
    prm.value = d_value; prm.probs = d_probs; prm.status = d_status;
    prm.g_trans = st.d_trans;
    prm.g_records = st.d_records;
    prm.trans_words = st.n_states * 4;
    prm.record_words = st.n_records * 4 + gmk::kPrefixWords;
    const size_t lds = static_cast<size_t>(kWaves * kPerWave + prm.trans_words + prm.record_words) * 4;
    if (lds > 160 * 1024) { gmk::set_error("K23: the pattern tables do not fit beside %d evaluator states in LDS", kWaves); return GMK_ERR_CAPACITY; }
    static bool attr_set = false;
    if (!attr_set) {
        GMK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pattern_states_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    const int rc = next_counter(hs, &prm.counter);
    if (rc != GMK_OK) return rc;
    const int grid = std::max(1, std::min((n + kWaves - 1) / kWaves, st.cu_count > 0 ? st.cu_count : 1));
    hipLaunchKernelGGL(pattern_states_kernel, dim3(grid), dim3(kThreads), lds, hs, prm);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_pattern_evaluate_states_host(const float* h_states, int n, int filter, int norm,
                                                float* h_value, float* h_probs, int32_t* h_status) {
    if (n < 0 || (n > 0 && (!h_states || !h_value || !h_probs)) || (filter != 0 && filter != 1) ||
        (norm != GMK_PATTERN_NORM_L2 && norm != GMK_PATTERN_NORM_SUM)) {
        gmk::set_error("gmk_pattern_evaluate_states_host: bad arguments");
        return GMK_ERR_ARG;
    }
    GMK_NEED_INIT();
    if (n == 0) return GMK_OK;
    const size_t un = static_cast<size_t>(n);
    gmk::Staging st("gmk_pattern_evaluate_states_host", gmk::kPoolKeeps);
    float *d_states, *d_value, *d_probs;
    int32_t* d_status;
    st.in(d_states, h_states, un * GMK_PATTERN_PLANES * kCells);
    st.out(d_probs, h_probs, un * kCells); st.out(d_value, h_value, un); st.out(d_status, h_status, un);
    int rc = st.take();
    if (rc == GMK_OK) rc = gmk_pattern_evaluate_states(d_states, n, filter, norm, d_value, d_probs, h_status ? d_status : nullptr, nullptr);
    if (rc != GMK_OK) return rc;
    GMK_STAGED(st, hipDeviceSynchronize());
    return st.download();
}

// the decode and the canonical list of include/gomoku_pattern_states.h, on the host: no GPU, no gmk_init
extern "C" int gmk_pattern_states_list_host(const float* h_states, int n, uint8_t* h_moves, int32_t* h_lens, int32_t* h_status) {
    if (n < 0 || (n > 0 && (!h_states || !h_moves || !h_lens || !h_status))) { gmk::set_error("gmk_pattern_states_list_host: bad arguments"); return GMK_ERR_ARG; }
    for (int i = 0; i < n; ++i)
        h_status[i] = gmk_pattern_list225(h_states + static_cast<size_t>(i) * GMK_PATTERN_PLANES * kCells, h_moves + static_cast<size_t>(i) * kCells, h_lens + i);
    return GMK_OK;
}

// the normalisation and the uniform fallback of the same header, on the host; it knows no evaluator status: a row that decodes counts as live
extern "C" int gmk_pattern_states_finish_host(const float* h_vec, const float* h_states, int n, int norm, float* h_probs) {
    if (n < 0 || (n > 0 && (!h_vec || !h_states || !h_probs)) || (norm != GMK_PATTERN_NORM_L2 && norm != GMK_PATTERN_NORM_SUM)) {
        gmk::set_error("gmk_pattern_states_finish_host: bad arguments");
        return GMK_ERR_ARG;
    }
    for (int i = 0; i < n; ++i) {
        gmk_pattern_masks m;
        gmk_pattern_masks_of(h_states + static_cast<size_t>(i) * GMK_PATTERN_PLANES * kCells, &m);
        gmk_pattern_finish225(h_vec + static_cast<size_t>(i) * kCells, norm, gmk_pattern_check(&m) == 0, m.own, m.opp, h_probs + static_cast<size_t>(i) * kCells);
    }
    return GMK_OK;
}
