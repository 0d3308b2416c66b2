// records_kernel.hip -- K4 + K5: game records -> training tuples on the device.
//
// A self-play record (moves, per-move root visit counts, winner) is what gmk_mcts_advance leaves in HBM.  The
// reference turns every move of a game into a sample while it plays (agents/utils.py:29-41, 55-59):
//     ( Board.encoded_states()  uint8[6][15][15]   (core/py_ext/src/game_ext.hpp:87-104)
//     , Player.calc_score(player to move, winner)  float
//     , MCTS::evalState's pi        float32[225]   (core/lib/src/MCTS.cpp:104-117, Statistical.hpp:37-42) )
// and then augments it eight-fold (network/data_helper.py:36-55: rot90^i and fliplr of it, i = 0..3).
// Here one workgroup produces one sample (x8 when augmenting) straight from the record:
//   K4  the six feature planes are rebuilt by replaying the first t moves of the record,
//   K5  pi = softmax(log(v / |v|_2 + [v != 0] + eps) / tau) in double, tau = 1 below 15 stones else 0.01.
// The same body serves the fixed-stride records (gmk_samples_from_records) and their wire form (gmk_samples_from_packed).
#include "capi_common.h"
#include "records_access.h"

namespace {

constexpr int kCells = 225;

// augment_source and the record accessors StrideRecords / PackedRecords: records_access.h (shared with replay_kernel.hip)
using gmk::augment_source;
using gmk::PackedRecords;
using gmk::StrideRecords;

// kPolicy (GMK_TARGET_POLICY, K21): the row is a distribution already (gmk_az_advance_gumbel's improved-policy row), and
//   pi_c = (float)((double)w_c / (double)sum w); the sum is an integer below 2^24, so it does not depend on the order it is added in.
template <bool kPolicy, class Records>
__device__ __forceinline__ void samples_body(const Records& rec, const int32_t* __restrict__ sample_game, const int32_t* __restrict__ sample_move,
                                             int n_samples, int augment, uint8_t* __restrict__ out_states, float* __restrict__ out_values,
                                             float* __restrict__ out_pi) {
    __shared__ int8_t s_cell[kCells];
    __shared__ float s_pi[kCells];
    __shared__ float s_red[256];
    __shared__ double s_redd[256];
    const int s = blockIdx.x;
    if (s >= n_samples) return;
    const int g = sample_game[s], t = sample_move[s], tid = threadIdx.x;
    const uint8_t* mv = rec.moves_of(g);

    // ---- K4: position before move t (black moves first), player to move, last two moves ----
    if (tid < kCells) s_cell[tid] = 0;
    __syncthreads();
    if (tid < t) s_cell[mv[tid]] = (tid & 1) ? -1 : 1;
    __syncthreads();
    const int cur = (t & 1) ? -1 : 1;

    // ---- K5: pi from the visit counts of move t ----
    const auto vrow = rec.visit_row(g, t);
    if constexpr (kPolicy) {
        __shared__ uint32_t s_total;
        const uint32_t w = tid < kCells ? vrow[tid] : 0u;
        if (tid == 0) s_total = 0u;
        __syncthreads();
        if (w) atomicAdd(&s_total, w);
        __syncthreads();
        const uint32_t total = s_total;
        if (tid < kCells) s_pi[tid] = total ? static_cast<float>(static_cast<double>(w) / static_cast<double>(total)) : 0.0f;
        __syncthreads();
    } else {
        float v = tid < kCells ? static_cast<float>(vrow[tid]) : 0.0f;
        s_red[tid] = v * v;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) { if (tid < w) s_red[tid] += s_red[tid + w]; __syncthreads(); }
        const float sq = s_red[0];
        if (sq > 0.0f) v = v / sqrtf(sq);                                 // VectorXf::normalized()
        v = v ? v + 1.0f : v;                                             // MCTS.cpp:112
        const float temperature = t < 15 ? 1.0f : 0.01f;                  // MCTS.cpp:114 (stones on the board = t)
        const float eps = 1.1920929e-07f;
        const double e = tid < kCells ? exp(static_cast<double>(logf(v + eps) / temperature)) : 0.0;   // Statistical.hpp:38-39
        __syncthreads();
        s_redd[tid] = e;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) { if (tid < w) s_redd[tid] += s_redd[tid + w]; __syncthreads(); }
        if (tid < kCells) { const float p = static_cast<float>(e / s_redd[0]); s_pi[tid] = p > eps ? p : 0.0f; }
        __syncthreads();
    }

    const int copies = augment ? 8 : 1;
    for (int a = 0; a < copies; ++a) {
        const size_t o = static_cast<size_t>(s) * copies + a;
        const int k = a >> 1;
        const bool flip = (a & 1) != 0;
        if (tid < kCells) {
            const int src = augment ? augment_source(tid, k, flip) : tid;
            const int8_t c = s_cell[src];
            uint8_t* st = out_states + o * 6 * kCells;
            st[0 * kCells + tid] = c == cur;                                          // stones of the player to move
            st[1 * kCells + tid] = c == -cur;                                         // opponent's stones
            st[2 * kCells + tid] = c == 0;                                            // empties
            st[3 * kCells + tid] = (t >= 1 && mv[t - 1] == src);                      // last move
            st[4 * kCells + tid] = (t >= 2 && mv[t - 2] == src);                      // the move before it
            st[5 * kCells + tid] = cur == 1;                                          // all ones iff black is to move
            out_pi[o * kCells + tid] = s_pi[src];
        }
        if (tid == 0) out_values[o] = static_cast<float>(cur) * static_cast<float>(rec.winner_of(g));   // CalcScore (Game.h:34-36)
    }
}

__global__ __launch_bounds__(256)
void samples_from_records_kernel(const uint8_t* __restrict__ moves, const int32_t* __restrict__ lens, const uint16_t* __restrict__ visits,
                                 const int8_t* __restrict__ winner, const int32_t* __restrict__ sample_game, const int32_t* __restrict__ sample_move,
                                 int n_samples, int augment, uint8_t* __restrict__ out_states, float* __restrict__ out_values, float* __restrict__ out_pi) {
    samples_body<false>(StrideRecords{moves, visits, winner}, sample_game, sample_move, n_samples, augment, out_states, out_values, out_pi);
}
__global__ __launch_bounds__(256)
void samples_from_records_policy_kernel(const uint8_t* __restrict__ moves, const int32_t* __restrict__ lens, const uint16_t* __restrict__ visits,
                                        const int8_t* __restrict__ winner, const int32_t* __restrict__ sample_game, const int32_t* __restrict__ sample_move,
                                        int n_samples, int augment, uint8_t* __restrict__ out_states, float* __restrict__ out_values, float* __restrict__ out_pi) {
    samples_body<true>(StrideRecords{moves, visits, winner}, sample_game, sample_move, n_samples, augment, out_states, out_values, out_pi);
}

__global__ __launch_bounds__(256)
void samples_from_packed_kernel(const uint8_t* __restrict__ buf, int n, const int64_t* __restrict__ offsets, const int32_t* __restrict__ sample_game,
                                const int32_t* __restrict__ sample_move, int n_samples, int augment, uint8_t* __restrict__ out_states,
                                float* __restrict__ out_values, float* __restrict__ out_pi) {
    samples_body<false>(PackedRecords{buf, offsets, n}, sample_game, sample_move, n_samples, augment, out_states, out_values, out_pi);
}
__global__ __launch_bounds__(256)
void samples_from_packed_policy_kernel(const uint8_t* __restrict__ buf, int n, const int64_t* __restrict__ offsets, const int32_t* __restrict__ sample_game,
                                       const int32_t* __restrict__ sample_move, int n_samples, int augment, uint8_t* __restrict__ out_states,
                                       float* __restrict__ out_values, float* __restrict__ out_pi) {
    samples_body<true>(PackedRecords{buf, offsets, n}, sample_game, sample_move, n_samples, augment, out_states, out_values, out_pi);
}

}  // namespace

static bool target_ok(const char* who, int target) {
    if (target == GMK_TARGET_VISITS || target == GMK_TARGET_POLICY) return true;
    gmk::set_error("%s: target %d is neither GMK_TARGET_VISITS nor GMK_TARGET_POLICY", who, target);
    return false;
}

// gmk_samples_from_records and gmk_samples_from_records_target
static int samples_from_records(const char* who, const uint8_t* d_moves, const int32_t* d_lens, const uint16_t* d_visits, const int8_t* d_winner,
                                const int32_t* d_sample_game, const int32_t* d_sample_move, int n_samples, int augment, int target,
                                uint8_t* d_states, float* d_values, float* d_pi, void* stream) {
    GMK_NEED_INIT();
    if (n_samples < 0 || (n_samples > 0 && (!d_moves || !d_lens || !d_visits || !d_winner || !d_sample_game || !d_sample_move || !d_states || !d_values || !d_pi))) {
        gmk::set_error("%s: bad arguments", who);
        return GMK_ERR_ARG;
    }
    if (!target_ok(who, target)) return GMK_ERR_ARG;
    if (n_samples == 0) return GMK_OK;
    hipLaunchKernelGGL(target == GMK_TARGET_POLICY ? samples_from_records_policy_kernel : samples_from_records_kernel, dim3(n_samples), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_moves, d_lens, d_visits, d_winner, d_sample_game, d_sample_move, n_samples, augment, d_states, d_values, d_pi);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}
extern "C" int gmk_samples_from_records(const uint8_t* d_moves, const int32_t* d_lens, const uint16_t* d_visits, const int8_t* d_winner,
                                        const int32_t* d_sample_game, const int32_t* d_sample_move, int n_samples, int augment,
                                        uint8_t* d_states, float* d_values, float* d_pi, void* stream) {
    return samples_from_records("gmk_samples_from_records", d_moves, d_lens, d_visits, d_winner, d_sample_game, d_sample_move, n_samples, augment, GMK_TARGET_VISITS, d_states,
                                d_values, d_pi, stream);
}
extern "C" int gmk_samples_from_records_target(const uint8_t* d_moves, const int32_t* d_lens, const uint16_t* d_visits, const int8_t* d_winner,
                                               const int32_t* d_sample_game, const int32_t* d_sample_move, int n_samples, int augment, int target,
                                               uint8_t* d_states, float* d_values, float* d_pi, void* stream) {
    return samples_from_records("gmk_samples_from_records_target", d_moves, d_lens, d_visits, d_winner, d_sample_game, d_sample_move, n_samples, augment, target, d_states,
                                d_values, d_pi, stream);
}

// gmk_samples_from_packed and gmk_samples_from_packed_target
static int samples_from_packed(const char* who, const uint8_t* d_buf, int n, const int64_t* d_offsets, const int32_t* d_sample_game,
                               const int32_t* d_sample_move, int n_samples, int augment, int target, uint8_t* d_states, float* d_values, float* d_pi,
                               void* stream) {
    GMK_NEED_INIT();
    if (n < 0 || n_samples < 0 || (n_samples > 0 && (n == 0 || !d_buf || !d_offsets || !d_sample_game || !d_sample_move || !d_states || !d_values || !d_pi))) {
        gmk::set_error("%s: bad arguments", who);
        return GMK_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(d_offsets) % 8) {
        gmk::set_error("%s: d_offsets must be 8-byte aligned", who);
        return GMK_ERR_ARG;
    }
    if (!target_ok(who, target)) return GMK_ERR_ARG;
    if (n == 0 || n_samples == 0) return GMK_OK;
    hipLaunchKernelGGL(target == GMK_TARGET_POLICY ? samples_from_packed_policy_kernel : samples_from_packed_kernel, dim3(n_samples), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_buf, n, d_offsets, d_sample_game, d_sample_move, n_samples, augment, d_states, d_values, d_pi);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}
extern "C" int gmk_samples_from_packed(const uint8_t* d_buf, int n, const int64_t* d_offsets, const int32_t* d_sample_game,
                                       const int32_t* d_sample_move, int n_samples, int augment, uint8_t* d_states, float* d_values, float* d_pi,
                                       void* stream) {
    return samples_from_packed("gmk_samples_from_packed", d_buf, n, d_offsets, d_sample_game, d_sample_move, n_samples, augment, GMK_TARGET_VISITS, d_states, d_values, d_pi,
                               stream);
}
extern "C" int gmk_samples_from_packed_target(const uint8_t* d_buf, int n, const int64_t* d_offsets, const int32_t* d_sample_game,
                                              const int32_t* d_sample_move, int n_samples, int augment, int target, uint8_t* d_states, float* d_values,
                                              float* d_pi, void* stream) {
    return samples_from_packed("gmk_samples_from_packed_target", d_buf, n, d_offsets, d_sample_game, d_sample_move, n_samples, augment, target, d_states, d_values, d_pi,
                               stream);
}
