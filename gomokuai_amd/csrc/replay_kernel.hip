// replay_kernel.hip -- the replay buffer: game records kept in HBM, training minibatches drawn from them.
//
// Takes the place of DataHelper.buffer + DataHelper.generate_batch (network/data_helper.py:67-83, 97-139): a bounded buffer whose oldest
// entries leave, and batch_size distinct samples per training step.  The reference keeps augmented tuples; this keeps RECORDS -- one byte
// per stored ply and one 450-byte visit row per sampled ply -- and builds the tuples of a batch when it is drawn (K4 + K5 for one sample
// and ONE symmetry per wavefront).  include/gomoku_hip.h ("replay buffer") states the layout, the eviction rule and the draw rule.
//
//   moves   uint8[cap]            ring of stored plies: ply t of a game is byte (mstart + t) % cap
//   visits  uint16[cap][225]      ring of the visit rows of SAMPLED plies (t >= first): row (sstart + t - first) % cap
//   desc    GameDesc[max_games]   ring of game descriptors, slot serial % max_games
//   state   uint64[8]             head, tail (serials held = [head, tail)), mhead, mtail, shead, stail (absolute ply counts, never wrapped)
// mstart / sstart count all stored / sampled plies appended before the game since the last reset, so the descriptors of the held games
// carry increasing sstart: a sample index is found by a binary search over them, whatever the ring positions are.
//
// Append = a planning workgroup (lengths checked, prefix sums, which new games fit, how many old ones leave, state update) and one
// workgroup per new game that copies it.  Draw = one wavefront per sample; lanes are cells (lane l owns cells l, l + 64, l + 128, l + 192),
// no LDS, no barrier.
#include "capi_common.h"
#include "records_access.h"
#include "replay_draw.h"
#include "replay_image.h"

namespace {

using gmk::PackedRecords;
using gmk::StrideRecords;

constexpr int kCells = 225;
constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / 64;

struct GameDesc {
    uint64_t serial;     // games appended before this one since the last reset
    uint64_t mstart;     // stored plies appended before it
    uint64_t sstart;     // sampled plies appended before it
    int16_t len;         // plies stored
    int16_t first;       // first sampled ply (the append's first_move)
    int8_t winner;
    int8_t pad[3];
};
static_assert(sizeof(GameDesc) == 32, "GameDesc is 32 bytes");

enum { kHead = 0, kTail, kMHead, kMTail, kSHead, kSTail, kStateWords = 8 };

struct Plan {
    int64_t j0;          // the first new game that is kept
    uint64_t serial0;    // serial, stored-ply and sampled-ply count of new game 0
    uint64_t m0, s0;
    int32_t ok;
};

__device__ __forceinline__ int sampled_of(int len, int first) { return len > first ? len - first : 0; }

// ---- append, step 1 (one workgroup): check, scan, decide, update the state ----
__global__ __launch_bounds__(kThreads)
void replay_plan_kernel(const int32_t* __restrict__ lens, int n, int first, uint64_t cap, uint64_t max_games, uint64_t* __restrict__ state,
                        const GameDesc* __restrict__ desc, int64_t* __restrict__ moff, int64_t* __restrict__ soff, Plan* __restrict__ plan,
                        int32_t* __restrict__ status) {
    __shared__ int64_t s_m[kThreads], s_s[kThreads];
    __shared__ int s_bad;
    __shared__ unsigned long long s_j0;
    const int tid = threadIdx.x;
    const int64_t per = (static_cast<int64_t>(n) + kThreads - 1) / kThreads;
    const int64_t lo = tid * per < n ? tid * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    if (tid == 0) { s_bad = 0; s_j0 = static_cast<unsigned long long>(n); }
    __syncthreads();
    int64_t m = 0, s = 0;
    bool bad = false;
    for (int64_t j = lo; j < hi; ++j) {
        const int l = lens[j];
        if (l < 0 || l > kCells) bad = true;
        else { m += l; s += sampled_of(l, first); }
    }
    if (bad) atomicOr(&s_bad, 1);
    s_m[tid] = m;
    s_s[tid] = s;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {             // inclusive Hillis-Steele scan of both sums
        const int64_t om = tid >= d ? s_m[tid - d] : 0, os = tid >= d ? s_s[tid - d] : 0;
        __syncthreads();
        s_m[tid] += om;
        s_s[tid] += os;
        __syncthreads();
    }
    if (s_bad) {                                          // a length outside [0, 225]: nothing is appended, the state stays
        if (tid == 0) { *status = GMK_REPLAY_BAD_LENGTH; plan->ok = 0; }
        return;
    }
    const int64_t T = s_m[kThreads - 1], S = s_s[kThreads - 1];
    int64_t em = s_m[tid] - m, es = s_s[tid] - s;
    bool found = false;
    for (int64_t j = lo; j < hi; ++j) {
        moff[j] = em;
        soff[j] = es;
        if (!found && static_cast<uint64_t>(T - em) <= cap) {      // games j .. n-1 fit by plies; the first such j of this thread
            atomicMin(&s_j0, static_cast<unsigned long long>(j));
            found = true;
        }
        const int l = lens[j];
        em += l;
        es += sampled_of(l, first);
    }
    if (tid == kThreads - 1) { moff[n] = T; soff[n] = S; }
    __syncthreads();
    if (tid != 0) return;
    int64_t j0 = static_cast<int64_t>(s_j0);
    if (static_cast<uint64_t>(n) > max_games && j0 < n - static_cast<int64_t>(max_games)) j0 = n - static_cast<int64_t>(max_games);
    const uint64_t head = state[kHead], tail = state[kTail], mtail = state[kMTail], stail = state[kSTail];
    uint64_t new_head, mhead, shead;
    if (j0 > 0) {                                         // not even the new games all fit: every older game leaves, and new games 0 .. j0-1 too
        new_head = tail + j0;
        mhead = mtail + moff[j0];
        shead = stail + soff[j0];
    } else {                                              // the oldest games leave until the new ones fit: the first h that passes (monotone in h)
        uint64_t a = head, b = tail;
        while (a < b) {
            const uint64_t mid = a + (b - a) / 2;
            const bool fits = (tail - mid) + n <= max_games && (mtail - desc[mid % max_games].mstart) + T <= cap;
            if (fits) b = mid; else a = mid + 1;
        }
        new_head = a;
        mhead = a < tail ? desc[a % max_games].mstart : mtail;
        shead = a < tail ? desc[a % max_games].sstart : stail;
    }
    plan->j0 = j0;
    plan->serial0 = tail;
    plan->m0 = mtail;
    plan->s0 = stail;
    plan->ok = 1;
    state[kHead] = new_head;
    state[kTail] = tail + n;
    state[kMHead] = mhead;
    state[kMTail] = mtail + T;
    state[kSHead] = shead;
    state[kSTail] = stail + S;
    *status = 0;
}

// ---- append, step 2: one workgroup per new game; only the kept ones write ----
template <class Records>
__device__ __forceinline__ void append_body(const Records& rec, const int32_t* __restrict__ lens, int first, uint64_t cap, uint64_t max_games,
                                            const Plan* __restrict__ plan, const int64_t* __restrict__ moff, const int64_t* __restrict__ soff,
                                            GameDesc* __restrict__ desc, uint8_t* __restrict__ ring_moves, uint16_t* __restrict__ ring_visits) {
    const int j = blockIdx.x, tid = threadIdx.x;
    if (!plan->ok || j < plan->j0) return;
    const int len = lens[j];
    const uint64_t serial = plan->serial0 + j, mstart = plan->m0 + moff[j], sstart = plan->s0 + soff[j];
    if (tid == 0) {
        GameDesc d;
        d.serial = serial;
        d.mstart = mstart;
        d.sstart = sstart;
        d.len = static_cast<int16_t>(len);
        d.first = static_cast<int16_t>(first);
        d.winner = rec.winner_of(j);
        d.pad[0] = d.pad[1] = d.pad[2] = 0;
        desc[serial % max_games] = d;
    }
    const uint8_t* mv = rec.moves_of(j);
    if (tid < len) ring_moves[(mstart + tid) % cap] = mv[tid];
    const int rows = sampled_of(len, first);
    for (int r = 0; r < rows; ++r) {
        const auto row = rec.visit_row(j, first + r);
        uint16_t* dst = ring_visits + ((sstart + r) % cap) * kCells;
        if (tid < kCells) dst[tid] = row[tid];
    }
}

__global__ __launch_bounds__(kThreads)
void replay_append_kernel(const uint8_t* __restrict__ moves, const int32_t* __restrict__ lens, const int8_t* __restrict__ winner,
                          const uint16_t* __restrict__ visits, int first, uint64_t cap, uint64_t max_games, const Plan* __restrict__ plan,
                          const int64_t* __restrict__ moff, const int64_t* __restrict__ soff, GameDesc* __restrict__ desc,
                          uint8_t* __restrict__ ring_moves, uint16_t* __restrict__ ring_visits) {
    append_body(StrideRecords{moves, visits, winner}, lens, first, cap, max_games, plan, moff, soff, desc, ring_moves, ring_visits);
}

__global__ __launch_bounds__(kThreads)
void replay_append_packed_kernel(const uint8_t* __restrict__ buf, int n, const int64_t* __restrict__ offsets, int first, uint64_t cap,
                                 uint64_t max_games, const Plan* __restrict__ plan, const int64_t* __restrict__ moff,
                                 const int64_t* __restrict__ soff, GameDesc* __restrict__ desc, uint8_t* __restrict__ ring_moves,
                                 uint16_t* __restrict__ ring_visits) {
    append_body(PackedRecords{buf, offsets, n}, reinterpret_cast<const int32_t*>(buf), first, cap, max_games, plan, moff, soff, desc, ring_moves,
                ring_visits);
}

// ---- draw: one wavefront per sample ----
// kPolicy (GMK_TARGET_POLICY, K21): the row is a distribution already, pi_c = (float)((double)w_c / (double)sum w); the sum is an integer below 2^24
template <class OutT, bool kPolicy>
__device__ __forceinline__ void replay_draw_body(const uint64_t* __restrict__ state, const GameDesc* __restrict__ desc, const uint8_t* __restrict__ ring_moves,
                                                 const uint16_t* __restrict__ ring_visits, uint64_t cap, uint64_t max_games, uint64_t seed, uint64_t step, int batch,
                                                 int augment, OutT* __restrict__ out_states, float* __restrict__ out_values, float* __restrict__ out_pi,
                                                 int64_t* __restrict__ out_picked, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));      // (uniform: what follows up to the lanes' loads is scalar work)
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave;
    const uint64_t head = state[kHead], tail = state[kTail], shead = state[kSHead], stail = state[kSTail];
    const uint64_t M = (stail - shead) * (augment ? 8 : 1);
    const int32_t code = M < static_cast<uint64_t>(batch) ? GMK_REPLAY_TOO_FEW : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = code;
    if (code || i >= batch) return;

    // which sample: the draw rule, then oldest-first (game, ply, symmetry) order
    const uint64_t p = gmk::replay_perm(static_cast<uint64_t>(i), M, gmk::replay_half_bits(M), seed, step);
    const uint64_t x = shead + (augment ? p >> 3 : p);            // absolute index of the sampled ply
    const int a = augment ? static_cast<int>(p & 7) : 0;
    uint64_t lo = head, hi = tail;                                // the last held game with sstart <= x (games without sampled plies share
    while (hi - lo > 1) {                                         // their sstart with the next game, so the last one is the one that has it)
        const uint64_t mid = lo + (hi - lo) / 2;
        if (desc[mid % max_games].sstart <= x) lo = mid; else hi = mid;
    }
    const GameDesc d = desc[lo % max_games];
    const int t = __builtin_amdgcn_readfirstlane(static_cast<int>(d.first + (x - d.sstart)));
    const int cur = (t & 1) ? -1 : 1;

    // ---- K4: the position before ply t, built in the OUTPUT orientation: every move goes to the cell that shows it ----
    int mv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = lane + 64 * q;
        const int c = idx < t ? ring_moves[(d.mstart + idx) % cap] : 0;
        mv[q] = gmk::augment_target(c, a);
    }
    int cell[4] = {0, 0, 0, 0};
    int last1 = -1, last2 = -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int cnt = t - 64 * q < 64 ? t - 64 * q : 64;
        for (int mm = 0; mm < cnt; ++mm) {                        // move 64 q + mm, black on even moves
            const int c = __builtin_amdgcn_readlane(mv[q], mm);
            const int col = (mm & 1) ? -1 : 1;
#pragma unroll
            for (int r = 0; r < 4; ++r) cell[r] = c == lane + 64 * r ? col : cell[r];
            last2 = last1;
            last1 = c;
        }
    }

    // ---- K5: pi from the visit row, in K5's summation order (records_kernel.hip reduces 256 LDS slots by slot[i] += slot[i + w],
    // w = 128 .. 1; slots 225.. are zero).  This lane holds slots l, l+64, l+128, l+192: w = 128 and w = 64 are the two local adds
    // (s0 + s2) + (s1 + s3), w = 32 .. 1 take lane l + w's partial sum, so lane 0 ends with the same association and the same bits.
    const uint16_t* vrow = ring_visits + (x % cap) * kCells;
    float pr[4];
    if constexpr (kPolicy) {
        uint32_t wv[4], ws = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = lane + 64 * q;
            wv[q] = idx < kCells ? vrow[idx] : 0u;
            ws += wv[q];
        }
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) ws += static_cast<uint32_t>(__shfl_xor(static_cast<int>(ws), w));
#pragma unroll
        for (int q = 0; q < 4; ++q) pr[q] = ws ? static_cast<float>(static_cast<double>(wv[q]) / static_cast<double>(ws)) : 0.0f;
    } else {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = lane + 64 * q;
            v[q] = idx < kCells ? static_cast<float>(vrow[idx]) : 0.0f;
        }
        float fs = (v[0] * v[0] + v[2] * v[2]) + (v[1] * v[1] + v[3] * v[3]);
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) fs += __shfl_down(fs, w);
        const float sq = __shfl(fs, 0);
        const float temperature = t < 15 ? 1.0f : 0.01f;                  // MCTS.cpp:114 (stones on the board = t)
        const float eps = 1.1920929e-07f;
        double e[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float u = v[q];
            if (sq > 0.0f) u = u / sqrtf(sq);                             // VectorXf::normalized()
            u = u ? u + 1.0f : u;                                         // MCTS.cpp:112
            e[q] = lane + 64 * q < kCells ? exp(static_cast<double>(logf(u + eps) / temperature)) : 0.0;   // Statistical.hpp:38-39
        }
        double ds = (e[0] + e[2]) + (e[1] + e[3]);
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) ds += __shfl_down(ds, w);
        const double total = __shfl(ds, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float f = static_cast<float>(e[q] / total);
            pr[q] = f > eps ? f : 0.0f;
        }
    }

    // ---- write the tuple; pi of output cell j is pi of source cell augment_source(j), held by lane src & 63 in register src >> 6 ----
    OutT* st = out_states + static_cast<size_t>(i) * 6 * kCells;
    float* po = out_pi + static_cast<size_t>(i) * kCells;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q;
        float pj = pr[q];
        if (a != 0) {                                                 // (uniform)
            const int src = j < kCells ? gmk::augment_source(j, a >> 1, (a & 1) != 0) : 0;
            const float g0 = __shfl(pr[0], src & 63), g1 = __shfl(pr[1], src & 63), g2 = __shfl(pr[2], src & 63), g3 = __shfl(pr[3], src & 63);
            const int r = src >> 6;
            pj = r == 0 ? g0 : r == 1 ? g1 : r == 2 ? g2 : g3;
        }
        if (j < kCells) {
            const int c = cell[q];
            st[0 * kCells + j] = static_cast<OutT>(c == cur);          // stones of the player to move
            st[1 * kCells + j] = static_cast<OutT>(c == -cur);         // opponent's stones
            st[2 * kCells + j] = static_cast<OutT>(c == 0);            // empties
            st[3 * kCells + j] = static_cast<OutT>(j == last1);        // last move
            st[4 * kCells + j] = static_cast<OutT>(j == last2);        // the move before it
            st[5 * kCells + j] = static_cast<OutT>(cur == 1);          // all ones iff black is to move
            po[j] = pj;
        }
    }
    if (lane == 0) {
        out_values[i] = static_cast<float>(cur) * static_cast<float>(d.winner);   // CalcScore (Game.h:34-36)
        if (out_picked) {
            out_picked[3 * i + 0] = static_cast<int64_t>(d.serial);
            out_picked[3 * i + 1] = t;
            out_picked[3 * i + 2] = a;
        }
    }
}
template <class OutT>
__global__ __launch_bounds__(kThreads)
void replay_draw_kernel(const uint64_t* __restrict__ state, const GameDesc* __restrict__ desc, const uint8_t* __restrict__ ring_moves,
                        const uint16_t* __restrict__ ring_visits, uint64_t cap, uint64_t max_games, uint64_t seed, uint64_t step, int batch,
                        int augment, OutT* __restrict__ out_states, float* __restrict__ out_values, float* __restrict__ out_pi,
                        int64_t* __restrict__ out_picked, int32_t* __restrict__ status) {
    replay_draw_body<OutT, false>(state, desc, ring_moves, ring_visits, cap, max_games, seed, step, batch, augment, out_states, out_values, out_pi, out_picked, status);
}
template <class OutT>
__global__ __launch_bounds__(kThreads)
void replay_draw_policy_kernel(const uint64_t* __restrict__ state, const GameDesc* __restrict__ desc, const uint8_t* __restrict__ ring_moves,
                               const uint16_t* __restrict__ ring_visits, uint64_t cap, uint64_t max_games, uint64_t seed, uint64_t step, int batch,
                               int augment, OutT* __restrict__ out_states, float* __restrict__ out_values, float* __restrict__ out_pi,
                               int64_t* __restrict__ out_picked, int32_t* __restrict__ status) {
    replay_draw_body<OutT, true>(state, desc, ring_moves, ring_visits, cap, max_games, seed, step, batch, augment, out_states, out_values, out_pi, out_picked, status);
}

// ---- the image (replay_image.h): the descriptors need a kernel each way, the plies and the visit rows are plain copies ----
// out: one thread per held game compacts its GameDesc into the 8-byte record; thread 0 also writes the header and the sections' padding
__global__ __launch_bounds__(kThreads)
void replay_snapshot_kernel(const GameDesc* __restrict__ desc, uint64_t max_games, uint64_t head, uint64_t n, uint64_t T, uint64_t S,
                            uint8_t* __restrict__ image, int32_t* __restrict__ status) {
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    uint64_t* words = reinterpret_cast<uint64_t*>(image);                 // (8-byte aligned: checked by the caller; the device is little-endian)
    if (g < n) {
        const GameDesc d = desc[(head + g) % max_games];
        uint8_t rec[8];
        gmk::replay_image_put_desc(rec, d.len, d.first, d.winner);
        words[gmk::kImageHeaderBytes / 8 + g] = gmk::image_u64(rec);
    }
    if (g != 0) return;
    const uint8_t magic[8] = {'G', 'M', 'K', 'R', 'P', 'L', 'Y', '1'};
    words[0] = gmk::image_u64(magic);
    words[1] = n;
    words[2] = T;
    words[3] = S;
    words[4] = head;
    words[5] = gmk::replay_image_size(n, T, S);
    words[6] = words[7] = 0;
    uint8_t* moves = image + gmk::kImageHeaderBytes + gmk::kImageDescBytes * n;
    for (uint64_t i = T; i < gmk::image_roundup8(T); ++i) moves[i] = 0;
    uint8_t* visits = moves + gmk::image_roundup8(T);
    for (uint64_t i = gmk::kImageRowBytes * S; i < gmk::image_roundup8(gmk::kImageRowBytes * S); ++i) visits[i] = 0;
    *status = 0;
}

// in (one workgroup, the chunked scan of replay_plan_kernel): every rule of replay_image.h but the host-only ones, then whether the games
// fit; with commit, also the GameDesc of every game -- mstart / sstart rebased so that the oldest game starts both rings at 0 -- and the
// state words.  A refusal writes *status and nothing else.  It runs twice per restore: commit = 0 before the rings are copied, commit = 1 after.
__global__ __launch_bounds__(kThreads)
void replay_restore_kernel(const uint8_t* __restrict__ image, uint64_t bytes, uint64_t cap, uint64_t max_games, int commit,
                           uint64_t* __restrict__ state, GameDesc* __restrict__ desc, int32_t* __restrict__ status) {
    __shared__ int64_t s_m[kThreads], s_s[kThreads];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    gmk::ReplayImageHeader h;
    if (gmk::replay_image_check_header(image, bytes, &h) != gmk::kImageOk) {      // (uniform: every thread reads the same 64 bytes)
        if (tid == 0) *status = GMK_REPLAY_BAD_IMAGE;
        return;
    }
    const uint8_t* recs = image + gmk::kImageHeaderBytes;                         // h.n of them lie inside the image: the header's formula
    const int64_t n = static_cast<int64_t>(h.n);
    const int64_t per = (n + kThreads - 1) / kThreads;
    const int64_t lo = tid * per < n ? tid * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int64_t m = 0, s = 0;
    bool bad = false;
    for (int64_t j = lo; j < hi; ++j) {
        int len, first, winner;
        if (gmk::replay_image_check_desc(recs + gmk::kImageDescBytes * j, &len, &first, &winner) != gmk::kImageOk) bad = true;
        else { m += len; s += gmk::image_sampled(len, first); }
    }
    if (bad) atomicOr(&s_bad, 1);
    s_m[tid] = m;
    s_s[tid] = s;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {             // inclusive Hillis-Steele scan of both sums
        const int64_t om = tid >= d ? s_m[tid - d] : 0, os = tid >= d ? s_s[tid - d] : 0;
        __syncthreads();
        s_m[tid] += om;
        s_s[tid] += os;
        __syncthreads();
    }
    int32_t code = 0;
    if (s_bad || static_cast<uint64_t>(s_m[kThreads - 1]) != h.T || static_cast<uint64_t>(s_s[kThreads - 1]) != h.S) code = GMK_REPLAY_BAD_IMAGE;
    else if (h.T > cap || h.n > max_games) code = GMK_REPLAY_NO_ROOM;
    if (code || !commit) {
        if (tid == 0) *status = code;
        return;
    }
    uint64_t em = static_cast<uint64_t>(s_m[tid] - m), es = static_cast<uint64_t>(s_s[tid] - s);
    for (int64_t j = lo; j < hi; ++j) {
        int len, first, winner;
        (void)gmk::replay_image_check_desc(recs + gmk::kImageDescBytes * j, &len, &first, &winner);
        GameDesc d;
        d.serial = h.head + static_cast<uint64_t>(j);
        d.mstart = em;
        d.sstart = es;
        d.len = static_cast<int16_t>(len);
        d.first = static_cast<int16_t>(first);
        d.winner = static_cast<int8_t>(winner);
        d.pad[0] = d.pad[1] = d.pad[2] = 0;
        desc[d.serial % max_games] = d;
        em += static_cast<uint64_t>(len);
        es += static_cast<uint64_t>(gmk::image_sampled(len, first));
    }
    if (tid != 0) return;
    state[kHead] = h.head;
    state[kTail] = h.head + h.n;
    state[kMHead] = 0;
    state[kMTail] = h.T;
    state[kSHead] = 0;
    state[kSTail] = h.S;
    *status = 0;
}

using gmk::misaligned;

constexpr int64_t kMaxCapacityPlies = int64_t(1) << 40;

}  // namespace

struct gmk_replay {
    uint64_t cap = 0, max_games = 0, seed = 0;
    uint64_t* d_state = nullptr;
    Plan* d_plan = nullptr;
    GameDesc* d_desc = nullptr;
    uint8_t* d_moves = nullptr;
    uint16_t* d_visits = nullptr;
    int64_t* d_scan = nullptr;           // moff int64[scan_games + 1] | soff int64[scan_games + 1]
    int64_t scan_games = 0;
};

namespace {

void free_all(gmk_replay* h) {
    (void)gmk::device_free(h->d_state);
    (void)gmk::device_free(h->d_plan);
    (void)gmk::device_free(h->d_desc);
    (void)gmk::device_free(h->d_moves);
    (void)gmk::device_free(h->d_visits);
    (void)gmk::device_free(h->d_scan);
    delete h;
}

// the scan rows hold n + 1 entries each; they grow (once per larger n) after the stream has drained what may still read the old ones
int reserve_scan(gmk_replay* h, int n, hipStream_t stream) {
    if (n <= h->scan_games) return GMK_OK;
    GMK_HIP_CHECK(hipStreamSynchronize(stream));
    (void)gmk::device_free(h->d_scan);
    h->d_scan = nullptr;
    h->scan_games = 0;
    GMK_HIP_CHECK(gmk::device_malloc(&h->d_scan, 2 * (static_cast<size_t>(n) + 1) * sizeof(int64_t)));
    h->scan_games = n;
    return GMK_OK;
}

}  // namespace

extern "C" int gmk_replay_create(int64_t capacity_plies, int64_t max_games, uint64_t seed, gmk_replay** out) {
    GMK_NEED_INIT();
    if (!out || capacity_plies < kCells || capacity_plies > kMaxCapacityPlies || max_games < 1 || max_games > capacity_plies) {
        gmk::set_error("gmk_replay_create: bad arguments (225 <= capacity_plies <= 2^40, 1 <= max_games <= capacity_plies)");
        return GMK_ERR_ARG;
    }
    gmk_replay* h = new gmk_replay;
    h->cap = static_cast<uint64_t>(capacity_plies);
    h->max_games = static_cast<uint64_t>(max_games);
    h->seed = seed;
    const int64_t scan0 = max_games < 65536 ? max_games : 65536;
    if (gmk::device_malloc(&h->d_state, kStateWords * sizeof(uint64_t)) != hipSuccess || gmk::device_malloc(&h->d_plan, sizeof(Plan)) != hipSuccess ||
        gmk::device_malloc(&h->d_desc, h->max_games * sizeof(GameDesc)) != hipSuccess || gmk::device_malloc(&h->d_moves, h->cap) != hipSuccess ||
        gmk::device_malloc(&h->d_visits, h->cap * kCells * sizeof(uint16_t)) != hipSuccess ||
        gmk::device_malloc(&h->d_scan, 2 * (static_cast<size_t>(scan0) + 1) * sizeof(int64_t)) != hipSuccess) {
        free_all(h);
        gmk::set_error("gmk_replay_create: device allocation failed (%lld plies of 451 bytes)", static_cast<long long>(capacity_plies));
        return GMK_ERR_HIP;
    }
    h->scan_games = scan0;
    if (hipMemset(h->d_state, 0, kStateWords * sizeof(uint64_t)) != hipSuccess || hipMemset(h->d_plan, 0, sizeof(Plan)) != hipSuccess ||
        hipStreamSynchronize(nullptr) != hipSuccess) {                  // (done before any stream of the caller's touches the handle)
        free_all(h);
        gmk::set_error("gmk_replay_create: hipMemset failed");
        return GMK_ERR_HIP;
    }
    *out = h;
    return GMK_OK;
}

extern "C" int gmk_replay_destroy(gmk_replay* h) {
    if (!h) return GMK_OK;
    free_all(h);
    return GMK_OK;
}

extern "C" int gmk_replay_reset(gmk_replay* h, void* stream) {
    GMK_NEED_INIT();
    if (!h) { gmk::set_error("gmk_replay_reset: no handle"); return GMK_ERR_ARG; }
    GMK_HIP_CHECK(hipMemsetAsync(h->d_state, 0, kStateWords * sizeof(uint64_t), static_cast<hipStream_t>(stream)));
    return GMK_OK;
}

extern "C" int gmk_replay_append(gmk_replay* h, const uint8_t* d_moves, const int32_t* d_lens, const int8_t* d_winner, const uint16_t* d_visits,
                                 int n, int first_move, int32_t* d_status, void* stream) {
    GMK_NEED_INIT();
    if (!h || n < 0 || first_move < 0 || first_move > kCells ||
        (n > 0 && (!d_moves || !d_lens || !d_winner || !d_visits || !d_status || misaligned(d_lens, 4) || misaligned(d_visits, 2) || misaligned(d_status, 4)))) {
        gmk::set_error("gmk_replay_append: bad arguments (0 <= first_move <= 225; d_lens and d_status 4-byte, d_visits 2-byte aligned)");
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = reserve_scan(h, n, s);
    if (rc != GMK_OK) return rc;
    int64_t* moff = h->d_scan;
    int64_t* soff = h->d_scan + h->scan_games + 1;
    hipLaunchKernelGGL(replay_plan_kernel, dim3(1), dim3(kThreads), 0, s, d_lens, n, first_move, h->cap, h->max_games, h->d_state, h->d_desc, moff, soff,
                       h->d_plan, d_status);
    GMK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(replay_append_kernel, dim3(n), dim3(kThreads), 0, s, d_moves, d_lens, d_winner, d_visits, first_move, h->cap, h->max_games,
                       h->d_plan, moff, soff, h->d_desc, h->d_moves, h->d_visits);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_replay_append_packed(gmk_replay* h, const uint8_t* d_buf, int n, const int64_t* d_offsets, int first_move, int32_t* d_status,
                                        void* stream) {
    GMK_NEED_INIT();
    if (!h || n < 0 || first_move < 0 || first_move > kCells ||
        (n > 0 && (!d_buf || !d_offsets || !d_status || misaligned(d_buf, 4) || misaligned(d_offsets, 8) || misaligned(d_status, 4)))) {
        gmk::set_error("gmk_replay_append_packed: bad arguments (0 <= first_move <= 225; d_buf and d_status 4-byte, d_offsets 8-byte aligned)");
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = reserve_scan(h, n, s);
    if (rc != GMK_OK) return rc;
    int64_t* moff = h->d_scan;
    int64_t* soff = h->d_scan + h->scan_games + 1;
    hipLaunchKernelGGL(replay_plan_kernel, dim3(1), dim3(kThreads), 0, s, reinterpret_cast<const int32_t*>(d_buf), n, first_move, h->cap, h->max_games,
                       h->d_state, h->d_desc, moff, soff, h->d_plan, d_status);
    GMK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(replay_append_packed_kernel, dim3(n), dim3(kThreads), 0, s, d_buf, n, d_offsets, first_move, h->cap, h->max_games, h->d_plan,
                       moff, soff, h->d_desc, h->d_moves, h->d_visits);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_replay_size(gmk_replay* h, int64_t* games, int64_t* plies, int64_t* population, int64_t* evicted_games, void* stream) {
    GMK_NEED_INIT();
    if (!h) { gmk::set_error("gmk_replay_size: no handle"); return GMK_ERR_ARG; }
    uint64_t w[kStateWords];
    hipStream_t s = static_cast<hipStream_t>(stream);
    GMK_HIP_CHECK(hipMemcpyAsync(w, h->d_state, sizeof(w), hipMemcpyDeviceToHost, s));
    GMK_HIP_CHECK(hipStreamSynchronize(s));
    if (games) *games = static_cast<int64_t>(w[kTail] - w[kHead]);
    if (plies) *plies = static_cast<int64_t>(w[kMTail] - w[kMHead]);
    if (population) *population = static_cast<int64_t>(w[kSTail] - w[kSHead]);
    if (evicted_games) *evicted_games = static_cast<int64_t>(w[kHead]);
    return GMK_OK;
}

// gmk_replay_sample and gmk_replay_sample_target: the mode is a property of the draw, not of the stored bytes
static int replay_sample(const char* who, gmk_replay* h, int batch, int64_t step, int augment, int target, int states_float, void* d_states, float* d_values, float* d_pi,
                         int64_t* d_picked, int32_t* d_status, void* stream) {
    GMK_NEED_INIT();
    if (!h || batch < 0 || (batch > 0 && (!d_states || !d_values || !d_pi || !d_status || misaligned(d_values, 4) || misaligned(d_pi, 4) ||
                                          misaligned(d_status, 4) || misaligned(d_picked, 8) || (states_float && misaligned(d_states, 4))))) {
        gmk::set_error("%s: bad arguments (batch >= 0; float outputs and d_status 4-byte, d_picked 8-byte aligned)", who);
        return GMK_ERR_ARG;
    }
    if (target != GMK_TARGET_VISITS && target != GMK_TARGET_POLICY) { gmk::set_error("%s: target %d is neither GMK_TARGET_VISITS nor GMK_TARGET_POLICY", who, target); return GMK_ERR_ARG; }
    if (batch == 0) return GMK_OK;
    const dim3 grid((batch + kWavesPerBlock - 1) / kWavesPerBlock), block(kThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (target == GMK_TARGET_POLICY) {
        if (states_float)
            hipLaunchKernelGGL(replay_draw_policy_kernel<float>, grid, block, 0, s, h->d_state, h->d_desc, h->d_moves, h->d_visits, h->cap, h->max_games, h->seed,
                               static_cast<uint64_t>(step), batch, augment, static_cast<float*>(d_states), d_values, d_pi, d_picked, d_status);
        else
            hipLaunchKernelGGL(replay_draw_policy_kernel<uint8_t>, grid, block, 0, s, h->d_state, h->d_desc, h->d_moves, h->d_visits, h->cap, h->max_games, h->seed,
                               static_cast<uint64_t>(step), batch, augment, static_cast<uint8_t*>(d_states), d_values, d_pi, d_picked, d_status);
    } else if (states_float)
        hipLaunchKernelGGL(replay_draw_kernel<float>, grid, block, 0, s, h->d_state, h->d_desc, h->d_moves, h->d_visits, h->cap, h->max_games, h->seed,
                           static_cast<uint64_t>(step), batch, augment, static_cast<float*>(d_states), d_values, d_pi, d_picked, d_status);
    else
        hipLaunchKernelGGL(replay_draw_kernel<uint8_t>, grid, block, 0, s, h->d_state, h->d_desc, h->d_moves, h->d_visits, h->cap, h->max_games, h->seed,
                           static_cast<uint64_t>(step), batch, augment, static_cast<uint8_t*>(d_states), d_values, d_pi, d_picked, d_status);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}
extern "C" int gmk_replay_sample(gmk_replay* h, int batch, int64_t step, int augment, int states_float, void* d_states, float* d_values, float* d_pi,
                                 int64_t* d_picked, int32_t* d_status, void* stream) {
    return replay_sample("gmk_replay_sample", h, batch, step, augment, GMK_TARGET_VISITS, states_float, d_states, d_values, d_pi, d_picked, d_status, stream);
}
extern "C" int gmk_replay_sample_target(gmk_replay* h, int batch, int64_t step, int augment, int target, int states_float, void* d_states, float* d_values, float* d_pi,
                                        int64_t* d_picked, int32_t* d_status, void* stream) {
    return replay_sample("gmk_replay_sample_target", h, batch, step, augment, target, states_float, d_states, d_values, d_pi, d_picked, d_status, stream);
}

extern "C" int gmk_replay_draw_host(uint64_t seed, int64_t step, int64_t population, int64_t batch, int64_t* h_index) {
    if (batch < 0 || population < 0 || batch > population || population > 8 * kMaxCapacityPlies || (batch > 0 && !h_index)) {
        gmk::set_error("gmk_replay_draw_host: bad arguments (0 <= batch <= population)");
        return GMK_ERR_ARG;
    }
    const uint64_t M = static_cast<uint64_t>(population);
    const int k = gmk::replay_half_bits(M);
    for (int64_t i = 0; i < batch; ++i) h_index[i] = static_cast<int64_t>(gmk::replay_perm(static_cast<uint64_t>(i), M, k, seed, static_cast<uint64_t>(step)));
    return GMK_OK;
}

// ---- the image: snapshot, restore, and the host's check ----
namespace {

// the state words on the host; drains the stream
int read_state(gmk_replay* h, uint64_t* w, hipStream_t s) {
    GMK_HIP_CHECK(hipMemcpyAsync(w, h->d_state, kStateWords * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    GMK_HIP_CHECK(hipStreamSynchronize(s));
    return GMK_OK;
}

// `count` units of `unit` bytes between a ring (unit `start` onwards, modulo cap units) and a linear run: at most two contiguous copies
int copy_ring(uint8_t* ring, uint8_t* linear, bool to_ring, uint64_t start, uint64_t count, uint64_t cap, uint64_t unit, hipStream_t s) {
    const uint64_t at = start % cap, one = count < cap - at ? count : cap - at;
    const uint64_t part[2][3] = {{at, 0, one}, {0, one, count - one}};     // ring unit, linear unit, units
    for (const auto& p : part) {
        if (p[2] == 0) continue;
        uint8_t *r = ring + p[0] * unit, *l = linear + p[1] * unit;
        GMK_HIP_CHECK(hipMemcpyAsync(to_ring ? r : l, to_ring ? l : r, p[2] * unit, hipMemcpyDeviceToDevice, s));
    }
    return GMK_OK;
}

}  // namespace

extern "C" int gmk_replay_image_bytes(gmk_replay* h, int64_t* bytes, void* stream) {
    GMK_NEED_INIT();
    if (!h || !bytes) { gmk::set_error("gmk_replay_image_bytes: no handle or no result pointer"); return GMK_ERR_ARG; }
    uint64_t w[kStateWords];
    const int rc = read_state(h, w, static_cast<hipStream_t>(stream));
    if (rc != GMK_OK) return rc;
    *bytes = static_cast<int64_t>(gmk::replay_image_size(w[kTail] - w[kHead], w[kMTail] - w[kMHead], w[kSTail] - w[kSHead]));
    return GMK_OK;
}

extern "C" int gmk_replay_snapshot(gmk_replay* h, uint8_t* d_image, int64_t capacity_bytes, int32_t* d_status, void* stream) {
    GMK_NEED_INIT();
    if (!h || !d_image || !d_status || capacity_bytes < 0 || misaligned(d_image, 8) || misaligned(d_status, 4)) {
        gmk::set_error("gmk_replay_snapshot: bad arguments (capacity_bytes >= 0; d_image 8-byte, d_status 4-byte aligned)");
        return GMK_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint64_t w[kStateWords];
    const int rc = read_state(h, w, s);
    if (rc != GMK_OK) return rc;
    const uint64_t n = w[kTail] - w[kHead], T = w[kMTail] - w[kMHead], S = w[kSTail] - w[kSHead];
    if (static_cast<uint64_t>(capacity_bytes) < gmk::replay_image_size(n, T, S)) {
        GMK_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_status), GMK_REPLAY_NO_ROOM, 1, s));
        return GMK_OK;
    }
    const unsigned blocks = static_cast<unsigned>(n / kThreads + 1);
    hipLaunchKernelGGL(replay_snapshot_kernel, dim3(blocks), dim3(kThreads), 0, s, h->d_desc, h->max_games, w[kHead], n, T, S, d_image, d_status);
    GMK_HIP_CHECK(hipGetLastError());
    uint8_t* moves = d_image + gmk::kImageHeaderBytes + gmk::kImageDescBytes * n;
    int rc2 = copy_ring(h->d_moves, moves, false, w[kMHead], T, h->cap, 1, s);
    if (rc2 == GMK_OK)
        rc2 = copy_ring(reinterpret_cast<uint8_t*>(h->d_visits), moves + gmk::image_roundup8(T), false, w[kSHead], S, h->cap, gmk::kImageRowBytes, s);
    return rc2;
}

extern "C" int gmk_replay_restore(gmk_replay* h, const uint8_t* d_image, int64_t bytes, int32_t* d_status, void* stream) {
    GMK_NEED_INIT();
    if (!h || !d_image || !d_status || bytes < static_cast<int64_t>(gmk::kImageHeaderBytes) || misaligned(d_image, 8) || misaligned(d_status, 4)) {
        gmk::set_error("gmk_replay_restore: bad arguments (bytes >= 64; d_image 8-byte, d_status 4-byte aligned)");
        return GMK_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // 1. the whole check, on the device; nothing of the handle is written yet
    hipLaunchKernelGGL(replay_restore_kernel, dim3(1), dim3(kThreads), 0, s, d_image, static_cast<uint64_t>(bytes), h->cap, h->max_games, 0, h->d_state,
                       h->d_desc, d_status);
    GMK_HIP_CHECK(hipGetLastError());
    int32_t code = 0;
    uint8_t header[gmk::kImageHeaderBytes];
    GMK_HIP_CHECK(hipMemcpyAsync(&code, d_status, sizeof(code), hipMemcpyDeviceToHost, s));
    GMK_HIP_CHECK(hipMemcpyAsync(header, d_image, sizeof(header), hipMemcpyDeviceToHost, s));
    GMK_HIP_CHECK(hipStreamSynchronize(s));
    if (code != 0) return GMK_OK;                                             // refused: *d_status says why
    // 2. the rings, from their start (the restored games are rebased to ply 0 of both), 3. the descriptors and the state words
    const uint64_t n = gmk::image_u64(header + 8), T = gmk::image_u64(header + 16), S = gmk::image_u64(header + 24);
    uint8_t* moves = const_cast<uint8_t*>(d_image) + gmk::kImageHeaderBytes + gmk::kImageDescBytes * n;
    int rc = copy_ring(h->d_moves, moves, true, 0, T, h->cap, 1, s);
    if (rc == GMK_OK) rc = copy_ring(reinterpret_cast<uint8_t*>(h->d_visits), moves + gmk::image_roundup8(T), true, 0, S, h->cap, gmk::kImageRowBytes, s);
    if (rc != GMK_OK) return rc;
    hipLaunchKernelGGL(replay_restore_kernel, dim3(1), dim3(kThreads), 0, s, d_image, static_cast<uint64_t>(bytes), h->cap, h->max_games, 1, h->d_state,
                       h->d_desc, d_status);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_replay_image_check_host(const uint8_t* image, int64_t bytes, int64_t info[5]) {
    if (!image || bytes < static_cast<int64_t>(gmk::kImageHeaderBytes)) {
        gmk::set_error("gmk_replay_image_check_host: bad arguments (an image of at least 64 bytes)");
        return GMK_ERR_ARG;
    }
    gmk::ReplayImageHeader h;
    const int fault = gmk::replay_image_check(image, static_cast<uint64_t>(bytes), &h);
    if (fault != gmk::kImageOk) {
        gmk::set_error("gmk_replay_image_check_host: %s", gmk::replay_image_fault_text(fault));
        return GMK_REPLAY_BAD_IMAGE;
    }
    if (info) {
        info[0] = static_cast<int64_t>(h.n);
        info[1] = static_cast<int64_t>(h.T);
        info[2] = static_cast<int64_t>(h.S);
        info[3] = static_cast<int64_t>(h.head);
        info[4] = 0;
    }
    return GMK_OK;
}
