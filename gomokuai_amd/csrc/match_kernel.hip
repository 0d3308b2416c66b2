// match_kernel.hip -- K12: the referee between two search handles that play one batch of games on the device.
//
// The reference evaluates its network in matches (network/train.py:88-126 evaluate_network -> agents/utils.py:66-100 eval_agents ->
// dual_play, :13-63): two agents, each with its own tree, take turns on one Board; the mover's agent searches, Board::applyMove plays
// its choice and decides the end of the game (core/lib/src/Game.cpp:37-49, 88-136), and both agents follow the move
// (MCTS::syncWithBoard, core/lib/src/MCTS.cpp:119-125).  Here the two trees live in a K7 handle and a K6 / K8 handle; the mover's handle
// leaves its choice in device memory (gmk_az_root_choice / gmk_trad_root_choice), this kernel is the Board, and both handles step from
// device memory (gmk_az_step_device / gmk_trad_step_device).  One wavefront per game; the position is rebuilt from the game's record.
#include "board_device.h"
#include "capi_common.h"

namespace {

constexpr int kCells = 225;

__global__ __launch_bounds__(64)
void match_referee_kernel(int n, int rows, const int16_t* __restrict__ cells, const uint16_t* __restrict__ visit_rows, const int32_t* __restrict__ row_of,
                          uint8_t* __restrict__ moves, int32_t* __restrict__ lens, int8_t* __restrict__ winner, uint16_t* __restrict__ visits,
                          int32_t* __restrict__ verdict, int32_t* __restrict__ status, int32_t* __restrict__ unfinished) {
    __shared__ uint32_t s_rows[16];
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot >= n) return;
    const int before = verdict[slot];
    if (before == GMK_MATCH_ENDED || before == GMK_MATCH_OVER) {            // the game ended on an earlier ply
        if (lane == 0) verdict[slot] = GMK_MATCH_OVER;
        return;
    }
    const int row = row_of ? row_of[slot] : slot;
    if (row < 0 || row >= rows) {
        if (lane == 0) { verdict[slot] = GMK_MATCH_REFUSED; status[slot] |= 2; atomicAdd(unfinished, 1); }
        return;
    }
    uint8_t* mv = moves + static_cast<size_t>(row) * kCells;
    const int len = min(max(lens[row], 0), kCells), cell = cells[slot];
    // the position: move i of the record is black's when i is even
    if (lane < 16) s_rows[lane] = 0u;
    __syncthreads();
    for (int i = lane; i < len; i += 64) {
        const uint32_t c = mv[i];
        if (c < 225u) atomicOr(&s_rows[c / 15u], 1u << (c % 15u + ((i & 1) ? 16u : 0u)));
    }
    __syncthreads();
    bool legal = cell >= 0 && cell < kCells && len < kCells;
    if (legal) legal = !((s_rows[cell / 15] >> (cell % 15)) & 0x10001u);
    if (!legal) {                                                           // off the board or occupied: the game does not move
        if (lane == 0) { verdict[slot] = GMK_MATCH_REFUSED; status[slot] |= 1; atomicAdd(unfinished, 1); }
        return;
    }
    if (visits) {                                                           // the mover's root visit counts: the searched ply's row of the record
        uint16_t* rv = visits + (static_cast<size_t>(row) * kCells + static_cast<size_t>(len)) * kCells;
        for (int i = lane; i < kCells; i += 64) rv[i] = visit_rows ? visit_rows[static_cast<size_t>(slot) * kCells + i] : static_cast<uint16_t>(0);
    }
    const int shift = (len & 1) ? 16 : 0;
    if (lane == 0) s_rows[cell / 15] |= 1u << (cell % 15 + shift);
    __syncthreads();
    const bool five = gmk::five_through<1>(s_rows, cell % 15, cell / 15, shift);
    if (lane == 0) {
        mv[len] = static_cast<uint8_t>(cell);
        lens[row] = len + 1;
        const bool over = five || len + 1 == kCells;
        if (over) winner[row] = static_cast<int8_t>(five ? (shift ? -1 : 1) : 0);
        else atomicAdd(unfinished, 1);
        verdict[slot] = over ? GMK_MATCH_ENDED : GMK_MATCH_MOVED;
    }
}

}  // namespace

extern "C" int gmk_match_referee(int n, int rows, const int16_t* d_cells, const uint16_t* d_visit_rows, const int32_t* d_row_of, uint8_t* d_moves, int32_t* d_lens,
                                 int8_t* d_winner, uint16_t* d_visits, int32_t* d_verdict, int32_t* d_status, int32_t* d_unfinished, void* stream) {
    GMK_NEED_INIT();
    if (n <= 0 || rows <= 0 || !d_cells || !d_moves || !d_lens || !d_winner || !d_verdict || !d_status || !d_unfinished) { gmk::set_error("gmk_match_referee: bad arguments"); return GMK_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    GMK_HIP_CHECK(hipMemsetAsync(d_unfinished, 0, 4, s));
    hipLaunchKernelGGL(match_referee_kernel, dim3(n), dim3(64), 0, s, n, rows, d_cells, d_visit_rows, d_row_of, d_moves, d_lens, d_winner, d_visits, d_verdict, d_status,
                       d_unfinished);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}
