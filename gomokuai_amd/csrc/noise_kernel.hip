// noise_kernel.hip -- gmk_noise_mix_rows: Default::AddNoise (noise_device.h: mix_root_priors) on rows of priors the CALLER supplies, by cell.
// A diagnostic entry: the search kernels (K3 mcts_kernel.hip, K6 / K8 trad_kernel.hip, K7 az_kernel.hip) wrap the same inlined mixing in their
// own child-to-cell gather and scatter and show it only through a search; here a test chooses the child set, the priors and the key
// (game id, stones, seed) of every row, and holds the result to the serial statement (include/gomoku_noise.h: gmk_noise_mix225), bit for bit
// (tests/test_noise_rows_gpu.py).
#include "capi_common.h"
#include "noise_device.h"

namespace {

constexpr int kCells = GMK_BOARD_CELLS;

// One wavefront per row: lane l holds the cells l + 64 j, as in every kernel that calls mix_root_priors.  draws (may be null): the gamma variate
// of every entry that takes a draw -- the entries whose prior is non-zero after the scaling by 1 - epsilon, mix_root_priors' own test -- before
// the normalisation, 0 elsewhere.
__global__ __launch_bounds__(64)
void noise_mix_rows_kernel(float* __restrict__ priors, float* __restrict__ draws, const uint32_t* __restrict__ game_ids, const uint32_t* __restrict__ stones,
                           int n, float alpha, float epsilon, uint32_t seed_lo, uint32_t seed_hi) {
    const int row = blockIdx.x, lane = threadIdx.x;
    if (row >= n) return;
    float* mine = priors + static_cast<size_t>(row) * kCells;
    const uint32_t game_id = game_ids[row], st = stones[row];
    float p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = lane + 64 * j < kCells ? mine[lane + 64 * j] : 0.0f;
    if (draws) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cell = lane + 64 * j;
            const float scaled = p[j] * (1 - epsilon);
            if (cell < kCells)
                draws[static_cast<size_t>(row) * kCells + cell] = scaled != 0.0f ? gmk::noise::gamma_draw(alpha, game_id, st, static_cast<uint32_t>(cell), seed_lo, seed_hi) : 0.0f;
        }
    }
    gmk::noise::mix_root_priors(p, lane, alpha, epsilon, game_id, st, seed_lo, seed_hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) if (lane + 64 * j < kCells) mine[lane + 64 * j] = p[j];
}

}  // namespace

extern "C" int gmk_noise_mix_rows(float* d_priors, float* d_draws, const uint32_t* d_game_ids, const uint32_t* d_stones,
                                  int n, float alpha, float epsilon, uint64_t seed, void* stream) {
    GMK_NEED_INIT();
    if (n < 0 || (n > 0 && (!d_priors || !d_game_ids || !d_stones || gmk::misaligned(d_priors, 4) || gmk::misaligned(d_draws, 4) ||
                            gmk::misaligned(d_game_ids, 4) || gmk::misaligned(d_stones, 4)))) {
        gmk::set_error("gmk_noise_mix_rows: bad arguments (n >= 0; for n > 0 d_priors, d_game_ids, d_stones non-null and every pointer 4-byte aligned)");
        return GMK_ERR_ARG;
    }
    if (!gmk::noise_args_ok("gmk_noise_mix_rows", alpha, epsilon)) return GMK_ERR_ARG;
    if (n == 0) return GMK_OK;
    hipLaunchKernelGGL(noise_mix_rows_kernel, dim3(n), dim3(64), 0, static_cast<hipStream_t>(stream), d_priors, d_draws, d_game_ids, d_stones, n, alpha, epsilon,
                       static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}
