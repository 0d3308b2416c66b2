// pvnet_sym_kernel.hip -- "K22": the policy-value network evaluated over the board's eight symmetries (gmk_pvnet_evaluate_sym).
//
// The rule is include/gomoku_symmetry.h.  Two small kernels around the UNCHANGED evaluate path (gmk_pvnet_evaluate: the trunk of the handle's
// precision and the dense kernel, both bit-isolated by row):
//   pvnet_sym_expand_kernel   n rows -> 8n rows (ALL: row 8 r + a = T_a of row r) or n rows (RANDOM: T_pick of row r, the pick computed here)
//   gmk_pvnet_evaluate        on the expanded rows, into the handle's workspace
//   pvnet_sym_reduce_kernel   the policy rows back-transformed and, for ALL, added up in the order a = 0 .. 7 and scaled by 1/8
// The index tables (8 x 225 bytes each way) are compile-time constants in constant memory; the expand kernel copies the rows it needs to LDS
// because it gathers through them 10 800 times per position.
#include <algorithm>

#include "../../include/gomoku_symmetry.h"
#include "capi_common.h"
#include "pvnet_pack.h"
#include "records_access.h"

namespace {

constexpr int kPix = GMK_SYM_CELLS, kRow = GMK_SYM_PLANES * GMK_SYM_CELLS, kSyms = GMK_SYM_COUNT;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTablePad = 228;                       // a table row in whole dwords

// The replay buffer's permutation (records_access.h: what the training augmentation feeds the network) and its inverse, tabulated.
struct SymTables {
    uint8_t src[kSyms][kTablePad];                   // src[a][j] = augment_source(j, a >> 1, a & 1)
    uint8_t dst[kSyms][kTablePad];                   // dst[a][c] = augment_target(c, a)
};

constexpr SymTables make_tables() {
    SymTables t{};
    for (int a = 0; a < kSyms; ++a)
        for (int j = 0; j < kPix; ++j) {
            t.src[a][j] = static_cast<uint8_t>(gmk::augment_source(j, a >> 1, (a & 1) != 0));
            t.dst[a][j] = static_cast<uint8_t>(gmk::augment_target(j, a));
        }
    return t;
}

// ... which are the closed forms gomoku_symmetry.h gives C callers, each a permutation of the cells and inverse to the other
constexpr bool tables_are_the_rule(const SymTables& t) {
    for (int a = 0; a < kSyms; ++a)
        for (int j = 0; j < kPix; ++j)
            if (t.src[a][j] != gmk_sym_source(j, a) || t.dst[a][j] != gmk_sym_target(j, a) || t.src[a][j] >= kPix || t.dst[a][t.src[a][j]] != j) return false;
    return true;
}

constexpr SymTables kHostTables = make_tables();
static_assert(tables_are_the_rule(kHostTables), "gomoku_symmetry.h states augment_source and augment_target");
__constant__ SymTables kTables = make_tables();

// One workgroup per source position.  mode ALL: eight output rows; mode RANDOM: one, in the symmetry wavefront 0 picks from the position's digest.
__global__ __launch_bounds__(kThreads)
void pvnet_sym_expand_kernel(const float* __restrict__ states, int n, int mode, uint32_t seed_lo, uint32_t seed_hi, float* __restrict__ out,
                             int32_t* __restrict__ picks) {
    __shared__ float s[kRow];
    __shared__ uint32_t table[kSyms * kTablePad / 4];
    __shared__ int pick;
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= n) return;
    const float* in = states + static_cast<size_t>(row) * kRow;
    for (int i = tid; i < kRow; i += kThreads) s[i] = in[i];
    __syncthreads();
    if (mode == GMK_PVNET_SYM_RANDOM) {
        if (tid < 64) {                                                              // wavefront 0: the digest, an order-free sum
            uint64_t d = tid == 0 ? gmk_sym_colour_term(s[5 * kPix] != 0.0f) : 0;
            for (int c = tid; c < kPix; c += 64) d += gmk_sym_cell_term(c, s[c] != 0.0f, s[kPix + c] != 0.0f);
            for (int off = 32; off >= 1; off >>= 1) d += __shfl_xor(static_cast<unsigned long long>(d), off, 64);
            if (tid == 0) {
                const int a = gmk_sym_pick(d, static_cast<uint64_t>(seed_lo) | static_cast<uint64_t>(seed_hi) << 32);
                pick = a;
                picks[row] = a;
            }
        }
        __syncthreads();
        const int a = pick;
        const uint32_t* src32 = reinterpret_cast<const uint32_t*>(kTables.src[a]);
        for (int i = tid; i < kTablePad / 4; i += kThreads) table[i] = src32[i];
        __syncthreads();
        const uint8_t* src = reinterpret_cast<const uint8_t*>(table);
        float* o = out + static_cast<size_t>(row) * kRow;
        for (int i = tid; i < kRow; i += kThreads) {
            const int p = i / kPix, j = i - p * kPix;
            o[i] = s[p * kPix + src[j]];
        }
        return;
    }
    const uint32_t* src32 = reinterpret_cast<const uint32_t*>(kTables.src);
    for (int i = tid; i < kSyms * kTablePad / 4; i += kThreads) table[i] = src32[i];
    __syncthreads();
    const uint8_t* src = reinterpret_cast<const uint8_t*>(table);
    float* o = out + static_cast<size_t>(row) * (kSyms * kRow);
    for (int i = tid; i < kSyms * kRow; i += kThreads) {                             // consecutive lanes, consecutive floats: coalesced stores, gathered LDS reads
        const int a = i / kRow, rem = i - a * kRow, p = rem / kPix, j = rem - p * kPix;
        o[i] = s[p * kPix + src[a * kTablePad + j]];
    }
}

// One wavefront per position; lanes take the cells c, c + 64, ...  ALL: ((q_0 + q_1) + .. + q_7) * 0.125f in float32, q_a = row 8 r + a read
// at dst_a(c); lane 0 does the same with the eight values.  RANDOM: the one row, back-transformed.
__global__ __launch_bounds__(kThreads)
void pvnet_sym_reduce_kernel(const float* __restrict__ v, const float* __restrict__ q, const int32_t* __restrict__ picks, int n, int mode,
                             float* __restrict__ value, float* __restrict__ probs) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * kWaves + static_cast<int>(threadIdx.x >> 6);
    if (r >= n) return;
    float* out = probs + static_cast<size_t>(r) * kPix;
    if (mode == GMK_PVNET_SYM_RANDOM) {
        const int a = picks[r] & 7;
        const float* qa = q + static_cast<size_t>(r) * kPix;
        for (int c = lane; c < kPix; c += 64) out[c] = qa[kTables.dst[a][c]];
        if (lane == 0) value[r] = v[r];
        return;
    }
    const float* q0 = q + static_cast<size_t>(r) * (kSyms * kPix);
    for (int c = lane; c < kPix; c += 64) {
        float acc = q0[kTables.dst[0][c]];
#pragma unroll
        for (int a = 1; a < kSyms; ++a) acc += q0[a * kPix + kTables.dst[a][c]];
        out[c] = acc * 0.125f;
    }
    if (lane == 0) {
        const float* v0 = v + static_cast<size_t>(r) * kSyms;
        float acc = v0[0];
#pragma unroll
        for (int a = 1; a < kSyms; ++a) acc += v0[a];
        value[r] = acc * 0.125f;
    }
}

// the workspace: [capacity] rows of expanded states (1350), values (1) and policy rows (225), then int32 picks [capacity]
constexpr size_t kWorkFloatsPerRow = kRow + 1 + kPix;

}  // namespace

extern "C" int gmk_pvnet_evaluate_sym(gmk_pvnet* net, const float* d_states, int n, int mode, uint64_t seed, float* d_value, float* d_probs,
                                      void* stream) {
    if (!net || n < 0 || (n > 0 && (!d_states || !d_value || !d_probs)) || mode < GMK_PVNET_SYM_NONE || mode > GMK_PVNET_SYM_RANDOM) {
        gmk::set_error("gmk_pvnet_evaluate_sym: bad arguments");
        return GMK_ERR_ARG;
    }
    GMK_NEED_INIT();
    if (mode == GMK_PVNET_SYM_NONE) return gmk_pvnet_evaluate(net, d_states, n, d_value, d_probs, stream);
    if (!net->has_dense) { gmk::set_error("gmk_pvnet_evaluate_sym: the dense layers have not been set (gmk_pvnet_set_dense)"); return GMK_ERR_STATE; }
    if (n == 0) return GMK_OK;
    if (n > (1 << 24)) { gmk::set_error("gmk_pvnet_evaluate_sym: more than 2^24 positions"); return GMK_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rows = mode == GMK_PVNET_SYM_ALL ? kSyms * n : n;
    if (rows > net->sym_capacity) {                              // grows, never shrinks; allocates, so not during a stream capture
        if (net->d_sym) { GMK_HIP_CHECK(hipStreamSynchronize(s)); (void)gmk::device_free(net->d_sym); net->d_sym = nullptr; net->sym_capacity = 0; }
        const int capacity = std::max(rows, 1024);
        GMK_HIP_CHECK(gmk::device_malloc(&net->d_sym, static_cast<size_t>(capacity) * (kWorkFloatsPerRow + 1) * sizeof(float)));
        net->sym_capacity = capacity;
    }
    const size_t cap = static_cast<size_t>(net->sym_capacity);
    float* d_x = net->d_sym;
    float* d_v = d_x + cap * kRow;
    float* d_q = d_v + cap;
    int32_t* d_picks = reinterpret_cast<int32_t*>(d_q + cap * kPix);
    hipLaunchKernelGGL(pvnet_sym_expand_kernel, dim3(n), dim3(kThreads), 0, s, d_states, n, mode, static_cast<uint32_t>(seed),
                       static_cast<uint32_t>(seed >> 32), d_x, d_picks);
    GMK_HIP_CHECK(hipGetLastError());
    const int rc = gmk_pvnet_evaluate(net, d_x, rows, d_v, d_q, stream);
    if (rc != GMK_OK) return rc;
    hipLaunchKernelGGL(pvnet_sym_reduce_kernel, dim3((n + kWaves - 1) / kWaves), dim3(kThreads), 0, s, d_v, d_q, d_picks, n, mode, d_value, d_probs);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_pvnet_sym_pick_host(const float* h_states, int n, uint64_t seed, int32_t* h_sym) {
    if (n < 0 || (n > 0 && (!h_states || !h_sym))) { gmk::set_error("gmk_pvnet_sym_pick_host: bad arguments"); return GMK_ERR_ARG; }
    for (int i = 0; i < n; ++i) h_sym[i] = gmk_sym_pick(gmk_sym_digest(h_states + static_cast<size_t>(i) * kRow), seed);
    return GMK_OK;
}

namespace gmk {
void pvnet_sym_release(gmk_pvnet* net) {
    if (net->d_sym) { (void)device_free(net->d_sym); net->d_sym = nullptr; net->sym_capacity = 0; }
}
}  // namespace gmk
