// train_kernel.hip -- K11: one training step of the policy-value network on the device (network/model_tf.py:73-135, network/train.py:62-86).
//
// A step is a forward pass that keeps its activations, the loss, the backward pass and TF1's Adam, float32 data, all on the caller's stream,
// bit-reproducible: no floating-point atomic anywhere, every sum runs in an order that depends on the shapes only.
//
// Activations are channels-last ([position][pixel][channel] = a row-major matrix of 225 n rows), parameters keep the layout gmk_pvnet_create
// takes ([cout][cin][3][3], [out][in]), so every layer is one GEMM on train_gemm_kernel:
//   conv3x3 forward      act[rows][cout]   = relu(col[rows][9 cin] . W^T + b)          col = im2col3x3 of the layer's input, column k = cin * 9 + tap
//   conv3x3 weights      dW[cout][9 cin]   = dY^T[cout][rows] . col[rows][9 cin]       K = rows: split-K
//   conv3x3 input        dcol[rows][9 cin] = dY[rows][cout] . W[cout][9 cin], then col2im3x3 (a gather) and the ReLU mask of the input
//   1x1 heads together   h6[rows][6]       = relu(act3 . W6^T + b6), stored as pflat [n][900] and vflat [n][450] (flattened (pixel, channel))
//   dense layers         logits = pflat . Wp^T + bp, hidden = relu(vflat . Wh^T + bh); the 64 -> 1 output is vector code in train_loss_kernel
//   bias gradients       db[N] = ones[1][rows] . dY[rows][N]: column sums through the same split-K path, in slab order
// The column matrix of the 3x3 layers is made for kSlabPos positions at a time (train_host.h) and made again in the backward pass; the weight
// gradients of all slabs land in one scratch buffer, one copy per K slab of kKSlabRows rows, and ONE reduction adds them in slab order.
//
// train_gemm_kernel is a plain LDS-tiled GEMM on v_mfma_f32_32x32x2_f32: a workgroup of four wavefronts takes a 128 x (128 | 64 | 32) tile of C,
// stages 16 k of A and B in LDS (k-major, so that an operand read is one conflict-free ds_read_b32 per lane: lane l reads [k = l >> 5][i = l & 31])
// and issues MFMAs with no vector work between them but the LDS reads.  It is not K9's loop: no software pipelining, no register-held weights.
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_common.h"
#include "train_host.h"

namespace {

using namespace gmk::train;
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------------------------------------
struct GemmArgs {
    const float* A; long sam, sak;                 // A(m, k) = A[m * sam + k * sak]
    const float* B; long sbk, sbn;                 // B(k, n) = B[k * sbk + n * sbn]
    int M, N, K;
    int kslab;                                     // k range of one blockIdx.z
    float* part;                                   // split-K: raw partial sums go to part[(z0 + blockIdx.z)][M][N] and nothing else happens
    int z0;
    // ---- the epilogue of the direct form ----
    float* C; long ldc;                            // C(m, n) = C[m * ldc + (n / cq) * cs + n % cq]; columns >= nsplit go to C2[m * ldc2 + n - nsplit]
    int cq; long cs;
    int nsplit; float* C2; long ldc2;
    const float* bias;                             // [N] or null
    int relu;
    const float* mask; long ldm;                   // null, or keep C(m, n) only where mask[m * ldm + n] > 0 (the ReLU mask of a saved activation)
};

__device__ __forceinline__ int cd_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

constexpr int kBK = 16;

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256)
void train_gemm_kernel(GemmArgs g) {
    static_assert(WM * WN == 4, "four wavefronts");
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    __shared__ float As[kBK][BM + 4], Bs[kBK][BN + 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave % WM, wn = wave / WM;
    const long m0 = static_cast<long>(blockIdx.y) * BM, n0 = static_cast<long>(blockIdx.x) * BN;
    const int kbeg = blockIdx.z * g.kslab, kend = min(g.K, kbeg + g.kslab);
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    const bool a_kfast = g.sak == 1, b_kfast = g.sbk == 1;        // walk the contiguous dimension with the lanes
    for (int k0 = kbeg; k0 < kend; k0 += kBK) {
#pragma unroll
        for (int it = 0; it < BM * kBK / 256; ++it) {
            const int i = tid + 256 * it;
            const int k = a_kfast ? i % kBK : i / BM, m = a_kfast ? i / kBK : i % BM;
            const long gm = m0 + m, gk = k0 + k;
            As[k][m] = (gm < g.M && gk < kend) ? g.A[gm * g.sam + gk * g.sak] : 0.0f;
        }
#pragma unroll
        for (int it = 0; it < BN * kBK / 256; ++it) {
            const int i = tid + 256 * it;
            const int k = b_kfast ? i % kBK : i / BN, n = b_kfast ? i / kBK : i % BN;
            const long gn = n0 + n, gk = k0 + k;
            Bs[k][n] = (gn < g.N && gk < kend) ? g.B[gk * g.sbk + gn * g.sbn] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kBK / 2; ++kk) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[2 * kk + (lane >> 5)][(wm * TM + i) * 32 + (lane & 31)];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[2 * kk + (lane >> 5)][(wn * TN + j) * 32 + (lane & 31)];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D: column = lane & 31, row = cd_row(register, lane)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const long n = n0 + (wn * TN + j) * 32 + (lane & 31);
            if (n >= g.N) continue;
            const float bias = (!g.part && g.bias) ? g.bias[n] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = m0 + (wm * TM + i) * 32 + cd_row(r, lane);
                if (m >= g.M) continue;
                float v = acc[i][j][r];
                if (g.part) { g.part[(static_cast<long>(g.z0 + blockIdx.z) * g.M + m) * g.N + n] = v; continue; }
                v += bias;
                if (g.relu) v = fmaxf(v, 0.0f);
                if (g.mask && !(g.mask[m * g.ldm + n] > 0.0f)) v = 0.0f;
                if (n >= g.nsplit) g.C2[m * g.ldc2 + (n - g.nsplit)] = v;
                else g.C[m * g.ldc + (n / g.cq) * g.cs + n % g.cq] = v;
            }
        }
}

// the second stage of the split-K form: out[i] = part[0][i] + part[1][i] + ... in slab order
__global__ __launch_bounds__(256)
void train_reduce_kernel(const float* __restrict__ part, int nz, long mn, float* __restrict__ out) {
    const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= mn) return;
    float s = 0.0f;
    for (int z = 0; z < nz; ++z) s += part[z * mn + i];
    out[i] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// im2col for a 3x3 'same' convolution.  The input element (position b, pixel p, channel c) is in[b * sb + p * sp + c * sc] (channels-last
// activations: sb = 225 C, sp = C, sc = 1; the network's input planes [n][6][225]: sb = 1350, sp = 1, sc = 225); col[row][c * 9 + tap].
__global__ __launch_bounds__(256)
void im2col3x3_kernel(const float* __restrict__ in, long sb, long sp, long sc, int C, int npos, float* __restrict__ col) {
    const long K = 9L * C, total = static_cast<long>(npos) * kPix * K;
    const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= total) return;
    const long row = i / K;
    const int k = static_cast<int>(i - row * K), c = k / 9, tap = k - 9 * c;
    const long b = row / kPix;
    const int p = static_cast<int>(row - b * kPix), y = p / 15 + tap / 3 - 1, x = p % 15 + tap % 3 - 1;
    col[i] = (y >= 0 && y < 15 && x >= 0 && x < 15) ? in[b * sb + (y * 15 + x) * sp + c * sc] : 0.0f;
}

// col2im as a gather: the gradient of input pixel (y, x), channel c is the sum of its at most nine appearances in the columns, taps in order;
// then the ReLU mask of the activation it belongs to (mask and out are channels-last [row][C])
__global__ __launch_bounds__(256)
void col2im3x3_kernel(const float* __restrict__ dcol, int C, int npos, const float* __restrict__ mask, float* __restrict__ out) {
    const long total = static_cast<long>(npos) * kPix * C;
    const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= total) return;
    const long row = i / C;
    const int c = static_cast<int>(i - row * C);
    const long b = row / kPix;
    const int p = static_cast<int>(row - b * kPix), y = p / 15, x = p % 15;
    const long K = 9L * C;
    float s = 0.0f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int yo = y - (tap / 3 - 1), xo = x - (tap % 3 - 1);            // the output pixel whose tap `tap` reads (y, x)
        if (yo >= 0 && yo < 15 && xo >= 0 && xo < 15) s += dcol[(b * kPix + yo * 15 + xo) * K + c * 9 + tap];
    }
    out[i] = mask[i] > 0.0f ? s : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The loss (model_tf.py:77-89), one wavefront per sample: softmax, the 64 -> 1 value output and tanh, the four per-sample terms, and the
// gradients of the logits and of the value path with the 1/n of the batch means folded in.
struct LossArgs {
    const float* logits; const float* hidden; const float* wo; const float* bo;        // [n][225], [n][64], [64], [1]
    const float* values; const float* pi; const float* old_probs;                      // targets (null: forward only), the KL's stored block or null
    int n; float inv_n;
    float* probs_out; float* value_out;                                                // or null
    float* dlogits; float* dz; float* dhid;                                            // [n][225], [n], [n][64]
    float* partial;                                                                    // [n][4]: cross-entropy, squared error, entropy, KL
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
    return v;
}

__global__ __launch_bounds__(256)
void train_loss_kernel(LossArgs a) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.n) return;
    const float* z = a.logits + static_cast<long>(b) * kPix;
    float x[4], p[4], lsm[4];
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < 4; ++e) { const int c = lane + 64 * e; x[e] = c < kPix ? z[c] : -INFINITY; m = fmaxf(m, x[e]); }
    m = wave_max(m);
    float sum = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { p[e] = expf(x[e] - m); sum += p[e]; }
    sum = wave_sum(sum);
    const float log_sum = logf(sum);
#pragma unroll
    for (int e = 0; e < 4; ++e) { lsm[e] = (x[e] - m) - log_sum; p[e] = p[e] / sum; }
    const float h = a.hidden[static_cast<long>(b) * 64 + lane], wo = a.wo[lane];
    const float s = wave_sum(h * wo) + a.bo[0];
    const float v = tanhf(s);
    if (a.probs_out) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const int c = lane + 64 * e; if (c < kPix) a.probs_out[static_cast<long>(b) * kPix + c] = p[e]; }
    }
    if (a.value_out && lane == 0) a.value_out[b] = v;
    if (!a.values) return;
    float t[4], ce = 0.0f, ent = 0.0f, kl = 0.0f, pisum = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = lane + 64 * e;
        if (c < kPix) {
            t[e] = a.pi[static_cast<long>(b) * kPix + c];
            ce -= t[e] * lsm[e];                                   // from the log-softmax: pi has exact zeros where log(probs) may be -inf
            pisum += t[e];
            ent -= p[e] * logf(p[e] + 1e-10f);
            if (a.old_probs) { const float o = a.old_probs[static_cast<long>(b) * kPix + c] + 1e-10f; kl += o * logf(o / (p[e] + 1e-10f)); }
        } else t[e] = 0.0f;
    }
    ce = wave_sum(ce); ent = wave_sum(ent); kl = wave_sum(kl); pisum = wave_sum(pisum);
    const float target = a.values[b], err = v - target;
    // d(mean cross-entropy) / d logit = (p * sum(pi) - pi) / n;  d(mean squared error) / d s = 2 (v - target) (1 - v^2) / n
#pragma unroll
    for (int e = 0; e < 4; ++e) { const int c = lane + 64 * e; if (c < kPix) a.dlogits[static_cast<long>(b) * kPix + c] = (p[e] * pisum - t[e]) * a.inv_n; }
    const float dz = 2.0f * err * (1.0f - v * v) * a.inv_n;
    a.dhid[static_cast<long>(b) * 64 + lane] = h > 0.0f ? dz * wo : 0.0f;
    if (lane == 0) {
        a.dz[b] = dz;
        float* out = a.partial + 4L * b;
        out[0] = ce; out[1] = err * err; out[2] = ent; out[3] = kl;
    }
}

struct Layout { int off[kTensors + 1]; unsigned weight_mask; };

// The batch sums in a fixed order (thread t takes samples t, t + 256, ...; then a tree over the 256 threads), and the L2 term
// 1e-4 * sum(w^2) / 2 over every tensor that is not a bias, summed the same way.  One workgroup.
// metrics: [0] loss = value loss + policy loss + L2, [1] entropy, [2] value loss, [3] policy loss, and with n_metrics = 5 [4] the KL (0 without old_probs)
__global__ __launch_bounds__(256)
void train_metrics_kernel(const float* __restrict__ partial, int n, const float* __restrict__ params, Layout lay, int has_kl, int n_metrics,
                          float* __restrict__ metrics) {
    __shared__ float red[5][256];
    float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int b = threadIdx.x; b < n; b += 256)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += partial[4L * b + q];
    for (int t = 0; t < kTensors; ++t)
        if (lay.weight_mask >> t & 1)
            for (int i = lay.off[t] + threadIdx.x; i < lay.off[t + 1]; i += 256) s[4] += params[i] * params[i];
#pragma unroll
    for (int q = 0; q < 5; ++q) red[q][threadIdx.x] = s[q];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (threadIdx.x < w)
#pragma unroll
            for (int q = 0; q < 5; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float inv = 1.0f / static_cast<float>(n);
        const float policy = red[0][0] * inv, value = red[1][0] * inv, l2 = 1e-4f * (0.5f * red[4][0]);
        metrics[0] = (value + policy) + l2;
        metrics[1] = red[2][0] * inv;
        metrics[2] = value;
        metrics[3] = policy;
        if (n_metrics > 4) metrics[4] = has_kl ? red[3][0] * inv : 0.0f;
    }
}

// TF1's Adam (tf.train.AdamOptimizer) over all sixteen tensors in one launch; weight tensors get the L2 term's gradient 1e-4 w.
// lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) comes from the host.  `delta` keeps the update that was applied: w_new = w - delta, exactly.
// Parameters, gradients and moments are float32; the few operations of one element run in float64, because g + 1e-4 w cancels on some
// elements and a float32 sum then carries the rounding of its operands into m, v and the update (measured: 1.7e-5 of the update on two of
// layer 2's 18 432 weights).  The kernel moves 28 bytes per element either way.
__global__ __launch_bounds__(256)
void train_adam_kernel(float* __restrict__ w, const float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v, float* __restrict__ delta,
                       Layout lay, double lr_t) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= lay.off[kTensors]) return;
    int t = 0;
    while (i >= lay.off[t + 1]) ++t;
    const float wi = w[i];
    const double g = (lay.weight_mask >> t & 1) ? static_cast<double>(grad[i]) + 1e-4 * static_cast<double>(wi) : static_cast<double>(grad[i]);
    const double mi = 0.9 * static_cast<double>(m[i]) + 0.1 * g;
    const double vi = 0.999 * static_cast<double>(v[i]) + 0.001 * (g * g);
    const float d = static_cast<float>(lr_t * (mi / (sqrt(vi) + 1e-8)));
    m[i] = static_cast<float>(mi); v[i] = static_cast<float>(vi); delta[i] = d;
    w[i] = wi - d;
}

// the canonical parameters into a gmk_pvnet's seven device buffers: dst[i] = table[i] ? params[table[i] - 1] : 0 (train_host.h, build_repack_table)
struct RepackArgs { float* dst[kRepackBuffers]; int seg[kRepackBuffers + 1]; };

__global__ __launch_bounds__(256)
void pvnet_repack_kernel(const float* __restrict__ params, const int32_t* __restrict__ table, RepackArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.seg[kRepackBuffers]) return;
    int b = 0;
    while (i >= a.seg[b + 1]) ++b;
    const int32_t id = table[i];
    a.dst[b][i - a.seg[b]] = id ? params[id - 1] : 0.0f;
}

Layout make_layout() {
    Layout l;
    l.weight_mask = 0;
    for (int t = 0; t <= kTensors; ++t) l.off[t] = offset_of(t);
    for (int t = 0; t < kTensors; ++t) if (kIsWeight[t]) l.weight_mask |= 1u << t;
    return l;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------------------
struct gmk_trainer {
    int max_batch = 0;
    long long step = 0;
    float *d_params = nullptr, *d_grads = nullptr, *d_m = nullptr, *d_v = nullptr, *d_delta = nullptr, *d_scratch = nullptr, *d_one = nullptr;
    int32_t* d_table = nullptr;
    size_t seg[kRepackBuffers + 1] = {};
    Scratch sz{};
    // the parts of d_scratch
    float *act1, *act2, *act3, *pflat, *vflat, *logits, *hidden, *probs, *value, *dlogits, *dz, *dhid, *dh6, *dact3, *dact2, *dact1, *col, *splitk, *partial;
    float* param(int t) const { return d_params + offset_of(t); }
    float* grad(float* block, int t) const { return block + offset_of(t); }
};

namespace {

GemmArgs gemm(const float* A, long sam, long sak, const float* B, long sbk, long sbn, int M, int N, int K, float* C, long ldc) {
    GemmArgs g{};
    g.A = A; g.sam = sam; g.sak = sak; g.B = B; g.sbk = sbk; g.sbn = sbn; g.M = M; g.N = N; g.K = K; g.kslab = K > 0 ? K : 1;
    g.C = C; g.ldc = ldc; g.cq = INT_MAX; g.cs = 0; g.nsplit = INT_MAX; g.C2 = nullptr; g.ldc2 = 0;
    return g;
}

// nz: 1 for the direct form; for the split-K form (g.part set) the number of k slabs of g.kslab
int launch_gemm(const GemmArgs& g, int nz, hipStream_t stream) {
    if (g.M <= 0 || g.N <= 0) return GMK_OK;
    const unsigned gy = (g.M + 127) / 128;
    if (g.N > 64) hipLaunchKernelGGL((train_gemm_kernel<2, 2, 2, 2>), dim3((g.N + 127) / 128, gy, nz), dim3(256), 0, stream, g);
    else if (g.N > 32) hipLaunchKernelGGL((train_gemm_kernel<4, 1, 1, 2>), dim3(1, gy, nz), dim3(256), 0, stream, g);
    else hipLaunchKernelGGL((train_gemm_kernel<4, 1, 1, 1>), dim3(1, gy, nz), dim3(256), 0, stream, g);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

#define GMK_TRY(expr) do { const int rc_ = (expr); if (rc_ != GMK_OK) return rc_; } while (0)

int launch_reduce(const float* part, int nz, long mn, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(train_reduce_kernel, dim3(static_cast<unsigned>((mn + 255) / 256)), dim3(256), 0, stream, part, nz, mn, out);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

int reduce_into(const gmk_trainer* T, int nz, long mn, float* out, hipStream_t stream) { return launch_reduce(T->splitk, nz, mn, out, stream); }

// out[N] = the column sums of X[rows][N], K slabs of kKSlabRows rows, added in slab order
int column_sums(const gmk_trainer* T, const float* X, long rows, int N, float* out, hipStream_t stream) {
    GemmArgs g = gemm(T->d_one, 0, 0, X, N, 1, 1, N, static_cast<int>(rows), nullptr, 0);     // A: a single 1.0f, both strides 0
    g.kslab = kKSlabRows; g.part = T->splitk; g.z0 = 0;
    const int nz = static_cast<int>((rows + kKSlabRows - 1) / kKSlabRows);
    GMK_TRY(launch_gemm(g, nz, stream));
    return reduce_into(T, nz, N, out, stream);
}

int launch_im2col(const float* in, long sb, long sp, long sc, int C, int npos, float* col, hipStream_t stream) {
    const long total = static_cast<long>(npos) * kPix * 9 * C;
    hipLaunchKernelGGL(im2col3x3_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, stream, in, sb, sp, sc, C, npos, col);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

int launch_col2im(const float* dcol, int C, int npos, const float* mask, float* out, hipStream_t stream) {
    const long total = static_cast<long>(npos) * kPix * C;
    hipLaunchKernelGGL(col2im3x3_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, stream, dcol, C, npos, mask, out);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

struct ConvLayer { int cin, cout, w, b; };
constexpr ConvLayer kConv[3] = {{6, 32, W1, B1}, {32, 64, W2, B2}, {64, 128, W3, B3}};

// the input of conv layer l for positions pos0 ..: the feature planes (l = 0) or the previous activations
void conv_input(const gmk_trainer* T, const float* d_states, int l, int pos0, const float*& in, long& sb, long& sp, long& sc) {
    if (l == 0) { in = d_states + static_cast<long>(pos0) * 6 * kPix; sb = 6 * kPix; sp = 1; sc = kPix; return; }
    const int C = kConv[l].cin;
    in = (l == 1 ? T->act1 : T->act2) + static_cast<long>(pos0) * kPix * C; sb = static_cast<long>(kPix) * C; sp = C; sc = 1;
}

int run_loss(const gmk_trainer* T, int n, const float* d_values, const float* d_pi, const float* d_old, float* d_value_out, float* d_probs_out,
             hipStream_t stream) {
    LossArgs a{};
    a.logits = T->logits; a.hidden = T->hidden; a.wo = T->param(WOUT); a.bo = T->param(BOUT);
    a.values = d_values; a.pi = d_pi; a.old_probs = d_old; a.n = n; a.inv_n = 1.0f / static_cast<float>(n);
    a.probs_out = d_probs_out; a.value_out = d_value_out;
    a.dlogits = T->dlogits; a.dz = T->dz; a.dhid = T->dhid; a.partial = T->partial;
    hipLaunchKernelGGL(train_loss_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, a);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

// the forward pass up to the logits and the hidden units, every activation kept
int run_forward(const gmk_trainer* T, const float* d_states, int n, hipStream_t stream) {
    float* acts[3] = {T->act1, T->act2, T->act3};
    for (int l = 0; l < 3; ++l) {
        const int K = 9 * kConv[l].cin, N = kConv[l].cout;
        for (int pos0 = 0; pos0 < n; pos0 += kSlabPos) {
            const int ns = std::min(kSlabPos, n - pos0), rows = ns * kPix;
            const float* in; long sb, sp, sc;
            conv_input(T, d_states, l, pos0, in, sb, sp, sc);
            GMK_TRY(launch_im2col(in, sb, sp, sc, kConv[l].cin, ns, T->col, stream));
            GemmArgs g = gemm(T->col, K, 1, T->param(kConv[l].w), 1, K, rows, N, K, acts[l] + static_cast<long>(pos0) * kPix * N, N);
            g.bias = T->param(kConv[l].b); g.relu = 1;
            GMK_TRY(launch_gemm(g, 1, stream));
        }
    }
    const int rows = n * kPix;
    {   // the two 1x1 heads: columns 0..3 -> pflat [n][900] = [rows][4], columns 4..5 -> vflat [n][450] = [rows][2]
        GemmArgs g = gemm(T->act3, 128, 1, T->param(WPC), 1, 128, rows, 6, 128, T->pflat, 4);
        g.bias = T->param(BPC); g.relu = 1; g.nsplit = 4; g.C2 = T->vflat; g.ldc2 = 2;
        GMK_TRY(launch_gemm(g, 1, stream));
    }
    {
        GemmArgs g = gemm(T->pflat, 900, 1, T->param(WPD), 1, 900, n, kPix, 900, T->logits, kPix);
        g.bias = T->param(BPD);
        GMK_TRY(launch_gemm(g, 1, stream));
    }
    {
        GemmArgs g = gemm(T->vflat, 450, 1, T->param(WHID), 1, 450, n, 64, 450, T->hidden, 64);
        g.bias = T->param(BHID); g.relu = 1;
        GMK_TRY(launch_gemm(g, 1, stream));
    }
    return GMK_OK;
}

// the backward pass: the gradients of the data loss (no L2 term) into `G`, a block in the parameters' order
int run_backward(const gmk_trainer* T, const float* d_states, int n, float* G, hipStream_t stream) {
    const int rows = n * kPix;
    // ---- value output (64 -> 1) and the dense layers: K = n, one k slab, so the direct form ----
    GMK_TRY(launch_gemm(gemm(T->hidden, 1, 64, T->dz, 1, 0, 64, 1, n, T->grad(G, WOUT), 1), 1, stream));
    GMK_TRY(column_sums(T, T->dz, n, 1, T->grad(G, BOUT), stream));
    GMK_TRY(launch_gemm(gemm(T->dhid, 1, 64, T->vflat, 450, 1, 64, 450, n, T->grad(G, WHID), 450), 1, stream));
    GMK_TRY(column_sums(T, T->dhid, n, 64, T->grad(G, BHID), stream));
    GMK_TRY(launch_gemm(gemm(T->dlogits, 1, kPix, T->pflat, 900, 1, kPix, 900, n, T->grad(G, WPD), 900), 1, stream));
    GMK_TRY(column_sums(T, T->dlogits, n, kPix, T->grad(G, BPD), stream));
    {   // the heads' pre-activation gradients, side by side as dh6 [rows][6]: policy columns 0..3, value columns 4..5
        GemmArgs g = gemm(T->dlogits, kPix, 1, T->param(WPD), 900, 1, n, 900, kPix, T->dh6, 6L * kPix);
        g.cq = 4; g.cs = 6; g.mask = T->pflat; g.ldm = 900;
        GMK_TRY(launch_gemm(g, 1, stream));
        GemmArgs h = gemm(T->dhid, 64, 1, T->param(WHID), 450, 1, n, 450, 64, T->dh6 + 4, 6L * kPix);
        h.cq = 2; h.cs = 6; h.mask = T->vflat; h.ldm = 450;
        GMK_TRY(launch_gemm(h, 1, stream));
    }
    {   // dW6 [6][128] = dh6^T . act3 (wp | wv are adjacent in the block, so are their biases)
        GemmArgs g = gemm(T->dh6, 1, 6, T->act3, 128, 1, 6, 128, rows, nullptr, 0);
        g.kslab = kKSlabRows; g.part = T->splitk; g.z0 = 0;
        const int nz = (rows + kKSlabRows - 1) / kKSlabRows;
        GMK_TRY(launch_gemm(g, nz, stream));
        GMK_TRY(reduce_into(T, nz, 6 * 128, T->grad(G, WPC), stream));
        GMK_TRY(column_sums(T, T->dh6, rows, 6, T->grad(G, BPC), stream));
        GemmArgs d = gemm(T->dh6, 6, 1, T->param(WPC), 128, 1, rows, 128, 6, T->dact3, 128);
        d.mask = T->act3; d.ldm = 128;
        GMK_TRY(launch_gemm(d, 1, stream));
    }
    // ---- the 3x3 layers, last first: per slab of positions the columns again, the weight gradient's k slabs, the input's gradient ----
    float* dacts[3] = {T->dact1, T->dact2, T->dact3};
    for (int l = 2; l >= 0; --l) {
        const int cin = kConv[l].cin, K = 9 * cin, N = kConv[l].cout;
        int z = 0;
        for (int pos0 = 0; pos0 < n; pos0 += kSlabPos) {
            const int ns = std::min(kSlabPos, n - pos0), srows = ns * kPix, nz = (srows + kKSlabRows - 1) / kKSlabRows;
            const float* in; long sb, sp, sc;
            conv_input(T, d_states, l, pos0, in, sb, sp, sc);
            const float* dy = dacts[l] + static_cast<long>(pos0) * kPix * N;
            GMK_TRY(launch_im2col(in, sb, sp, sc, cin, ns, T->col, stream));
            GemmArgs g = gemm(dy, 1, N, T->col, K, 1, N, K, srows, nullptr, 0);
            g.kslab = kKSlabRows; g.part = T->splitk; g.z0 = z;
            GMK_TRY(launch_gemm(g, nz, stream));
            z += nz;
            if (l > 0) {   // dcol takes the columns' place, then the gather
                GMK_TRY(launch_gemm(gemm(dy, N, 1, T->param(kConv[l].w), K, 1, srows, K, N, T->col, K), 1, stream));
                const long at = static_cast<long>(pos0) * kPix * cin;
                GMK_TRY(launch_col2im(T->col, cin, ns, (l == 1 ? T->act1 : T->act2) + at, dacts[l - 1] + at, stream));
            }
        }
        GMK_TRY(reduce_into(T, z, static_cast<long>(N) * K, T->grad(G, kConv[l].w), stream));
        GMK_TRY(column_sums(T, dacts[l], rows, N, T->grad(G, kConv[l].b), stream));
    }
    return GMK_OK;
}

int run_metrics(const gmk_trainer* T, int n, bool has_kl, int n_metrics, float* d_metrics, hipStream_t stream) {
    hipLaunchKernelGGL(train_metrics_kernel, dim3(1), dim3(256), 0, stream, T->partial, n, T->d_params, make_layout(), has_kl ? 1 : 0, n_metrics, d_metrics);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

bool not_ready() {
    if (gmk::device_state().ready) return false;
    gmk::set_error("gmk_init has not succeeded (no CPU fallback)");
    return true;
}

}  // namespace

extern "C" int gmk_train_destroy(gmk_trainer* T) {
    if (!T) return GMK_OK;
    (void)hipFree(T->d_params); (void)hipFree(T->d_grads); (void)hipFree(T->d_m); (void)hipFree(T->d_v); (void)hipFree(T->d_delta);
    (void)hipFree(T->d_table); (void)hipFree(T->d_one); (void)gmk::device_free(T->d_scratch);
    delete T;
    return GMK_OK;
}

namespace {
int set_params(gmk_trainer* T, const float* const* h_arrays) {
    if (not_ready()) return GMK_ERR_STATE;
    if (!T || !h_arrays) { gmk::set_error("gmk_train_set_params: bad arguments"); return GMK_ERR_ARG; }
    std::vector<float> block(kParams);
    for (int a = 0; a < kTensors; ++a) {
        if (!h_arrays[a]) { gmk::set_error("gmk_train_set_params: array %d is NULL", a); return GMK_ERR_ARG; }
        std::memcpy(block.data() + offset_of(kArgTensor[a]), h_arrays[a], static_cast<size_t>(kSizes[kArgTensor[a]]) * 4);
    }
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(T->d_params, block.data(), static_cast<size_t>(kParams) * 4, hipMemcpyHostToDevice));
    return GMK_OK;
}
}  // namespace

#define GMK_TRAIN_16(T_) T_ h_w1, T_ h_b1, T_ h_w2, T_ h_b2, T_ h_w3, T_ h_b3, T_ h_w_policy_conv, T_ h_b_policy_conv, T_ h_w_value_conv, T_ h_b_value_conv, \
                         T_ h_w_policy, T_ h_b_policy, T_ h_w_hidden, T_ h_b_hidden, T_ h_w_out, T_ h_b_out
#define GMK_TRAIN_16_LIST {h_w1, h_b1, h_w2, h_b2, h_w3, h_b3, h_w_policy_conv, h_b_policy_conv, h_w_value_conv, h_b_value_conv, h_w_policy, h_b_policy, h_w_hidden, h_b_hidden, h_w_out, h_b_out}

extern "C" int gmk_train_set_params(gmk_trainer* T, GMK_TRAIN_16(const float*)) {
    const float* const h_arrays[kTensors] = GMK_TRAIN_16_LIST;
    return set_params(T, h_arrays);
}

extern "C" int gmk_train_params(gmk_trainer* T, GMK_TRAIN_16(float*)) {
    float* const h_arrays[kTensors] = GMK_TRAIN_16_LIST;
    if (not_ready()) return GMK_ERR_STATE;
    if (!T) { gmk::set_error("gmk_train_params: bad arguments"); return GMK_ERR_ARG; }
    for (int a = 0; a < kTensors; ++a) if (!h_arrays[a]) { gmk::set_error("gmk_train_params: array %d is NULL", a); return GMK_ERR_ARG; }
    std::vector<float> block(kParams);
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(block.data(), T->d_params, static_cast<size_t>(kParams) * 4, hipMemcpyDeviceToHost));
    for (int a = 0; a < kTensors; ++a) std::memcpy(h_arrays[a], block.data() + offset_of(kArgTensor[a]), static_cast<size_t>(kSizes[kArgTensor[a]]) * 4);
    return GMK_OK;
}

extern "C" int gmk_train_create(GMK_TRAIN_16(const float*), int max_batch, gmk_trainer** out) {
    const float* const h_arrays[kTensors] = GMK_TRAIN_16_LIST;
    if (not_ready()) return GMK_ERR_STATE;
    if (!out || !valid_max_batch(max_batch)) { gmk::set_error("gmk_train_create: bad arguments (max_batch in [1, %d])", kMaxBatchLimit); return GMK_ERR_ARG; }
    for (int a = 0; a < kTensors; ++a) if (!h_arrays[a]) { gmk::set_error("gmk_train_create: array %d is NULL", a); return GMK_ERR_ARG; }
    std::vector<int32_t> table;
    gmk_trainer* T = new gmk_trainer;
    T->max_batch = max_batch;
    if (!build_repack_table(table, T->seg)) { delete T; gmk::set_error("gmk_train_create: the packers are not pure gathers"); return GMK_ERR_STATE; }
    T->sz = scratch_floats(max_batch);
    const size_t pb = static_cast<size_t>(kParams) * 4;
    const float one = 1.0f;                        // the A operand of the column sums
    const bool ok = hipMalloc(&T->d_params, pb) == hipSuccess && hipMalloc(&T->d_grads, pb) == hipSuccess && hipMalloc(&T->d_m, pb) == hipSuccess &&
                    hipMalloc(&T->d_v, pb) == hipSuccess && hipMalloc(&T->d_delta, pb) == hipSuccess && hipMalloc(&T->d_one, 4) == hipSuccess && hipMemcpy(T->d_one, &one, 4, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMalloc(&T->d_table, table.size() * 4) == hipSuccess && gmk::device_malloc(&T->d_scratch, T->sz.total * 4) == hipSuccess &&
                    hipMemset(T->d_m, 0, pb) == hipSuccess && hipMemset(T->d_v, 0, pb) == hipSuccess && hipMemset(T->d_delta, 0, pb) == hipSuccess &&
                    hipMemset(T->d_grads, 0, pb) == hipSuccess &&
                    hipMemcpy(T->d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { gmk_train_destroy(T); gmk::set_error("gmk_train_create: device allocation or copy failed"); return GMK_ERR_HIP; }
    float* p = T->d_scratch;
    const Scratch& s = T->sz;
    auto take = [&p](size_t floats) { float* q = p; p += floats; return q; };
    T->act1 = take(s.act1); T->act2 = take(s.act2); T->act3 = take(s.act3); T->pflat = take(s.pflat); T->vflat = take(s.vflat);
    T->logits = take(s.logits); T->hidden = take(s.hidden); T->probs = take(s.probs); T->value = take(s.value);
    T->dlogits = take(s.dlogits); T->dz = take(s.dz); T->dhid = take(s.dhid); T->dh6 = take(s.dh6);
    T->dact3 = take(s.dact3); T->dact2 = take(s.dact2); T->dact1 = take(s.dact1); T->col = take(s.col); T->splitk = take(s.splitk); T->partial = take(s.partial);
    const int rc = set_params(T, h_arrays);
    if (rc != GMK_OK) { gmk_train_destroy(T); return rc; }
    *out = T;
    return GMK_OK;
}

extern "C" int gmk_train_forward(gmk_trainer* T, const float* d_states, int n, float* d_value, float* d_probs, void* stream) {
    if (not_ready()) return GMK_ERR_STATE;
    const void* req[3] = {d_states, d_value, d_probs};
    if (!T || !valid_batch(n, T->max_batch, req, 3, nullptr, 0)) { gmk::set_error("gmk_train_forward: bad arguments (n in [1, max_batch], aligned device pointers)"); return GMK_ERR_ARG; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    GMK_TRY(run_forward(T, d_states, n, st));
    return run_loss(T, n, nullptr, nullptr, nullptr, d_value, d_probs, st);
}

extern "C" int gmk_train_grads(gmk_trainer* T, const float* d_states, const float* d_values, const float* d_pi, int n, float* d_grads, float* d_metrics,
                               void* stream) {
    if (not_ready()) return GMK_ERR_STATE;
    const void* req[5] = {d_states, d_values, d_pi, d_grads, d_metrics};
    if (!T || !valid_batch(n, T->max_batch, req, 5, nullptr, 0)) { gmk::set_error("gmk_train_grads: bad arguments (n in [1, max_batch], aligned device pointers)"); return GMK_ERR_ARG; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    GMK_TRY(run_forward(T, d_states, n, st));
    GMK_TRY(run_loss(T, n, d_values, d_pi, nullptr, nullptr, nullptr, st));
    GMK_TRY(run_metrics(T, n, false, 4, d_metrics, st));
    return run_backward(T, d_states, n, d_grads, st);
}

extern "C" int gmk_train_step(gmk_trainer* T, const float* d_states, const float* d_values, const float* d_pi, int n, float lr, const float* d_old_probs,
                              float* d_probs_out, float* d_metrics, void* stream) {
    if (not_ready()) return GMK_ERR_STATE;
    const void* req[4] = {d_states, d_values, d_pi, d_metrics};
    const void* opt[2] = {d_old_probs, d_probs_out};
    if (!T || !valid_batch(n, T->max_batch, req, 4, opt, 2) || !(lr >= 0.0f)) { gmk::set_error("gmk_train_step: bad arguments (n in [1, max_batch], aligned device pointers, lr >= 0)"); return GMK_ERR_ARG; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    GMK_TRY(run_forward(T, d_states, n, st));
    GMK_TRY(run_loss(T, n, d_values, d_pi, d_old_probs, nullptr, d_probs_out, st));       // the probabilities from BEFORE the update
    GMK_TRY(run_metrics(T, n, d_old_probs != nullptr, 5, d_metrics, st));
    GMK_TRY(run_backward(T, d_states, n, T->d_grads, st));
    T->step += 1;
    const double lr_t = adam_lr_t(static_cast<double>(lr), T->step);
    hipLaunchKernelGGL(train_adam_kernel, dim3((kParams + 255) / 256), dim3(256), 0, st, T->d_params, T->d_grads, T->d_m, T->d_v, T->d_delta, make_layout(), lr_t);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_train_export(gmk_trainer* T, gmk_pvnet* net, void* stream) {
    if (not_ready()) return GMK_ERR_STATE;
    if (!T || !net) { gmk::set_error("gmk_train_export: bad arguments"); return GMK_ERR_ARG; }
    if (!net->has_dense || !net->d_wp || !net->d_dense) { gmk::set_error("gmk_train_export: the network has no dense layers yet (gmk_pvnet_set_dense)"); return GMK_ERR_STATE; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    RepackArgs a;
    float* dst[kRepackBuffers] = {net->d_w1, net->d_w2, net->d_w3, net->d_wh, net->d_b, net->d_wp, net->d_dense};
    for (int b = 0; b < kRepackBuffers; ++b) a.dst[b] = dst[b];
    for (int b = 0; b <= kRepackBuffers; ++b) a.seg[b] = static_cast<int>(T->seg[b]);
    hipLaunchKernelGGL(pvnet_repack_kernel, dim3((a.seg[kRepackBuffers] + 255) / 256), dim3(256), 0, st, T->d_params, T->d_table, a);
    GMK_HIP_CHECK(hipGetLastError());
    if (net->precision == GMK_PVNET_BF16) GMK_TRY(gmk::pvnet_bf16_refresh(net, stream));      // the bf16 trunk streams its own roundings of these weights
    // the output bias is a by-value kernel argument of K9's dense kernel, so it lives in the handle on the host: four bytes are read back here
    float b_out = 0.0f;
    GMK_HIP_CHECK(hipMemcpyAsync(&b_out, T->param(BOUT), sizeof(float), hipMemcpyDeviceToHost, st));
    GMK_HIP_CHECK(hipStreamSynchronize(st));
    net->b_out = b_out;
    return GMK_OK;
}

extern "C" int gmk_train_get_block(gmk_trainer* T, int which, float* h_block) {
    if (not_ready()) return GMK_ERR_STATE;
    if (!T || !h_block || which < 0 || which > 3) { gmk::set_error("gmk_train_get_block: bad arguments"); return GMK_ERR_ARG; }
    const float* src[4] = {T->d_params, T->d_m, T->d_v, T->d_delta};
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(h_block, src[which], static_cast<size_t>(kParams) * 4, hipMemcpyDeviceToHost));
    return GMK_OK;
}

extern "C" int gmk_train_set_block(gmk_trainer* T, int which, const float* h_block) {
    if (not_ready()) return GMK_ERR_STATE;
    if (!T || !h_block || which < 0 || which > 2) { gmk::set_error("gmk_train_set_block: bad arguments"); return GMK_ERR_ARG; }
    float* dst[3] = {T->d_params, T->d_m, T->d_v};
    GMK_HIP_CHECK(hipDeviceSynchronize());
    GMK_HIP_CHECK(hipMemcpy(dst[which], h_block, static_cast<size_t>(kParams) * 4, hipMemcpyHostToDevice));
    return GMK_OK;
}

extern "C" int gmk_train_set_step_count(gmk_trainer* T, int64_t step) {
    if (not_ready()) return GMK_ERR_STATE;
    if (!T || step < 0) { gmk::set_error("gmk_train_set_step_count: bad arguments"); return GMK_ERR_ARG; }
    T->step = step;
    return GMK_OK;
}

extern "C" int gmk_train_info(gmk_trainer* T, int64_t* h_step, int64_t* h_scratch_bytes, int32_t* h_max_batch, int32_t* h_param_floats) {
    if (not_ready()) return GMK_ERR_STATE;
    if (!T) { gmk::set_error("gmk_train_info: bad arguments"); return GMK_ERR_ARG; }
    if (h_step) *h_step = T->step;
    if (h_scratch_bytes) *h_scratch_bytes = static_cast<int64_t>(T->sz.total) * 4;
    if (h_max_batch) *h_max_batch = T->max_batch;
    if (h_param_floats) *h_param_floats = kParams;
    return GMK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The kernels on their own (include/gomoku_hip.h): the trainer's launchers on the caller's operands, after train_host.h has held every index
// the kernel can form to the extents the caller states.  Nothing is launched for a descriptor that does not fit.
extern "C" int gmk_train_kernel_gemm(const gmk_train_gemm_desc* d, void* stream) {
    if (not_ready()) return GMK_ERR_STATE;
    if (!d) { gmk::set_error("gmk_train_kernel_gemm: desc is NULL"); return GMK_ERR_ARG; }
    if (const char* bad = gemm_fits(*d)) { gmk::set_error("gmk_train_kernel_gemm: refused, field %s (addressing must stay inside the stated extents)", bad); return GMK_ERR_ARG; }
    GemmArgs g = gemm(d->A, d->sam, d->sak, d->B, d->sbk, d->sbn, d->M, d->N, d->K, d->C, d->ldc);
    g.kslab = d->kslab; g.part = d->part; g.z0 = d->z0;
    g.cq = d->cq; g.cs = d->cs; g.nsplit = d->nsplit; g.C2 = d->C2; g.ldc2 = d->ldc2;
    g.bias = d->bias; g.relu = d->relu; g.mask = d->mask; g.ldm = d->ldm;
    return launch_gemm(g, d->nz, static_cast<hipStream_t>(stream));
}

extern "C" int gmk_train_kernel_reduce(const float* part, int nz, int64_t mn, float* out, void* stream) {
    if (not_ready()) return GMK_ERR_STATE;
    if (const char* bad = reduce_fits(part, nz, mn, out)) { gmk::set_error("gmk_train_kernel_reduce: refused, argument %s", bad); return GMK_ERR_ARG; }
    return launch_reduce(part, nz, static_cast<long>(mn), out, static_cast<hipStream_t>(stream));
}

extern "C" int gmk_train_kernel_im2col(const float* in, int64_t in_floats, int64_t sb, int64_t sp, int64_t sc, int C, int npos, float* col, void* stream) {
    if (not_ready()) return GMK_ERR_STATE;
    if (const char* bad = im2col_fits(in, in_floats, sb, sp, sc, C, npos, col)) { gmk::set_error("gmk_train_kernel_im2col: refused, argument %s", bad); return GMK_ERR_ARG; }
    return launch_im2col(in, static_cast<long>(sb), static_cast<long>(sp), static_cast<long>(sc), C, npos, col, static_cast<hipStream_t>(stream));
}

extern "C" int gmk_train_kernel_col2im(const float* dcol, int C, int npos, const float* mask, float* out, void* stream) {
    if (not_ready()) return GMK_ERR_STATE;
    if (const char* bad = col2im_fits(dcol, C, npos, mask, out)) { gmk::set_error("gmk_train_kernel_col2im: refused, argument %s", bad); return GMK_ERR_ARG; }
    return launch_col2im(dcol, C, npos, mask, out, static_cast<hipStream_t>(stream));
}
