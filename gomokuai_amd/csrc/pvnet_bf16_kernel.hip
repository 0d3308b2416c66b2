// pvnet_bf16_kernel.hip -- "K9 in bf16": the network's convolutional trunk on v_mfma_f32_32x32x16_bf16, opt-in per handle
// (gmk_pvnet_set_precision).  The numeric contract is in include/gomoku_hip.h; the float32 kernels of pvnet_kernel.hip are untouched and stay
// the default.  pvnet_dense_kernel runs behind either trunk on float32 rows.
//
// Formulation: as in the float32 kernel every layer is Out^T[cout][pixel] = sum_k W^T[cout][k] Act[k][pixel], one workgroup (4 wavefronts) per
// position at a time, activations in LDS only.  What the bf16 instruction changes is the layout: a B operand is 8 consecutive k per lane
// (lane l: column l & 31, k = 8 (l >> 5) + e), so activations live in LDS as act[17 x 17 pixel][channel] in bf16 with the zero border.  A
// k-step of 16 is one tap and 16 channels, a tap is an address offset, and a lane's B fragment is ONE ds_read_b128 at
// pixel * stride + 32 * channel group + 16 * (l >> 5).
//   * Pixel strides are the row + 16 bytes: 80 bytes for 32 channels, 144 for 64 (5 and 9 sixteen-byte slots: odd, so the 16 lanes that a
//     ds_read_b128 serves together, consecutive pixels, fall into 16 different slots of the 256-byte bank row; 64 and 128 would put them on 4 or 2).
//   * A operands (weights) are packed in lane order (pvnet_bf16_pack.h) and stream from L2, one 16-byte load per lane and k-step, fetched two
//     steps ahead; a wave holds its A fragment across all its pixel tiles (8 in layer 3: one load and eight LDS reads per eight MFMAs).
//   * C/D has the pixel on the lane and 16 output channels in registers, four runs of four consecutive channels: after ReLU a lane rounds them
//     to bf16 and writes four 8-byte pieces into the next layer's image.
//   * Layer 1 (6 channels, K = 54): the input image is [pixel][8 channels] (16 bytes, channels 6 and 7 zero) and a k-step is TWO taps, one per
//     lane half; five steps, the tenth tap has zero weights and reads the image's zero corner.
//   * 225 pixels are eight tiles of 32; the eighth holds the corner (14, 14) alone, its other lanes read that pixel's neighbourhood and are
//     never stored.
//   * The 1x1 heads take the layer-3 accumulators as B operands directly (registers 8 s .. 8 s + 7 after ReLU and v_cvt_pk_bf16_f32 are the
//     fragment of k-step s; the head weights are packed in that k order): two MFMAs per pixel tile, rows 0..5 of the result are the heads.
//     Each wave holds 32 of the 128 channels, so the four partial sums go through LDS and are added in wave order, then bias and ReLU.
// Wave w owns output channels [32 w, 32 w + 32) of layer 3 for all eight pixel tiles (128 accumulator registers), channel tile w & 1 and pixel
// tiles 4 (w >> 1) .. + 3 of layer 2, pixel tiles 2 w, 2 w + 1 of layer 1.
#include <algorithm>
#include <vector>

#include "capi_common.h"
#include "pvnet_pack.h"
#include "pvnet_bf16_pack.h"

namespace {

namespace Q = gmk::bf16pack;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kPix = 225, kPad = 289, kTiles = 8, kHeadRows = 6;
constexpr int kStrideIn = 16, kStride1 = 80, kStride2 = 144;                 // bytes per pixel of the three images
// LDS (bytes): input image | layer-1 activations | layer-2 activations | the four waves' partial head sums [4][256 pixels][8 rows] f32 | biases b1 b2 b3
constexpr int oIn = 0, oAct1 = oIn + kPad * kStrideIn, oAct2 = oAct1 + kPad * kStride1, oPart = oAct2 + kPad * kStride2, oBias = oPart + 4 * 256 * 8 * 4,
              kLdsBytes = oBias + (32 + 64 + 128) * 4;
static_assert(oAct1 % 16 == 0 && oAct2 % 16 == 0 && oPart % 16 == 0 && oBias % 16 == 0, "16-byte reads and writes");
static_assert(kLdsBytes <= 160 * 1024, "LDS of one CU");

struct PvBf16Params {
    const float* states;                         // [n][6][225]
    int n;
    const uint4* q;                              // the bf16 weights, pvnet_bf16_pack.h, as 16-byte fragments
    const float* b;                              // b1 | b2 | b3 | head biases [6]
    float* pflat;                                // [n][900]
    float* vflat;                                // [n][450]
};

__device__ __forceinline__ int padded_index(int p) { return (p / 15 + 1) * 17 + (p % 15) + 1; }
__device__ __forceinline__ int cd_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {              // two floats -> two bf16, round to nearest even (v_cvt_pk_bf16_f32)
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// One convolution layer with CIN = 16 * PER_TAP input channels for NP pixel tiles and one tile of 32 output channels.  `in`: the input image,
// base[t] = (padded_index(pixel) - 18) * STRIDE + 16 * (lane >> 5): tap (ky, kx) of channel group g adds (17 ky + kx) * STRIDE + 32 g.
// `w`: this lane's fragment of the tile's first k-step; the next step's is 64 fragments on.
template <int PER_TAP, int STRIDE, int NP>
__device__ __forceinline__ void conv_bf16(const char* in, const uint4* __restrict__ w, const uint32_t (&base)[NP], f32x16 (&acc)[NP]) {
    constexpr int STEPS = 9 * PER_TAP;
    uint4 a[3];
    a[0] = w[0];
    a[1] = w[64];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int tap = s / PER_TAP, off = ((tap / 3) * 17 + tap % 3) * STRIDE + 32 * (s % PER_TAP);
        if (s + 2 < STEPS) a[(s + 2) % 3] = w[(s + 2) * 64];
        bf16x8 b[NP];
#pragma unroll
        for (int t = 0; t < NP; ++t) b[t] = *reinterpret_cast<const bf16x8*>(in + base[t] + off);
        const bf16x8 av = __builtin_bit_cast(bf16x8, a[s % 3]);
#pragma unroll
        for (int t = 0; t < NP; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b[t], acc[t], 0, 0, 0);
    }
}

// ReLU, rounding to bf16 and the store of a C/D tile (32 channels from cout0 x 32 pixels) into the next layer's image; valid pixels only
template <int STRIDE>
__device__ __forceinline__ void store_tile(char* out, const f32x16& acc, int cout0, int tile, int lane) {
    const int p = tile * 32 + (lane & 31);
    if (p >= kPix) return;
    char* dst = out + padded_index(p) * STRIDE + (cout0 + 4 * (lane >> 5)) * 2;
#pragma unroll
    for (int g = 0; g < 4; ++g) {                                            // registers 4 g .. 4 g + 3 = channels cout0 + 8 g + 4 (lane >> 5) + 0 .. 3
        uint2 v;
        v.x = pack2(fmaxf(acc[4 * g], 0.0f), fmaxf(acc[4 * g + 1], 0.0f));
        v.y = pack2(fmaxf(acc[4 * g + 2], 0.0f), fmaxf(acc[4 * g + 3], 0.0f));
        *reinterpret_cast<uint2*>(dst + 16 * g) = v;
    }
}

__global__ __launch_bounds__(256)
void pvnet_bf16_trunk_kernel(PvBf16Params prm) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5;
    float* lds_f = reinterpret_cast<float*>(lds);
    for (int i = threadIdx.x; i < kLdsBytes / 4; i += 256) lds_f[i] = i >= oBias / 4 ? prm.b[i - oBias / 4] : 0.0f;      // the zero borders are written once
    // the pixel a lane reads for tile t (past the image: pixel 224's neighbourhood, a column that is never stored)
    auto tile_pixel = [lane](int t) { return padded_index(min(t * 32 + (lane & 31), kPix - 1)) - 18; };

    // the input planes of a position travel through registers: fetched while the previous position computes.  Thread p < 225 owns pixel p.
    float in_next[6];
    auto fetch_input = [&](int img) {
        const float* src = prm.states + static_cast<size_t>(min(img, prm.n - 1)) * 6 * kPix;
#pragma unroll
        for (int c = 0; c < 6; ++c) in_next[c] = threadIdx.x < kPix ? src[c * kPix + threadIdx.x] : 0.0f;
    };
    auto store_input = [&]() {
        if (threadIdx.x < kPix) {
            uint32_t h[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) h[c] = Q::rne_bits(__float_as_uint(in_next[c]));
            const uint4 v = {h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), 0u};
            *reinterpret_cast<uint4*>(lds + oIn + padded_index(threadIdx.x) * kStrideIn) = v;
        }
    };
    // the head weights' two A fragments stay in registers; every other weight streams per position
    const bf16x8 ah0 = __builtin_bit_cast(bf16x8, prm.q[Q::kQh / 8 + (wave * 2 + 0) * 64 + lane]);
    const bf16x8 ah1 = __builtin_bit_cast(bf16x8, prm.q[Q::kQh / 8 + (wave * 2 + 1) * 64 + lane]);
    const uint4* w1 = prm.q + Q::kQ1 / 8 + lane;
    const uint4* w2 = prm.q + Q::kQ2 / 8 + (wave & 1) * 18 * 64 + lane;
    const uint4* w3 = prm.q + Q::kQ3 / 8 + wave * 36 * 64 + lane;
    const float* bias = reinterpret_cast<const float*>(lds + oBias);
    const float* bh = prm.b + 224;

    fetch_input(blockIdx.x);
    for (int img = blockIdx.x; img < prm.n; img += gridDim.x) {
        __syncthreads();                                                      // the first position: the zeroed LDS; later ones: nothing reads the old image any more
        store_input();
        fetch_input(img + gridDim.x);
        __syncthreads();

        // ---- layer 1: 6 -> 32, wave w takes pixel tiles 2 w, 2 w + 1; k-step s = taps 2 s (lower lane half) and 2 s + 1 (upper) ----
        {
            f32x16 acc[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = bias[cd_row(r, lane)];
            const uint32_t base[2] = {static_cast<uint32_t>(oIn + tile_pixel(2 * wave) * kStrideIn), static_cast<uint32_t>(oIn + tile_pixel(2 * wave + 1) * kStrideIn)};
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const int t0 = 2 * s, t1 = 2 * s + 1;
                const int off0 = ((t0 / 3) * 17 + t0 % 3) * kStrideIn, off1 = ((t1 / 3) * 17 + t1 % 3) * kStrideIn;
                const bf16x8 av = __builtin_bit_cast(bf16x8, w1[s * 64]);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    // the tenth tap does not exist: its weights are zero and it reads padded pixel 0, which is always zero
                    const uint32_t at = half ? (t1 < 9 ? base[t] + off1 : static_cast<uint32_t>(oIn)) : base[t] + off0;
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, *reinterpret_cast<const bf16x8*>(lds + at), acc[t], 0, 0, 0);
                }
            }
            store_tile<kStride1>(lds + oAct1, acc[0], 0, 2 * wave, lane);
            store_tile<kStride1>(lds + oAct1, acc[1], 0, 2 * wave + 1, lane);
        }
        __syncthreads();

        // ---- layer 2: 32 -> 64, wave w takes channel tile w & 1 and pixel tiles 4 (w >> 1) .. + 3 ----
        {
            const int ct = wave & 1, t0 = 4 * (wave >> 1);
            f32x16 acc[4];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = acc[2][r] = acc[3][r] = bias[32 + 32 * ct + cd_row(r, lane)];
            uint32_t base[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) base[t] = static_cast<uint32_t>(oAct1 + tile_pixel(t0 + t) * kStride1 + 16 * half);
            conv_bf16<2, kStride1, 4>(lds, w2, base, acc);
#pragma unroll
            for (int t = 0; t < 4; ++t) store_tile<kStride2>(lds + oAct2, acc[t], 32 * ct, t0 + t, lane);
        }
        __syncthreads();

        // ---- layer 3: 64 -> 128, wave w takes channel tile w and all eight pixel tiles; its output never leaves the registers ----
        f32x16 acc[kTiles];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float b3 = bias[96 + 32 * wave + cd_row(r, lane)];
#pragma unroll
            for (int t = 0; t < kTiles; ++t) acc[t][r] = b3;
        }
        {
            uint32_t base[kTiles];
#pragma unroll
            for (int t = 0; t < kTiles; ++t) base[t] = static_cast<uint32_t>(oAct2 + tile_pixel(t) * kStride2 + 16 * half);
            conv_bf16<4, kStride2, kTiles>(lds, w3, base, acc);
        }

        // ---- heads: Out6^T[j][pixel] = sum_c W6^T[j][c] relu(Out3^T[c][pixel]): the accumulator tile is the B operand, registers 8 s .. 8 s + 7
        //      of k-step s.  Rows 0..3 of the result (policy) are registers 0..3 of the lower lane half, rows 4..5 (value) registers 0..1 of the
        //      upper: each lane writes its four as 16 bytes into part[wave][pixel][4 half ..] ----
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
            uint4 x[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                x[s].x = pack2(fmaxf(acc[t][8 * s + 0], 0.0f), fmaxf(acc[t][8 * s + 1], 0.0f));
                x[s].y = pack2(fmaxf(acc[t][8 * s + 2], 0.0f), fmaxf(acc[t][8 * s + 3], 0.0f));
                x[s].z = pack2(fmaxf(acc[t][8 * s + 4], 0.0f), fmaxf(acc[t][8 * s + 5], 0.0f));
                x[s].w = pack2(fmaxf(acc[t][8 * s + 6], 0.0f), fmaxf(acc[t][8 * s + 7], 0.0f));
            }
            f32x16 h = {};
            h = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah0, __builtin_bit_cast(bf16x8, x[0]), h, 0, 0, 0);
            h = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah1, __builtin_bit_cast(bf16x8, x[1]), h, 0, 0, 0);
            const float4 v = {h[0], h[1], h[2], h[3]};
            *reinterpret_cast<float4*>(lds + oPart + ((wave * 256 + t * 32 + (lane & 31)) * 8 + 4 * half) * 4) = v;
        }
        __syncthreads();

        // ---- the four waves' partial sums in wave order, bias, ReLU, flattened (pixel, channel): policy outputs first, then value ----
        float* pf = prm.pflat + static_cast<size_t>(img) * 4 * kPix;
        float* vf = prm.vflat + static_cast<size_t>(img) * 2 * kPix;
        const float* part = reinterpret_cast<const float*>(lds + oPart);
#pragma unroll
        for (int it = 0; it < (kHeadRows * kPix + 255) / 256; ++it) {
            const int i = threadIdx.x + 256 * it;
            if (i >= kHeadRows * kPix) break;
            const bool policy = i < 4 * kPix;
            const int k = policy ? i : i - 4 * kPix;
            const int p = policy ? k >> 2 : k >> 1, j = policy ? (k & 3) : 4 + (k & 1);
            const float* src = part + p * 8 + j;
            const float v = fmaxf((((src[0] + src[1 * 256 * 8]) + src[2 * 256 * 8]) + src[3 * 256 * 8]) + bh[j], 0.0f);
            if (policy) pf[i] = v; else vf[k] = v;
        }
        // the partial sums are next written behind the next position's barriers
    }
}

// d_q from the handle's float32 buffers: the host packer's functions, one element per thread
__global__ __launch_bounds__(256)
void pvnet_bf16_pack_kernel(const float* w1, const float* w2, const float* w3, const float* wh, unsigned short* q) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q::kElements) return;
    int b = 0;
    const int at = Q::source(i, b);
    const float* src = b == 0 ? w1 : b == 1 ? w2 : b == 2 ? w3 : wh;
    q[i] = at < 0 ? static_cast<unsigned short>(0) : Q::rne_bits(__float_as_uint(src[at]));
}

}  // namespace

int gmk::pvnet_bf16_refresh(gmk_pvnet* net, void* stream) {
    if (!net->d_q) { gmk::set_error("the bf16 weights of this handle have not been allocated (gmk_pvnet_set_precision)"); return GMK_ERR_STATE; }
    hipLaunchKernelGGL(pvnet_bf16_pack_kernel, dim3((Q::kElements + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       net->d_w1, net->d_w2, net->d_w3, net->d_wh, net->d_q);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

int gmk::pvnet_bf16_launch(gmk_pvnet* net, const float* d_states, int n, float* d_pflat, float* d_vflat, void* stream) {
    gmk::DeviceState& st = gmk::device_state();
    if (!net->d_q) { gmk::set_error("the bf16 weights of this handle have not been allocated (gmk_pvnet_set_precision)"); return GMK_ERR_STATE; }
    if (!net->bf16_attr_set) {
        GMK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pvnet_bf16_trunk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        net->bf16_attr_set = true;
    }
    PvBf16Params prm;
    prm.states = d_states; prm.n = n;
    prm.q = reinterpret_cast<const uint4*>(net->d_q);
    prm.b = net->d_b;
    prm.pflat = d_pflat; prm.vflat = d_vflat;
    const int grid = std::min(n, st.cu_count > 0 ? st.cu_count : 256);        // one workgroup per CU, each takes every grid-th position
    hipLaunchKernelGGL(pvnet_bf16_trunk_kernel, dim3(grid), dim3(256), static_cast<size_t>(kLdsBytes), static_cast<hipStream_t>(stream), prm);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_bf16_round_host(const float* src, size_t n, uint16_t* dst) {
    if (n > 0 && (!src || !dst)) { gmk::set_error("gmk_bf16_round_host: bad arguments"); return GMK_ERR_ARG; }
    for (size_t i = 0; i < n; ++i) dst[i] = Q::rne(src[i]);
    return GMK_OK;
}

extern "C" int gmk_pvnet_get_precision(gmk_pvnet* net, int* precision) {
    if (!net || !precision) { gmk::set_error("gmk_pvnet_get_precision: bad arguments"); return GMK_ERR_ARG; }
    *precision = net->precision;
    return GMK_OK;
}

extern "C" int gmk_pvnet_set_precision(gmk_pvnet* net, int precision) {
    if (!net || (precision != GMK_PVNET_F32 && precision != GMK_PVNET_BF16)) { gmk::set_error("gmk_pvnet_set_precision: bad arguments"); return GMK_ERR_ARG; }
    GMK_NEED_INIT();
    if (precision == GMK_PVNET_BF16) {
        // the float32 buffers hold the weights exactly (pure gathers): read them back, pack on the host, copy -- all blocking, like gmk_pvnet_set_dense
        const size_t n1 = (1 * 7 + 2) * 256, n2 = (2 * 36 + 5) * 256, n3 = (4 * 72 + 5) * 256, nh = gmk::pvpack::kHeadFloats;   // pack_layer's sizes
        std::vector<float> w1(n1), w2(n2), w3(n3), wh(nh);
        std::vector<uint16_t> q(Q::kElements);
        GMK_HIP_CHECK(hipDeviceSynchronize());
        GMK_HIP_CHECK(hipMemcpy(w1.data(), net->d_w1, n1 * 4, hipMemcpyDeviceToHost));
        GMK_HIP_CHECK(hipMemcpy(w2.data(), net->d_w2, n2 * 4, hipMemcpyDeviceToHost));
        GMK_HIP_CHECK(hipMemcpy(w3.data(), net->d_w3, n3 * 4, hipMemcpyDeviceToHost));
        GMK_HIP_CHECK(hipMemcpy(wh.data(), net->d_wh, nh * 4, hipMemcpyDeviceToHost));
        Q::pack(w1.data(), w2.data(), w3.data(), wh.data(), q.data());
        if (!net->d_q) GMK_HIP_CHECK(hipMalloc(&net->d_q, static_cast<size_t>(Q::kElements) * 2));
        GMK_HIP_CHECK(hipMemcpy(net->d_q, q.data(), static_cast<size_t>(Q::kElements) * 2, hipMemcpyHostToDevice));
    }
    net->precision = precision;
    return GMK_OK;
}
