// records_wire.hip -- the wire form of game records on the device: scan, pack and unpack.
//
// selfplay.pack_records sends a rank's records to rank 0 as ONE byte block instead of the 101 KB per game fixed-stride arrays:
//     lens int32[n] | winner int8[n] | moves uint8[T] | visits uint16[T][225]          T = sum(lens), the last section optional
// These kernels make and read that block without the host: the offsets of every game's moves in it (an exclusive prefix sum of lens),
// the pack, and the unpack back into fixed-stride rows.  K4 + K5 read the block directly (records_kernel.hip, gmk_samples_from_packed).
//
// Game g's played visit rows are one run of 450 len bytes, at g * 101 250 in the fixed-stride array (2-byte aligned) and at
// 5n + T + 450 offsets[g] in the block (odd whenever 5n + T is).  A run is copied with 16-byte stores to the aligned interior of its
// destination, each built from two 16-byte aligned source loads funnel-shifted by the source's misalignment (v_alignbyte), and with byte
// stores only for the at most 15 bytes at either edge.  A 16-byte chunk of the destination is therefore written by one game alone and
// neighbouring games need no atomics.  A 16-byte aligned load that holds one byte of a run lies in the same page as that byte.
#include "capi_common.h"

namespace {

constexpr int kCells = 225;
constexpr int kRowBytes = 2 * kCells;                  // one visit row
constexpr int64_t kGameVisitBytes = int64_t(kCells) * kRowBytes;   // 101 250: one game's visit rows in the fixed-stride array
constexpr int kThreads = 256;
constexpr int kScanPer = 8;                            // lens per thread in the scan
constexpr int kScanChunk = kThreads * kScanPer;        // lens per workgroup in the scan

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Plain stores, although the outputs are streamed: non-temporal ones were slower here in an alternating A/B on the MI355X (32 768 games:
// unpack 0.991 against 0.926 ms, pack 0.264 against 0.260 ms; DESIGN.md, "Game records on the wire").
template <class T>
__device__ __forceinline__ void store(T v, T* p) { *p = v; }

// The scan marks a length outside [0, 225] with -1, and -1 absorbs everything it is added to: offsets[n] < 0 iff some length was bad.
__device__ __forceinline__ int64_t combine(int64_t a, int64_t b) { return (a < 0 || b < 0) ? -1 : a + b; }

__device__ __forceinline__ int64_t wire_bytes(int n, int64_t T, bool has_visits) {
    return 5 * static_cast<int64_t>(n) + T * (has_visits ? 1 + kRowBytes : 1);
}

// Inclusive scan of one value per thread over the workgroup (Hillis-Steele in LDS); s[kThreads - 1] holds the total on return.
__device__ __forceinline__ int64_t block_scan(int64_t v, int64_t* s) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const int64_t o = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        if (tid >= d) s[tid] = combine(o, s[tid]);
        __syncthreads();
    }
    return s[tid];
}

// ---- scan, step 1: chunk-local exclusive sums.  The first entry of a chunk is 0 locally, so its slot holds the previous chunk's total
// until step 3 (chunk c's total goes to offsets[min((c + 1) * kScanChunk, n)]: offsets[n] for the last chunk).
__global__ __launch_bounds__(kThreads)
void records_scan_local_kernel(const int32_t* __restrict__ lens, int n, int64_t* __restrict__ offsets) {
    __shared__ int64_t s[kThreads];
    const int tid = threadIdx.x;
    const int64_t c0 = static_cast<int64_t>(blockIdx.x) * kScanChunk;
    const int64_t i0 = c0 + static_cast<int64_t>(tid) * kScanPer;
    int64_t l[kScanPer];
    int64_t mine = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        const int32_t x = i0 + j < n ? lens[i0 + j] : 0;
        l[j] = (x < 0 || x > kCells) ? -1 : x;
        mine = combine(mine, l[j]);
    }
    block_scan(mine, s);
    int64_t e = tid ? s[tid - 1] : 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        const int64_t i = i0 + j;
        if (i < n && i != c0) offsets[i] = e;
        e = combine(e, l[j]);
    }
    if (blockIdx.x == 0 && tid == 0) offsets[0] = 0;
    if (tid == kThreads - 1) offsets[c0 + kScanChunk < n ? c0 + kScanChunk : n] = s[kThreads - 1];
}

// ---- scan, step 2 (one workgroup): the chunk totals, in their slots, become inclusive sums = the first offset of the next chunk; offsets[n] = T.
__global__ __launch_bounds__(kThreads)
void records_scan_totals_kernel(int n, int64_t n_chunks, int64_t* __restrict__ offsets) {
    __shared__ int64_t s[kThreads];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int64_t base = 0; base < n_chunks; base += kThreads) {
        const int64_t c = base + tid;
        const int64_t slot = c + 1 < n_chunks ? (c + 1) * kScanChunk : n;
        const int64_t v = c < n_chunks ? offsets[slot] : 0;
        const int64_t incl = combine(carry, block_scan(v, s));
        if (c < n_chunks) offsets[slot] = incl;
        carry = combine(carry, s[kThreads - 1]);
        __syncthreads();
    }
}

// ---- scan, step 3: chunk c >= 1 adds its first offset (step 2) to its other entries.
__global__ __launch_bounds__(kThreads)
void records_scan_add_kernel(int n, int64_t* __restrict__ offsets) {
    const int64_t c0 = (static_cast<int64_t>(blockIdx.x) + 1) * kScanChunk;
    const int64_t base = offsets[c0];
    const int64_t i0 = c0 + static_cast<int64_t>(threadIdx.x) * kScanPer;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        const int64_t i = i0 + j;
        if (i < n && i != c0) offsets[i] = combine(base, offsets[i]);
    }
}

// ---- copies of byte runs ----
// Interior of a run: 16-byte chunks dst[16 k], k < chunks (dst 16-byte aligned), from the source bytes at src_base + r + 16 k (src_base
// 16-byte aligned, 0 < r < 16 = 4 Q + b): words Q..Q+4 of the two aligned loads, shifted right by b bytes.
template <int Q>
__device__ __forceinline__ void copy_interior_shifted(uint8_t* dst, const uint8_t* src_base, int b, int64_t chunks) {
    for (int64_t k = threadIdx.x; k < chunks; k += kThreads) {
        const u32x4 lo = *reinterpret_cast<const u32x4*>(src_base + 16 * k);
        const u32x4 hi = *reinterpret_cast<const u32x4*>(src_base + 16 * k + 16);
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        u32x4 o;
        o.x = __builtin_amdgcn_alignbyte(w[Q + 1], w[Q + 0], b);
        o.y = __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], b);
        o.z = __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], b);
        o.w = __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], b);
        store(o, reinterpret_cast<u32x4*>(dst + 16 * k));
    }
}

__device__ __forceinline__ void copy_interior_aligned(uint8_t* dst, const uint8_t* src, int64_t chunks) {
    for (int64_t k = threadIdx.x; k < chunks; k += kThreads)
        store(*reinterpret_cast<const u32x4*>(src + 16 * k), reinterpret_cast<u32x4*>(dst + 16 * k));
}

// The bytes [d0, d1) of a run that lie outside its aligned 16-byte interior [a, e): at most 15 at the head (lanes 0..15) and 15 at the tail
// (lanes 16..31).  src_at(i) is the byte that goes to d0 + i.
template <class Src>
__device__ __forceinline__ void run_edges(uint8_t* d0, int64_t nbytes, uint8_t* a, uint8_t* e, Src src_at) {
    const int tid = threadIdx.x;
    const int64_t head = (a < d0 + nbytes ? a : d0 + nbytes) - d0;
    const int64_t tail_at = e - d0 > head ? e - d0 : head;
    if (tid < head) store(src_at(tid), d0 + tid);
    if (tid >= 16 && tid < 32 && tail_at + (tid - 16) < nbytes) store(src_at(tail_at + (tid - 16)), d0 + tail_at + (tid - 16));
}

// (by pointer arithmetic, not through an integer, so that the compiler keeps seeing global memory and emits global_*, not flat_*, accesses)
__device__ __forceinline__ uint8_t* align_up16(uint8_t* p) { return p + ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15); }
__device__ __forceinline__ uint8_t* align_down16(uint8_t* p) { return p - (reinterpret_cast<uintptr_t>(p) & 15); }

// The whole workgroup copies src[0, nbytes) to dst[0, nbytes); any alignment of either.
__device__ __forceinline__ void copy_run(uint8_t* dst, const uint8_t* src, int64_t nbytes) {
    if (nbytes <= 0) return;
    uint8_t* a = align_up16(dst);
    uint8_t* e = align_down16(dst + nbytes);
    if (a < e) {
        const int64_t chunks = (e - a) / 16;
        const uint8_t* s = src + (a - dst);
        const int r = static_cast<int>(reinterpret_cast<uintptr_t>(s) & 15);
        const uint8_t* s_base = s - r;
        switch (r >> 2) {                                   // uniform over the workgroup
            case 0: if (r == 0) copy_interior_aligned(a, s, chunks); else copy_interior_shifted<0>(a, s_base, r & 3, chunks); break;
            case 1: copy_interior_shifted<1>(a, s_base, r & 3, chunks); break;
            case 2: copy_interior_shifted<2>(a, s_base, r & 3, chunks); break;
            default: copy_interior_shifted<3>(a, s_base, r & 3, chunks); break;
        }
    }
    run_edges(dst, nbytes, a, e, [src](int64_t i) { return src[i]; });
}

// The whole workgroup zeroes dst[0, nbytes).
__device__ __forceinline__ void zero_run(uint8_t* dst, int64_t nbytes) {
    if (nbytes <= 0) return;
    uint8_t* a = align_up16(dst);
    uint8_t* e = align_down16(dst + nbytes);
    if (a < e) {
        const int64_t chunks = (e - a) / 16;
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int64_t k = threadIdx.x; k < chunks; k += kThreads) store(z, reinterpret_cast<u32x4*>(a + 16 * k));
    }
    run_edges(dst, nbytes, a, e, [](int64_t) { return uint8_t(0); });
}

// ---- pack: one workgroup per game.  Every workgroup checks offsets[n] and out_bytes first: on a bad length or a short buffer nothing is written
// but *status (workgroup 0).
__global__ __launch_bounds__(kThreads)
void records_pack_kernel(const uint8_t* __restrict__ moves, const int32_t* __restrict__ lens, const int8_t* __restrict__ winner,
                         const uint16_t* __restrict__ visits, int n, const int64_t* __restrict__ offsets, uint8_t* __restrict__ out,
                         uint64_t out_bytes, int32_t* __restrict__ status) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const int64_t T = offsets[n];
    const int32_t code = T < 0 ? GMK_WIRE_BAD_LENGTH
                       : static_cast<uint64_t>(wire_bytes(n, T, visits != nullptr)) > out_bytes ? GMK_WIRE_BAD_SIZE : 0;
    if (g == 0 && tid == 0) *status = code;
    if (code) return;
    const int64_t o = offsets[g];
    const int64_t len = offsets[g + 1] - o;
    if (len < 0 || len > kCells) return;                // offsets that are not the scan of these lens: not reached from the C entries
    if (tid == 0) {
        store(lens[g], reinterpret_cast<int32_t*>(out) + g);
        store(static_cast<uint8_t>(winner[g]), out + 4 * static_cast<int64_t>(n) + g);
    }
    const int64_t moves_at = 5 * static_cast<int64_t>(n);
    if (tid < len) store(moves[static_cast<int64_t>(g) * kCells + tid], out + moves_at + o + tid);
    if (visits)
        copy_run(out + moves_at + T + kRowBytes * o, reinterpret_cast<const uint8_t*>(visits) + g * kGameVisitBytes, kRowBytes * len);
}

// ---- unpack: one workgroup per game; writes every byte of the game's fixed-stride rows (zeros past its length).
__global__ __launch_bounds__(kThreads)
void records_unpack_kernel(const uint8_t* __restrict__ buf, uint64_t n_bytes, int n, int has_visits, const int64_t* __restrict__ offsets,
                           uint8_t* __restrict__ moves, int32_t* __restrict__ lens, int8_t* __restrict__ winner, uint16_t* __restrict__ visits,
                           int32_t* __restrict__ status) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const int64_t T = offsets[n];
    const int32_t code = T < 0 ? GMK_WIRE_BAD_LENGTH
                       : static_cast<uint64_t>(wire_bytes(n, T, has_visits != 0)) != n_bytes ? GMK_WIRE_BAD_SIZE : 0;
    if (g == 0 && tid == 0) *status = code;
    if (code) return;
    const int64_t o = offsets[g];
    const int64_t len = offsets[g + 1] - o;
    const int64_t moves_at = 5 * static_cast<int64_t>(n);
    if (tid == 0) {
        lens[g] = static_cast<int32_t>(len);
        winner[g] = static_cast<int8_t>(buf[4 * static_cast<int64_t>(n) + g]);
    }
    if (tid < kCells) store(tid < len ? buf[moves_at + o + tid] : uint8_t(0), moves + static_cast<int64_t>(g) * kCells + tid);
    if (has_visits) {
        uint8_t* dst = reinterpret_cast<uint8_t*>(visits) + g * kGameVisitBytes;
        copy_run(dst, buf + moves_at + T + kRowBytes * o, kRowBytes * len);
        zero_run(dst + kRowBytes * len, kGameVisitBytes - kRowBytes * len);
    }
}

using gmk::misaligned;

// The three scan launches on `stream` (n > 0).
int scan(const int32_t* d_lens, int n, int64_t* d_offsets, hipStream_t stream) {
    const int64_t n_chunks = (static_cast<int64_t>(n) + kScanChunk - 1) / kScanChunk;
    hipLaunchKernelGGL(records_scan_local_kernel, dim3(static_cast<unsigned>(n_chunks)), dim3(kThreads), 0, stream, d_lens, n, d_offsets);
    GMK_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(records_scan_totals_kernel, dim3(1), dim3(kThreads), 0, stream, n, n_chunks, d_offsets);
    GMK_HIP_CHECK(hipGetLastError());
    if (n_chunks > 1) {
        hipLaunchKernelGGL(records_scan_add_kernel, dim3(static_cast<unsigned>(n_chunks - 1)), dim3(kThreads), 0, stream, n, d_offsets);
        GMK_HIP_CHECK(hipGetLastError());
    }
    return GMK_OK;
}

}  // namespace

extern "C" int gmk_records_scan(const int32_t* d_lens, int n, int64_t* d_offsets, void* stream) {
    GMK_NEED_INIT();
    if (n < 0 || (n > 0 && (!d_lens || !d_offsets || misaligned(d_lens, 4) || misaligned(d_offsets, 8)))) {
        gmk::set_error("gmk_records_scan: bad arguments (n >= 0; d_lens 4-byte and d_offsets 8-byte aligned)");
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    return scan(d_lens, n, d_offsets, static_cast<hipStream_t>(stream));
}

extern "C" int gmk_records_packed_bytes(const int64_t* d_offsets, int n, int has_visits, uint64_t* h_bytes, void* stream) {
    GMK_NEED_INIT();
    if (n < 0 || !h_bytes || (n > 0 && (!d_offsets || misaligned(d_offsets, 8)))) {
        gmk::set_error("gmk_records_packed_bytes: bad arguments");
        return GMK_ERR_ARG;
    }
    if (n == 0) { *h_bytes = 0; return GMK_OK; }
    int64_t T = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    GMK_HIP_CHECK(hipMemcpyAsync(&T, d_offsets + n, sizeof(T), hipMemcpyDeviceToHost, s));
    GMK_HIP_CHECK(hipStreamSynchronize(s));
    if (T < 0) {
        gmk::set_error("gmk_records_packed_bytes: a game length was outside [0, 225]");
        return GMK_ERR_ARG;
    }
    *h_bytes = static_cast<uint64_t>(5 * static_cast<int64_t>(n) + T * (has_visits ? 1 + kRowBytes : 1));
    return GMK_OK;
}

extern "C" int gmk_records_pack(const uint8_t* d_moves, const int32_t* d_lens, const int8_t* d_winner, const uint16_t* d_visits, int n,
                                const int64_t* d_offsets, uint8_t* d_out, uint64_t out_bytes, int32_t* d_status, void* stream) {
    GMK_NEED_INIT();
    if (n < 0 || (n > 0 && (!d_moves || !d_lens || !d_winner || !d_offsets || !d_out || !d_status || misaligned(d_lens, 4) || misaligned(d_offsets, 8) ||
                            misaligned(d_out, 4) || misaligned(d_status, 4) || misaligned(d_visits, 2)))) {
        gmk::set_error("gmk_records_pack: bad arguments (d_out and d_lens 4-byte, d_offsets 8-byte, d_visits 2-byte aligned)");
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    hipLaunchKernelGGL(records_pack_kernel, dim3(n), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       d_moves, d_lens, d_winner, d_visits, n, d_offsets, d_out, out_bytes, d_status);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_records_unpack(const uint8_t* d_buf, uint64_t n_bytes, int n, int has_visits, int64_t* d_offsets, uint8_t* d_moves,
                                  int32_t* d_lens, int8_t* d_winner, uint16_t* d_visits, int32_t* d_status, void* stream) {
    GMK_NEED_INIT();
    if (n < 0 || (n > 0 && (!d_buf || !d_offsets || !d_moves || !d_lens || !d_winner || !d_status || (has_visits && !d_visits) ||
                            n_bytes < 5 * static_cast<uint64_t>(n) || misaligned(d_buf, 4) || misaligned(d_offsets, 8) ||
                            misaligned(d_lens, 4) || misaligned(d_status, 4) || misaligned(d_visits, 2)))) {
        gmk::set_error("gmk_records_unpack: bad arguments (n_bytes >= 5n; d_buf and d_lens 4-byte, d_offsets 8-byte, d_visits 2-byte aligned)");
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = scan(reinterpret_cast<const int32_t*>(d_buf), n, d_offsets, s);
    if (rc != GMK_OK) return rc;
    hipLaunchKernelGGL(records_unpack_kernel, dim3(n), dim3(kThreads), 0, s,
                       d_buf, n_bytes, n, has_visits, d_offsets, d_moves, d_lens, d_winner, d_visits, d_status);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}
