// vct_kernel.hip -- K17: the forced win by continuous threats (fours and threes), exact and batched.
//
// The contract is in include/gomoku_hip.h ("K17", second block).  The search is an AND/OR tree walked level by level for all roots at once: the
// three exact solvers do the work (K14 gmk_vcf_solve: "does the side to move win by fours?"; gmk_vcf_threats: "which of its moves threaten
// to?"; K15 gmk_vcf_defend: "which replies hold?"), each as one batched call over a level's move lists, and the small kernels below turn one
// call's verdicts into the next call's lists.  The driver is host code; lists, verdicts and the tree stay on the device, and per level the host
// reads per-root scalars only: the root's depth, the number of candidates, the number of children per root.
//
// A level is an array of positions, a root's positions contiguous and in the order of the contract: by parent, then candidate, then reply,
// all ascending.  Level 0 is the caller's own lists; the lists of deeper levels have stride 225.  Per level the tree keeps the own solve
// (status, length, pv), the depth (-1: not proven), and after its expansion the candidates: position i owns candidates cand_begin[i] ..
// cand_begin[i + 1], candidate k owns child_count[k] positions of the next level from child_begin[k] on (-1: the candidate was dropped, or
// its root has ended).  Offsets come from one-workgroup scans; nothing here is a hot loop, the solvers are.  No float, no atomics: the only
// value several threads write is the flag root_cut[root] = 1.
#include <algorithm>
#include <cstring>
#include <exception>
#include <vector>

#include "capi_common.h"
#include "host_staging.h"

namespace {

constexpr int kCells = 225;
constexpr int kListStride = 225;                                // of the lists of levels 1 ..
constexpr long long kMaxLevel = 1ll << 22;                      // positions of one level over the whole batch: keeps every offset far inside 63 bits

// What the kernels that walk the tree (resolve, write) read of one level.
struct LevelView {
    const int32_t* status;                                      // own solve
    const int32_t* length;
    const uint8_t* pv;
    int32_t* depth;
    const uint8_t* lists;                                       // levels 1 .. only
    const int32_t* lens;
    const long long* cand_begin;                                // NULL until the level is expanded
    const uint8_t* cand_cell;
    const int32_t* child_begin;
    const int32_t* child_count;
};

__global__ void vct_mark_kernel(const int32_t* status, const int32_t* root, int count, int last, int32_t* depth, int32_t* root_cut) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int s = status[i];
    depth[i] = s == GMK_VCF_WIN ? 0 : -1;
    if (s == GMK_VCF_DEPTH || s == GMK_VCF_BUDGET || (last && s != GMK_VCF_WIN)) root_cut[root[i]] = 1;
}

// depth = 1 + min over the kept candidates whose children all have a depth of (max over those children), or -1
__global__ void vct_resolve_kernel(LevelView v, const int32_t* next_depth, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count || v.status[i] == GMK_VCF_WIN || !v.cand_begin) return;
    int best = -1;
    for (long long k = v.cand_begin[i]; k < v.cand_begin[i + 1]; ++k) {
        const int at = v.child_begin[k];
        if (at < 0) continue;
        int deepest = 0;
        bool proven = true;
        for (int j = 0; j < v.child_count[k] && proven; ++j) {
            const int d = next_depth[at + j];
            proven = d >= 0;
            deepest = d > deepest ? d : deepest;
        }
        if (proven && (best < 0 || deepest + 1 < best)) best = deepest + 1;
    }
    v.depth[i] = best;
}

// the lists that are expanded: a position that is won, or whose root has ended, is handed on as "no position" (length -1), which costs one job
__global__ void vct_prepare_kernel(const int32_t* lens, const int32_t* status, const int32_t* root, const int32_t* alive, int count, int32_t* expand_lens) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    expand_lens[i] = alive[root[i]] && status[i] != GMK_VCF_WIN ? lens[i] : -1;
}

__global__ void vct_count_candidates_kernel(const uint8_t* verdict, const int32_t* root, int count, int32_t* cand_count, int32_t* root_cut) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint8_t* row = verdict + static_cast<size_t>(i) * kCells;
    int found = 0;
    bool unknown = false;
    for (int c = 0; c < kCells; ++c) {
        const int v = row[c];
        found += v == GMK_VCF_THREAT_WINS || v == GMK_VCF_THREAT_FOUR;
        unknown |= v == GMK_VCF_THREAT_UNKNOWN;
    }
    cand_count[i] = found;
    if (unknown) root_cut[root[i]] = 1;
}

// out[i] = in[0] + .. + in[i - 1] for i = 0 .. count: one workgroup, every thread a contiguous piece
__global__ __launch_bounds__(1024) void vct_scan_kernel(const int32_t* in, long long count, long long* out) {
    __shared__ long long part[1024];
    const long long piece = (count + 1023) / 1024;
    const long long lo = std::min<long long>(count, threadIdx.x * piece), hi = std::min<long long>(count, lo + piece);
    long long sum = 0;
    for (long long i = lo; i < hi; ++i) sum += in[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int t = 0; t < 1024; ++t) { const long long v = part[t]; part[t] = run; run += v; }
        out[count] = run;
    }
    __syncthreads();
    sum = part[threadIdx.x];
    for (long long i = lo; i < hi; ++i) { out[i] = sum; sum += in[i]; }
}

// candidate k of position i: the list Q + [c]
__global__ void vct_emit_candidates_kernel(const uint8_t* lists, int stride, const int32_t* expand_lens, const uint8_t* verdict, const long long* cand_begin,
                                           int count, uint8_t* cand_lists, int32_t* cand_lens, int32_t* cand_pos, uint8_t* cand_cell) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const long long end = cand_begin[i + 1];
    long long k = cand_begin[i];
    if (k == end) return;                                       // also every list that was handed on as "no position"
    const int len = expand_lens[i];
    const uint8_t* list = lists + static_cast<size_t>(i) * static_cast<size_t>(stride);
    const uint8_t* row = verdict + static_cast<size_t>(i) * kCells;
    for (int c = 0; c < kCells && k < end; ++c) {
        const int v = row[c];
        if (v != GMK_VCF_THREAT_WINS && v != GMK_VCF_THREAT_FOUR) continue;
        uint8_t* to = cand_lists + static_cast<size_t>(k) * kListStride;
        for (int m = 0; m < len; ++m) to[m] = list[m];          // a candidate is an empty cell, so len < 225
        to[len] = static_cast<uint8_t>(c);
        cand_lens[k] = len + 1;
        cand_pos[k] = i;
        cand_cell[k] = static_cast<uint8_t>(c);
        ++k;
    }
}

// a candidate is dropped when a reply is UNKNOWN (cut) or FIVE; otherwise its children are the replies that hold
__global__ void vct_count_children_kernel(const uint8_t* verdict, const int32_t* cand_pos, const int32_t* root, long long count, int32_t* kept,
                                          int32_t* child_count, int32_t* root_cut) {
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const uint8_t* row = verdict + static_cast<size_t>(k) * kCells;
    int holds = 0;
    bool unknown = false, five = false;
    for (int c = 0; c < kCells; ++c) {
        const int v = row[c];
        holds += v == GMK_VCF_CELL_HOLDS;
        unknown |= v == GMK_VCF_CELL_UNKNOWN;
        five |= v == GMK_VCF_CELL_FIVE;
    }
    const bool keep = !unknown && !five;
    kept[k] = keep;
    child_count[k] = keep ? holds : 0;
    if (unknown) root_cut[root[cand_pos[k]]] = 1;
}

// a root's positions are contiguous, so are their candidates and those candidates' children: the root's share is a difference of offsets
__global__ void vct_root_counts_kernel(const long long* pos_begin, const long long* cand_begin, const long long* child_offset, int n,
                                       long long* root_first, long long* root_count) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const long long first = child_offset[cand_begin[pos_begin[g]]], end = child_offset[cand_begin[pos_begin[g + 1]]];
    root_first[g] = first;
    root_count[g] = end - first;
}

// the children of candidate k, Q + [c, r], at their place in the next level; the level of a root that has ended is left out
__global__ void vct_emit_children_kernel(const uint8_t* cand_lists, const int32_t* cand_lens, const int32_t* cand_pos, const int32_t* root,
                                         const uint8_t* verdict, const int32_t* kept, const long long* child_offset, const long long* root_first,
                                         const long long* next_pos_begin, const int32_t* alive, long long count, int32_t* child_begin,
                                         int32_t* child_count, uint8_t* next_lists, int32_t* next_lens, int32_t* next_root) {
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const int g = root[cand_pos[k]];
    if (!alive[g] || !kept[k]) { child_begin[k] = -1; child_count[k] = 0; return; }
    long long at = next_pos_begin[g] + (child_offset[k] - root_first[g]);
    child_begin[k] = static_cast<int32_t>(at);
    const int len = cand_lens[k];
    const uint8_t* list = cand_lists + static_cast<size_t>(k) * kListStride;
    const uint8_t* row = verdict + static_cast<size_t>(k) * kCells;
    for (int r = 0; r < kCells; ++r) {
        if (row[r] != GMK_VCF_CELL_HOLDS) continue;
        uint8_t* to = next_lists + static_cast<size_t>(at) * kListStride;
        for (int m = 0; m < len; ++m) to[m] = list[m];          // a reply is an empty cell of a list of len cells, so len < 225
        to[len] = static_cast<uint8_t>(r);
        next_lens[at] = len + 1;
        next_root[at] = g;
        ++at;
    }
}

// The outputs of root g.  A WIN's line: the lowest candidate of minimal depth, its child of greatest depth (the lowest reply on ties), and so
// on down to a candidate that no reply holds against, or to a position with a win by fours of its own, whose pv ends the line.
__global__ void vct_write_kernel(const LevelView* levels, int n, const int32_t* final_status, const uint32_t* final_positions, int32_t* status,
                                 int32_t* move, int32_t* threats, uint32_t* positions, uint8_t* pv) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const bool win = final_status[g] == GMK_VCF_WIN;
    if (status) status[g] = final_status[g];
    if (positions) positions[g] = final_positions[g];
    if (threats) threats[g] = win ? levels[0].depth[g] : 0;
    uint8_t* line = pv ? pv + static_cast<size_t>(g) * GMK_VCT_PV : nullptr;
    int cells = 0, first = -1;
    const auto put = [&](int c) {
        if (cells == 0) first = c;
        if (line && cells < GMK_VCT_PV) line[cells] = static_cast<uint8_t>(c);
        ++cells;
    };
    if (win) {
        int level = 0, q = g;
        for (;;) {
            const LevelView v = levels[level];
            if (v.status[q] == GMK_VCF_WIN) {
                const uint8_t* own = v.pv + static_cast<size_t>(q) * GMK_VCF_PV;
                for (int i = 0; i < 2 * v.length[q] - 1; ++i) put(own[i]);
                break;
            }
            const int32_t* below = levels[level + 1].depth;
            int child = -1;
            long long chosen = -1;
            for (long long k = v.cand_begin[q]; k < v.cand_begin[q + 1] && chosen < 0; ++k) {
                const int at = v.child_begin[k];
                if (at < 0) continue;
                int deepest = 0;
                bool proven = true;
                child = -1;
                for (int j = 0; j < v.child_count[k] && proven; ++j) {
                    const int d = below[at + j];
                    proven = d >= 0;
                    if (child < 0 || d > deepest) { deepest = d; child = at + j; }
                }
                if (proven && deepest + 1 == v.depth[q]) chosen = k;
            }
            if (chosen < 0) break;                                 // cannot be: a position with a depth has such a candidate
            put(v.cand_cell[chosen]);
            if (child < 0) break;                                  // no reply holds
            const LevelView w = levels[level + 1];
            put(w.lists[static_cast<size_t>(child) * kListStride + w.lens[child] - 1]);
            q = child;
            ++level;
        }
    }
    if (move) move[g] = first;
    if (line)
        for (int i = cells; i < GMK_VCT_PV; ++i) line[i] = 255;
}

using gmk::misaligned;

bool bad_arguments(const void* moves, int stride, const void* lens, int n, int max_depth, int flags, int max_threats, int max_positions) {
    return n < 0 || stride < 1 || max_depth < 1 || max_depth > GMK_VCF_MAX_DEPTH || (flags & ~GMK_VCF_ITERATIVE) != 0 || max_threats < 1 ||
           max_threats > GMK_VCT_MAX_THREATS || max_positions < 1 || (n > 0 && (!moves || !lens));
}

using gmk::Blocks;                                              // the workspace: a few blocks per level (host_staging.h)

struct Level {
    LevelView view{};
    const uint8_t* lists = nullptr;
    int stride = 0;
    const int32_t* lens = nullptr;
    int32_t* root = nullptr;
    int32_t* own_status = nullptr;                              // what the view reads, writable
    int32_t* own_length = nullptr;
    uint8_t* own_pv = nullptr;
    long long* pos_begin = nullptr;                             // [n + 1]: where each root's positions start
    int count = 0;
};

inline unsigned blocks_for(long long count) { return static_cast<unsigned>((count + 255) / 256); }

int vct_solve(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int max_depth, uint32_t budget, int flags, int max_threats,
              int max_positions, int32_t* d_status, int32_t* d_move, int32_t* d_threats, uint32_t* d_positions, uint8_t* d_pv, void* stream) {
    GMK_NEED_INIT();
    if (bad_arguments(d_moves, stride, d_lens, n, max_depth, flags, max_threats, max_positions) || misaligned(d_lens, 4) || misaligned(d_status, 4) ||
        misaligned(d_move, 4) || misaligned(d_threats, 4) || misaligned(d_positions, 4)) {
        gmk::set_error("gmk_vct_solve: bad arguments (n >= 0, stride >= 1, max_depth in [1, %d], flags 0 or GMK_VCF_ITERATIVE, max_threats in [1, %d], "
                       "max_positions >= 1; d_lens and the 4-byte outputs 4-byte aligned)", GMK_VCF_MAX_DEPTH, GMK_VCT_MAX_THREATS);
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    // every level, the roots included, holds at most kMaxLevel positions: so the candidates of a level, at most 225 each, fit an int
    if (n > kMaxLevel) { gmk::set_error("gmk_vct_solve: %d roots, more than %lld", n, kMaxLevel); return GMK_ERR_CAPACITY; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t un = static_cast<size_t>(n);
    Blocks tree, scratch;                                          // the tree lives for the call, the scratch for one level's expansion
    const auto no_memory = [&](int level) {
        gmk::set_error("gmk_vct_solve: level %d does not fit in device memory", level);
        return GMK_ERR_HIP;
    };
    // the host's side of the roots
    std::vector<int32_t> alive(un, 1), status(un, GMK_VCF_NONE), word(un);
    std::vector<uint32_t> positions(un, 1u);
    std::vector<long long> begin(un + 1), counts(un);
    std::vector<Level> levels(static_cast<size_t>(max_threats) + 1);      // never resized: the blocks write into its pointers
    // a level's own arrays: asked for with the block they belong to, then filled in
    const auto want_level = [&](Level& lv, int count) {
        const size_t c = static_cast<size_t>(count);
        lv.count = count;
        tree.want(lv.pos_begin, un + 1);
        tree.want(lv.own_status, c);
        tree.want(lv.own_length, c);
        tree.want(lv.own_pv, c * GMK_VCF_PV);
        tree.want(lv.view.depth, c);
    };
    const auto set_level = [&](Level& lv, const std::vector<long long>& pos_begin) {
        lv.view.status = lv.own_status; lv.view.length = lv.own_length; lv.view.pv = lv.own_pv;
        return hipMemcpyAsync(lv.pos_begin, pos_begin.data(), (un + 1) * 8, hipMemcpyHostToDevice, s) == hipSuccess &&
               hipStreamSynchronize(s) == hipSuccess;         // pos_begin is the caller's vector: the copy is done before it changes
    };
    int32_t *d_alive, *d_cut, *d_final_status;
    uint32_t* d_final_positions;
    long long *d_root_first, *d_root_count;
    LevelView* d_views;
    for (size_t g = 0; g <= un; ++g) begin[g] = static_cast<long long>(g);
    {
        Level& root = levels[0];
        root.lists = d_moves; root.stride = stride; root.lens = d_lens;
        tree.want(d_alive, un); tree.want(d_cut, un); tree.want(d_final_status, un); tree.want(d_final_positions, un);
        tree.want(d_root_first, un); tree.want(d_root_count, un); tree.want(d_views, GMK_VCT_MAX_THREATS + 1);
        tree.want(root.root, un);
        want_level(root, n);
        if (!tree.take() || !set_level(root, begin)) return no_memory(0);
        GMK_HIP_CHECK(hipMemsetAsync(d_cut, 0, un * 4, s));
        for (size_t g = 0; g < un; ++g) word[g] = static_cast<int32_t>(g);
        GMK_HIP_CHECK(hipMemcpyAsync(root.root, word.data(), un * 4, hipMemcpyHostToDevice, s));
        GMK_HIP_CHECK(hipStreamSynchronize(s));
    }

    int living = n;
    for (int t = 0; t <= max_threats && living > 0; ++t) {
        Level& lv = levels[static_cast<size_t>(t)];
        // ---- the own solves of the level, and what they prove above it ----
        if (lv.count > 0) {
            const int rc = gmk_vcf_solve(lv.lists, lv.stride, lv.lens, lv.count, max_depth, budget, flags, lv.own_status, nullptr, lv.own_length, nullptr,
                                         lv.own_pv, s);
            if (rc != GMK_OK) return rc;
            hipLaunchKernelGGL(vct_mark_kernel, dim3(blocks_for(lv.count)), dim3(256), 0, s, lv.view.status, lv.root, lv.count, t == max_threats ? 1 : 0,
                               lv.view.depth, d_cut);
        }
        for (int up = t - 1; up >= 0; --up) {
            const Level& above = levels[static_cast<size_t>(up)];
            if (above.count > 0)
                hipLaunchKernelGGL(vct_resolve_kernel, dim3(blocks_for(above.count)), dim3(256), 0, s, above.view, levels[static_cast<size_t>(up) + 1].view.depth,
                                   above.count);
        }
        GMK_HIP_CHECK(hipGetLastError());
        GMK_HIP_CHECK(hipMemcpyAsync(word.data(), levels[0].view.depth, un * 4, hipMemcpyDeviceToHost, s));
        GMK_HIP_CHECK(hipStreamSynchronize(s));
        for (size_t g = 0; g < un; ++g)
            if (alive[g] && word[g] >= 0) { alive[g] = 0; status[g] = GMK_VCF_WIN; --living; }
        if (t == 0) {                                              // a root that is over or no position ends as that
            GMK_HIP_CHECK(hipMemcpyAsync(word.data(), levels[0].view.status, un * 4, hipMemcpyDeviceToHost, s));
            GMK_HIP_CHECK(hipStreamSynchronize(s));
            for (size_t g = 0; g < un; ++g)
                if (alive[g] && (word[g] == GMK_VCF_OVER || word[g] == GMK_VCF_BAD)) { alive[g] = 0; status[g] = word[g]; --living; }
        }
        if (t == max_threats || living == 0 || lv.count == 0) break;

        // ---- the level's candidates: the cells whose stone wins by fours unless it is answered, or makes a four ----
        const size_t pc = static_cast<size_t>(lv.count);
        GMK_HIP_CHECK(hipMemcpyAsync(d_alive, alive.data(), un * 4, hipMemcpyHostToDevice, s));
        int32_t *expand_lens, *own_again, *cand_count;             // own_again: launch one of gmk_vcf_threats, BAD where the list was handed on as no position
        uint8_t* threat;
        long long* cand_begin;
        scratch.want(expand_lens, pc); scratch.want(own_again, pc); scratch.want(threat, pc * kCells); scratch.want(cand_count, pc);
        tree.want(cand_begin, pc + 1);
        if (!scratch.take() || !tree.take()) return no_memory(t);
        hipLaunchKernelGGL(vct_prepare_kernel, dim3(blocks_for(lv.count)), dim3(256), 0, s, lv.lens, lv.view.status, lv.root, d_alive, lv.count, expand_lens);
        int rc = gmk_vcf_threats(lv.lists, lv.stride, expand_lens, lv.count, max_depth, budget, flags, own_again, nullptr, nullptr, nullptr, nullptr, threat,
                                 nullptr, nullptr, s);
        if (rc != GMK_OK) return rc;
        hipLaunchKernelGGL(vct_count_candidates_kernel, dim3(blocks_for(lv.count)), dim3(256), 0, s, threat, lv.root, lv.count, cand_count, d_cut);
        hipLaunchKernelGGL(vct_scan_kernel, dim3(1), dim3(1024), 0, s, cand_count, static_cast<long long>(lv.count), cand_begin);
        GMK_HIP_CHECK(hipGetLastError());
        long long candidates = 0;
        GMK_HIP_CHECK(hipMemcpyAsync(&candidates, cand_begin + lv.count, 8, hipMemcpyDeviceToHost, s));
        GMK_HIP_CHECK(hipStreamSynchronize(s));
        lv.view.cand_begin = cand_begin;
        const size_t kc = static_cast<size_t>(candidates);
        uint8_t *cand_cell, *cand_lists, *threat_pv, *reply;
        int32_t *child_begin, *child_count, *cand_lens, *cand_pos, *threat_status, *threat_length, *kept;
        long long* child_offset;
        tree.want(cand_cell, kc); tree.want(child_begin, kc); tree.want(child_count, kc);
        scratch.want(cand_lists, kc * kListStride); scratch.want(cand_lens, kc); scratch.want(cand_pos, kc); scratch.want(threat_status, kc);
        scratch.want(threat_length, kc); scratch.want(threat_pv, kc * GMK_VCF_PV); scratch.want(reply, kc * kCells); scratch.want(kept, kc);
        scratch.want(child_offset, kc + 1);
        if (!scratch.take() || !tree.take()) return no_memory(t + 1);
        lv.view.cand_cell = cand_cell; lv.view.child_begin = child_begin; lv.view.child_count = child_count;

        // ---- the replies that hold against each candidate are the next level ----
        if (candidates > 0) {
            hipLaunchKernelGGL(vct_emit_candidates_kernel, dim3(blocks_for(lv.count)), dim3(256), 0, s, lv.lists, lv.stride, expand_lens, threat, cand_begin,
                               lv.count, cand_lists, cand_lens, cand_pos, cand_cell);
            rc = gmk_vcf_defend(cand_lists, kListStride, cand_lens, static_cast<int>(candidates), max_depth, budget, flags, threat_status, threat_length,
                                threat_pv, nullptr, reply, nullptr, nullptr, s);
            if (rc != GMK_OK) return rc;
            hipLaunchKernelGGL(vct_count_children_kernel, dim3(blocks_for(candidates)), dim3(256), 0, s, reply, cand_pos, lv.root, candidates, kept,
                               child_count, d_cut);
        }
        hipLaunchKernelGGL(vct_scan_kernel, dim3(1), dim3(1024), 0, s, child_count, candidates, child_offset);
        hipLaunchKernelGGL(vct_root_counts_kernel, dim3(blocks_for(n)), dim3(256), 0, s, lv.pos_begin, cand_begin, child_offset, n, d_root_first, d_root_count);
        GMK_HIP_CHECK(hipGetLastError());
        GMK_HIP_CHECK(hipMemcpyAsync(counts.data(), d_root_count, un * 8, hipMemcpyDeviceToHost, s));
        GMK_HIP_CHECK(hipStreamSynchronize(s));
        long long next_count = 0;
        for (size_t g = 0; g < un; ++g) {
            begin[g] = next_count;
            if (!alive[g]) continue;
            if (counts[g] > max_positions) { alive[g] = 0; status[g] = GMK_VCT_BUDGET; --living; continue; }      // its level is discarded
            positions[g] += static_cast<uint32_t>(counts[g]);
            next_count += counts[g];
        }
        begin[un] = next_count;
        if (next_count > kMaxLevel) {
            gmk::set_error("gmk_vct_solve: level %d has %lld positions over the batch, more than %lld; lower max_positions or the batch", t + 1, next_count, kMaxLevel);
            return GMK_ERR_CAPACITY;
        }
        Level& next = levels[static_cast<size_t>(t) + 1];
        const size_t nc = static_cast<size_t>(next_count);
        uint8_t* next_lists;
        int32_t* next_lens;
        tree.want(next_lists, nc * kListStride); tree.want(next_lens, nc); tree.want(next.root, nc);
        want_level(next, static_cast<int>(next_count));
        if (!tree.take() || !set_level(next, begin)) return no_memory(t + 1);
        next.lists = next_lists; next.stride = kListStride; next.lens = next_lens;
        next.view.lists = next_lists; next.view.lens = next_lens;
        GMK_HIP_CHECK(hipMemcpyAsync(d_alive, alive.data(), un * 4, hipMemcpyHostToDevice, s));
        if (candidates > 0)
            hipLaunchKernelGGL(vct_emit_children_kernel, dim3(blocks_for(candidates)), dim3(256), 0, s, cand_lists, cand_lens, cand_pos, lv.root, reply, kept,
                               child_offset, d_root_first, next.pos_begin, d_alive, candidates, child_begin, child_count, next_lists, next_lens, next.root);
        GMK_HIP_CHECK(hipGetLastError());
        GMK_HIP_CHECK(hipStreamSynchronize(s));                    // the scratch is read until here, and `alive` is the host's
        scratch.release();
    }

    // ---- what is left has no win: NONE, or DEPTH where something was cut ----
    GMK_HIP_CHECK(hipMemcpyAsync(word.data(), d_cut, un * 4, hipMemcpyDeviceToHost, s));
    GMK_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t g = 0; g < un; ++g)
        if (alive[g]) status[g] = word[g] ? GMK_VCF_DEPTH : GMK_VCF_NONE;
    std::vector<LevelView> views(GMK_VCT_MAX_THREATS + 1);
    for (size_t t = 0; t < levels.size(); ++t) views[t] = levels[t].view;
    GMK_HIP_CHECK(hipMemcpyAsync(d_views, views.data(), views.size() * sizeof(LevelView), hipMemcpyHostToDevice, s));
    GMK_HIP_CHECK(hipMemcpyAsync(d_final_status, status.data(), un * 4, hipMemcpyHostToDevice, s));
    GMK_HIP_CHECK(hipMemcpyAsync(d_final_positions, positions.data(), un * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(vct_write_kernel, dim3(blocks_for(n)), dim3(256), 0, s, d_views, n, d_final_status, d_final_positions, d_status, d_move, d_threats,
                       d_positions, d_pv);
    GMK_HIP_CHECK(hipGetLastError());
    GMK_HIP_CHECK(hipStreamSynchronize(s));                        // the workspace goes when this returns
    return GMK_OK;
}

}  // namespace

extern "C" int gmk_vct_solve(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int max_depth, uint32_t budget, int flags,
                             int max_threats, int max_positions, int32_t* d_status, int32_t* d_move, int32_t* d_threats, uint32_t* d_positions,
                             uint8_t* d_pv, void* stream) {
    try {                                                          // the driver keeps its books in std::vector: nothing is thrown across the C boundary
        return vct_solve(d_moves, stride, d_lens, n, max_depth, budget, flags, max_threats, max_positions, d_status, d_move, d_threats, d_positions, d_pv, stream);
    } catch (const std::exception& e) {
        gmk::set_error("gmk_vct_solve: out of host memory (%s)", e.what());
        return GMK_ERR_HIP;
    }
}

extern "C" int gmk_vct_solve_host(const uint8_t* h_moves, int stride, const int32_t* h_lens, int n, int max_depth, uint32_t budget, int flags,
                                  int max_threats, int max_positions, int32_t* h_status, int32_t* h_move, int32_t* h_threats, uint32_t* h_positions,
                                  uint8_t* h_pv) {
    GMK_NEED_INIT();
    if (bad_arguments(h_moves, stride, h_lens, n, max_depth, flags, max_threats, max_positions)) {
        gmk::set_error("gmk_vct_solve_host: bad arguments (n >= 0, stride >= 1, max_depth in [1, %d], flags 0 or GMK_VCF_ITERATIVE, max_threats in [1, %d], "
                       "max_positions >= 1)", GMK_VCF_MAX_DEPTH, GMK_VCT_MAX_THREATS);
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    // one device block: moves | lens | status | move | threats | positions | pv
    const size_t un = static_cast<size_t>(n);
    gmk::Staging st("gmk_vct_solve_host");
    uint8_t *d_moves, *d_pv;
    int32_t *d_lens, *d_status, *d_move, *d_threats;
    uint32_t* d_positions;
    st.in(d_moves, h_moves, un * static_cast<size_t>(stride)); st.in(d_lens, h_lens, un);
    st.out(d_status, h_status, un); st.out(d_move, h_move, un); st.out(d_threats, h_threats, un); st.out(d_positions, h_positions, un);
    st.out(d_pv, h_pv, un * GMK_VCT_PV);
    int rc = st.take();
    if (rc == GMK_OK)
        rc = gmk_vct_solve(d_moves, stride, d_lens, n, max_depth, budget, flags, max_threats, max_positions, d_status, d_move, d_threats, d_positions, d_pv, nullptr);
    if (rc != GMK_OK) return rc;                                  // the device form's code and text, untouched
    GMK_STAGED(st, hipDeviceSynchronize());
    return st.download();
}
