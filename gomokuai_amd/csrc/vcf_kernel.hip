// vcf_kernel.hip -- K14: the forced-win solver by continuous fours (VCF), exact and batched.
//
// The contract is the walk in include/gomoku_hip.h ("K14"): the attacker makes a four, the defender's one reply is forced, and so on until a
// double four or a five.  Everything is geometry on two 15 x 15 bit planes; the pattern automaton is not involved and there is no float.
// The walk itself is vcf_device.h's, where the mapping is told: one board ROW per lane, sixteen lanes per position, four positions per wavefront,
// one wavefront per workgroup; a pass of the loop (gmk::vcf::pass) in the same instructions for every group, and then a few group-uniform
// decisions (start, step): win, budget, descend (one LDS word per lane and level), or undo by XOR and climb.  A child never has a completing
// cell of its own (its parent's only one was just taken), so completing(attacker) is evaluated once per node, for the candidate test that
// counts the node.  Four-making cells are found plane-wide: the empties of a five-window with three attacker stones and no defender stone (with
// no completing cell on the board "at least three" is "exactly three"); whatever that mask offers is still held to F != {} before it counts, so
// `nodes` is the contract's count.
// This file is K14's own around that walk: the move-list loader with its BAD verdicts, iterative deepening, and a finish that writes the whole
// principal variation.  Divergent trees cost idle passes, not divergent code; a group that has finished takes the next position of its
// wavefront's slice in the same pass.  No atomics, no barrier, nothing allocated: the device entry is one launch.
#include <algorithm>

#include "vcf_device.h"
#include "host_staging.h"

namespace {

using namespace gmk::vcf;
using gmk::misaligned;

struct VcfParams {
    const uint8_t* moves;
    const int32_t* lens;
    int stride, n, max_depth, flags, per_wave;
    uint32_t budget;
    int32_t* status;
    int32_t* move;
    int32_t* length;
    uint32_t* nodes;
    uint8_t* pv;
};

__global__ __launch_bounds__(64) void vcf_kernel(VcfParams p) {
    __shared__ Stack stack;
    const Lane ln;
    const int y = ln.y;
    const bool iterative = (p.flags & GMK_VCF_ITERATIVE) != 0;
    // this wavefront's slice of the batch: `left` positions from `next` on
    const long long first = static_cast<long long>(blockIdx.x) * p.per_wave;
    int next = first < p.n ? static_cast<int>(first) : p.n;
    int left = (first + p.per_wave < p.n ? static_cast<int>(first + p.per_wave) : p.n) - next;

    Walk w;
    int pos = -1;

    // The group's result.  t0 .. t2 are the cells that end a winning line after the 2 * depth cells on the stack (255: none).
    const auto finish = [&](int status, int t0, int t1, int t2) {
        const bool win = status == GMK_VCF_WIN;
        if (y == 0) {
            if (p.status) p.status[pos] = status;
            if (p.move) p.move[pos] = !win ? -1 : w.depth > 0 ? level_c(stack[0][ln.lane]) : t0;
            if (p.length) p.length[pos] = !win ? 0 : w.depth + (t1 == 255 ? 1 : 2);
            if (p.nodes) p.nodes[pos] = w.nodes;
        }
        if (p.pv) {
            uint8_t* out = p.pv + static_cast<size_t>(pos) * GMK_VCF_PV + 4 * y;
#pragma unroll
            for (int i = 0; i < 4; ++i) out[i] = static_cast<uint8_t>(win ? line_cell(stack, ln, w.depth, 4 * y + i, t0, t1, t2) : 255u);
        }
        w.state = kIdle;
    };
    const auto failed = [&]() { limit_failed(w, iterative, p.max_depth, [&](int status) { finish(status, 255, 255, 255); }); };

    for (;;) {
        // ---- groups without a position take the next ones of this wavefront's slice ----
        const HandOut ho = hand_out(w.state, ln, left);
        if (w.state == kIdle && ho.rank < left) {
            pos = next + ho.rank;
            const Planes pl = load_moves<true>(p.moves, p.stride, p.lens, pos, ln);
            const bool black_attacks = ((pl.len & 1) == 0) != ((p.flags & GMK_VCF_OPPONENT) != 0);
            w.reset(black_attacks ? pl.black : pl.white, black_attacks ? pl.white : pl.black, iterative ? 1 : p.max_depth);
            if (pl.bad) finish(GMK_VCF_BAD, 255, 255, 255);
        }
        left -= ho.taken;
        next += ho.taken;
        if (__ballot(w.state != kIdle) == 0ull) {                  // nothing to walk: only lists that were no positions, or the slice is done
            if (left == 0) break;
            continue;
        }

        const Pass ps = pass(w, ln);

        // ---- decisions, the same in all sixteen lanes of a group ----
        if (w.state == kInit) {
            if (ps.over) finish(GMK_VCF_OVER, 255, 255, 255);
            else if (ps.f1 >= 0) finish(GMK_VCF_WIN, ps.f1, 255, 255);
            else start(w, ps, failed);
        } else if (w.state == kRun) {
            step(w, ln, ps, p.budget, stack, [&](int c, int f1, int f2) { finish(GMK_VCF_WIN, c, f1, f2); },
                 [&]() { finish(GMK_VCF_BUDGET, 255, 255, 255); }, failed);
        }
    }
}


constexpr int kKnownFlags = GMK_VCF_OPPONENT | GMK_VCF_ITERATIVE;

}  // namespace

extern "C" int gmk_vcf_solve(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int max_depth, uint32_t budget, int flags,
                             int32_t* d_status, int32_t* d_move, int32_t* d_length, uint32_t* d_nodes, uint8_t* d_pv, void* stream) {
    GMK_NEED_INIT();
    if (n < 0 || stride < 1 || max_depth < 1 || max_depth > GMK_VCF_MAX_DEPTH || (flags & ~kKnownFlags) != 0 || (n > 0 && (!d_moves || !d_lens)) ||
        misaligned(d_lens, 4) || misaligned(d_status, 4) || misaligned(d_move, 4) || misaligned(d_length, 4) || misaligned(d_nodes, 4)) {
        gmk::set_error("gmk_vcf_solve: bad arguments (n >= 0, stride >= 1, max_depth in [1, %d], flags in [0, 3]; d_lens and the int32 outputs 4-byte aligned)",
                       GMK_VCF_MAX_DEPTH);
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    VcfParams prm{};
    prm.moves = d_moves; prm.lens = d_lens; prm.stride = stride; prm.n = n; prm.max_depth = max_depth; prm.flags = flags; prm.budget = budget;
    prm.status = d_status; prm.move = d_move; prm.length = d_length; prm.nodes = d_nodes; prm.pv = d_pv;
    // A wavefront walks a slice of the batch, four positions at a time.  Small batches spread over the chip one quartet per wavefront; large ones
    // give every wavefront sixteen positions, so that a group whose tree was small has others to take while a neighbour is still deep in one.
    const int cus = std::max(1, gmk::device_state().cu_count);
    prm.per_wave = n <= 4 * 8 * cus ? 4 : 16;
    const int grid = (n + prm.per_wave - 1) / prm.per_wave;
    hipLaunchKernelGGL(vcf_kernel, dim3(grid), dim3(64), 0, static_cast<hipStream_t>(stream), prm);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_vcf_solve_host(const uint8_t* h_moves, int stride, const int32_t* h_lens, int n, int max_depth, uint32_t budget, int flags,
                                  int32_t* h_status, int32_t* h_move, int32_t* h_length, uint32_t* h_nodes, uint8_t* h_pv) {
    GMK_NEED_INIT();
    if (n < 0 || stride < 1 || max_depth < 1 || max_depth > GMK_VCF_MAX_DEPTH || (flags & ~kKnownFlags) != 0 || (n > 0 && (!h_moves || !h_lens))) {
        gmk::set_error("gmk_vcf_solve_host: bad arguments (n >= 0, stride >= 1, max_depth in [1, %d], flags in [0, 3])", GMK_VCF_MAX_DEPTH);
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    // one device block: moves | lens | status | move | length | nodes | pv
    const size_t un = static_cast<size_t>(n);
    gmk::Staging st("gmk_vcf_solve_host");
    uint8_t *d_moves, *d_pv;
    int32_t *d_lens, *d_status, *d_move, *d_length;
    uint32_t* d_nodes;
    st.in(d_moves, h_moves, un * static_cast<size_t>(stride)); st.in(d_lens, h_lens, un);
    st.out(d_status, h_status, un); st.out(d_move, h_move, un); st.out(d_length, h_length, un); st.out(d_nodes, h_nodes, un);
    st.out(d_pv, h_pv, un * GMK_VCF_PV);
    int rc = st.take();
    if (rc == GMK_OK) rc = gmk_vcf_solve(d_moves, stride, d_lens, n, max_depth, budget, flags, d_status, d_move, d_length, d_nodes, d_pv, nullptr);
    if (rc != GMK_OK) return rc;                                  // the device form's code and text, untouched
    GMK_STAGED(st, hipDeviceSynchronize());
    return st.download();
}
