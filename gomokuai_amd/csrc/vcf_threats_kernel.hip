// vcf_threats_kernel.hip -- K17: what a stone of the side to move threatens, for every cell, exact and batched.
//
// The contract is in include/gomoku_hip.h ("K17").  gmk_vcf_threats is two launches on the caller's stream: K14's kernel for the side to move
// into the own outputs, then the kernel below over jobs (position, cell), one 16-lane group per job, on K14's representation and with K14's
// walk, both vcf_device.h's (pass, start, step).  This file is what K17 puts around them: the jobs, the cheap verdicts at a root and the cells'
// verdicts.  A job puts the attacker's stone on its cell in registers and starts K14's walk for the attacker on that board, as if the defender
// had passed.  The walk's first pass already holds the three cheap verdicts, in the contract's order: a five stands (the position itself has
// none, so the stone made it: FIVE), the defender has a completing cell (IGNORES), the attacker has one (FOUR, one cell or several).  Only a
// cell with none of the three is searched, with the whole budget.
// Occupied cells are settled when the job is taken.  A position that is over or no position is settled by the job of its cell 0 alone, every
// lane writing its row; its other 224 jobs are nothing.  A group keeps the planes of the position it loaded last, so consecutive jobs of one
// position read the list once.  A group that has finished takes the next job of its wavefront's slice in the same pass.  No float, no
// atomics, no barrier, nothing allocated.
#include <algorithm>

#include "vcf_device.h"
#include "host_staging.h"

namespace {

using namespace gmk::vcf;
using gmk::misaligned;

struct ThreatsParams {
    const uint8_t* moves;
    const int32_t* lens;
    int stride, n, max_depth, flags, per_wave;
    uint32_t budget;
    const int32_t* own_status;
    uint8_t* verdict;
    uint8_t* cell_length;
    uint32_t* cell_nodes;
};

__global__ __launch_bounds__(64) void vcf_threats_kernel(ThreatsParams p) {
    __shared__ Stack stack;
    const Lane ln;
    const int y = ln.y, gbase = ln.gbase;
    const bool iterative = (p.flags & GMK_VCF_ITERATIVE) != 0;
    // this wavefront's slice of the n * 225 jobs: `left` jobs from (next_pos, next_cell) on; the grid covers exactly the jobs there are
    const long long total = static_cast<long long>(p.n) * kCells, first = static_cast<long long>(blockIdx.x) * p.per_wave;
    int next_pos = static_cast<int>(first / kCells), next_cell = static_cast<int>(first % kCells);
    int left = first < total ? static_cast<int>(std::min<long long>(p.per_wave, total - first)) : 0;

    Walk w;
    int pos = -1, cell = 0;
    // the position this group loaded last: its own status, and once `planes` is set its two planes (this lane's row)
    int held = -1, ostatus = GMK_VCF_BAD;
    bool planes = false;
    uint32_t base_att = 0, base_def = 0;

    const auto settle = [&](int verdict, int length, uint32_t count) {
        if (y == 0) {
            const size_t at = static_cast<size_t>(pos) * kCells + cell;
            p.verdict[at] = static_cast<uint8_t>(verdict);
            if (p.cell_length) p.cell_length[at] = static_cast<uint8_t>(length);
            if (p.cell_nodes) p.cell_nodes[at] = count;
        }
        w.state = kIdle;
    };
    // the search's result (K14's finish, without a pv)
    const auto finish = [&](int status, int length) {
        settle(status == GMK_VCF_WIN ? GMK_VCF_THREAT_WINS : status == GMK_VCF_NONE ? GMK_VCF_THREAT_QUIET : GMK_VCF_THREAT_UNKNOWN, length, w.nodes);
    };
    const auto failed = [&]() { limit_failed(w, iterative, p.max_depth, [&](int status) { finish(status, 0); }); };

    for (;;) {
        // ---- groups without a job take the next ones of this wavefront's slice ----
        const HandOut ho = hand_out(w.state, ln, left);
        if (w.state == kIdle && ho.rank < left) {
            pos = next_pos;
            cell = next_cell + ho.rank;
            if (cell >= kCells) { cell -= kCells; ++pos; }
            if (pos != held) {
                held = pos;
                planes = false;
                ostatus = p.own_status[pos];
            }
            const bool searched = ostatus == GMK_VCF_NONE || ostatus == GMK_VCF_WIN || ostatus == GMK_VCF_DEPTH || ostatus == GMK_VCF_BUDGET;
            if (searched && !planes) {
                // the own status says that the list is a position; the length's tests stay, so that nothing outside it is read whatever it says
                const Planes pl = load_moves<false>(p.moves, p.stride, p.lens, pos, ln);
                const bool black_attacks = pl.bad || (pl.len & 1) == 0;    // the attacker is the side to move
                base_att = black_attacks ? pl.black : pl.white;
                base_def = black_attacks ? pl.white : pl.black;
                planes = true;
            }
            if (searched) {
                const int jy = cell / 15;
                const uint32_t jbit = y == jy ? 1u << (cell - 15 * jy) : 0u;
                const bool taken = group_rows(((base_att | base_def) & jbit) != 0, gbase) != 0;
                if (taken) settle(GMK_VCF_THREAT_NONE, 0, 0u);
                else w.reset(base_att | jbit, base_def, iterative ? 1 : p.max_depth);      // P + [c], the defender passes: K14's root with GMK_VCF_OPPONENT
            } else if (cell == 0) {
                // over, or no position: every cell at once
                if (y < 15) {
                    const size_t at = static_cast<size_t>(pos) * kCells + 15 * y;
                    for (int x = 0; x < 15; ++x) {
                        p.verdict[at + x] = static_cast<uint8_t>(GMK_VCF_THREAT_NONE);
                        if (p.cell_length) p.cell_length[at + x] = 0;
                        if (p.cell_nodes) p.cell_nodes[at + x] = 0u;
                    }
                }
            }
            // else: a cell of such a position, which the job of its cell 0 writes
        }
        left -= ho.taken;
        next_cell += ho.taken;
        if (next_cell >= kCells) { next_cell -= kCells; ++next_pos; }
        if (__ballot(w.state != kIdle) == 0ull) {                  // nothing to walk: only jobs that were settled as they were taken, or the slice is done
            if (left == 0) break;
            continue;
        }

        const Pass ps = pass(w, ln);

        // ---- decisions, the same in all sixteen lanes of a group ----
        if (w.state == kInit) {
            // the three cheap verdicts hold at every limit of an iterative walk alike, so only its first pass can meet them
            if (ps.over) settle(GMK_VCF_THREAT_FIVE, 0, 0u);
            else if (ps.t1 >= 0) settle(GMK_VCF_THREAT_IGNORES, 0, 0u);
            else if (ps.f1 >= 0) settle(GMK_VCF_THREAT_FOUR, ps.f2 >= 0 ? 2 : 1, 0u);
            else start(w, ps, failed);                             // its t2 >= 0 cannot be: the defender has no completing cell
        } else if (w.state == kRun) {
            step(w, ln, ps, p.budget, stack, [&](int, int, int) { finish(GMK_VCF_WIN, w.depth + 2); }, [&]() { finish(GMK_VCF_BUDGET, 0); }, failed);
        }
    }
}


bool bad_arguments(const void* moves, int stride, const void* lens, int n, int max_depth, int flags, const void* status, const void* verdict) {
    return n < 0 || stride < 1 || max_depth < 1 || max_depth > GMK_VCF_MAX_DEPTH || (flags & ~GMK_VCF_ITERATIVE) != 0 ||
           (n > 0 && (!moves || !lens || !status || !verdict));
}

}  // namespace

extern "C" int gmk_vcf_threats(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int max_depth, uint32_t budget, int flags,
                               int32_t* d_own_status, int32_t* d_own_move, int32_t* d_own_length, uint32_t* d_own_nodes, uint8_t* d_own_pv,
                               uint8_t* d_verdict, uint8_t* d_cell_length, uint32_t* d_cell_nodes, void* stream) {
    GMK_NEED_INIT();
    if (bad_arguments(d_moves, stride, d_lens, n, max_depth, flags, d_own_status, d_verdict) || misaligned(d_lens, 4) || misaligned(d_own_status, 4) ||
        misaligned(d_own_move, 4) || misaligned(d_own_length, 4) || misaligned(d_own_nodes, 4) || misaligned(d_cell_nodes, 4)) {
        gmk::set_error("gmk_vcf_threats: bad arguments (n >= 0, stride >= 1, max_depth in [1, %d], flags 0 or GMK_VCF_ITERATIVE; d_own_status and "
                       "d_verdict not NULL; d_lens and the 4-byte outputs 4-byte aligned)", GMK_VCF_MAX_DEPTH);
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    const int rc = gmk_vcf_solve(d_moves, stride, d_lens, n, max_depth, budget, flags, d_own_status, d_own_move, d_own_length, d_own_nodes, d_own_pv, stream);
    if (rc != GMK_OK) return rc;
    ThreatsParams prm{};
    prm.moves = d_moves; prm.lens = d_lens; prm.stride = stride; prm.n = n; prm.max_depth = max_depth; prm.flags = flags; prm.budget = budget;
    prm.own_status = d_own_status;
    prm.verdict = d_verdict; prm.cell_length = d_cell_length; prm.cell_nodes = d_cell_nodes;
    const SlicePlan plan = cell_slices(n, gmk::device_state().cu_count);       // K15's slices
    prm.per_wave = plan.per_wave;
    hipLaunchKernelGGL(vcf_threats_kernel, dim3(plan.grid), dim3(64), 0, static_cast<hipStream_t>(stream), prm);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_vcf_threats_host(const uint8_t* h_moves, int stride, const int32_t* h_lens, int n, int max_depth, uint32_t budget, int flags,
                                    int32_t* h_own_status, int32_t* h_own_move, int32_t* h_own_length, uint32_t* h_own_nodes, uint8_t* h_own_pv,
                                    uint8_t* h_verdict, uint8_t* h_cell_length, uint32_t* h_cell_nodes) {
    GMK_NEED_INIT();
    if (bad_arguments(h_moves, stride, h_lens, n, max_depth, flags, h_own_status, h_verdict)) {
        gmk::set_error("gmk_vcf_threats_host: bad arguments (n >= 0, stride >= 1, max_depth in [1, %d], flags 0 or GMK_VCF_ITERATIVE; h_own_status and "
                       "h_verdict not NULL)", GMK_VCF_MAX_DEPTH);
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    // one device block: moves | lens | own status | move | length | nodes | pv | verdict | cell length | cell nodes
    const size_t un = static_cast<size_t>(n), cells = un * 225;
    gmk::Staging st("gmk_vcf_threats_host");
    uint8_t *d_moves, *d_pv, *d_verdict, *d_cell_length;
    int32_t *d_lens, *d_status, *d_move, *d_length;
    uint32_t *d_nodes, *d_cell_nodes;
    st.in(d_moves, h_moves, un * static_cast<size_t>(stride)); st.in(d_lens, h_lens, un);
    st.out(d_status, h_own_status, un); st.out(d_move, h_own_move, un); st.out(d_length, h_own_length, un); st.out(d_nodes, h_own_nodes, un);
    st.out(d_pv, h_own_pv, un * GMK_VCF_PV); st.out(d_verdict, h_verdict, cells); st.out(d_cell_length, h_cell_length, cells);
    st.out(d_cell_nodes, h_cell_nodes, cells);
    int rc = st.take();
    if (rc == GMK_OK)
        rc = gmk_vcf_threats(d_moves, stride, d_lens, n, max_depth, budget, flags, d_status, d_move, d_length, d_nodes, d_pv, d_verdict, d_cell_length, d_cell_nodes,
                             nullptr);
    if (rc != GMK_OK) return rc;                                  // the device form's code and text, untouched
    GMK_STAGED(st, hipDeviceSynchronize());
    return st.download();
}
