// vcf_defend_kernel.hip -- K15: the moves that refute a forced win by continuous fours, exact and batched.
//
// The contract is in include/gomoku_hip.h ("K15").  gmk_vcf_defend is two launches on the caller's stream: K14's kernel with GMK_VCF_OPPONENT
// into the threat outputs, then the kernel below over jobs (position, cell), one 16-lane group per job, on K14's representation and with K14's
// walk, both vcf_device.h's (pass, start, step).  This file is what K15 puts around them: the jobs, the follow mode and the cells' verdicts.
// A job of a threatened position puts the defender's stone on its cell in registers and walks in one of two modes:
//     follow   the attacker's candidates of level i are reduced to pv[2 i], the threat's own move there: one pass per level, no stack, no
//              node.  It ends in LOSES (the line still wins), in FIVE (the stone made five: the init pass's "over" test) or in FAIL;
//     search   after FAIL the same group starts again from P + c as K14's full walk, with the whole budget.
// Occupied cells are settled when the job is taken.  A position whose threat is not WIN is settled by the job of its cell 0 alone: one pass for
// completing(defender), the FIVE cells, and every lane writes its row; its other 224 jobs are nothing.  A group keeps the planes, the threat
// and pv of the position it loaded last, so consecutive jobs of one position read the list once.  A group that has finished takes the next
// job of its wavefront's slice in the same pass.  No float, no atomics, no barrier, nothing allocated.
#include <algorithm>

#include "vcf_device.h"
#include "host_staging.h"

namespace {

using namespace gmk::vcf;
using gmk::misaligned;

enum : int { kSearch = 0, kFollow = 1, kWhole = 2 };

struct DefendParams {
    const uint8_t* moves;
    const int32_t* lens;
    int stride, n, max_depth, flags, per_wave;
    uint32_t budget;
    const int32_t* threat_status;
    const int32_t* threat_length;
    const uint8_t* threat_pv;
    uint8_t* verdict;
    uint8_t* cell_length;
    uint32_t* cell_nodes;
};

__global__ __launch_bounds__(64) void vcf_defend_kernel(DefendParams p) {
    __shared__ Stack stack;                                    // search mode only
    const Lane ln;
    const int y = ln.y, gbase = ln.gbase;
    const bool iterative = (p.flags & GMK_VCF_ITERATIVE) != 0;
    // this wavefront's slice of the n * 225 jobs: `left` jobs from (next_pos, next_cell) on; the grid covers exactly the jobs there are
    const long long total = static_cast<long long>(p.n) * kCells, first = static_cast<long long>(blockIdx.x) * p.per_wave;
    int next_pos = static_cast<int>(first / kCells), next_cell = static_cast<int>(first % kCells);
    int left = first < total ? static_cast<int>(std::min<long long>(p.per_wave, total - first)) : 0;

    Walk w;
    int mode = kSearch, pos = -1, cell = 0;
    // the position this group loaded last: its threat, and once `planes` is set its two planes (this lane's row) and this lane's four pv cells
    int held = -1, tstatus = GMK_VCF_BAD, tlen = 0;
    bool planes = false;
    uint32_t base_att = 0, base_def = 0, pvw = 0xFFFFFFFFu;

    const auto settle = [&](int verdict, int length, uint32_t count) {
        if (y == 0) {
            const size_t at = static_cast<size_t>(pos) * kCells + cell;
            p.verdict[at] = static_cast<uint8_t>(verdict);
            if (p.cell_length) p.cell_length[at] = static_cast<uint8_t>(length);
            if (p.cell_nodes) p.cell_nodes[at] = count;
        }
        w.state = kIdle;
    };
    // every cell of the position at once: occupied cells and positions that are over or no positions NONE, the cells of `fives` FIVE, the rest `other`
    const auto settle_rows = [&](uint32_t occupied, uint32_t fives, int other) {
        if (y < 15) {
            const size_t at = static_cast<size_t>(pos) * kCells + 15 * y;
            for (int x = 0; x < 15; ++x) {
                const int v = (occupied >> x) & 1u ? GMK_VCF_CELL_NONE : (fives >> x) & 1u ? GMK_VCF_CELL_FIVE : other;
                p.verdict[at + x] = static_cast<uint8_t>(v);
                if (p.cell_length) p.cell_length[at + x] = 0;
                if (p.cell_nodes) p.cell_nodes[at + x] = 0u;
            }
        }
        w.state = kIdle;
    };
    // P + c, nothing played: where follow starts, and where the search starts after it
    const auto to_root = [&](int new_mode) {
        const int jy = cell / 15;
        mode = new_mode;
        w.reset(base_att, base_def | (y == jy ? 1u << (cell - 15 * jy) : 0u), iterative ? 1 : p.max_depth);
    };
    // the search's result (K14's finish, without a pv)
    const auto finish = [&](int status, int length) {
        settle(status == GMK_VCF_WIN ? GMK_VCF_CELL_LOSES : status == GMK_VCF_NONE ? GMK_VCF_CELL_HOLDS : GMK_VCF_CELL_UNKNOWN, length, w.nodes);
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
                tstatus = p.threat_status[pos];
            }
            const bool win = tstatus == GMK_VCF_WIN;
            const bool searched = tstatus == GMK_VCF_NONE || tstatus == GMK_VCF_DEPTH || tstatus == GMK_VCF_BUDGET;
            if ((win || (searched && cell == 0)) && !planes) {
                // the threat's status says that the list is a position; the length's tests stay, so that nothing outside it is read whatever it says
                const Planes pl = load_moves<false>(p.moves, p.stride, p.lens, pos, ln);
                const bool black_attacks = !pl.bad && (pl.len & 1) != 0;   // the attacker is the side that is NOT to move
                base_att = black_attacks ? pl.black : pl.white;
                base_def = black_attacks ? pl.white : pl.black;
                tlen = p.threat_length[pos];
                const uint8_t* line = p.threat_pv + static_cast<size_t>(pos) * GMK_VCF_PV + 4 * y;
                pvw = static_cast<uint32_t>(line[0]) | static_cast<uint32_t>(line[1]) << 8 | static_cast<uint32_t>(line[2]) << 16 | static_cast<uint32_t>(line[3]) << 24;
                planes = true;
            }
            if (win) {
                const int jy = cell / 15;
                const bool taken = group_rows(y == jy && (((base_att | base_def) >> (cell - 15 * jy)) & 1u) != 0, gbase) != 0;
                if (taken) settle(GMK_VCF_CELL_NONE, 0, 0u);
                else to_root(kFollow);
            } else if (cell == 0) {
                if (searched) {
                    mode = kWhole;
                    w.reset(base_att, base_def, 0);                // one pass and no walk: no limit is read
                } else settle_rows(kRowMask, 0u, GMK_VCF_CELL_NONE);
            }
            // else: a cell of a position without a threat to follow, which the job of its cell 0 writes
        }
        left -= ho.taken;
        next_cell += ho.taken;
        if (next_cell >= kCells) { next_cell -= kCells; ++next_pos; }
        if (__ballot(w.state != kIdle) == 0ull) {                  // nothing to walk: only jobs that were settled as they were taken, or the slice is done
            if (left == 0) break;
            continue;
        }

        const Pass ps = pass(w, ln);
        const Follow fo = follow_level(w, ln, ps, pvw, tlen);

        // ---- decisions, the same in all sixteen lanes of a group ----
        if (w.state == kInit) {
            if (mode == kWhole) {
                settle_rows(w.att | w.def, ps.T, tstatus == GMK_VCF_NONE ? GMK_VCF_CELL_HOLDS : GMK_VCF_CELL_UNKNOWN);
            } else if (mode == kFollow) {
                if (ps.over) settle(GMK_VCF_CELL_FIVE, 0, 0u);
                else if (ps.f1 >= 0) settle(GMK_VCF_CELL_LOSES, 1, 0u);
                else if (fo.follows) { w.mask = fo.abit; w.state = kRun; }
                else to_root(kSearch);
            } else {
                if (ps.f1 >= 0) finish(GMK_VCF_WIN, 1);            // follow has settled these; kept so that the search is K14's walk whole
                else start(w, ps, failed);
            }
        } else if (w.state == kRun && mode == kFollow) {
            if (ps.f1 < 0) to_root(kSearch);                       // the threat's move is no four any more
            else if (ps.f2 >= 0) settle(GMK_VCF_CELL_LOSES, w.depth + 2, 0u);
            else if (fo.follows) { ++w.depth; w.mask = fo.abit; }  // a and its forced reply stay on the board
            else to_root(kSearch);
        } else if (w.state == kRun) {
            step(w, ln, ps, p.budget, stack, [&](int, int, int) { finish(GMK_VCF_WIN, w.depth + 2); }, [&]() { finish(GMK_VCF_BUDGET, 0); }, failed);
        }
    }
}


bool bad_arguments(const void* moves, int stride, const void* lens, int n, int max_depth, int flags, const void* status, const void* length,
                   const void* pv, const void* verdict) {
    return n < 0 || stride < 1 || max_depth < 1 || max_depth > GMK_VCF_MAX_DEPTH || (flags & ~GMK_VCF_ITERATIVE) != 0 ||
           (n > 0 && (!moves || !lens || !status || !length || !pv || !verdict));
}

}  // namespace

extern "C" int gmk_vcf_defend(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int max_depth, uint32_t budget, int flags,
                              int32_t* d_threat_status, int32_t* d_threat_length, uint8_t* d_threat_pv, uint32_t* d_threat_nodes,
                              uint8_t* d_verdict, uint8_t* d_cell_length, uint32_t* d_cell_nodes, void* stream) {
    GMK_NEED_INIT();
    if (bad_arguments(d_moves, stride, d_lens, n, max_depth, flags, d_threat_status, d_threat_length, d_threat_pv, d_verdict) || misaligned(d_lens, 4) ||
        misaligned(d_threat_status, 4) || misaligned(d_threat_length, 4) || misaligned(d_threat_nodes, 4) || misaligned(d_cell_nodes, 4)) {
        gmk::set_error("gmk_vcf_defend: bad arguments (n >= 0, stride >= 1, max_depth in [1, %d], flags 0 or GMK_VCF_ITERATIVE; the threat's status, length "
                       "and pv and d_verdict not NULL; d_lens and the 4-byte outputs 4-byte aligned)", GMK_VCF_MAX_DEPTH);
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    const int rc = gmk_vcf_solve(d_moves, stride, d_lens, n, max_depth, budget, flags | GMK_VCF_OPPONENT, d_threat_status, nullptr, d_threat_length,
                                 d_threat_nodes, d_threat_pv, stream);
    if (rc != GMK_OK) return rc;
    DefendParams prm{};
    prm.moves = d_moves; prm.lens = d_lens; prm.stride = stride; prm.n = n; prm.max_depth = max_depth; prm.flags = flags; prm.budget = budget;
    prm.threat_status = d_threat_status; prm.threat_length = d_threat_length; prm.threat_pv = d_threat_pv;
    prm.verdict = d_verdict; prm.cell_length = d_cell_length; prm.cell_nodes = d_cell_nodes;
    const SlicePlan plan = cell_slices(n, gmk::device_state().cu_count);
    prm.per_wave = plan.per_wave;
    hipLaunchKernelGGL(vcf_defend_kernel, dim3(plan.grid), dim3(64), 0, static_cast<hipStream_t>(stream), prm);
    GMK_HIP_CHECK(hipGetLastError());
    return GMK_OK;
}

extern "C" int gmk_vcf_defend_host(const uint8_t* h_moves, int stride, const int32_t* h_lens, int n, int max_depth, uint32_t budget, int flags,
                                   int32_t* h_threat_status, int32_t* h_threat_length, uint8_t* h_threat_pv, uint32_t* h_threat_nodes,
                                   uint8_t* h_verdict, uint8_t* h_cell_length, uint32_t* h_cell_nodes) {
    GMK_NEED_INIT();
    if (bad_arguments(h_moves, stride, h_lens, n, max_depth, flags, h_threat_status, h_threat_length, h_threat_pv, h_verdict)) {
        gmk::set_error("gmk_vcf_defend_host: bad arguments (n >= 0, stride >= 1, max_depth in [1, %d], flags 0 or GMK_VCF_ITERATIVE; the threat's status, "
                       "length and pv and h_verdict not NULL)", GMK_VCF_MAX_DEPTH);
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    // one device block: moves | lens | threat status | length | nodes | pv | verdict | cell length | cell nodes
    const size_t un = static_cast<size_t>(n), cells = un * 225;
    gmk::Staging st("gmk_vcf_defend_host");
    uint8_t *d_moves, *d_pv, *d_verdict, *d_cell_length;
    int32_t *d_lens, *d_status, *d_length;
    uint32_t *d_nodes, *d_cell_nodes;
    st.in(d_moves, h_moves, un * static_cast<size_t>(stride)); st.in(d_lens, h_lens, un);
    st.out(d_status, h_threat_status, un); st.out(d_length, h_threat_length, un); st.out(d_nodes, h_threat_nodes, un);
    st.out(d_pv, h_threat_pv, un * GMK_VCF_PV); st.out(d_verdict, h_verdict, cells); st.out(d_cell_length, h_cell_length, cells);
    st.out(d_cell_nodes, h_cell_nodes, cells);
    int rc = st.take();
    if (rc == GMK_OK)
        rc = gmk_vcf_defend(d_moves, stride, d_lens, n, max_depth, budget, flags, d_status, d_length, d_pv, d_nodes, d_verdict, d_cell_length, d_cell_nodes, nullptr);
    if (rc != GMK_OK) return rc;                                  // the device form's code and text, untouched
    GMK_STAGED(st, hipDeviceSynchronize());
    return st.download();
}
