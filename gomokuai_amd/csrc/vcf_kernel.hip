// vcf_kernel.hip -- K14: the forced-win solver by continuous fours (VCF), exact and batched.
//
// The contract is the walk in include/gomoku_hip.h ("K14"): the attacker makes a four, the defender's one reply is forced, and so on until a
// double four or a five.  Everything is geometry on two 15 x 15 bit planes; the pattern automaton is not involved and there is no float.
// Mapping: one board ROW per lane, sixteen lanes per position (lane 15 of a group is an off-board row of zeros), four positions per wavefront,
// one wavefront per workgroup.  Horizontal neighbours are bit shifts; vertical and diagonal neighbours are the rows y-4 .. y+4, fetched with
// DPP row shifts, which stay inside a 16-lane row and deliver zero from outside it -- exactly a board edge.  One pass of the loop is, for every
// group at once and in the same instructions:
//     take the lowest candidate c of the current level, play it, F = completing(attacker)                 (8 row shifts)
//     if F is one cell r: play r, T = completing(defender), C = the four-making cells of the child       (16 row shifts)
// and then a few group-uniform decisions: win, budget, descend (push mask, c, r: one LDS word per lane and level), or undo by XOR and climb
// while the levels above have no candidate left.  A child never has a completing cell of its own (its parent's only one was just taken), so
// completing(attacker) is evaluated once per node, for the candidate test that counts the node.  Four-making cells are found plane-wide: the
// empties of a five-window with three attacker stones and no defender stone (with no completing cell on the board "at least three" is
// "exactly three"); whatever that mask offers is still held to F != {} before it counts, so `nodes` is the contract's count.
// Divergent trees cost idle passes, not divergent code; a group that has finished takes the next position of its wavefront's slice in the
// same pass.  No atomics, no barrier, nothing allocated: the device entry is one launch.
// The row gather and the geometry of fours are in vcf_device.h, which K15 (vcf_defend_kernel.hip) shares.
#include <algorithm>

#include "vcf_device.h"

namespace {

using namespace gmk::vcf;

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
    __shared__ uint32_t stack[kLevels][64];                    // per level and lane: candidates left 0..14, "the level has more" 15, c 16..23, r 24..31
    const int lane = threadIdx.x, y = lane & 15, group = lane >> 4, gbase = lane & 48;
    const uint32_t board_row = y < 15 ? kRowMask : 0u;
    const bool iterative = (p.flags & GMK_VCF_ITERATIVE) != 0;
    const long long first = static_cast<long long>(blockIdx.x) * p.per_wave;
    int next = first < p.n ? static_cast<int>(first) : p.n;
    const int end = first + p.per_wave < p.n ? static_cast<int>(first + p.per_wave) : p.n;

    int state = kIdle, pos = -1, depth = 0, limit = 0;
    bool cut = false, more = false;
    uint32_t nodes = 0, att = 0, def = 0, mask = 0;

    // The group's result.  t0 .. t2 are the cells that end a winning line after the 2 * depth cells on the stack (255: none).
    const auto finish = [&](int status, int t0, int t1, int t2) {
        const bool win = status == GMK_VCF_WIN;
        if (y == 0) {
            if (p.status) p.status[pos] = status;
            if (p.move) p.move[pos] = !win ? -1 : depth > 0 ? static_cast<int>((stack[0][lane] >> 16) & 255u) : t0;
            if (p.length) p.length[pos] = !win ? 0 : depth + (t1 == 255 ? 1 : 2);
            if (p.nodes) p.nodes[pos] = nodes;
        }
        if (p.pv) {
            uint8_t* out = p.pv + static_cast<size_t>(pos) * GMK_VCF_PV + 4 * y;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 4 * y + i, tail = k - 2 * depth;
                uint32_t v = 255u;
                if (win) {
                    if (tail < 0) { const uint32_t w = stack[k >> 1][lane]; v = (k & 1) ? w >> 24 : (w >> 16) & 255u; }
                    else if (tail < 3) v = static_cast<uint32_t>(tail == 0 ? t0 : tail == 1 ? t1 : t2);
                }
                out[i] = static_cast<uint8_t>(v);
            }
        }
        state = kIdle;
    };
    // The walk at this limit has failed at the root, with every move undone.
    const auto limit_failed = [&]() {
        if (!cut) finish(GMK_VCF_NONE, 255, 255, 255);
        else if (iterative && limit < p.max_depth) { ++limit; cut = false; state = kInit; }
        else finish(GMK_VCF_DEPTH, 255, 255, 255);
    };

    for (;;) {
        // ---- groups without a position take the next ones of this wavefront's slice ----
        const unsigned long long idle = __ballot(state == kIdle);
        int rank = 0, takers = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int is_idle = static_cast<int>((idle >> (16 * g)) & 1ull);
            if (g < group) rank += is_idle;
            takers += is_idle;
        }
        if (state == kIdle && next + rank < end) {
            pos = next + rank;
            const int len = p.lens[pos];
            bool bad = len < 0 || len > kCells || len > p.stride;
            uint32_t black = 0, white = 0;
            bool clash = false;
            if (!bad) {
                const uint8_t* list = p.moves + static_cast<size_t>(pos) * static_cast<size_t>(p.stride);
                for (int i = 0; i < len; ++i) {
                    const int cell = list[i];
                    if (cell >= kCells) { bad = true; continue; }
                    const int r = cell / 15;
                    if (r != y) continue;
                    const uint32_t bit = 1u << (cell - 15 * r);
                    clash |= ((black | white) & bit) != 0;
                    if (i & 1) white |= bit; else black |= bit;
                }
            }
            bad |= group_rows(clash, gbase) != 0;
            const bool black_attacks = ((len & 1) == 0) != ((p.flags & GMK_VCF_OPPONENT) != 0);
            att = black_attacks ? black : white;
            def = black_attacks ? white : black;
            nodes = 0; depth = 0; cut = false; more = false; mask = 0;
            limit = iterative ? 1 : p.max_depth;
            state = kInit;
            if (bad) finish(GMK_VCF_BAD, 255, 255, 255);
        }
        next = next + takers < end ? next + takers : end;
        if (__ballot(state != kIdle) == 0ull) {                    // nothing to walk: only lists that were no positions, or the slice is done
            if (next >= end) break;
            continue;
        }

        // ---- the pass: every group in the same instructions ----
        const bool trying = state == kRun;                         // such a group has a candidate: `mask` is not empty
        uint32_t popped = trying ? mask : 0u;
        const int c = take_lowest(popped, y, gbase);
        const uint32_t left = group_rows(popped != 0, gbase);
        const int cy = trying ? c / 15 : 0;
        const uint32_t cbit = trying ? 1u << (c - 15 * cy) : 0u;
        if (trying) {
            mask = popped;
            more = left != 0;
            if (y == cy) att |= cbit;
        }
        uint32_t A[9], D[9], N[9];
        gather_rows(att, A);
        uint32_t F = completing(A, board_row & ~(att | def));
        const int f1 = take_lowest(F, y, gbase), f2 = take_lowest(F, y, gbase);
        const bool replied = trying && f1 >= 0 && f2 < 0;          // the forced reply goes on the board
        const int ry = replied ? f1 / 15 : 0;
        const uint32_t rbit = replied ? 1u << (f1 - 15 * ry) : 0u;
        if (replied && y == ry) def |= rbit;
        const uint32_t empty = board_row & ~(att | def);
        gather_rows(def, D);
        gather_rows(empty | att, N);
        uint32_t T = completing(D, empty);
        uint32_t C = four_making(A, N, empty);
        if (group_rows(T != 0, gbase)) C &= T;                     // a defender four: only its blocking cell is a candidate
        const int t1 = take_lowest(T, y, gbase), t2 = take_lowest(T, y, gbase);
        (void)t1;
        const bool child_has = group_rows(C != 0, gbase) != 0;
        bool over = false;
        if (__ballot(state == kInit) != 0ull) over = group_rows((five(A) | five(D)) != 0, gbase) != 0;

        // ---- decisions, the same in all sixteen lanes of a group ----
        if (state == kInit) {
            if (over) finish(GMK_VCF_OVER, 255, 255, 255);
            else if (f1 >= 0) finish(GMK_VCF_WIN, f1, 255, 255);
            else {
                bool fail = t2 >= 0;
                if (!fail && 2 > limit) { cut = true; fail = true; }
                if (!fail && !child_has) fail = true;
                if (fail) limit_failed();
                else { mask = C; more = true; state = kRun; }
            }
        } else if (trying) {
            bool retract = true;
            if (f1 < 0) {
                // not a four: no candidate and no node (the plane-wide mask does not offer such a cell; this keeps the count exact regardless)
            } else if (nodes == p.budget) {
                finish(GMK_VCF_BUDGET, 255, 255, 255);
            } else {
                ++nodes;
                if (f2 >= 0) finish(GMK_VCF_WIN, c, f1, f2);
                else {
                    bool fail = t2 >= 0;
                    if (!fail && depth + 3 > limit) { cut = true; fail = true; }
                    if (!fail && !child_has) fail = true;
                    if (!fail) {
                        stack[depth][lane] = mask | (more ? 0x8000u : 0u) | (static_cast<uint32_t>(c) << 16) | (static_cast<uint32_t>(f1) << 24);
                        ++depth;
                        mask = C; more = true; retract = false;
                    } else if (y == ry) def ^= rbit;
                }
            }
            if (state == kRun && retract) {
                if (y == cy) att ^= cbit;
                while (!more) {                                    // climb while the level has nothing left
                    if (depth == 0) { limit_failed(); break; }
                    --depth;
                    const uint32_t w = stack[depth][lane];
                    mask = w & kRowMask;
                    more = (w & 0x8000u) != 0;
                    const int uc = static_cast<int>((w >> 16) & 255u), ur = static_cast<int>(w >> 24);
                    if (y == uc / 15) att ^= 1u << (uc % 15);
                    if (y == ur / 15) def ^= 1u << (ur % 15);
                }
            }
        }
    }
}

bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

constexpr int kKnownFlags = GMK_VCF_OPPONENT | GMK_VCF_ITERATIVE;

}  // namespace

extern "C" int gmk_vcf_solve(const uint8_t* d_moves, int stride, const int32_t* d_lens, int n, int max_depth, uint32_t budget, int flags,
                             int32_t* d_status, int32_t* d_move, int32_t* d_length, uint32_t* d_nodes, uint8_t* d_pv, void* stream) {
    if (!gmk::device_state().ready) { gmk::set_error("gmk_init has not succeeded (no CPU fallback)"); return GMK_ERR_STATE; }
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
    if (!gmk::device_state().ready) { gmk::set_error("gmk_init has not succeeded (no CPU fallback)"); return GMK_ERR_STATE; }
    if (n < 0 || stride < 1 || max_depth < 1 || max_depth > GMK_VCF_MAX_DEPTH || (flags & ~kKnownFlags) != 0 || (n > 0 && (!h_moves || !h_lens))) {
        gmk::set_error("gmk_vcf_solve_host: bad arguments (n >= 0, stride >= 1, max_depth in [1, %d], flags in [0, 3])", GMK_VCF_MAX_DEPTH);
        return GMK_ERR_ARG;
    }
    if (n == 0) return GMK_OK;
    // one device block: moves | lens | status | move | length | nodes | pv, each part 16-byte aligned
    const auto up16 = [](size_t b) { return (b + 15) & ~size_t(15); };
    const size_t un = static_cast<size_t>(n);
    const size_t o_lens = up16(un * static_cast<size_t>(stride)), o_status = o_lens + up16(un * 4), o_move = o_status + up16(un * 4),
                 o_length = o_move + up16(un * 4), o_nodes = o_length + up16(un * 4), o_pv = o_nodes + up16(un * 4), total = o_pv + up16(un * GMK_VCF_PV);
    char* d = nullptr;
    GMK_HIP_CHECK(gmk::device_malloc(&d, total));
    int rc = GMK_OK;
    if (hipMemcpy(d, h_moves, un * static_cast<size_t>(stride), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + o_lens, h_lens, un * 4, hipMemcpyHostToDevice) != hipSuccess) rc = GMK_ERR_HIP;
    if (rc == GMK_OK)
        rc = gmk_vcf_solve(reinterpret_cast<const uint8_t*>(d), stride, reinterpret_cast<const int32_t*>(d + o_lens), n, max_depth, budget, flags,
                           h_status ? reinterpret_cast<int32_t*>(d + o_status) : nullptr, h_move ? reinterpret_cast<int32_t*>(d + o_move) : nullptr,
                           h_length ? reinterpret_cast<int32_t*>(d + o_length) : nullptr, h_nodes ? reinterpret_cast<uint32_t*>(d + o_nodes) : nullptr,
                           h_pv ? reinterpret_cast<uint8_t*>(d + o_pv) : nullptr, nullptr);
    if (rc == GMK_OK && hipDeviceSynchronize() != hipSuccess) rc = GMK_ERR_HIP;
    if (rc == GMK_OK && ((h_status && hipMemcpy(h_status, d + o_status, un * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
                         (h_move && hipMemcpy(h_move, d + o_move, un * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
                         (h_length && hipMemcpy(h_length, d + o_length, un * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
                         (h_nodes && hipMemcpy(h_nodes, d + o_nodes, un * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
                         (h_pv && hipMemcpy(h_pv, d + o_pv, un * GMK_VCF_PV, hipMemcpyDeviceToHost) != hipSuccess))) rc = GMK_ERR_HIP;
    if (rc == GMK_ERR_HIP) gmk::set_error("gmk_vcf_solve_host: a HIP call failed: %s", hipGetErrorString(hipGetLastError()));
    (void)gmk::device_free(d);
    return rc;
}
