// vcf_device.h -- K14's forced-win walk by continuous fours, once, for every kernel that runs it: vcf_kernel.hip (K14), vcf_defend_kernel.hip
// (K15), vcf_threats_kernel.hip (K17) and the three az_*_leaves kernels of az_kernel.hip (K7 + K14, K7 + K15).
// The board of one position is one ROW per lane, sixteen lanes per position (lane 15 of a group is an off-board row of zeros), four positions per
// wavefront.  Horizontal neighbours are bit shifts; vertical and diagonal neighbours are the rows y-4 .. y+4 of a plane, fetched with DPP row
// shifts, which stay inside a 16-lane row and deliver zero from outside it -- exactly a board edge.  On top of that geometry stand the walk's
// state (Walk, registers only), its LDS stack word, the pass that every group makes in the same instructions (pass), the decisions behind it
// (start, step, limit_failed), the hand-out of a wavefront's slice to its idle groups (hand_out) and the move-list loader (load_moves).  A kernel
// brings its loader, its own verdicts at a root and its endings, which step takes as callables that inline.  Device code only; the LDS stack is
// declared by the kernel and passed by reference.
#pragma once
#include "capi_common.h"

namespace gmk::vcf {

constexpr int kCells = 225;
constexpr uint32_t kRowMask = 0x7FFFu;
constexpr int kLevels = GMK_VCF_MAX_DEPTH;                  // pushes stop at depth 29 (a push needs depth + 3 <= limit <= 32)

enum : int { kIdle = 0, kInit = 1, kRun = 2 };

// rows[4 + k] = the plane's row y + k for k = -4 .. 4, zero where that row is off the board (DPP row shifts never leave the 16-lane group).
template <int K>
__device__ __forceinline__ uint32_t row_from_below(uint32_t v) {      // lane i <- lane i + K
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x100 + K, 0xF, 0xF, true));
}
template <int K>
__device__ __forceinline__ uint32_t row_from_above(uint32_t v) {      // lane i <- lane i - K
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x110 + K, 0xF, 0xF, true));
}
__device__ __forceinline__ void gather_rows(uint32_t v, uint32_t (&rows)[9]) {
    rows[4] = v;
    rows[5] = row_from_below<1>(v); rows[6] = row_from_below<2>(v); rows[7] = row_from_below<3>(v); rows[8] = row_from_below<4>(v);
    rows[3] = row_from_above<1>(v); rows[2] = row_from_above<2>(v); rows[1] = row_from_above<3>(v); rows[0] = row_from_above<4>(v);
}

__device__ __forceinline__ uint32_t shifted(uint32_t v, int k) { return k >= 0 ? v >> k : v << -k; }

// The plane's value k steps along direction D from every cell of this row: 0 horizontal, 1 vertical, 2 and 3 the diagonals.
template <int D>
__device__ __forceinline__ uint32_t along(const uint32_t (&rows)[9], int k) {
    if (D == 0) return shifted(rows[4], k);
    if (D == 1) return rows[4 + k];
    if (D == 2) return shifted(rows[4 + k], k);
    return shifted(rows[4 - k], k);
}

// Cells at which one more stone of the plane makes a run of five or more: the stones adjacent on both sides add up to four.
template <int D>
__device__ __forceinline__ uint32_t completing_dir(const uint32_t (&s)[9]) {
    const uint32_t l1 = along<D>(s, -1), l2 = l1 & along<D>(s, -2), l3 = l2 & along<D>(s, -3), l4 = l3 & along<D>(s, -4);
    const uint32_t r1 = along<D>(s, 1), r2 = r1 & along<D>(s, 2), r3 = r2 & along<D>(s, 3), r4 = r3 & along<D>(s, 4);
    return l4 | (l3 & r1) | (l2 & r2) | (l1 & r3) | r4;
}
__device__ __forceinline__ uint32_t completing(const uint32_t (&s)[9], uint32_t empty) {
    return empty & (completing_dir<0>(s) | completing_dir<1>(s) | completing_dir<2>(s) | completing_dir<3>(s));
}

// Runs of five or more that already stand.
template <int D>
__device__ __forceinline__ uint32_t five_dir(const uint32_t (&s)[9]) {
    return s[4] & along<D>(s, 1) & along<D>(s, 2) & along<D>(s, 3) & along<D>(s, 4);
}
__device__ __forceinline__ uint32_t five(const uint32_t (&s)[9]) { return five_dir<0>(s) | five_dir<1>(s) | five_dir<2>(s) | five_dir<3>(s); }

// Four-making cells: a five-window through the cell whose other four cells are free (attacker or empty, on the board) and hold at least three
// attacker stones.  a = attacker rows, f = free rows.
__device__ __forceinline__ uint32_t three_of(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (a & b & (c | d)) | (c & d & (a | b)); }
template <int D>
__device__ __forceinline__ uint32_t four_making_dir(const uint32_t (&a)[9], const uint32_t (&f)[9]) {
    uint32_t A[9], F[9];
#pragma unroll
    for (int k = -4; k <= 4; ++k) {
        if (k == 0) continue;
        A[4 + k] = along<D>(a, k);
        F[4 + k] = along<D>(f, k);
    }
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {                                    // the cell is the window's j-th
        const int o0 = -j + (0 >= j ? 1 : 0), o1 = -j + 1 + (1 >= j ? 1 : 0), o2 = -j + 2 + (2 >= j ? 1 : 0), o3 = -j + 3 + (3 >= j ? 1 : 0);
        any |= F[4 + o0] & F[4 + o1] & F[4 + o2] & F[4 + o3] & three_of(A[4 + o0], A[4 + o1], A[4 + o2], A[4 + o3]);
    }
    return any;
}
__device__ __forceinline__ uint32_t four_making(const uint32_t (&a)[9], const uint32_t (&f)[9], uint32_t empty) {
    return empty & (four_making_dir<0>(a, f) | four_making_dir<1>(a, f) | four_making_dir<2>(a, f) | four_making_dir<3>(a, f));
}

// One bit per row of this lane's group.
__device__ __forceinline__ uint32_t group_rows(bool p, int gbase) { return static_cast<uint32_t>(__ballot(p) >> gbase) & 0xFFFFu; }

// What lane `src` (0 .. 63) of the wavefront holds in `v`.  The permute itself, not __shfl, which masks the index and adds the wavefront's base
// again: two more instructions at each of a pass's five uses, unless the compiler sees through all of it.
__device__ __forceinline__ uint32_t from_lane(uint32_t v, int src) {
    return static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src << 2, static_cast<int>(v)));
}

// The lowest cell of a plane, or -1; the cell is taken out of `v`.
__device__ __forceinline__ int take_lowest(uint32_t& v, int y, int gbase) {
    const uint32_t rows = group_rows(v != 0, gbase);
    const int row = rows ? __builtin_ctz(rows) : 0;
    const uint32_t bits = from_lane(v, gbase + row);
    const int x = bits ? __builtin_ctz(bits) : 0;
    if (y == row) v &= ~(1u << x);
    return rows ? row * 15 + x : -1;
}

// ---- the walk ----
// What a lane knows of its place: its board row y, its 16-lane group and that group's first lane.
struct Lane {
    int lane, y, group, gbase;
    uint32_t board_row;
    __device__ __forceinline__ Lane() : lane(threadIdx.x), y(lane & 15), group(lane >> 4), gbase(lane & 48), board_row(y < 15 ? kRowMask : 0u) {}
};

// A group's walk, the same in its sixteen lanes but for att, def and mask, which are this lane's row of the two planes and of the current level's
// candidates.  `more` says that the level has candidates left, `cut` that the limit ended a line somewhere below the root.
struct Walk {
    int state = kIdle, depth = 0, limit = 0;
    bool cut = false, more = false;
    uint32_t nodes = 0, att = 0, def = 0, mask = 0;
    // a new root: these planes, nothing played and nothing counted
    __device__ __forceinline__ void reset(uint32_t attacker, uint32_t defender, int new_limit) {
        att = attacker; def = defender;
        nodes = 0; depth = 0; cut = false; more = false; mask = 0;
        limit = new_limit;
        state = kInit;
    }
};

// The stack's word of a level, per lane: candidates left 0..14, "the level has more" 15, the attacker's move c 16..23, the forced reply r 24..31.
using Stack = uint32_t[kLevels][64];
__device__ __forceinline__ uint32_t pack_level(uint32_t mask, bool more, int c, int r) {
    return mask | (more ? 0x8000u : 0u) | (static_cast<uint32_t>(c) << 16) | (static_cast<uint32_t>(r) << 24);
}
__device__ __forceinline__ uint32_t level_mask(uint32_t w) { return w & kRowMask; }
__device__ __forceinline__ bool level_more(uint32_t w) { return (w & 0x8000u) != 0; }
__device__ __forceinline__ int level_c(uint32_t w) { return static_cast<int>((w >> 16) & 255u); }
__device__ __forceinline__ int level_r(uint32_t w) { return static_cast<int>(w >> 24); }

// Cell k of a winning line: the levels' (c, r) on the stack, then t0 .. t2, the cells that end the line (255: none).
__device__ __forceinline__ uint32_t line_cell(const Stack& stack, const Lane& ln, int depth, int k, int t0, int t1, int t2) {
    const int tail = k - 2 * depth;
    if (tail < 0) { const uint32_t w = stack[k >> 1][ln.lane]; return static_cast<uint32_t>((k & 1) ? level_r(w) : level_c(w)); }
    return tail < 3 ? static_cast<uint32_t>(tail == 0 ? t0 : tail == 1 ? t1 : t2) : 255u;
}

// What a pass leaves for the decisions, the same in all sixteen lanes of a group but for the row masks cbit, rbit, T, C and empty.
struct Pass {
    int c, cy;                                   // the candidate played (a running group only), its row
    uint32_t cbit;
    int f1, f2;                                  // the attacker's two lowest completing cells, -1 for none
    int ry;                                      // the forced reply f1, where it went on the board (f1 alone completes)
    uint32_t rbit;
    int t1, t2;                                  // the defender's two lowest completing cells
    uint32_t T, C, empty;                        // completing(defender) whole, the child's candidates, the empty cells
    bool child_has, over;                        // C is not empty; a five stands (looked for only while some group is at a root)
};

// One pass, every group in the same instructions: a running group takes the lowest candidate c of its level and plays it, F = completing(attacker)
// (8 row shifts); if F is one cell the reply goes on the board, T = completing(defender), C = the four-making cells of the child (16 row shifts).
__device__ __forceinline__ Pass pass(Walk& w, const Lane& ln) {
    Pass ps;
    const int y = ln.y, gbase = ln.gbase;
    const bool trying = w.state == kRun;                           // such a group has a candidate: `mask` is not empty
    uint32_t popped = trying ? w.mask : 0u;
    ps.c = take_lowest(popped, y, gbase);
    const uint32_t left = group_rows(popped != 0, gbase);
    ps.cy = trying ? ps.c / 15 : 0;
    ps.cbit = trying ? 1u << (ps.c - 15 * ps.cy) : 0u;
    if (trying) {
        w.mask = popped;
        w.more = left != 0;
        if (y == ps.cy) w.att |= ps.cbit;
    }
    uint32_t A[9], D[9], N[9];
    gather_rows(w.att, A);
    uint32_t F = completing(A, ln.board_row & ~(w.att | w.def));
    ps.f1 = take_lowest(F, y, gbase);
    ps.f2 = take_lowest(F, y, gbase);
    const bool replied = trying && ps.f1 >= 0 && ps.f2 < 0;        // the forced reply goes on the board
    ps.ry = replied ? ps.f1 / 15 : 0;
    ps.rbit = replied ? 1u << (ps.f1 - 15 * ps.ry) : 0u;
    if (replied && y == ps.ry) w.def |= ps.rbit;
    ps.empty = ln.board_row & ~(w.att | w.def);
    gather_rows(w.def, D);
    gather_rows(ps.empty | w.att, N);
    uint32_t T = completing(D, ps.empty);
    ps.T = T;
    ps.C = four_making(A, N, ps.empty);
    if (group_rows(T != 0, gbase)) ps.C &= T;                      // a defender four: only its blocking cell is a candidate
    ps.t1 = take_lowest(T, y, gbase);
    ps.t2 = take_lowest(T, y, gbase);
    ps.child_has = group_rows(ps.C != 0, gbase) != 0;
    ps.over = false;
    if (__ballot(w.state == kInit) != 0ull) ps.over = group_rows((five(A) | five(D)) != 0, gbase) != 0;
    return ps;
}

// K14's decisions at a root that has no five and no completing cell of the attacker's: fail, or run with the root's candidates.
template <class Failed>
__device__ __forceinline__ void start(Walk& w, const Pass& ps, Failed&& failed) {
    bool fail = ps.t2 >= 0;
    if (!fail && 2 > w.limit) { w.cut = true; fail = true; }
    if (!fail && !ps.child_has) fail = true;
    if (fail) failed();
    else { w.mask = ps.C; w.more = true; w.state = kRun; }
}

// A running group's decisions after its pass: the candidate was no four (no node), the budget is spent, a double four wins, the line fails (the
// defender's reply makes two completing cells, the limit cuts it, the child has no candidate) or goes one level down; a candidate that did not
// go down is undone, and the group climbs while the levels above have nothing left.  The endings are the kernel's: win(c, f1, f2), budget() and
// failed(), the last with every move undone at the root.  An ending leaves state != kRun unless the group is to walk on.
template <class Win, class Budget, class Failed>
__device__ __forceinline__ void step(Walk& w, const Lane& ln, const Pass& ps, uint32_t budget, Stack& stack, Win&& win, Budget&& on_budget,
                                     Failed&& failed) {
    const int y = ln.y;
    bool retract = true;
    if (ps.f1 < 0) {
        // not a four: no candidate and no node (the plane-wide mask does not offer such a cell; this keeps the count exact regardless)
    } else if (w.nodes == budget) {
        on_budget();
    } else {
        ++w.nodes;
        if (ps.f2 >= 0) win(ps.c, ps.f1, ps.f2);
        else {
            bool fail = ps.t2 >= 0;
            if (!fail && w.depth + 3 > w.limit) { w.cut = true; fail = true; }
            if (!fail && !ps.child_has) fail = true;
            if (!fail) {
                stack[w.depth][ln.lane] = pack_level(w.mask, w.more, ps.c, ps.f1);
                ++w.depth;
                w.mask = ps.C; w.more = true; retract = false;
            } else if (y == ps.ry) w.def ^= ps.rbit;
        }
    }
    if (w.state == kRun && retract) {
        if (y == ps.cy) w.att ^= ps.cbit;
        while (!w.more) {                                          // climb while the level has nothing left
            if (w.depth == 0) { failed(); break; }
            --w.depth;
            const uint32_t word = stack[w.depth][ln.lane];
            w.mask = level_mask(word);
            w.more = level_more(word);
            const int uc = level_c(word), ur = level_r(word);
            if (y == uc / 15) w.att ^= 1u << (uc % 15);
            if (y == ur / 15) w.def ^= 1u << (ur % 15);
        }
    }
}

// The walk at this limit has failed at the root: nothing was cut (NONE), or the next limit of an iterative walk starts, or the last one was cut.
template <class Finish>
__device__ __forceinline__ void limit_failed(Walk& w, bool iterative, int max_depth, Finish&& finish) {
    if (!w.cut) finish(GMK_VCF_NONE);
    else if (iterative && w.limit < max_depth) { ++w.limit; w.cut = false; w.state = kInit; }
    else finish(GMK_VCF_DEPTH);
}

// K15's follow mode, the next level on the board the pass left: the threat's move there (pvw: this lane's four cells of the line, tlen its
// length), which must be free and, against a defender four, its block.  abit is this lane's row of that move.
struct Follow {
    uint32_t abit;
    bool follows;
};
__device__ __forceinline__ Follow follow_level(const Walk& w, const Lane& ln, const Pass& ps, uint32_t pvw, int tlen) {
    const int level = w.state == kRun ? w.depth + 1 : w.depth;
    const uint32_t pv_word = from_lane(pvw, ln.gbase + ((level >> 1) & 15));
    const int a = static_cast<int>((pv_word >> (16 * (level & 1))) & 255u), ay = a / 15;         // 255 past the line's end: row 17, no lane's
    Follow f;
    f.abit = ln.y == ay ? 1u << (a - 15 * ay) : 0u;
    const bool a_free = group_rows((ps.empty & f.abit) != 0, ln.gbase) != 0;
    f.follows = ps.t2 < 0 && level < tlen && a_free && (ps.t1 < 0 || a == ps.t1);
    return f;
}

// ---- around the walk ----
// The idle groups take the next jobs of their wavefront's slice, in group order: `rank` is this group's place among them, and an idle group
// with rank < left has a job; `taken` jobs leave the slice.
struct HandOut {
    int rank, taken;
};
__device__ __forceinline__ HandOut hand_out(int state, const Lane& ln, int left) {
    const unsigned long long idle = __ballot(state == kIdle);
    int rank = 0, takers = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int is_idle = static_cast<int>((idle >> (16 * g)) & 1ull);
        if (g < ln.group) rank += is_idle;
        takers += is_idle;
    }
    return {rank, takers < left ? takers : left};
}

// This lane's row of the two planes of move list `pos` (black moves first).  bad: the length is no length of a position or exceeds the stride
// -- then nothing is read -- and with kStrict, K14's, also a cell off the board or played twice; the other callers come behind K14's verdict.
struct Planes {
    uint32_t black, white;
    int len;
    bool bad;
};
template <bool kStrict>
__device__ __forceinline__ Planes load_moves(const uint8_t* moves, int stride, const int32_t* lens, int pos, const Lane& ln) {
    Planes pl{0u, 0u, lens[pos], false};
    pl.bad = pl.len < 0 || pl.len > kCells || pl.len > stride;
    bool clash = false;
    if (!pl.bad) {
        const uint8_t* list = moves + static_cast<size_t>(pos) * static_cast<size_t>(stride);
        for (int i = 0; i < pl.len; ++i) {
            const int cell = list[i];
            if (kStrict && cell >= kCells) { pl.bad = true; continue; }
            const int r = cell / 15;
            if (r != ln.y) continue;
            const uint32_t bit = 1u << (cell - 15 * r);
            if (kStrict) clash |= ((pl.black | pl.white) & bit) != 0;
            if (i & 1) pl.white |= bit; else pl.black |= bit;
        }
    }
    if (kStrict) pl.bad |= group_rows(clash, ln.gbase) != 0;
    return pl;
}

// ---- the host's side of K15 and K17: the slices of n * 225 jobs ----
// A wavefront walks a slice of the jobs, four at a time.  Small batches spread over the chip one quartet per wavefront -- one position is 57
// wavefronts; large ones give every wavefront 64 jobs, so that a group reads a position once for sixteen of its cells and has other jobs to
// take while a neighbour is deep in a search.  The grid stays below 2^30 workgroups for any n.
struct SlicePlan {
    int per_wave;
    unsigned grid;
};
inline SlicePlan cell_slices(int n, int cu_count) {
    const long long jobs = static_cast<long long>(n) * kCells, cus = cu_count > 1 ? cu_count : 1, large = (jobs >> 30) + 1;
    const int per_wave = jobs <= 4ll * 8 * cus ? 4 : static_cast<int>(large > 64 ? large : 64);
    return {per_wave, static_cast<unsigned>((jobs + per_wave - 1) / per_wave)};
}

}  // namespace gmk::vcf
