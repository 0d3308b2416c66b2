// eval_kernel.hip -- K1: batched from-scratch position evaluation on gfx950 (MI355X).
//
// For every board (two 15x15 bit-planes, 64 B) the kernel produces what the reference's incrementally
// maintained Evaluator holds after those stones were played (core/lib/src/Pattern.cpp:111-386):
// scores[4][225], density[2][2][225], pattern / compound totals and winner.  The formulation is the one
// validated against in-order replay in tests/test_formulation.py.
//
// What binds it (rocprofv3 PMC of the round-4 build, profiles/r04_k1_*): 842 vector, 356 scalar and 142 LDS wave-instructions per board; a wave64
// vector instruction occupies its SIMD for 4 cycles whatever it does (tools/valu_probe.hip), so the vector units are ~75 % and the LDS pipe ~60 % busy
// (41 % of its cycles bank conflicts) with sixteen boards of LDS per CU; HBM traffic = 1.05 x the algorithmic bytes.  Neither the store path nor
// HBM bandwidth is the limit (tools/store_probe.hip): instructions and dependent LDS round trips are.  So: few wave-instructions per board, few
// dependent round trips, and the one dense piece on the matrix cores:
//   * one 64-lane wavefront per board, sixteen boards in flight per 1024-thread workgroup (one workgroup per CU); the automaton
//     (dense DFA 556x4 words + emission records, ~14 KB) is staged at LDS address 0 ONCE per workgroup, so a DFA step's address is
//     just (next-row offset | symbol * 4): one v_bfe + one v_bfi; after that single barrier the waves never wait for each other (phases of one
//     board are ordered by wavefront-scope fences only).  A workgroup owns a contiguous run of groups of SIXTEEN boards and hands its boards
//     (and the density bursts of its groups) out one at a time from counters in LDS;
//   * phase 0: the two bit-planes become 88 "line words" (rows, columns, both diagonals) that already hold the 2-bit
//     DFA symbols of their cells (one LDS XOR per stone and line); where a colour's density count is positive (the area
//     bonus) comes from the rows dilated by the three row patterns of the 7x7 mask, with DPP row shifts; the score block -- [cell][4 groups] in
//     LDS -- is written ONCE, with the bonus in it;
//   * phase 1: the 72 lines that can hold a pattern (>= 5 cells) are spread over the 64 lanes (the 8 shortest ride
//     behind the shortest primaries of their own direction: 17 symbols per lane, fully unrolled); a lane's lines are one stream of 2-bit symbols without leading pads,
//     walked from the state the root reaches on '?'; the first four symbols are one read of a 256-entry table, every further one is one LDS lookup: 14 round trips, and the first ten carry a piece of phase 0 in their shadow; emitting transitions are queued by ballot prefix, in the shadow of the next step's lookup (the queue's fill
//     level lives on the scalar unit, clamped there: no per-lane bounds check).  A queue entry is the table word with its low 17 bits replaced by
//     the PLACE of the consumed symbol -- bits 0..8 its cell (0..256), 9..10 the direction, 11..16 minus the stride, signed -- which the scan lane keeps
//     as a running value: the lane record's place word, + the stride per step, + a jump across the seam of a two-line lane ("Lane -> lines" below);
//   * phase 2: one lane per queued transition: cell, direction and the step back are three field extracts of the entry (nothing is looked up:
//     until round 14 the entry held (lane, step) and every deposit round decoded the lane's jobs from a table in LDS), one 16-byte record read gives the (<= 2) matches, each with a
//     compact list of <= 4 score deposits -- a colour's own and opponent view of a cell are the halves of one 64-bit word, so a deposit is ONE
//     ds_add_u64 whose value decides -- and 4-bit per-(cell, colour, direction, type) counters;
//   * phase 3: one lane per cell: compound candidates from the counters -- a colour's half word h of the OR-ed counters makes one iff
//     h & ((h - 1) | 0xEEEE): v_or3, v_pk_add_u16, v_bitop3, v_cmp per pass in front of the ballot (the static listing, profiles/r10_k1_frame_counts.txt); phase 3b: four lanes per (candidate, colour), sixteen pairs per round (round 15):
//     the compound decision in closed form (components n, threes s) in every lane of the quad, +-600 deposits by its lane 0, the two components queued
//     by its lanes 0 and 1 -- one entry per lane, slots by a ballot prefix over quads -- with their line word and slot in the entry.  The reference's density
//     gate "count >= 2" is not evaluated: a pair that gets here always passes it (phase 3b says why; tests/test_eval_density_gate.py);
//   * phase 4: seven lanes per compound component, nine per round: its counter-move cells from the 13-symbol window around it (one
//     v_alignbit of the line word with its '?' pads), walked as one read of the root's four-symbol prefix table and three or four lookups; whether the
//     match found has its '_' on the cell is one zero-nibble test of its four deposit fields (counter_match; tests/test_eval_nibble_match.py);
//   * phase 5: the 3.6 KB score block leaves LDS transposed to [group][cell]: sixteen non-temporal dword stores of 256 contiguous bytes, in
//     ADDRESS order (the two parts of a cache line that two pieces share reach the L2 back to back);
//   * phase D, once per group, by the wavefront that is handed board 12 k of its workgroup's run for the run's k-th group: the density planes of the
//     sixteen boards on the matrix cores -- Out[board, colour][cell] = Stone[board, colour][cell'] * W[cell'][cell], the stones as
//     the A operand and the constant banded weight matrix (rows of a 6 KB table in LDS) as the B operand of
//     v_mfma_i32_32x32x32_i8 (14 passes of 3-5 MFMAs, small integers: exact), stored as 2 x 128 contiguous bytes per instruction.  A group whose
//     sixteen boards all exist (every group but the last of a launch whose board count is not a multiple of sixteen) stores without guards, one
//     straight-line block per pass: per pair of stores three vector instructions (the occupied bit, two XORs) and two scalar ones (the board's
//     block added to a 64-bit scalar base: global_store_dword offset, value, s[base]); the occupied bits come from 7 x 16 words the burst puts
//     in LDS once (two 16-byte reads per pass).  Everything the prologue reads is one image the host builds once: 24 KB staged 16 bytes per lane, 32 bytes of constants per lane, all loads issued at once.
// HBM traffic per board: 64 B in, 7 248 B out (7 312 B algorithmic); everything else stays on chip.
// Round 11 (profiles/r11_k1_*) shortened each board's chain of dependent LDS round trips: the scan lost its two leading-pad steps
// (19 -> 17: -1.3 % of the launch on its own), and what phase 0 writes for phase 2 and later moved out of the way of the line words into the scan's
// first lookups (-0.5 % on top).  Asking for the next hand-out behind phase 5's block reads and fetching the next deposit round's record and jobs
// ahead were built, measured as no gain (+0.3 % and +-0.1 %) and are not in the source.
// Round 12 (profiles/r12_k1_*) took lookups whose reports nobody uses out of the same chain: the scan's first four symbols are cells, and no four cells
// from its start state report a match, so they are one 16-bit read of a 256-entry table of the row they lead to (14 round trips where there were 17, four
// ballots and pushes fewer: -1.6 % of the launch on its own); a rescan lane's first four symbols from the root are one read of DeviceTables::dev_prefix4,
// as in K2's window matcher (5 reads where there were 8: -1.2 % on its own); together -3.3 %.  Both tables are staged with the others (+1 KB of LDS).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "capi_common.h"
#include "host_staging.h"

namespace {

constexpr int kBoardsPerBlock = 16;               // wavefronts per workgroup, one board in flight each
constexpr int kGroupBoards = 16;                  // boards whose density planes are one unit of work (the columns of phase D's matrix product)
constexpr int kThreads = 64 * kBoardsPerBlock;
constexpr int kCells = 225;
constexpr int kQueueCap = 448;
constexpr int kMaxBlocksPerCu = 1;
constexpr int kBurstEvery = 12;                    // a workgroup's k-th density burst goes with board kBurstEvery * k of its run (<= kGroupBoards; measured: 16 -0.9 %, 14 -2.8 %,
                                                  // 12 -3.3 % of the step against the bursts taken in turns, profiles/r09_k1_ab.txt)
static_assert(kBurstEvery >= 1 && kBurstEvery <= kGroupBoards, "every burst of a run needs a board of the run to go with");
[[maybe_unused]] constexpr int kTimelineSlots = 8;  // clock values per wavefront of the profiling flavour's timeline (the kernel says which)

// per-board LDS region (32-bit words)
constexpr int kScoreWords = 4 * kCells;          // 900, 16-byte aligned block.  In LDS the block is [cell][4 groups]: a colour's own and opponent view of a
                                                 // cell are the halves of one 64-bit word (white: groups 0, 1; black: 2, 3), so a deposit into both is ONE ds_add_u64
constexpr int kCntWords = 3 * kCells + 1;        // [LiveThree, DeadThree, LiveTwo][cell]: eight 4-bit counters per word, field = colour * 4 + direction:
                                                 // how many '_' pieces of matches of that type lie on the cell (<= 15: at most 8 transitions x 2 matches reach a cell;
                                                 // the most any board of the test sets or of the saturation search reaches is 2)
constexpr int kZeroWords = kScoreWords + kCntWords;                   // cleared for every board (a multiple of 4)
constexpr int kLineWords = 96;                   // line words, 2 bits per cell = its DFA symbol (0 black, 1 white, 3 blank): rows [0,15) cell x at bits 2x,
                                                 // columns [20,35) cell y at bits 2y, diagonals x-y+14 at [36,65) at bits 2x, anti-diagonals x+y at [65,94) at bits 2y
                                                 // (a stone's shift is then 2x for its row and diagonal, 2y for its column and anti-diagonal: two shifted
                                                 // codes per stone instead of four; a reader shifts a diagonal's word down to its first cell)
constexpr int kColBase = 20, kDiagBase = 36, kAntiBase = 65;
#ifndef GMK_K1_TOTALS_COPIES
#define GMK_K1_TOTALS_COPIES 8
#endif
constexpr int kTotalsCopies = GMK_K1_TOTALS_COPIES;   // of the per-type totals, in the queue's last words (phase 0 says why); 8 x copies <= 64
constexpr int kMiscWords = 48;                   // [0] stones black | white << 16, [1] winner bits, [2] error, [3] unused, [4..14] totals,
                                                 // [19..33] the rows (black | white << 16) between three zero rows on either side ([16..18], [34..36])
constexpr int kBoardWords = kZeroWords + kLineWords + kQueueCap + kMiscWords;
static_assert(kZeroWords % 4 == 0 && kBoardWords % 4 == 0, "16-byte alignment of the per-board blocks");
constexpr int kPrefixTableWords = gmk::kPrefixWords;   // a table of the row reached over four symbols: 256 entries of 16 bits, key s0 | s1 << 2 | s2 << 4 | s3 << 6
constexpr int kStaticTableWords = kLineWords + 512 + 1560 + 2 * kPrefixTableWords + 4;   // the lines' '?' pads (phase 4), the bits-to-bytes table, the weight table of phase D,
                                                                        // the two prefix tables (from S for the scan, from the root for the rescans: DeviceTables::dev_prefix4),
                                                                        // and the workgroup's hand-out counter (four words: [0] the counter, [1] the row of S, the state the scan's prefix table is walked from: the host's note, no kernel reads it)

// Lane -> lines.  A lane walks one line, or two of the SAME direction (lanes 56..59: an 8-cell diagonal or anti-diagonal with a 5-cell one behind it,
// lanes 60..63: 7 cells with 6 behind), so direction and stride are lane constants, and what the scan needs of its lines is two words of the lane's record:
//   the lines word   bits 0..4 symbols in the first line's stream segment (len + 2: its cells and two trailing pads), 5..9 the second's (2: no line),
//                    10..16 and 17..23 the two line word indices, 24..31 (byte 3, which an SDWA operand selects) the cell stride;
//   the place word   bits 0..16 the place of the stream's symbol 4 as a queue entry carries it -- 0..8 the cell (up to 256: the main diagonal's second
//                    trailing pad), 9..10 the direction, 11..16 MINUS the stride as a signed 6-bit field --, 17..26 the jump, signed: what is added
//                    besides the stride where the stream steps from the first line's second pad to the second line's first cell, step 10 on lanes
//                    56..59 and step 9 on lanes 60..63 (first cell of the second line - (first cell of the first + segment * stride)); 0 elsewhere.
// The place of step s is the place word + (s - 4) * stride (+ the jump): plain integer adds on the packed word, exact in its low 17 bits because the
// true cell is never negative and never above 511; what the adds leave above bit 16 is not looked at.  The host checks both words against the plain
// statement -- segment, place on the line, first cell + place * stride -- for every lane and step when it builds the image (lane_tables).
// Everything a launch reads besides the boards is ONE image in device memory that the host builds once (build_stage_image): first what every workgroup
// stages in LDS, in LDS order and ready to use -- the automaton, the emission records, the lines' '?' pads, the bits-to-bytes table, the
// weight table of phase D, the two four-symbol prefix tables (phases 1 and 4), the hand-out counter's start value and the row of the scan's start state -- copied 16 bytes per lane; behind it a 32-byte record per lane with what the prologue
// would otherwise derive from the lane number: its lines word and place word, its two all-blank line words ((1 << 2 len) - 1: words lane and 64 + lane), then [0] row * 4
// and [1] column of the lane's cell in each of the four passes over the board (cell = 64 pass + lane, the last one clamped to 224), a byte per pass, and
// [2], [3] where the first cell of the lane's two lines sits in its line word (bit 2 x0 for a diagonal, 2 y0 for an anti-diagonal, 0 for rows and columns).
// Every load of the prologue is issued before the first of them is waited for: their latencies overlap.  (They used to be a dozen loops and
// constant-memory reads, each waiting for its own load: a dozen memory latencies in a row at the head of every launch.)
constexpr int kLaneRecordVecs = 2;
constexpr int kSegPads = 2;                       // the '?' behind a line's cells in its stream segment (none in front: phase 1 says why)
constexpr int kScanSteps = 17;                    // symbols in the longest lane stream (lane_tables checks it)
constexpr int kScanPrefixSyms = 4;                // of them, the leading ones that one read of the scan's prefix table stands for (lane_tables checks that they are cells)
constexpr int kPairedLanes = 8, kFirstPairedLane = 64 - kPairedLanes;        // the lanes that walk two lines: the last eight, the longer first lines in front
constexpr int kSeamStepLong = 8 + kSegPads, kSeamStepShort = 7 + kSegPads;   // the step that is the second line's first cell: lanes 56..59 (8 cells first), lanes 60..63 (7 cells)

__device__ __forceinline__ int dir_stride(int dir) { return (0x0E100F01u >> (8 * dir)) & 0xFFu; }      // 1, 15, 16, 14: a shift, not three branches

// cells '?' '?' of one line as a symbol stream, first symbol in the low bits: exactly 2 * (len + 2) bits
// (no leading and 2 trailing pads instead of the reference's 6 + 6; '?' = 2 is the off-board symbol)
__device__ __forceinline__ uint64_t line_symbols(uint32_t line_word, int len) {
    return static_cast<uint64_t>(line_word) | (0xAull << (2 * len));
}

// Phases of one board only exchange data between lanes of the SAME wavefront through LDS.  LDS instructions of
// one wave execute in issue order, so all that is needed between phases is that the compiler keeps the order:
// a wavefront-scope fence (no instruction) instead of a workgroup barrier, which would make the independent
// boards of a block wait for each other at every phase.
// the 32-bit word at a byte address of LDS (no base added: the staged automaton starts at address 0)
__device__ __forceinline__ const __attribute__((address_space(3))) uint32_t* lds_word(uint32_t byte_address) {
    return reinterpret_cast<const __attribute__((address_space(3))) uint32_t*>(static_cast<uintptr_t>(byte_address));
}

// ... and the 16-bit one (an entry of a prefix table)
__device__ __forceinline__ const __attribute__((address_space(3))) uint16_t* lds_half(uint32_t byte_address) {
    return reinterpret_cast<const __attribute__((address_space(3))) uint16_t*>(static_cast<uintptr_t>(byte_address));
}

__device__ __forceinline__ __attribute__((address_space(3))) uint32_t* lds_word_rw(uint32_t byte_address) {
    return reinterpret_cast<__attribute__((address_space(3))) uint32_t*>(static_cast<uintptr_t>(byte_address));
}

// (table word & 0x3FF3) | (four & 12) for four < 16: the lookup address of a DFA step as ONE v_bfi_b32 (written out: the compiler turns the
// expression back into a shift, a mask and an and-or)
__device__ __forceinline__ uint32_t dfa_address(uint32_t table_word, uint32_t four) {
    uint32_t addr;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(addr) : "s"(0x3FF3u), "v"(table_word), "v"(four));
    return addr;
}

// The scan's running place (the lane record's place word, see "Lane -> lines") one step on: + the stride, byte 3 of the lines word, selected by the
// instruction itself.  Output and input are separate operands: tied, the compiler copies the place on every step.
__device__ __forceinline__ uint32_t place_advance(uint32_t place, uint32_t lines_word) {
    uint32_t next;
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(next) : "v"(place), "v"(lines_word));
    return next;
}

// ... and across the seam of a two-line lane: + the jump, on the four lanes kFirstLane .. kFirstLane + 3 only: they are one bank (four lanes) of one DPP
// row (sixteen), and the row and bank masks leave every other lane's place as it is: no compare, no exec mask.
// A DPP operand must not be read within two wait states of the vector instruction that wrote it, and the compiler pads nothing for an instruction it
// cannot see: the s_nop 1 in front belongs to the add (the jump's field extract is a lane constant the compiler may hoist or work out right here).
template <int kFirstLane>
__device__ __forceinline__ uint32_t place_jump(uint32_t place, int jump) {
    static_assert(kFirstLane >= 0 && kFirstLane < 64 && kFirstLane % 4 == 0, "four lanes of one DPP bank");
    constexpr int kRow = kFirstLane / 16, kBank = (kFirstLane % 16) / 4;
    asm("s_nop 1\n\tv_add_u32_dpp %0, %1, %0 quad_perm:[0,1,2,3] row_mask:%2 bank_mask:%3" : "+v"(place) : "v"(jump), "n"(1 << kRow), "n"(1 << kBank));
    return place;
}

// a queue entry: the table word with its low 17 bits replaced by the place's, one v_bfi_b32
__device__ __forceinline__ uint32_t queue_entry(uint32_t table_word, uint32_t place) {
    uint32_t entry;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(entry) : "s"(0x1FFFFu), "v"(place), "v"(table_word));
    return entry;
}

// both 16-bit halves of a word decremented, no borrow from the low half into the high one: one v_pk_sub_u16
typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_dec_u16(uint32_t word) {
    const v2u16 ones = {1, 1};
    return __builtin_bit_cast(uint32_t, static_cast<v2u16>(__builtin_bit_cast(v2u16, word) - ones));
}

// global_store_dword with the address as a wave-uniform 64-bit base in scalar registers plus the lane's unsigned 32-bit byte offset, written out: from
// C++ the compiler adds the two as a 64-bit vector value first (two vector instructions per store where the base changes from store to store).
// A plain store, not a non-temporal one.
__device__ __forceinline__ void store_saddr(uint32_t byte_offset, int32_t value, unsigned long long base) {
    asm volatile("global_store_dword %0, %1, %2" : : "v"(byte_offset), "v"(value), "s"(base) : "memory");
}

// The same with an immediate byte offset (13 bits, signed, on gfx950: -4096 .. 4095) and, for kNt, the non-temporal bit: a board's whole 3 600-byte
// score block lies within reach of ONE scalar base and ONE lane offset, so its sixteen stores need no address arithmetic between them.
template <int kImm, bool kNt>
__device__ __forceinline__ void store_saddr_imm(uint32_t byte_offset, int32_t value, unsigned long long base) {
    static_assert(kImm >= 0 && kImm < 4096, "the immediate offset of a global store has 13 bits, signed");
    if (kNt) asm volatile("global_store_dword %0, %1, %2 offset:%3 nt" : : "v"(byte_offset), "v"(value), "s"(base), "n"(kImm) : "memory");
    else asm volatile("global_store_dword %0, %1, %2 offset:%3" : : "v"(byte_offset), "v"(value), "s"(base), "n"(kImm) : "memory");
}

__device__ __forceinline__ void wave_phase_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Score deposits of one match (Evaluator::Updater::updatePatterns, Pattern.cpp:138-165).  w0 / w1: emission
// record words (pattern_tables.h).  cell_at = cell of the symbol the transition consumed.
// back_step = -stride: the cells of a match lie behind the symbol that ended it, one multiply-add each.
__device__ __forceinline__ void deposit_match(uint32_t w0, uint32_t w1, int cell_at, int dir, int back_step,
                                              uint32_t* s_scores, uint32_t* s_cnt, uint32_t* s_misc, uint32_t* totals /* this lane's copy of the eight per-type totals */) {
    const int type = w0 & 15, fav = (w0 >> 4) & 1;
    if (type == 8) { atomicOr(&s_misc[1], fav ? 1u : 2u); return; }                 // Five: winner only (Pattern.cpp:140-145)
    atomicAdd(&totals[type], fav ? 0x10000u : 1u);                                  // totals row (Pattern.cpp:147, 390-393)
    const int endcell = cell_at + static_cast<int>((w0 >> 27) & 1u) * back_step;
    const uint32_t score = dir >= 2 ? (w1 >> 16) : (w1 & 0xFFFFu);                  // int(1.2 * score) on diagonals (Pattern.cpp:151-152)
    // Group(favour, favour) is the owner's view, Group(favour, -favour) the opponent's (Pattern.h:159-161): '_' adds the score to both,
    // '^' to the opponent's only.  The two views of a cell are one 64-bit word of the block (white: own low / opp high, black: opp low /
    // own high): one add either way, the value decides.
    unsigned long long* pair = reinterpret_cast<unsigned long long*>(s_scores) + fav;
    const uint32_t lo_opp = fav ? score : 0u, hi_opp = fav ? 0u : score;
    const uint32_t tslot = 5u - static_cast<uint32_t>(type);                         // LiveThree 0, DeadThree 1, LiveTwo 2 feed compounds (no branches: one compare)
    const bool feeds = tslot < 3u;
    uint32_t* cnt = s_cnt + (feeds ? tslot : 0u) * kCells;
    const uint32_t one = 1u << (4 * (fav * 4 + dir));
    const int n_dep = (w0 >> 8) & 7;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (d >= n_dep) break;
        const uint32_t f = (w0 >> (11 + 4 * d)) & 15u;
        const int c = endcell + static_cast<int>(f & 7u) * back_step;
        const bool both = (f & 8u) != 0u;                                           // '_'
        atomicAdd(&pair[2 * c], (static_cast<unsigned long long>(both ? score : hi_opp) << 32) | (both ? score : lo_opp));
        if (both && feeds) atomicAdd(&cnt[c], one);
    }
}

// Compound::updateAntis (Pattern.cpp:520-543) for one match met at window index k: it qualifies if it is of the wanted
// type, covers the centre cell q and has '_' there; returns the piece index (from the match's end) lying on q, or -1
__device__ __forceinline__ int counter_match(uint32_t w0, int k, int want) {
    const int type = w0 & 15, len = (w0 >> 5) & 7;
    const int back = k - static_cast<int>((w0 >> 27) & 1u) - 6;
    if (!w0 || type != want || back < 0 || back >= len) return -1;
    const int n_dep = (w0 >> 8) & 7;
    // Is one of the first n_dep deposit fields (four bits each, from bit 11) the '_' at `back`, 8 | back?  XOR-ed with that value in every nibble the
    // sought field is a ZERO nibble, and (x - 0x1111) & ~x & 0x8888 flags the lowest zero nibble of x exactly; above it the borrow may flag nibbles
    // that hold 1, which does not matter for "any": a wrong flag has a true one below it, inside the mask whenever it is itself
    // (tests/test_eval_nibble_match.py: every record word of the tables and every 16-bit field, against the four compares this replaces)
    const uint32_t x = ((w0 >> 11) & 0xFFFFu) ^ (static_cast<uint32_t>(back) * 0x1111u + 0x8888u);
    const bool on_q = ((x - 0x1111u) & ~x & 0x8888u & ((1u << (4 * n_dep)) - 1u)) != 0u;   // '_' on q (n_dep <= 7: the shift stays below 32)
    return on_q ? back : -1;
}

// ... and its other scored blanks get +600 in the opponent's view (opp = the opponent group's word of cell 0 in the [cell][4] block)
__device__ __forceinline__ void add_counter_cells(uint32_t w0, int back, int q, int stride, uint32_t* opp) {
    const int n_dep = (w0 >> 8) & 7, endcell = q + back * stride;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t f = (w0 >> (11 + 4 * d)) & 15u;
        if (d < n_dep && static_cast<int>(f & 7u) != back) atomicAdd(&opp[4 * (endcell - static_cast<int>(f & 7u) * stride)], 600u);
    }
}

// ---- phase D: the density stencil of sixteen boards on the matrix cores ----
// Evaluator::Updater::updateBlock (Pattern.cpp:236-272) adds, for every stone, the 7x7 BlockWeights (Pattern.cpp:598-609) around
// it to its colour's weight plane and their non-zero mask to its count plane: as a function of the position,
//   weight[c][q] = sum over cells q' of W[q' - q] * stone_c[q'],  count[c][q] likewise with W != 0,
// a product of a constant banded 225 x 225 matrix with the stone planes.  Sixteen boards x two colours are the 32 columns
// of v_mfma_i32_32x32x32_i8; an M tile is 32 consecutive cells (7 tiles cover cells 0..223, cell 224 is done by hand), a K tile
// two board rows of 16 (k = 16 y + x: the stones of a row become the bytes of its tile as they lie).  A tile of cells only
// reaches rows y0-3 .. y1+3, so 31 (M, K) tile pairs per plane kind hold non-zeros.
[[maybe_unused]] constexpr int kDensTiles = 7;       // M tiles of 32 cells (cells 0 .. 223; cell 224 is done by hand)
__host__ __device__ constexpr int dens_kt_lo(int m) { return (((32 * m) / 15 - 3) < 0 ? 0 : (32 * m) / 15 - 3) / 2; }
__host__ __device__ constexpr int dens_kt_hi(int m) { return (((32 * m + 31) / 15 + 3) > 14 ? 14 : (32 * m + 31) / 15 + 3) / 2; }
// The weight operand of lane (cell c = (yo, xo), k half h) at K tile kt holds the taps from row y = 2 kt + h, columns 0..15, to c:
// byte j = w(y - yo, j - xo).  It depends on (dy, xo) only, so ALL weight operands are rows of one small table in LDS,
// [plane kind][dy + 6][xo] x 16 bytes (6 240 B), read with one ds_read_b128 per MFMA; going up one K tile is +2 in dy = +480 bytes,
// an immediate offset.  (A table in global memory, 62 KB read by every wavefront for every group, cost 380 MB of L2 traffic per
// launch and a global-load latency per MFMA.)
constexpr int kWtabDy = 13, kWtabEntryWords = 4, kWtabKindWords = kWtabDy * 15 * kWtabEntryWords, kWtabWords = 2 * kWtabKindWords;
// BlockWeights by |dy| and dx + 3 (the matrix is symmetric in both axes)
__host__ __device__ constexpr int block_weight(int dy, int dx) {
    constexpr int w[4][7] = {{1, 3, 4, 0, 4, 3, 1}, {0, 3, 5, 4, 5, 3, 0}, {0, 4, 3, 3, 3, 4, 0}, {2, 0, 0, 1, 0, 0, 2}};
    return w[dy < 0 ? -dy : dy][dx + 3];
}

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// ---- phase D: one plane kind of one M tile of a group of sixteen boards leaves for HBM ----
// Here the BOARDS are on the accumulator rows (A = stones, B = weights): lane (n, h) holds cell 32 M + n of sixteen board-colour
// columns, so a store instruction writes 2 x 128 contiguous bytes (with the cells on the rows a lane would own 16 bytes of 64
// different cache lines: measured 2.4 TB/s for the density planes alone).  Spreading the fourteen passes over the group's board
// iterations spreads the 3.6 KB per board over the kernel's run time instead of one burst at its start.
// The stones are read again (64 B per board from L2) and become operand bytes through a 256-entry table in LDS (byte -> 8 bytes).
// Which cells are occupied (they hold ~v) comes from s_occ, the burst's [M tile][16 boards] words in LDS (density_planes_out): the eight
// boards of this lane's half are eight consecutive words, two 16-byte reads per pass in front of its MFMAs.
// kFull: all sixteen boards of the group exist (decided once per burst, on the scalar unit).  The eight store pairs are then one straight-line
// block, and what differs between them -- the board's block, b * 3 600 bytes -- is added to the group's base on the scalar unit: a store is
// global_store_dword <lane's 32-bit offset>, <value>, <64-bit scalar base>, no vector address arithmetic between the pairs of a pass.
// Only the last group of a launch whose board count is not a multiple of sixteen takes the guarded form (columns without a board are not stored).
template <bool kFull, int KIND, int M>
__device__ __forceinline__ void density_tile_pass(const uint32_t (&own_rows)[8], int n_live, int lane,
                                                  const v4i* __restrict__ s_wtab, const uint4* __restrict__ s_occ, int32_t* __restrict__ group_out,
                                                  unsigned long long& board_base /* kFull: group_out, in scalar registers */, const uint2* __restrict__ s_lut, int plane_stride) {
    constexpr int lo = dens_kt_lo(M), hi = dens_kt_hi(M), nk = hi - lo + 1;
    const int n = lane & 31, h = lane >> 5;
    const uint4 occ_lo = s_occ[4 * M + 2 * h], occ_hi = s_occ[4 * M + 2 * h + 1];
    const uint32_t occ[8] = {occ_lo.x, occ_lo.y, occ_lo.z, occ_lo.w, occ_hi.x, occ_hi.y, occ_hi.z, occ_hi.w};
    const int cell = 32 * M + n, yo = (cell * 0x8889) >> 19, xo = cell - 15 * yo;
    const v4i* w = s_wtab + KIND * (kWtabKindWords / kWtabEntryWords) + (2 * lo + h - yo + 6) * 15 + xo;
    v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < nk; ++k) {
        const uint32_t r = (own_rows[lo + k] >> (16 * h)) & 0x7FFFu;
        const uint2 b0 = s_lut[r & 255u], b1 = s_lut[r >> 8];
        const v4i stones = {static_cast<int>(b0.x), static_cast<int>(b0.y), static_cast<int>(b1.x), static_cast<int>(b1.y)};
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(stones, w[30 * k], acc, 0, 0, 0);
    }
    // accumulator i = board-colour column 8 (i / 4) + 4 h + (i % 4) at cell 32 M + n; columns 2 b, 2 b + 1 are board b
    const uint32_t at = static_cast<uint32_t>(KIND * plane_stride + 32 * M + n + h * (2 * 4 * plane_stride));      // this lane's word in the block of board b
    if (kFull) {
        // the lane's two byte offsets within a board's block (white, black) once per pass, the board's block on the scalar unit
        const uint32_t at_white = 4u * at, at_black = 4u * (at + 2u * static_cast<uint32_t>(plane_stride));
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
            const int neg = __builtin_amdgcn_sbfe(static_cast<int>(occ[i / 2]), n, 1);      // occupied cells hold -v - 1 = ~v (Pattern.cpp:253-265)
            store_saddr(at_black, acc[i] ^ neg, board_base);                                // column 2 b: black, the second colour block
            store_saddr(at_white, acc[i + 1] ^ neg, board_base);                            // column 2 b + 1: white, the first
            // boards 0, 1, 4, 5, 8, 9, 12, 13 (+ 2 h), then back to the group's first for the next pass: ONE scalar register pair, advanced in place
            // (left to itself the compiler keeps all eight boards' bases in sixteen scalar registers across the burst, and the board loop spills for it)
            board_base += static_cast<long long>(i == 14 ? -13 : i % 4 ? 3 : 1) * (4 * 4 * plane_stride);
            asm volatile("" : "+s"(board_base));
        }
    } else {
        int32_t* out = group_out + at;
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
            const int b = 4 * (i / 4) + (i % 4) / 2;    // + 2 h
            const int neg = __builtin_amdgcn_sbfe(static_cast<int>(occ[i / 2]), n, 1);
            asm volatile("" : "+s"(n_live));            // (the guard is worked out pair by pair: eight lane masks kept across the burst are sixteen scalar registers)
            if (b + 2 * h < n_live && plane_stride > 0) {
                out[b * 4 * plane_stride + 1 * 2 * plane_stride] = acc[i] ^ neg;
                out[b * 4 * plane_stride + 0 * 2 * plane_stride] = acc[i + 1] ^ neg;
            }
        }
    }
}

// All fourteen passes of a group, back to back: the group's density planes are one contiguous block of 16 x 3 600 bytes, and written
// within a few microseconds by one wavefront they reach DRAM as whole cache lines, row after row.  (One pass per board iteration --
// each line written in two pieces a board's work apart, each board's block in fourteen -- ran into the DRAM controller's write
// credits: TCC_EA0_WRREQ 9.7 M per launch instead of 3.9 M for the scores alone, a fifth of them 32-byte pieces.)
// The bursts of a workgroup are spread over its run (the caller takes burst k with board kBurstEvery * k of the run), so that most of the time
// one or two wavefronts per CU are storing planes while the others evaluate boards.
// s_occ: 7 x 16 words of this wavefront's LDS that nothing else uses at this point (the caller passes its transition queue).
template <bool kFull>
__device__ __forceinline__ void density_planes_out(const uint16_t* __restrict__ planes, int n_boards, int first_board, int lane,
                                                   const v4i* __restrict__ s_wtab, uint32_t* __restrict__ s_occ, int32_t* __restrict__ out_density,
                                                   const uint2* __restrict__ s_lut, int plane_stride) {
    const int n = lane & 31, plane = n & 1, board = first_board + (n >> 1);
    uint32_t own[8], other[8];
    {
        // (columns without a board read the group's first board: what they compute is never stored)
        const uint4* p = reinterpret_cast<const uint4*>(planes + static_cast<size_t>(kFull || board < n_boards ? board : first_board) * 32);
        const uint4 a0 = p[plane * 2], a1 = p[plane * 2 + 1], b0 = p[2 - plane * 2], b1 = p[3 - plane * 2];
        own[0] = a0.x; own[1] = a0.y; own[2] = a0.z; own[3] = a0.w; own[4] = a1.x; own[5] = a1.y; own[6] = a1.z; own[7] = a1.w;
        other[0] = b0.x; other[1] = b0.y; other[2] = b0.z; other[3] = b0.w; other[4] = b1.x; other[5] = b1.y; other[6] = b1.z; other[7] = b1.w;
    }
    // The occupied cells 32 M .. 32 M + 31 of every board, once per burst: one lane per board puts the word of each M tile where the
    // lanes of the half that stores the board read it.  Half h stores boards 4 j + 2 h and 4 j + 2 h + 1 in its pairs 2 j and 2 j + 1: board B
    // is word 8 (B / 2 & 1) + 2 (B / 4) + (B & 1) of a tile's sixteen.  (LDS instructions of a wavefront run in issue order: no wait between this
    // and the passes' reads.  Before: a ds_bpermute and a wait in front of each of the 112 store pairs.)
    if ((lane & 33) == 0) {
        const int bg = lane >> 1;
        uint32_t* slot = s_occ + 8 * ((bg >> 1) & 1) + 2 * (bg >> 2) + (bg & 1);
#pragma unroll
        for (int m = 0; m < kDensTiles; ++m) {
            const int y0 = (32 * m) / 15, y1 = (32 * m + 31) / 15;
            uint32_t occ = 0;
#pragma unroll
            for (int y = y0; y <= y1; ++y) {
                const uint32_t both = own[y / 2] | other[y / 2];
                const uint32_t r = ((y & 1) ? both >> 16 : both) & 0x7FFFu;
                const int at = 15 * y - 32 * m;
                occ |= at >= 0 ? r << at : r >> -at;
            }
            slot[16 * m] = occ;
        }
    }
    // cell 224 = (14, 14), which no tile covers: the taps dy, dx in -3 .. 0 that lie on the board, by hand (one lane per column)
    if ((lane >> 5) == 0 && (kFull || (board < n_boards && plane_stride > 0))) {
        uint32_t c224 = 0, w224 = 0;
#pragma unroll
        for (int dy = -3; dy <= 0; ++dy) {
            const int y = 14 + dy;
            const uint32_t r = (y & 1) ? own[y >> 1] >> 16 : own[y >> 1] & 0xFFFFu;
#pragma unroll
            for (int dx = -3; dx <= 0; ++dx) {
                if (block_weight(dy, dx) == 0) continue;
                const uint32_t bit = (r >> (14 + dx)) & 1u;
                c224 += bit;
                w224 += bit * static_cast<uint32_t>(block_weight(dy, dx));
            }
        }
        const uint32_t neg = 0u - (((own[7] | other[7]) >> 14) & 1u);             // occupied cells hold -v - 1 = ~v (Pattern.cpp:253-265)
        int32_t* out = out_density + static_cast<size_t>(board) * 4 * plane_stride + (1 - plane) * 2 * plane_stride;
        out[224] = static_cast<int32_t>(c224 ^ neg);
        out[plane_stride + 224] = static_cast<int32_t>(w224 ^ neg);
    }
    const int n_live = __builtin_amdgcn_readfirstlane(n_boards - first_board);      // >= 16 except in the last group
    int32_t* group_out = out_density + static_cast<size_t>(first_board) * 4 * plane_stride;        // wave-uniform
    const uint4* occ_words = reinterpret_cast<const uint4*>(s_occ);
    // (readfirstlane: the 64-bit product in the address may have been worked out on the vector unit)
    const unsigned long long group_bits = reinterpret_cast<unsigned long long>(group_out);
    unsigned long long board_base = static_cast<unsigned long long>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(group_bits >> 32)))) << 32
                                    | static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(group_bits)));
    asm volatile("" : "+s"(board_base));
#define GMK_PASS(K, M) density_tile_pass<kFull, K, M>(own, n_live, lane, s_wtab, occ_words, group_out, board_base, s_lut, plane_stride); __builtin_amdgcn_sched_barrier(0);
    GMK_PASS(0, 0) GMK_PASS(1, 0) GMK_PASS(0, 1) GMK_PASS(1, 1) GMK_PASS(0, 2) GMK_PASS(1, 2) GMK_PASS(0, 3) GMK_PASS(1, 3)
    GMK_PASS(0, 4) GMK_PASS(1, 4) GMK_PASS(0, 5) GMK_PASS(1, 5) GMK_PASS(0, 6) GMK_PASS(1, 6)
#undef GMK_PASS
}

__global__ __launch_bounds__(kThreads)
void eval_positions_kernel(const uint16_t* __restrict__ planes, int n_boards, int groups_each, int groups_extra,
                           int32_t* __restrict__ out_scores, int32_t* __restrict__ out_density,
                           uint32_t* __restrict__ out_totals, int32_t* __restrict__ out_status,
                           const uint4* __restrict__ g_stage, int stage_vecs, int trans_words, int record_words,
                           int phase_mask_arg, unsigned long long* __restrict__ prof, unsigned long long* __restrict__ timeline) {
    // Profiling aids, -DGMK_PROFILE build only (the production build runs every phase and reads no clock): phase_mask bit p runs
    // phase p, bit 6 phase D (bit 8: its planes 1 KB apart, bit 9: passes without stores, bit 10: no passes; bit 11: no compounds =
    // phases 3b and 4 skipped; bit 12: consecutive groups to different workgroups), any mask but 0x7F sets the error bit of every
    // board's status word; prof != nullptr: s_memtime cycles per phase, summed over the wavefronts; timeline != nullptr: eight clock values per
    // wavefront (kTimelineSlots, tools/k1_timeline.py), each written by lane 0 with an ordinary vector store.
#ifdef GMK_PROFILE
    // [0] entry, [1] end of the prologue, [2] arrival at the barrier, [3] leaving it, [4] end of the wavefront's last board, [5] exit,
    // [6] density bursts taken in or behind the last board's iteration | boards done << 16, [7] the clocks those bursts took
    unsigned long long* const tl_row = timeline ? timeline + (static_cast<size_t>(blockIdx.x) * kBoardsPerBlock + (threadIdx.x >> 6)) * kTimelineSlots : nullptr;
#define GMK_TL(slot, value) do { if (tl_row && (threadIdx.x & 63) == 0) tl_row[slot] = (value); } while (0)
    GMK_TL(0, __builtin_amdgcn_s_memtime());
    unsigned long long tl_last_board = 0, tl_burst_clocks = 0;
    int tl_bursts = 0;
    const int phase_mask = phase_mask_arg;
    unsigned long long t_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, t_prev = __builtin_amdgcn_s_memtime();
#define GMK_STAMP(k) do { if (prof) { const unsigned long long t_now_ = __builtin_amdgcn_s_memtime(); t_acc[k] += t_now_ - t_prev; t_prev = t_now_; } } while (0)
#else
    constexpr int phase_mask = 0x7F;
    (void)phase_mask_arg; (void)prof; (void)timeline;
#define GMK_TL(slot, value) do { } while (0)
#ifdef GMK_K1_MARKERS
#define GMK_STAMP(k) asm volatile("; gmk_mark " #k)      // (tools/k1_frame_counts.py counts the assembly between two marks)
#else
#define GMK_STAMP(k) do { } while (0)
#endif
#endif
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    // layout: [trans (LDS address 0)][records (16-byte aligned)][line pads 96][the other tables of kStaticTableWords][boards: kBoardsPerBlock * kBoardWords]
    const uint4* s_rec = reinterpret_cast<const uint4*>(lds + trans_words);
    uint32_t* s_static = lds + trans_words + record_words;

    // the loads of the prologue, all of them in front of their first use: the staged image (two pieces of 16 bytes per lane cover 32 KB; the
    // automaton's image is 24 KB) and this lane's record
    const int tid = threadIdx.x;
    const uint4 stage_a = g_stage[min(tid, stage_vecs - 1)], stage_b = g_stage[min(tid + kThreads, stage_vecs - 1)];
    const uint4* lane_record = g_stage + stage_vecs + kLaneRecordVecs * (tid & 63);
    const uint4 lane_lines = lane_record[0], lane_consts = lane_record[1];
    uint32_t* s_pads = s_static;                                             // a line word's '?' pads: symbol 2 in every 2-bit slot of the word that is not one of the
                                                                             // line's cells (phase 4 ORs them in: its window then reads '?' off the line wherever the line starts in its word)
    uint2* s_lut = reinterpret_cast<uint2*>(s_static + kLineWords);      // byte -> its eight bits as bytes (the stone operands of phase D)
    uint32_t* s_wtab_words = s_static + kLineWords + 512;
    const v4i* s_wtab = reinterpret_cast<const v4i*>(s_wtab_words);
    // the prefix tables' byte addresses (the kernel's LDS starts at address 0): the scan's, walked from S, and behind it the rescans', walked from the root
    const uint32_t scan_prefix_at = static_cast<uint32_t>(trans_words + record_words + kLineWords + 512 + kWtabWords) * 4u;
    const uint32_t root_prefix_at = scan_prefix_at + 4u * kPrefixTableWords;
    uint32_t* s_handout = s_wtab_words + kWtabWords + 2 * kPrefixTableWords;        // [0] boards handed out: starts at 2 x kBoardsPerBlock (every wavefront's first two boards are its own: see below)

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane0 = threadIdx.x & 63;
    uint32_t* s_scores = lds + trans_words + record_words + kStaticTableWords + wave * kBoardWords;      // int32 scores, accumulated with ds_add
    uint32_t* s_cnt = s_scores + kScoreWords;
    uint32_t* s_lines = s_scores + kZeroWords;
    uint32_t* s_queue = s_lines + kLineWords;
    uint32_t* s_misc = s_queue + kQueueCap;
#ifndef GMK_K1_TOTALS_HOT
    uint32_t* const my_totals = s_queue + kQueueCap - 8 * kTotalsCopies + (lane0 & (kTotalsCopies - 1)) * 8;  // this lane's copy of the per-type totals (phase 0 says why)
#else
    uint32_t* const my_totals = s_misc + 4;
#endif

    // (no barrier here: the tables are on their way while every wavefront runs phase 0 of its first board, which needs none of them; the one
    // barrier of the kernel stands in front of that board's phase 1)
    GMK_STAMP(0);

    // ---- work distribution: see the hand-out counter below ----
    const bool planes_out = out_density != nullptr && (phase_mask & 64) && !(phase_mask & 1024);
    int lane = lane0;
    // (from the lane's record, not from the staged copies: those are not there yet)
    const uint32_t lines_word = lane_lines.x, place_word = lane_lines.y;      // ("Lane -> lines" above)
    const uint32_t line_init_lo = lane_lines.z, line_init_hi = lane_lines.w;
    const uint32_t cell_row4 = lane_consts.x, cell_col = lane_consts.y, norm_a = lane_consts.z, norm_b = lane_consts.w;
    uint32_t* s_rows = s_misc + 16;                      // row y at [3 + y]
    // a board's 64 B are fetched while the board before it is evaluated.  No branch around the loads (every lane reads some valid
    // row, the result is masked where it is used), and the two halves stay apart until they are used: any arithmetic on a loaded
    // value makes the compiler wait for it on the spot, and the wait covers every store issued before.
    const uint16_t* row_ptr = planes + (lane & 15);
    uint32_t next_black = 0, next_white = 0, cur_black = 0, cur_white = 0;
    auto fetch_row = [&](int b) {
        const uint16_t* p = row_ptr + static_cast<size_t>(min(b, n_boards - 1)) * 32;
        next_black = p[0];                              // (bit 15 of a row is zero, the planes' contract in include/gomoku_hip.h: phase 0's packed gate shifts and the
                                                        //  white stone count rely on it, nothing here clears it)
        next_white = p[16];
    };
    auto take_row = [&](int lane_m, int b) -> uint32_t { return lane_m < 16 && b < n_boards ? cur_black | (cur_white << 16) : 0u; };

    // The workgroup owns one contiguous run of groups (what a CU writes at any time lies within a few hundred kilobytes) and hands its
    // boards out one at a time from a counter in LDS: the sixteen wavefronts -- four per SIMD, and a SIMD's vector unit is what the kernel
    // is bound by -- finish within one board of each other instead of 16 boards x (the spread of a board's work, ~ +-25 %) apart.
    // The density bursts of its groups go with boards of the run that are fixed in advance (phase D below).
    // (Round 2 measured a dynamic hand-out -- chunks of four, stealing round a ring of workgroups -- as no gain and concluded the wavefronts'
    // waits were the limit.  They are not: tools/valu_probe.hip shows a wave-instruction costs a SIMD 4 cycles whatever its type, K1's ~950
    // per board make the vector unit ~90 % busy while all sixteen wavefronts run, and what the static hand-out lost was whole SIMDs idling
    // behind the slowest one: 0.1544 -> 0.1402 ms.)
    // (groups_each = groups / grid and groups_extra = groups % grid come from the host: the first groups_extra workgroups own one group more.  Worked
    // out here as floor(groups * block / grid) it was two 64-bit divisions, ~200 scalar instructions per wavefront and launch.)
    const int wg_block = static_cast<int>(blockIdx.x);
    const int wg_g0 = groups_each * wg_block + min(wg_block, groups_extra);
    const int wg_groups = groups_each + (wg_block < groups_extra ? 1 : 0);
    const int wg_first = wg_g0 * kGroupBoards, wg_boards = min(wg_groups * kGroupBoards, n_boards - wg_first);
    auto hand_out = [&]() -> int {
        uint32_t v = 0;
        if (lane0 == 0) v = atomicAdd(s_handout, 1u);
        return __builtin_amdgcn_readfirstlane(static_cast<int>(v));
    };
    // A wavefront's first two boards are fixed (boards w and 16 + w of the workgroup's run; the counter starts behind them): the first dynamic hand-out
    // then comes after the kernel's one barrier.
    int idx = wave, boards_done = 0;
    if (idx < wg_boards) fetch_row(wg_first + idx);
    // the image goes to LDS (address 0 on) once every load of the prologue is on its way
    {
        uint4* s_stage = reinterpret_cast<uint4*>(lds);
        if (tid < stage_vecs) s_stage[tid] = stage_a;
        if (tid + kThreads < stage_vecs) s_stage[tid + kThreads] = stage_b;
        for (int i = tid + 2 * kThreads; i < stage_vecs; i += kThreads) s_stage[i] = g_stage[i];
    }
    asm volatile("" : "+v"(next_black), "+v"(next_white));        // (once: wait for them here)
    GMK_TL(1, __builtin_amdgcn_s_memtime());
#pragma unroll 1
    for (;;) {
#ifdef GMK_K1_MARKERS
        GMK_STAMP(10);                                          // (the loop's top: what lies in front of it is the prologue, not the loop head)
#endif
        const bool live = idx < wg_boards;
        const int board = wg_first + idx;
        cur_black = next_black; cur_white = next_white;
        int idx_next = idx;
        if (live) { idx_next = boards_done == 0 ? kBoardsPerBlock + wave : hand_out(); fetch_row(wg_first + min(idx_next, wg_boards - 1)); }
        GMK_STAMP(11);

        // Phase 0 in two parts.  In front of the scan stands only what its first lookup needs: the blank line words, the stones' XORs, and the clear of
        // s_misc (the scan flags into s_misc[2]).  Everything else of phase 0 -- the counters' and the totals copies' clears, the stone count, the area
        // bonus and the score block's four 16-byte writes -- is read by phase 2 at the earliest and is issued INSIDE the scan, one piece behind each of
        // its first lookups (late_piece): LDS serves a wavefront in order, so in front of the line words those seven wide writes (~13 cycles each on the
        // store path) and four ds_bpermute stood between every board and its first lookup.
        uint32_t late_row = 0;
        int late_lane = lane, late_gate = 0, late_gw = 0;         // (late_gw: the gate word the next score-block piece uses, asked for one lookup ahead)
        auto late_piece = [&](int piece) {
            if (piece == 0) {
#ifndef GMK_K1_TOTALS_HOT
                // (in front of the scan's first queue write, as it always was: a flagged board's last entries may lie where the copies do)
                if (lane < 8 * kTotalsCopies) s_queue[kQueueCap - 8 * kTotalsCopies + lane] = 0;
#endif
            } else if (piece <= 3) {
                // (the counters; the score block is written below, with the area bonus in it)
                constexpr int kVecs = kCntWords / 4;
                static_assert(kVecs > 128 && kVecs <= 192, "three pieces of 64 lanes clear the counters");
                const int i = 64 * (piece - 1);
                if (i + 64 <= kVecs || late_lane < kVecs - i) (reinterpret_cast<uint4*>(s_cnt) + lane)[i] = make_uint4(0u, 0u, 0u, 0u);
            } else if (piece == 4) {
                // stones per colour: a row reduction in registers (an atomicAdd of fifteen lanes on one word is turned by the compiler
                // into a serial loop over those lanes)
                uint32_t cnt = static_cast<uint32_t>(__popc(late_row & 0x7FFFu)) | (static_cast<uint32_t>(__popc(late_row >> 16)) << 16);
                cnt += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(cnt), 0x118, 0xF, 0xF, false));       // row_shr:8
                cnt += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(cnt), 0x114, 0xF, 0xF, false));       // row_shr:4
                cnt += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(cnt), 0x112, 0xF, 0xF, false));       // row_shr:2
                cnt += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(cnt), 0x111, 0xF, 0xF, false));       // row_shr:1
                if (late_lane == 15) s_misc[0] = cnt;             // lane 15 holds the sum of lanes 0 .. 15 (the row is zero in lane 15)
            } else if (piece == 5) {
                // Where is a colour's density count positive (<=> its weight positive: the +160 of Pattern.cpp:268)?  Wherever a stone
                // of the colour lies under the 7x7 BlockWeights mask (Pattern.cpp:598-609) around the cell: the rows, dilated by the
                // mask's row patterns -- 1001001 three rows away, 0111110 one and two rows away, 1110111 in the row itself -- and OR-ed
                // over the seven rows, for both colours at once (black in the low, white in the high half word), restricted to empty cells.
                const uint32_t r = late_row;
                // packed 16-bit shifts: nothing crosses from one half word into the other, so no masks.  Bit 15 of a row is zero (the planes'
                // contract, include/gomoku_hip.h), so nothing comes down from it; what a left shift leaves there is cut off by `empty` below.
                const v2u16 rr = __builtin_bit_cast(v2u16, r);
                const uint32_t l1 = __builtin_bit_cast(uint32_t, static_cast<v2u16>(rr << 1)), l2 = __builtin_bit_cast(uint32_t, static_cast<v2u16>(rr << 2)), l3 = __builtin_bit_cast(uint32_t, static_cast<v2u16>(rr << 3));
                const uint32_t r1 = __builtin_bit_cast(uint32_t, static_cast<v2u16>(rr >> 1)), r2 = __builtin_bit_cast(uint32_t, static_cast<v2u16>(rr >> 2)), r3 = __builtin_bit_cast(uint32_t, static_cast<v2u16>(rr >> 3));
                const int far = static_cast<int>(r | l3 | r3), near = static_cast<int>(r | l1 | l2 | r1 | r2);
                uint32_t g = l1 | l2 | l3 | r1 | r2 | r3;
                g |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, near, 0x111, 0xF, 0xF, true)) | static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, near, 0x101, 0xF, 0xF, true));     // rows y -+ 1
                g |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, near, 0x112, 0xF, 0xF, true)) | static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, near, 0x102, 0xF, 0xF, true));     // rows y -+ 2
                g |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, far, 0x113, 0xF, 0xF, true)) | static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, far, 0x103, 0xF, 0xF, true));       // rows y -+ 3
                const uint32_t empty = ~(r | (r >> 16)) & 0x7FFFu;
                if (lane < 15) s_rows[3 + lane] = r;            // (three zero rows on either side: phase 3b's density gate read rows y - 3 .. y + 3 unchecked until round 15; nothing reads them now)
                late_gate = static_cast<int>(g & (empty | (empty << 16)));
                // (the first score-block piece's gate word: asked for here, one lookup ahead of its use, see below)
                late_gw = __builtin_amdgcn_ds_bpermute(static_cast<int>(cell_row4 & 0xFFu), late_gate);
            } else if (piece <= 9) {
                // The score block starts at the area bonus instead of zero: +160 in a colour's own view where its gate bit is set
                // (Pattern.cpp:268), one 16-byte write per cell [white own, white opp, black opp, black own]; the gate word of the
                // cell's row comes from that row's lane.  The ds_bpermute that fetches it is issued by the piece BEFORE, behind that piece's own write: it
                // then comes back ahead of the lookup this step waits for anyway.  Issued here it came back behind that lookup, and the wait in front of
                // the next lookup's address covered it, the queue write and the lookup together.
                // No lane mask on the fourth write, so that the wait behind it is a counted one: its 31 lanes behind the last cell fetch the gate word
                // of lane 16, which holds no row and is zero on every board (lane_tables), and write 16 bytes of zeros onto the first counter words,
                // which the pieces before have cleared and nobody has counted into yet.
                const int pass = piece - 6;
                const uint32_t gw = static_cast<uint32_t>(late_gw) >> ((cell_col >> (8 * pass)) & 0xFFu);
                static_assert(4 * 256 - kScoreWords <= kCntWords, "the fourth write's lanes behind the last cell land on counter words");
                reinterpret_cast<uint4*>(s_scores)[64 * pass + lane] = make_uint4(static_cast<uint32_t>(__builtin_amdgcn_sbfe(static_cast<int>(gw), 16, 1)) & 160u, 0u, 0u,
                                                                                  static_cast<uint32_t>(__builtin_amdgcn_sbfe(static_cast<int>(gw), 0, 1)) & 160u);
                if (pass < 3) late_gw = __builtin_amdgcn_ds_bpermute(static_cast<int>((cell_row4 >> (8 * (pass + 1))) & 0xFFu), late_gate);
            }
        };
        constexpr int kLatePieces = 10;
        static_assert(kLatePieces <= kScanSteps - kScanPrefixSyms + 1, "a piece per lookup");
        if (live) {
            // ---- phase 0, the part in front of the scan: take the two bit-planes (64 B), turn them into line words ----
            // The lane masks of this phase come from a copy of the lane number that the compiler cannot see through: a compare per board each.  Hoisted
            // out of the board loop they are scalar register pairs that do not fit and come back by two v_readlane each, per board.
            int lane_m = lane;
            asm volatile("" : "+v"(lane_m));
            s_lines[lane] = line_init_lo;                       // (the all-blank line words wait in two registers, not in LDS: no read before the write)
            if (lane_m < kLineWords - 64) s_lines[64 + lane] = line_init_hi;
            if (lane_m < kMiscWords) s_misc[lane] = 0;
            const uint32_t my_row = take_row(lane_m, board);
            late_row = my_row; late_lane = lane_m;
            wave_phase_fence();
            {
                // a stone turns its cell's blank (3) into black (0) or white (1) in the four lines through it: one XOR each.
                // Four lanes share a row (cells 0-3, 4-7, 8-11, 12-14), so the loop runs as long as the fullest quarter row.
                const int y = lane >> 2, part = lane & 3;
                const uint32_t row = __shfl(my_row, min(y, 14));
                uint32_t row_sym = 0;
                // (what the loop needs of y, worked out in front of it: left to itself the compiler recomputes both for every stone)
                uint32_t y2 = 2u * static_cast<uint32_t>(y), y4 = 4u * static_cast<uint32_t>(y);
                asm volatile("" : "+v"(y2), "+v"(y4));
                for (uint32_t m = lane < 60 ? (row | (row >> 16)) & (0xFu << (4 * part)) & 0x7FFFu : 0u; m; m &= m - 1u) {
                    const int x = __ffs(m) - 1;
                    const uint32_t code = ((row >> x) & 1u) | 2u;                      // black 3, white 2
                    const uint32_t at_x = code << (2 * x), at_y = code << y2;
                    row_sym |= at_x;
                    // (the three words lie at the column's word -+ y: one shift-add and two adds, the bases are immediate offsets)
                    char* const col = reinterpret_cast<char*>(s_lines + x);
                    atomicXor(reinterpret_cast<uint32_t*>(col) + kColBase, at_y);
                    atomicXor(reinterpret_cast<uint32_t*>(col - y4) + (kDiagBase + 14), at_x);
                    atomicXor(reinterpret_cast<uint32_t*>(col + y4) + kAntiBase, at_y);
                }
                if (row_sym) atomicXor(&s_lines[y], row_sym);
            }
            wave_phase_fence();
            GMK_STAMP(1);
        }
#ifdef GMK_PROFILE
        if (boards_done == 0) GMK_TL(2, __builtin_amdgcn_s_memtime());
#endif
        if (boards_done == 0) __syncthreads();                  // the tables are staged (the automaton at LDS address 0, the records, the pads, the tables of phase D,
                                                                // the hand-out counter): from here on the wavefronts never wait for each other
#ifdef GMK_PROFILE
        if (boards_done == 0) GMK_TL(3, __builtin_amdgcn_s_memtime());
        if (live) { tl_bursts = 0; tl_burst_clocks = 0; }
#endif
        if (live) {
            // ---- phase 1: walk the DFA along this lane's lines; transitions that emit go to the queue ----
            // The lane's one or two lines become ONE stream of 2-bit DFA symbols:
            //   cells '?' '?'  [cells '?' '?']  '?' '?' ...
            // walked from S, the state the root reaches on '?', and not from the root.  The root on '?' goes to S and emits nothing, S on '?' stays in S and
            // emits nothing, and from every state "??" leads to S (scan_start_row checks all three when the image is built and refuses a table without them):
            // a leading '?' in front of either line would be a lookup that reports nothing and changes nothing, so there is none -- seventeen steps where
            // there were nineteen -- and there is no reset between the two lines.  BOTH trailing pads stay: of the 21 523 239 lines of 5 to 15 cells, 59 050
            // report a match on the symbol behind the first trailing pad (a match ending one symbol back, found while falling back); sharing that symbol
            // with the second line's first cell would put the first line's late match into a record of the second line.  The stream is kept shifted left by 2, so a step is: symbol * 4 = low word & 12, LDS
            // address = (previous word's next-row offset) | symbol * 4, one lookup.  Emitting transitions are queued as
            // (record, place of the symbol: `push` below); the slot is a ballot prefix (this wave is the only producer), phase 2 uses the entry as it is.
            int n_queued = 0;                                       // wave-uniform
            if (phase_mask & 2) {
                const int len_a = static_cast<int>(lines_word & 31u) - kSegPads, len_b = static_cast<int>((lines_word >> 5) & 31u) - kSegPads;
                uint64_t syms = line_symbols(s_lines[(lines_word >> 10) & 127u] >> norm_a, len_a);      // (a diagonal's word shifted down to its first cell)
                syms |= line_symbols(s_lines[(lines_word >> 17) & 127u] >> norm_b, len_b) << (2 * (len_a + kSegPads));
                syms |= 0xAAAAAAAAAAAAAAAAull << (2 * (len_a + len_b + 2 * kSegPads));
                // The stream is kept shifted left by 2: symbol s at bits 2 s + 2, so that the four bits from 2 s up are (symbol s - 1, symbol s) and
                // one v_bfe + one v_bfi make the lookup address: (table word & 0x3FF3) | (those four bits & 12) -- the row offsets are multiples of 16.
                const uint32_t cur = static_cast<uint32_t>(syms) << 2;        // symbols 0..14 at bits 2..31
                const uint32_t rest = static_cast<uint32_t>(syms >> 28);      // symbols 15.. at bits 2.. (bits 0, 1: symbol 14)
                // The emission of step s is worked out BEHIND the lookup of step s + 1 (the next address needs the table word only): the
                // prefix count runs in the shadow of that lookup's LDS round trip; the write follows behind lookup s + 2 (below).  A queue entry is the table
                // word itself with the low 17 bits (next row, kinds) replaced by the place of the symbol (`push`): the record number stays where it is.
                // Where the queue stands is a byte address kept by the scalar unit; a lane adds its prefix count (the vector unit is
                // what this kernel is bound by: 4 cycles per wave-instruction on a SIMD whatever the lanes do).
                const uint32_t q_base = static_cast<uint32_t>(s_queue - lds) * 4u;     // (the kernel's LDS starts at address 0)
                // The scalar unit keeps the fill level at most 64 entries below the capacity: a step's (at most 64) entries then fit whatever the
                // lanes add, without a per-lane clamp (a vector instruction per step); a board that gets there is flagged below.
                constexpr int kQueueFlagAt = kQueueCap - 64;        // the most entries the scan leaves: n_queued <= kQueueFlagAt
                const uint32_t q_full = q_base + 4u * kQueueFlagAt;
                // (phase 2 reads one round ahead, entry m + 64 for m < n_queued: inside the queue without a clamp)
                static_assert(kQueueFlagAt > 0 && (kQueueFlagAt - 1) + 64 < kQueueCap, "the deposits' read one round ahead stays inside the queue");
                uint32_t q_at = q_base;                             // wave-uniform
                // A step's queue write is DEFERRED by one lookup more: `push` only works out a lane's address and entry (in the shadow of lookup s + 1) and
                // `flush` writes them immediately behind lookup s + 2, one instruction after it.  The write is conditional, so the compiler's wait in front
                // of the next lookup's address is lgkmcnt(0) wherever a path around a write exists, and LDS answers a wavefront in order: written where it
                // was worked out, five vector instructions behind the lookup, the write's acknowledgement stood on every step's chain.  (Every lane writing,
                // the idle ones into 64 dump words, makes the waits counted at the price of a v_cndmask per step and measured less: DESIGN.md, round 13.)
                uint32_t pend_at = 0, pend_entry = 0;
                bool pend = false;
                auto flush = [&]() { if (pend) *lds_word_rw(pend_at) = pend_entry; };
                // The entry carries the PLACE of the consumed symbol -- cell, direction, minus the stride, as the deposits use them -- and not (lane, step):
                // the place runs along with the steps, one add each (the stride comes out of the lines word by an SDWA byte select; the jump across a
                // two-line lane's seam is one DPP add on its four lanes at step 9 and one at step 10), where lane | step << 6 was one OR each.
                uint32_t place = place_word;                        // the place of step kScanPrefixSyms, the first step pushed
                const int seam_jump = __builtin_amdgcn_sbfe(static_cast<int>(place_word), 17, 10);
                auto push = [&](uint32_t word, int step) {
                    const bool emits = word > 0x1FFFFu;
                    const unsigned long long emitters = __ballot(emits);
                    const uint32_t ahead = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(emitters >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(emitters), 0u));
                    pend = emits;
                    pend_at = q_at + 4u * ahead;
                    if (step > kScanPrefixSyms) place = place_advance(place, lines_word);
                    static_assert(kPairedLanes == 8, "two banks of four lanes: the long first lines in front");
                    if (step == kSeamStepShort) place = place_jump<kFirstPairedLane + 4>(place, seam_jump);   // lanes 60..63
                    if (step == kSeamStepLong) place = place_jump<kFirstPairedLane>(place, seam_jump);        // lanes 56..59
                    pend_entry = queue_entry(word, place);
                    asm volatile("" : "+v"(pend_at), "+v"(pend_entry));       // (worked out HERE: left to itself the compiler sinks both to where they are written)
                    q_at = min(q_at + 4u * static_cast<uint32_t>(__popcll(emitters)), q_full);
                };
                // The first four symbols are cells of the lane's first line (every first line has five or more), and no walk of four cells from S
                // reports anything (scan_prefix_table checks all 81 when the image is built): ONE 16-bit read of the row S reaches over them, at
                // table + 2 * (the stream's first eight bits), stands for four lookups, ballots and pushes -- fourteen dependent round trips where
                // there were seventeen.  `cur` is the stream shifted left by 2 with bit 1 clear, so twice the key is its bits 1..9 (at most 510:
                // the read cannot leave the table).  The pushes keep their steps' numbers, 4..16: the queue is what seventeen lookups would leave.
                uint32_t tw = *lds_half(scan_prefix_at + __builtin_amdgcn_ubfe(cur, 1, 9));      // the previous step's table word (here a bare row offset)
                __builtin_amdgcn_sched_barrier(0);
                late_piece(0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int step = kScanPrefixSyms; step < kScanSteps; ++step) {
                    const int nth = step - kScanPrefixSyms + 1;         // which lookup of the scan this is, the prefix read being the first
                    const uint32_t four = step < 15 ? __builtin_amdgcn_ubfe(cur, 2 * step, 4) : __builtin_amdgcn_ubfe(rest, 2 * (step - 15), 4);
                    const uint32_t addr = dfa_address(tw, four);
                    const uint32_t before = tw;
                    tw = *lds_word(addr);                       // (the table is at LDS address 0: the address is used as it is)
                    flush();                                    // (the entries of step - 2, back to back with the lookup and held there)
                    __builtin_amdgcn_sched_barrier(0);
                    if (step > kScanPrefixSyms) push(before, step - 1);
                    // (a piece of phase 0 in this lookup's shadow, and held there: left to itself the compiler gathers the pieces in front of the scan again)
                    if (nth < kLatePieces) { late_piece(nth); __builtin_amdgcn_sched_barrier(0); }
                }
                flush();                                        // (the last two steps' entries: no lookup left to stand behind)
                push(tw, kScanSteps - 1);
                flush();
                n_queued = static_cast<int>((q_at - q_base) >> 2);
                if (q_at >= q_full) s_misc[2] = 1;                  // (flagged at kQueueCap - 64 = 384 entries: 2.0 x the 192 of the synthetic and dense test boards,
                                                                    //  1.14 x the 338 of the heaviest legal position a search found, DESIGN.md "K1's fixed capacities")
            }
#ifdef GMK_PROFILE
            else {                                                  // (profiling flavour, a mask without the scan: phase 0's pieces on their own)
#pragma unroll
                for (int piece = 0; piece < kLatePieces; ++piece) late_piece(piece);
            }
#endif
            wave_phase_fence();
            GMK_STAMP(2);

            // ---- phase 2: one lane per emitting transition: the score deposits of its 1-2 matches ----
            if (phase_mask & 4) {
                uint32_t qe_next = s_queue[lane];                   // (entry: record number << 17 | minus the stride << 11 | direction << 9 | cell)
                for (int m = lane; m < n_queued; m += 64) {
                    const uint32_t qe = qe_next;
                    qe_next = s_queue[m + 64];                      // (the next round's entry is on its way while this one is worked on; m + 64 < n_queued + 64
                                                                    //  <= kQueueCap, the scan's assert: no clamp.  Fetching its record ahead as well measured no gain)
                    // the entry says where the consumed symbol lies and how to walk back from it: nothing to look up, nothing to work out
                    const uint4 rec_now = s_rec[qe >> 17];
                    const int cell_at = qe & 511u, dir = (qe >> 9) & 3u;
                    const int back_step = __builtin_amdgcn_sbfe(static_cast<int>(qe), 11, 6);
                    deposit_match(rec_now.x, rec_now.y, cell_at, dir, back_step, s_scores, s_cnt, s_misc, my_totals);
                    if (rec_now.z) deposit_match(rec_now.z, rec_now.w, cell_at, dir, back_step, s_scores, s_cnt, s_misc, my_totals);
                }
            }
            wave_phase_fence();
#ifndef GMK_K1_TOTALS_HOT
            // the copies of the per-type totals (see my_totals) become the totals row; their place is the queue's again from phase 3b on
            if (lane < 8) {
                const uint32_t* t = s_queue + kQueueCap - 8 * kTotalsCopies + lane;
                uint32_t sum = 0;
#pragma unroll
                for (int c = 0; c < kTotalsCopies; ++c) sum += t[8 * c];
                s_misc[4 + lane] = sum;
            }
#endif
            GMK_STAMP(3);

            // ---- phase 3: one lane per cell: compound candidates (the area bonus is in the block since phase 0) ----
            int n_cand = 0;                                         // wave-uniform
            if (phase_mask & 8) {
                // (the reads of all four passes first: four round trips in a row are four waits)
                uint32_t any_cnt[4];
    #pragma unroll
                for (int pass = 0; pass < 4; ++pass) {
                    const int qc = min(64 * pass + lane, kCells - 1);               // the last pass has 33 cells
                    any_cnt[pass] = s_cnt[qc] | s_cnt[kCells + qc] | s_cnt[2 * kCells + qc];
                }
    #pragma unroll
                for (int pass = 0; pass < 4; ++pass) {
                    const int q = 64 * pass + lane;
                    // compound candidates (Compound::Test, Pattern.cpp:424-433): cells whose LiveThree / DeadThree / LiveTwo '_' counters, each
                    // clipped to 2 (the reference's 2-bit shift flags), OR-ed over the types, sum to two or more over the directions (only
                    // empty cells have counters: a '_' piece is a blank).  Decided in phase 3b, with the density gate of Pattern.cpp:182.
                    const uint32_t any = any_cnt[pass];
                    // A colour's half word h holds its four direction nibbles; "the clipped counts sum to two or more" is "a nibble is >= 2 or two
                    // nibbles are non-zero", and that is h & ((h - 1) | 0xEEEE) != 0: a nibble >= 2 has one of its upper three bits set; with every
                    // nibble 0 or 1, h & (h - 1) is h without its lowest set bit.  Both colours at once: a packed 16-bit decrement (no borrow
                    // from white's half into black's) and one three-operand bit operation.  The exact sums are not needed: phase 3b works
                    // everything out from the counters again and only asks which colour made the cell a candidate.
                    const uint32_t hot = any & (pk_dec_u16(any) | 0xEEEEEEEEu);
                    // (the last pass has 33 cells: the lanes behind them read cell 224 again and are cut out of the ballot on the scalar unit)
                    const unsigned long long pushers = __ballot(hot != 0u) & (pass < 3 ? ~0ull : (1ull << (kCells - 192)) - 1ull);
                    if (pushers) {
                        if (hot != 0u && (pass < 3 || lane < kCells - 192)) {
                            const int slot = n_cand + static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(pushers >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(pushers), 0u)));
                            // the entry: the cell, bit 8: white's counters made it a candidate, bit 9: black's
                            if (slot < kQueueCap / 2) s_queue[slot] = static_cast<uint32_t>(q) | ((hot & 0xFFFFu) ? 0x100u : 0u) | ((hot >> 16) ? 0x200u : 0u);
                        }
                        n_cand += __popcll(pushers);
                    }
                }
            }
            wave_phase_fence();
            GMK_STAMP(4);

            // ---- phase 3b: four lanes (a quad) per candidate cell and colour, sixteen such pairs per round: the compound decision
            //      (Pattern.cpp:440-486) in every lane of the quad, critical-point deposits by its lane 0, the two counter-move rescans queued in
            //      the upper half of the queue by its lanes 0 and 1, one entry each.  What a board pays for is the length of the round, not the
            //      lanes it leaves idle (a typical board has two to four pairs): a lane builds ONE entry where it built two ----
            // (an empty cell is a candidate at most once and a board with a counter has a stone: n_cand <= 224 = kQueueCap / 2, the list cannot overflow)
            if (n_cand > kQueueCap / 2) { s_misc[2] = 1; n_cand = kQueueCap / 2; }
            if (phase_mask & 2048) n_cand = 0;
            // The rescan queue works in ROUNDS: a round of phase 3b queues at most 16 x 2 entries, and phase 4 empties the queue once the next
            // round's might not fit, and behind the last round.  (Legal positions queue more than the upper half holds -- 116 compounds of this
            // kind = 232 entries on a position of tests/golden/k1_saturated.npz -- and used to be flagged with their rescans dropped.)  The
            // benchmark's boards have a median of under two candidates and at most 32: one round on most, four at the most, phase 4 once; a board
            // without candidates skips both.  A saturated position (121 candidates) takes 16 rounds where it took 4 with 64 pairs per round.
            constexpr int kPairsPerRound = 16;                      // (candidate, colour) pairs per round: four lanes each
            constexpr int kRescanFlush = kQueueCap / 2 - 2 * kPairsPerRound;    // fill level above which another round might not fit
            static_assert(kRescanFlush > 0 && kRescanFlush + 2 * kPairsPerRound <= kQueueCap / 2, "a round of phase 3b fits behind the flush level");
            int n_comp_q = 0;                                       // components queued for phase 4 (wave-uniform: slots by ballot prefix)
            if (phase_mask & 8)
            for (int v0 = 0; v0 < 2 * n_cand; v0 += kPairsPerRound) {      // four lanes per (candidate cell, colour): 0 white, 1 black
                int lane_3 = lane;                                  // (an opaque copy: the quad's place is derived here, not kept in registers across the board loop)
                asm volatile("" : "+v"(lane_3));
                const int j = lane_3 & 3, v = v0 + (lane_3 >> 2);
                const int flag_shift = 8 + (v & 1);                // this pair's colour flag in a candidate entry (bit 8 white, bit 9 black)
                const uint32_t ce = s_queue[v >> 1];                // (< n_cand + 8 <= 232: inside the queue; pairs past the end are masked below.  One address per quad: a broadcast)
                const int q = ce & 255, c = v & 1;
                bool queue = false;
                uint32_t ent = 0;
                if (v < 2 * n_cand && ((ce >> flag_shift) & 1u)) {  // (the same in the four lanes of a quad)
                    // this colour's four direction nibbles of the three counter words
                    const uint32_t f3 = (s_cnt[q] >> (16 * c)) & 0xFFFFu, fd = (s_cnt[kCells + q] >> (16 * c)) & 0xFFFFu, f2 = (s_cnt[2 * kCells + q] >> (16 * c)) & 0xFFFFu;
                    const int qy = (q * 0x8889) >> 19, qx = q - 15 * qy;
                    // The reference's density gate (Pattern.cpp:182: the colour's density COUNT at the cell must be two or more) is not evaluated: it holds for
                    // every pair that gets here.  The pair's flag says that a LiveThree, DeadThree or LiveTwo match of the colour has a '_' on q; in every such
                    // pattern every '_' has two or more of the pattern's own stones within three cells on its line, and the count's 7x7 mask covers all
                    // eight line directions out to three cells (tests/test_eval_density_gate.py checks both on the tables; until round 15 seven row reads,
                    // masks and popcounts per pair worked the count out, about 35 of the round's 140 vector instructions, and no board ever failed it).
                    {
                        // The reference walks the directions in order through a state machine S0, L2, LD3, To33, To43, To44 (Pattern.cpp:440-486); in
                        // each direction the component is the first of LiveThree, DeadThree, LiveTwo with a non-zero counter, taken once or twice (the
                        // counters count like its 2-bit shift flags: 0, 1, 2 or more, Pattern.cpp:395-400).  Its outcome does not depend on the order:
                        // with n components of which s are threes (weight 2, a LiveTwo 1), the state ends at 3 + min(2, s) for n >= 2 -- the first two
                        // transitions add w1 + w2 + 1, every further one w - 1, capped at 5 -- and the "triple" flag is n >= 3.  So: nibble masks.
                        // (Worked out in every lane of the quad: the instructions are wave-wide anyway.)
                        const uint32_t up3 = (f3 >> 1) | (f3 >> 2) | (f3 >> 3), upd = (fd >> 1) | (fd >> 2) | (fd >> 3), up2 = (f2 >> 1) | (f2 >> 2) | (f2 >> 3);
                        const uint32_t sel3 = (f3 | up3) & 0x1111u;                                          // directions whose component is a LiveThree
                        const uint32_t seld = (fd | upd) & 0x1111u & ~sel3;                                  // ... a DeadThree
                        const uint32_t sel2 = (f2 | up2) & 0x1111u & ~(sel3 | seld);                         // ... a LiveTwo
                        const uint32_t strong = sel3 | seld, any_dir = strong | sel2;
                        const uint32_t twice_strong = (sel3 & up3) | (seld & upd), twice = twice_strong | (sel2 & up2);     // taken twice (counter >= 2)
                        const int n_comp = __popc(any_dir) + __popc(twice), threes = __popc(strong) + __popc(twice_strong);
                        if (n_comp < 2) {
                            if (j == 0) s_misc[2] = 1;                                                       // reference reads out of bounds here
                        } else {
                            if (j == 0) {                                                                    // once per pair
                                const int ctype = min(threes, 2);
                                atomicAdd(&s_misc[12 + ctype], c ? 0x10000u : 1u);
                                // updateCritical, both perspectives: the colour's pair of the cell
                                const uint32_t crit = 600u * static_cast<uint32_t>(n_comp);
                                atomicAdd(reinterpret_cast<unsigned long long*>(s_scores) + 2 * q + c, (static_cast<unsigned long long>(crit) << 32) | crit);
                            }
                            // exactly two components, no live three among them: queue their counter-move rescans, in direction order, with what
                            // phase 4 needs of each line ready in the entry: q | colour << 8 | direction << 9 | type slot << 11 | line word << 13 |
                            // q's slot in the word << 20.  A line word holds cell x at slot x (rows, diagonals) or y (columns, anti-diagonals), so
                            // per direction d = 0..3 the word is byte d of `lines` and the slot nibble d of `slots`.  Lane 0 of the quad builds the
                            // first component's entry, lane 1 the second's (lanes 2 and 3 build it too and write nothing)
                            queue = n_comp < 3 && !sel3;
                            const uint32_t others = any_dir & (any_dir - 1u);
                            const uint32_t pick = (j == 0 || !others) ? any_dir : others;                    // a component taken twice is both entries
                            const uint32_t b = static_cast<uint32_t>(__ffs(pick) - 1);                       // 4 d
                            const uint32_t ux = static_cast<uint32_t>(qx), uy = static_cast<uint32_t>(qy);
                            const uint32_t lines = (static_cast<uint32_t>(kColBase) << 8 | static_cast<uint32_t>(kDiagBase + 14) << 16 | static_cast<uint32_t>(kAntiBase) << 24)
                                                   + ((ux << 8) * 0x10101u) + uy * 0xFF0001u;               // y | 20 + x | 50 + x - y | 65 + x + y
                            const uint32_t slots = ux * 0x0101u + uy * 0x1010u;                              // x | y | x | y
                            const uint32_t tslot = ((seld >> b) & 1u) ? 1u : 2u;                             // DeadThree 1, LiveTwo 2
                            ent = static_cast<uint32_t>(q) | (static_cast<uint32_t>(c) << 8) | (b >> 2) << 9 | tslot << 11 | __builtin_amdgcn_ubfe(lines, 2 * b, 8) << 13
                                  | __builtin_amdgcn_ubfe(slots, b, 4) << 20;
                        }
                    }
                }
                // quads are counted, not lanes: of each quad only its LAST lane stays in the ballot, so that what a lane counts below itself is the
                // queueing quads in front of its own, whichever lane of the quad it is
                const unsigned long long queuers = __ballot(queue) & 0x8888888888888888ull;
                if (queue && j < 2) {
                    const uint32_t slot = static_cast<uint32_t>(n_comp_q) + 2u * __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(queuers >> 32),
                                                                                                          __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(queuers), 0u));
                    // (slot + j <= kRescanFlush + 2 * 15 + 1 < kQueueCap / 2: no bounds check)
                    s_queue[kQueueCap / 2 + slot + static_cast<uint32_t>(j)] = ent;
                }
                n_comp_q += 2 * __popcll(queuers);
                if (v0 + kPairsPerRound < 2 * n_cand && n_comp_q <= kRescanFlush) continue;      // more candidates and room for their round: on with phase 3b
            wave_phase_fence();
            GMK_STAMP(5);

            // ---- phase 4: the counter-move cells of every compound component: the FIRST match of its type that runs through
            //      the cell with a blank there (Compound::updateAntis, Pattern.cpp:520-543), scanning the 13-symbol window
            //      centred on the cell.  Such a match ends at window index 6..12; seven lanes share a component (nine components
            //      per round, lane 63 idle), lane kk looks at the transition at index 6 + kk only (the automaton forgets its start
            //      state after 7 symbols, so <= 8 symbols from the root bring it to the right state: one read of the root's prefix table and <= 4 lookups), and the lowest lane with a hit applies it ----
            if (phase_mask & 16) {
                const int n_comp = n_comp_q;
                int lane_4 = lane;                                  // (an opaque copy: the lane's place is derived here, not kept in registers
                asm volatile("" : "+v"(lane_4));                    //  across the whole board loop)
                const int grp = lane_4 / 7, kk = lane_4 - 7 * grp, k = 6 + kk, start = k > 7 ? k - 7 : 0;
                for (int m0 = 0; m0 < n_comp; m0 += 9) {
                    const int m = m0 + grp;
                    const bool on = lane < 63 && m < n_comp;
                    const uint32_t ent = on ? s_queue[kQueueCap / 2 + m] : 0u;
                    const int q = ent & 255, c = (ent >> 8) & 1, dir = (ent >> 9) & 3, tslot = (ent >> 11) & 3;
                    const int stride = dir_stride(dir);
                    uint32_t hit_w0 = 0;
                    int hit_back = -1;
                    if (on) {
                        // the line through q in this direction, '?' off the line, and its symbols from window index `start` on (window index
                        // 0 = six cells before q): slot `first` of the word and the ones after it, '?' beyond either end of the word
                        const uint32_t line = (ent >> 13) & 127u;
                        const uint32_t word = s_lines[line] | s_pads[line];
                        const int first = static_cast<int>((ent >> 20) & 15u) + start - 6;                  // -6 .. 13
                        const uint32_t cur = __builtin_amdgcn_alignbit(first >= 0 ? 0xAAAAAAAAu : word, first >= 0 ? word : 0xAAAAAAAAu,
                                                                       static_cast<uint32_t>(2 * first) & 31u) << 2;      // kept shifted left by 2 as in phase 1
                        // Only the last transition's report is used, so the first four symbols from the root ('?' among them) are ONE read of
                        // DeviceTables::dev_prefix4, as in the incremental evaluator's window matcher (evalstate_device.h); four ordinary lookups
                        // follow, of which the lane of window index 6 (started at index 0 like that of index 7) keeps the third's word.
                        uint32_t tw = *lds_half(root_prefix_at + __builtin_amdgcn_ubfe(cur, 1, 9)), tw_third = 0;
    #pragma unroll
                        for (int i = 4; i < 8; ++i) {
                            if (i == 7) tw_third = tw;
                            tw = *lds_word(dfa_address(tw, __builtin_amdgcn_ubfe(cur, 2 * i, 4)));      // v_bfe + v_bfi, as in phase 1
                        }
                        if (kk == 0) tw = tw_third;
                        if ((gmk::dev_trans_kinds(tw) >> tslot) & 1u) {                     // the record holds the wanted type
                            const uint4 rec = s_rec[gmk::dev_trans_record(tw)];
                            const int want = 5 - tslot;                                     // LiveThree 5, DeadThree 4, LiveTwo 3
                            hit_back = counter_match(rec.x, k, want);
                            hit_w0 = rec.x;
                            if (hit_back < 0) { hit_back = counter_match(rec.z, k, want); hit_w0 = rec.z; }
                        }
                    }
                    const unsigned long long hits = __ballot(hit_back >= 0);
                    const uint32_t mine = static_cast<uint32_t>(hits >> (7 * grp)) & 0x7Fu;
                    if (hit_back >= 0 && (mine & ((1u << kk) - 1u)) == 0u) add_counter_cells(hit_w0, hit_back, q, stride, s_scores + (c ? 2 : 1));
                }
            }
            n_comp_q = 0;                                           // the queue is empty again (its entries are read before the next round writes: LDS runs in order)
            wave_phase_fence();
            GMK_STAMP(6);
            }                                                       // (the rounds of phases 3b and 4)

        }

        asm volatile("" : "+v"(next_black), "+v"(next_white));    // the wait for the next board's planes (a use the compiler must honour)
        GMK_STAMP(7);

        // ---- phase D: density planes of the workgroup's groups.  The burst of the run's k-th group belongs to the run's board kBurstEvery * k: whichever
        //      wavefront is handed that board takes the burst with it.  Every board is handed out once, so every burst is taken once, without a counter;
        //      a run of G groups has more than 16 (G - 1) >= kBurstEvery (G - 1) boards, so every burst has its board.  On a run of sixteen groups the last
        //      burst starts 76 boards -- almost five board times, a burst takes one and a half -- before the run's end: no wavefront is left with a burst
        //      when the boards have run out.  (Taken in turns, wavefront w in its w-th board, two bursts per workgroup were left for the end, and each
        //      held the launch's end back.)  A burst reads the boards' planes and nothing of their evaluation: it may run ahead of its group's boards. ----
        if (!live) break;
        const int burst = idx / kBurstEvery;
        if (planes_out && burst * kBurstEvery == idx && burst < wg_groups) {
#ifdef GMK_PROFILE
            const unsigned long long tl_burst_from = __builtin_amdgcn_s_memtime();
#endif
            int lane_p = lane0, first_p = (wg_g0 + burst) * kGroupBoards;      // opaque copies: what the passes derive from them is computed here
            asm volatile("" : "+v"(lane_p), "+s"(first_p));
            const int plane_stride = (phase_mask & 512) ? 0 : (phase_mask & 256) ? 256 : kCells;
            // (the queue is free here: phase 4 has read it, the next board's phase 0 fills it again)
            if (first_p + kGroupBoards <= n_boards && plane_stride > 0) density_planes_out<true>(planes, n_boards, first_p, lane_p, s_wtab, s_queue, out_density, s_lut, plane_stride);
            else density_planes_out<false>(planes, n_boards, first_p, lane_p, s_wtab, s_queue, out_density, s_lut, plane_stride);
            GMK_STAMP(8);
#ifdef GMK_PROFILE
            ++tl_bursts; tl_burst_clocks += __builtin_amdgcn_s_memtime() - tl_burst_from;
#endif
        }
        // ---- phase 5: results leave LDS ----
#ifdef GMK_K1_MARKERS
        GMK_STAMP(12);
#endif
        if (live && (phase_mask & 32)) {
            int lane_b = lane;                                  // (a copy the compiler cannot see through: the store addresses are computed here,
            asm volatile("" : "+v"(lane_b));                    // not kept in registers across the density pass)
            // Every store of the phase is global_store_dword <lane * 4>, <value>, s[base] offset:<immediate>: the board is wave-uniform, so its
            // blocks' addresses are worked out on the scalar unit, and what differs between the stores of a block is an immediate.
            const uint32_t lane_off = 4u * static_cast<uint32_t>(lane_b);
            if (out_scores) {
                // the block is [cell][group] in LDS and [group][cell] in memory: a lane reads the sixteen bytes of its cell and writes one
                // word into each group's plane, 256 contiguous bytes per store instruction
                const unsigned long long dst = reinterpret_cast<unsigned long long>(out_scores + static_cast<size_t>(board) * kScoreWords);
                const int4* src = reinterpret_cast<const int4*>(s_scores);
                // (all reads first: one LDS round trip instead of four)
                const int4 v0 = src[lane_b], v1 = src[lane_b + 64], v2 = src[lane_b + 128], v3 = src[min(lane_b + 192, kCells - 1)];
#ifdef GMK_K1_PLAIN_SCORES
                constexpr bool kNt = false;
#else
                constexpr bool kNt = true;                          // (non-temporal: 0.1575 -> 0.1543 ms)
#endif
#define GMK_STORE(words, v) store_saddr_imm<4 * (words), kNt>(lane_off, v, dst)
                // in ADDRESS order (the board's 3 600 bytes are one contiguous run: piece after piece, so that the two parts of a cache line that two
                // pieces share reach the L2 back to back)
                const bool tail = lane_b + 192 < kCells;
                GMK_STORE(0, v0.x); GMK_STORE(64, v1.x); GMK_STORE(128, v2.x); if (tail) GMK_STORE(192, v3.x);
                GMK_STORE(kCells, v0.y); GMK_STORE(kCells + 64, v1.y); GMK_STORE(kCells + 128, v2.y); if (tail) GMK_STORE(kCells + 192, v3.y);
                GMK_STORE(2 * kCells, v0.z); GMK_STORE(2 * kCells + 64, v1.z); GMK_STORE(2 * kCells + 128, v2.z); if (tail) GMK_STORE(2 * kCells + 192, v3.z);
                GMK_STORE(3 * kCells, v0.w); GMK_STORE(3 * kCells + 64, v1.w); GMK_STORE(3 * kCells + 128, v2.w); if (tail) GMK_STORE(3 * kCells + 192, v3.w);
#undef GMK_STORE
            }
            if (out_totals) {
                const unsigned long long dst = reinterpret_cast<unsigned long long>(out_totals + static_cast<size_t>(board) * 11);
                if (lane_b < 11) store_saddr_imm<0, false>(lane_off, static_cast<int32_t>(s_misc[4 + lane_b]), dst);
            }
            if (out_status) {
                // stones, winner bits and the error flag are one value per board: every lane reads them (one broadcast read each), the
                // scalar unit does the arithmetic, lane 0 stores the word
                const uint32_t stones = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(s_misc[0])));
                const uint32_t wbits = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(s_misc[1])));
                const uint32_t flagged = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(s_misc[2])));
                const int stones_b = stones & 0xFFFFu, stones_w = stones >> 16;
                // the side that completed five is the only one that can own a Five (the game stops there)
                const int winner = (wbits & 1u) ? 1 : (wbits & 2u) ? -1 : 0;
                const bool over = winner != 0 || stones_b + stones_w == kCells;
                const int to_move = over ? 0 : (stones_b == stones_w ? 1 : -1);
                const int word = (over ? 1 : 0) | ((flagged || phase_mask != 0x7F) ? 2 : 0) | ((winner & 0xFF) << 8) | ((to_move & 0xFF) << 16);
                const unsigned long long dst = reinterpret_cast<unsigned long long>(out_status + board);
                if (lane_b == 0) store_saddr_imm<0, false>(lane_off, word, dst);
            }
        }
        wave_phase_fence();
        GMK_STAMP(9);
#ifdef GMK_PROFILE
        tl_last_board = __builtin_amdgcn_s_memtime();
#endif
        idx = idx_next; ++boards_done;
    }
#ifdef GMK_PROFILE
    GMK_TL(4, tl_last_board);
    GMK_TL(6, static_cast<unsigned long long>(tl_bursts) | static_cast<unsigned long long>(boards_done) << 16);
    GMK_TL(7, tl_burst_clocks);
    GMK_TL(5, __builtin_amdgcn_s_memtime());
    // [0] table staging, [1] phase 0, [2] scan, [3] deposits, [4] phase 3, [5] phase 3b, [6] rescans, [7] wait for the next planes,
    // [8] phase D, [9] phase 5, [11] loop head; [15] wavefronts
    if (prof && lane0 == 0) {
        for (int k = 0; k < 12; ++k) atomicAdd(&prof[k], t_acc[k]);
        atomicAdd(&prof[15], 1ull);
    }
#endif
#undef GMK_STAMP
#undef GMK_TL
}

// ---- host side ----
struct LineJob { int len, x0, y0, dir; };

// The '?' pads as they lie in LDS (pads_out: kLineWords) and the 64 lane records (records_out: 8 words each), the lines word and the place word
// ("Lane -> lines" above) checked against the plain statement: a record that differs from it is an error, not a wrong score.
int lane_tables(uint32_t* pads_out, uint32_t* records_out) {
    std::vector<LineJob> lines;
    for (int i = 0; i < 15; ++i) lines.push_back({15, 0, i, 0});
    for (int i = 0; i < 15; ++i) lines.push_back({15, i, 0, 1});
    for (int d = -10; d <= 10; ++d) lines.push_back({15 - std::abs(d), d > 0 ? d : 0, d > 0 ? 0 : -d, 2});
    for (int k = 4; k <= 24; ++k) { const int x0 = std::min(k, 14); lines.push_back({std::min(k, 28 - k) + 1, x0, k - x0, 3}); }
    std::stable_sort(lines.begin(), lines.end(), [](const LineJob& a, const LineJob& b) { return a.len > b.len; });
    if (lines.size() != 64 + kPairedLanes) { gmk::set_error("lane lines: %zu lines for 64 lanes and %d second lines", lines.size(), kPairedLanes); return GMK_ERR_STATE; }
    auto line_word = [](const LineJob& l) { return l.dir == 0 ? l.y0 : l.dir == 1 ? kColBase + l.x0 : l.dir == 2 ? kDiagBase + l.x0 - l.y0 + 14 : kAntiBase + l.x0 + l.y0; };
    auto stride_of = [](int dir) { return dir == 0 ? 1 : dir == 1 ? 15 : dir == 2 ? 16 : 14; };
    auto first_cell = [](const LineJob& l) { return l.y0 * 15 + l.x0; };
    // The eight leftovers ride behind the eight shortest primaries, each behind a line of its OWN direction (the sort is stable: of every length the
    // two diagonals stand in front of the two anti-diagonals): the 5-cell lines 68..71 behind the 8-cell lines of lanes 56..59, the 6-cell lines 64..67
    // behind the 7-cell lines of lanes 60..63.  8 + 2 + 5 + 2 = 7 + 2 + 6 + 2 = 17 symbols.
    auto second_line = [](int lane) { return lane < kFirstPairedLane ? -1 : lane < kFirstPairedLane + 4 ? lane + 12 : lane + 4; };
    uint32_t lines_words[64], place_words[64];
    int steps = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const LineJob& a = lines[lane];
        const LineJob* b = second_line(lane) < 0 ? nullptr : &lines[second_line(lane)];
        if (a.len < kScanPrefixSyms) { gmk::set_error("lane lines: lane %d starts with a line of %d cells, the scan's prefix read takes %d", lane, a.len, kScanPrefixSyms); return GMK_ERR_STATE; }
        if (b && b->dir != a.dir) { gmk::set_error("lane lines: lane %d walks lines of directions %d and %d", lane, a.dir, b->dir); return GMK_ERR_STATE; }
        const int seg_a = a.len + kSegPads, seg_b = b ? b->len + kSegPads : kSegPads, stride = stride_of(a.dir);
        // (where the kernel adds the jump is fixed in its text: place_jump's lanes and steps)
        if (b && seg_a != (lane < kFirstPairedLane + 4 ? kSeamStepLong : kSeamStepShort)) { gmk::set_error("lane lines: lane %d steps to its second line at step %d", lane, seg_a); return GMK_ERR_STATE; }
        const int jump = b ? first_cell(*b) - (first_cell(a) + seg_a * stride) : 0;
        if (jump < -512 || jump > 511) { gmk::set_error("lane lines: lane %d jumps %d cells", lane, jump); return GMK_ERR_STATE; }
        // "no line": length 0 (two pads) on line word 15, which stays zero
        lines_words[lane] = static_cast<uint32_t>(seg_a | seg_b << 5 | line_word(a) << 10 | (b ? line_word(*b) : 15) << 17 | stride << 24);
        place_words[lane] = static_cast<uint32_t>(first_cell(a) + kScanPrefixSyms * stride) | static_cast<uint32_t>(a.dir) << 9 | (static_cast<uint32_t>(-stride) & 63u) << 11
                            | (static_cast<uint32_t>(jump) & 1023u) << 17;
        steps = std::max(steps, seg_a + (b ? seg_b : 0));
        // The two words against the plain statement, every step the scan pushes: which segment, the place on its line, first cell + place * stride,
        // direction and stride -- what phase 2 used to work out from (lane, step) -- against the kernel's arithmetic on the packed word.  (A lane with one
        // line goes on along it behind its pads: the stream's filler, which reports nothing.)
        uint32_t place = place_words[lane];
        const int jump_field = static_cast<int>(place_words[lane] << 5) >> 22;                       // v_bfe_i32 17, 10
        for (int step = kScanPrefixSyms; step < kScanSteps; ++step) {
            if (step > kScanPrefixSyms) place += lines_words[lane] >> 24;
            if (step == kSeamStepShort && lane >= kFirstPairedLane + 4) place += static_cast<uint32_t>(jump_field);
            if (step == kSeamStepLong && lane >= kFirstPairedLane && lane < kFirstPairedLane + 4) place += static_cast<uint32_t>(jump_field);
            const bool second = b && step >= seg_a;
            const LineJob& l = second ? *b : a;
            const int cell = first_cell(l) + (step - (second ? seg_a : 0)) * stride_of(l.dir);
            const uint32_t want = static_cast<uint32_t>(cell) | static_cast<uint32_t>(l.dir) << 9 | (static_cast<uint32_t>(-stride_of(l.dir)) & 63u) << 11;
            if (cell < 0 || cell > 511 || (place & 0x1FFFFu) != want) {
                gmk::set_error("lane lines: lane %d step %d carries place 0x%05x, the plain statement gives 0x%05x", lane, step, place & 0x1FFFFu, want);
                return GMK_ERR_STATE;
            }
        }
    }
    uint32_t init[kLineWords] = {};                              // every cell of every line blank (symbol 3)
    for (int i = 0; i < 15; ++i) init[i] = init[kColBase + i] = 0x3FFFFFFFu;
    // (a diagonal's cells sit at bits 2 x, an anti-diagonal's at bits 2 y: the line starts at x = max(0, x - y) resp. y = max(0, x + y - 14))
    for (int d = 0; d <= 28; ++d) init[kDiagBase + d] = init[kAntiBase + d] = ((1u << (2 * (15 - std::abs(d - 14)))) - 1u) << (2 * std::max(0, d - 14));
    uint32_t consts[64][4];
    for (int lane = 0; lane < 64; ++lane) {
        uint32_t row4 = 0, col = 0;
        for (int pass = 0; pass < 4; ++pass) {
            const int c = std::min(64 * pass + lane, kCells - 1);
            // (behind the last cell: the gate word of lane 16, which holds no row and is zero on every board -- the 16 bytes such a lane writes
            // are zeros on the first counter words, which are zero there: phase 0's fourth score-block write needs no lane mask)
            if (64 * pass + lane >= kCells) { row4 |= static_cast<uint32_t>(4 * 16) << (8 * pass); continue; }
            row4 |= static_cast<uint32_t>(4 * (c / 15)) << (8 * pass);
            col |= static_cast<uint32_t>(c % 15) << (8 * pass);
        }
        consts[lane][0] = row4;
        consts[lane][1] = col;
        for (int k = 0; k < 2; ++k) {
            const int at = k == 0 ? lane : second_line(lane);
            consts[lane][2 + k] = at < 0 ? 0u : lines[at].dir == 2 ? 2u * static_cast<uint32_t>(lines[at].x0) : lines[at].dir == 3 ? 2u * static_cast<uint32_t>(lines[at].y0) : 0u;
        }
    }
    for (int i = 0; i < kLineWords; ++i) pads_out[i] = ~init[i] & 0xAAAAAAAAu;
    for (int lane = 0; lane < 64; ++lane) {
        uint32_t* r = records_out + 8 * lane;
        r[0] = lines_words[lane]; r[1] = place_words[lane];
        r[2] = init[lane]; r[3] = init[std::min(64 + lane, kLineWords - 1)];
        for (int k = 0; k < 4; ++k) r[4 + k] = consts[lane][k];
    }
    if (steps != kScanSteps) { gmk::set_error("lane lines: %d scan steps, the kernel is built for %d", steps, kScanSteps); return GMK_ERR_STATE; }
    return GMK_OK;
}

// The weight table of phase D (kWtab*): [plane kind: count, weight][dy + 6][xo] x 16 bytes, byte j = the tap from column j of a row
// dy below the cell's to a cell in column xo: BlockWeights (Pattern.cpp:598-609) at (dy, j - xo), its non-zero mask for the count planes.
int density_weights(int8_t* t /* kWtabWords * 4 bytes, zeroed */) {
    for (int kind = 0; kind < 2; ++kind)
        for (int dy = -3; dy <= 3; ++dy)
            for (int xo = 0; xo < 15; ++xo)
                for (int j = 0; j < 15; ++j) {
                    if (std::abs(j - xo) > 3) continue;
                    const int w = block_weight(dy, j - xo);
                    t[((static_cast<size_t>(kind) * kWtabDy + dy + 6) * 15 + xo) * 16 + j] = static_cast<int8_t>(kind == 0 ? (w != 0) : w);
                }
    // every row offset a lane can ask for lies inside the table: dy = 2 kt + h - yo for the K tiles its M tile visits
    for (int cell = 0; cell < 224; ++cell)
        for (int kt = dens_kt_lo(cell / 32); kt <= dens_kt_hi(cell / 32); ++kt)
            for (int h = 0; h < 2; ++h) {
                const int dy = 2 * kt + h - cell / 15;
                if (dy < -6 || dy > 6) { gmk::set_error("density weight table: dy %d of cell %d out of range", dy, cell); return GMK_ERR_STATE; }
            }
    // ... and every tap of every cell lies in one of the K tiles its M tile visits
    for (int cell = 0; cell < 224; ++cell)
        for (int dy = -3; dy <= 3; ++dy) {
            const int y = cell / 15 + dy, m = cell / 32;
            if (y < 0 || y > 14) continue;
            if (y / 2 < dens_kt_lo(m) || y / 2 > dens_kt_hi(m)) { gmk::set_error("density weight table: row %d of cell %d is not covered", y, cell); return GMK_ERR_STATE; }
        }
    return GMK_OK;
}

// Where the scan starts and what lets a lane's stream do without leading pads (phase 1): the root on '?' emits nothing and goes to a state S;
// S on '?' stays in S and emits nothing; from EVERY state "??" leads to S.  So a segment "cells ? ?" walked from S reports what "? cells ? ?"
// reports from the root, and leaves the automaton in S for the lane's second segment.  row_out: the row offset of S, the table word the scan
// starts from.  A table without these properties is an error, not a slower path.
int scan_start_row(const gmk::DeviceTables& t, uint32_t* row_out) {
    constexpr uint32_t kPad = 2;                                  // '?' in the device's symbol codes
    const std::vector<uint32_t>& tr = t.dev_trans;
    const uint32_t n = static_cast<uint32_t>(t.n_states);
    if (n == 0 || tr.size() != static_cast<size_t>(n) * 4) { gmk::set_error("K1 scan: no automaton"); return GMK_ERR_STATE; }
    const uint32_t first = tr[kPad], start = gmk::dev_trans_row(first);
    if (gmk::dev_trans_record(first) != 0 || start % 16 != 0 || start / 16 >= n) { gmk::set_error("K1 scan: the root emits on '?' or leaves the table"); return GMK_ERR_STATE; }
    const uint32_t loop = tr[start / 4 + kPad];
    if (gmk::dev_trans_record(loop) != 0 || gmk::dev_trans_row(loop) != start) { gmk::set_error("K1 scan: state %u does not loop on '?' without emitting", start / 16); return GMK_ERR_STATE; }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t mid = gmk::dev_trans_row(tr[s * 4 + kPad]);
        if (mid % 16 != 0 || mid / 16 >= n || gmk::dev_trans_row(tr[mid / 4 + kPad]) != start) { gmk::set_error("K1 scan: \"??\" from state %u does not lead to state %u", s, start / 16); return GMK_ERR_STATE; }
    }
    *row_out = start;
    return GMK_OK;
}

// The scan's prefix table: entry s0 | s1 << 2 | s2 << 4 | s3 << 6 is the row offset S (`start`, from scan_start_row) reaches over those four symbols.
// The scan reads it in place of its first four lookups and queues nothing for them, which is right only if none of the 3^4 walks over four CELL
// symbols (black 0, white 1, blank 3: a lane's first four symbols are cells, lane_tables) reports anything on any of its transitions.  With the
// production table none does, and 24 of the 243 walks over five cells do: four is the limit (tests/test_eval_scan_prefix.py).  A table where a walk
// over four does report is an error, not a slower path.
// (The root's table, DeviceTables::dev_prefix4, cannot serve: S is not the root, and 30 of the 256 keys end elsewhere from it.)
int scan_prefix_table(const gmk::DeviceTables& t, uint32_t start, uint16_t* out /* 256 entries */) {
    const std::vector<uint32_t>& tr = t.dev_trans;
    for (uint32_t key = 0; key < 256; ++key) {
        uint32_t row = start;
        bool cells = true, reports = false;
        for (int i = 0; i < kScanPrefixSyms; ++i) {
            const uint32_t sym = (key >> (2 * i)) & 3u;
            if (row % 16 != 0 || row / 4 + sym >= tr.size()) { gmk::set_error("K1 scan prefix: a walk from state %u leaves the table", start / 16); return GMK_ERR_STATE; }
            const uint32_t tw = tr[row / 4 + sym];
            cells = cells && sym != 2u;
            reports = reports || gmk::dev_trans_record(tw) != 0;
            row = gmk::dev_trans_row(tw);
        }
        if (cells && reports) { gmk::set_error("K1 scan prefix: the cells of key 0x%02x report a match within four symbols of state %u", key, start / 16); return GMK_ERR_STATE; }
        out[key] = static_cast<uint16_t>(row);
    }
    return GMK_OK;
}

// The image of the kernel's tables (see kLaneRecordVecs): [automaton][records][pads][bits-to-bytes 512][weights][scan prefix 128][root prefix 128][hand-out 4], then the lane
// records.  Built once; the automaton and the records are copied from the device state's tables.
int build_stage_image(const gmk::DeviceState& st, uint4** d_out, int* stage_vecs) {
    const size_t trans_words = static_cast<size_t>(st.n_states) * 4, record_words = static_cast<size_t>(st.n_records) * 4;
    std::vector<uint32_t> rest(kStaticTableWords + 64 * 4 * kLaneRecordVecs, 0u);
    uint32_t* pads = rest.data(), *lut = pads + kLineWords, *wtab = lut + 512, *scan_prefix = wtab + kWtabWords, *root_prefix = scan_prefix + kPrefixTableWords,
              *handout = root_prefix + kPrefixTableWords, *records = handout + 4;
    int rc = lane_tables(pads, records);
    if (rc != GMK_OK) return rc;
    for (uint32_t b = 0; b < 256; ++b) { lut[2 * b] = ((b & 15u) * 0x204081u) & 0x01010101u; lut[2 * b + 1] = ((b >> 4) * 0x204081u) & 0x01010101u; }
    rc = density_weights(reinterpret_cast<int8_t*>(wtab));
    if (rc != GMK_OK) return rc;
    handout[0] = 2u * kBoardsPerBlock;
    const gmk::DeviceTables& tables = gmk::production_automaton().device();
    rc = scan_start_row(tables, &handout[1]);
    if (rc != GMK_OK) return rc;
    // the two prefix tables, 256 entries of 16 bits each, two entries to a word: the scan's from S, the rescans' from the root
    uint16_t halves[256];
    rc = scan_prefix_table(tables, handout[1], halves);
    if (rc != GMK_OK) return rc;
    if (tables.dev_prefix4.size() != 256) { gmk::set_error("K1 tables: no four-symbol prefix table of the root"); return GMK_ERR_STATE; }
    for (int i = 0; i < kPrefixTableWords; ++i) {
        scan_prefix[i] = static_cast<uint32_t>(halves[2 * i]) | static_cast<uint32_t>(halves[2 * i + 1]) << 16;
        root_prefix[i] = static_cast<uint32_t>(tables.dev_prefix4[2 * i]) | static_cast<uint32_t>(tables.dev_prefix4[2 * i + 1]) << 16;
    }
    const size_t staged_words = trans_words + record_words + kStaticTableWords;
    if (staged_words % 4 != 0) { gmk::set_error("K1 tables: %zu staged words are not whole 16-byte pieces", staged_words); return GMK_ERR_STATE; }
    uint32_t* d = nullptr;
    GMK_HIP_CHECK(hipMalloc(&d, (trans_words + record_words + rest.size()) * sizeof(uint32_t)));
    GMK_HIP_CHECK(hipMemcpy(d, st.d_trans, trans_words * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    GMK_HIP_CHECK(hipMemcpy(d + trans_words, st.d_records, record_words * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    GMK_HIP_CHECK(hipMemcpy(d + trans_words + record_words, rest.data(), rest.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    *d_out = reinterpret_cast<uint4*>(d);
    *stage_vecs = static_cast<int>(staged_words / 4);
    return GMK_OK;
}

struct Launch { int grid, n_groups, groups_each, groups_extra; size_t lds; };

Launch plan_launch(int n, const gmk::DeviceState& st) {
    Launch l;
    l.n_groups = (n + kGroupBoards - 1) / kGroupBoards;
    l.grid = std::max(1, std::min(l.n_groups, st.cu_count * kMaxBlocksPerCu));
    l.groups_each = l.n_groups / l.grid;                      // a workgroup's run: groups_each groups, one more in the first groups_extra workgroups
    l.groups_extra = l.n_groups % l.grid;
    l.lds = static_cast<size_t>(kBoardsPerBlock * kBoardWords + st.n_states * 4 + st.n_records * 4 + kStaticTableWords) * 4;
    return l;
}

bool g_jobs_uploaded = false;
uint4* g_stage = nullptr;
int g_stage_vecs = 0;
}  // namespace

extern "C" int gmk_eval_batch(const uint16_t* d_planes, int n, int32_t* d_scores, int32_t* d_density,
                              uint32_t* d_totals, int32_t* d_status, void* stream) {
    gmk::DeviceState& st = gmk::device_state();
    GMK_NEED_INIT();
    if (n < 0 || (n > 0 && !d_planes)) { gmk::set_error("gmk_eval_batch: bad arguments"); return GMK_ERR_ARG; }
    if (n == 0) return GMK_OK;
    if (!g_jobs_uploaded) {
        const int rc = build_stage_image(st, &g_stage, &g_stage_vecs);
        if (rc != GMK_OK) return rc;
        GMK_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(eval_positions_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        g_jobs_uploaded = true;
    }
    const Launch l = plan_launch(n, st);
    if (l.lds > 160u * 1024u) { gmk::set_error("gmk_eval_batch: tables do not fit in LDS (%zu bytes)", l.lds); return GMK_ERR_CAPACITY; }
    static const int phase_mask = gmk::profile_env("GMK_EVAL_PHASE_MASK") ? std::atoi(gmk::profile_env("GMK_EVAL_PHASE_MASK")) : 0x7F;
    unsigned long long* d_prof = nullptr;
    static const bool stamps = gmk::profile_env("GMK_EVAL_PROFILE") != nullptr;
    if (stamps) {
        GMK_HIP_CHECK(hipMalloc(&d_prof, 16 * sizeof(unsigned long long)));
        GMK_HIP_CHECK(hipMemset(d_prof, 0, 16 * sizeof(unsigned long long)));
    }
    // (profile build only) GMK_EVAL_TIMELINE=<file>: every launch leaves its wavefronts' clock values there (tools/k1_timeline.py reads them)
    static const char* const timeline_path = gmk::profile_env("GMK_EVAL_TIMELINE");
    unsigned long long* d_timeline = nullptr;
    const size_t timeline_words = static_cast<size_t>(l.grid) * kBoardsPerBlock * kTimelineSlots;
    hipEvent_t tl_from = nullptr, tl_to = nullptr;
    if (timeline_path) {
        GMK_HIP_CHECK(hipMalloc(&d_timeline, timeline_words * sizeof(unsigned long long)));
        GMK_HIP_CHECK(hipMemset(d_timeline, 0, timeline_words * sizeof(unsigned long long)));
        GMK_HIP_CHECK(hipEventCreate(&tl_from));
        GMK_HIP_CHECK(hipEventCreate(&tl_to));
        GMK_HIP_CHECK(hipDeviceSynchronize());
        GMK_HIP_CHECK(hipEventRecord(tl_from, static_cast<hipStream_t>(stream)));
    }
    hipLaunchKernelGGL(eval_positions_kernel, dim3(l.grid), dim3(kThreads), l.lds, static_cast<hipStream_t>(stream),
                       d_planes, n, l.groups_each, l.groups_extra, d_scores, d_density, d_totals, d_status,
                       g_stage, g_stage_vecs, st.n_states * 4, st.n_records * 4, phase_mask, d_prof, d_timeline);
    GMK_HIP_CHECK(hipGetLastError());
    if (timeline_path) {
        // the file: grid, wavefronts per workgroup, slots per wavefront, the launch's time between two events in nanoseconds; then the slots
        GMK_HIP_CHECK(hipEventRecord(tl_to, static_cast<hipStream_t>(stream)));
        GMK_HIP_CHECK(hipEventSynchronize(tl_to));
        float wall_ms = 0.f;
        GMK_HIP_CHECK(hipEventElapsedTime(&wall_ms, tl_from, tl_to));
        std::vector<unsigned long long> h(4 + timeline_words);
        h[0] = static_cast<unsigned long long>(l.grid); h[1] = kBoardsPerBlock; h[2] = kTimelineSlots; h[3] = static_cast<unsigned long long>(wall_ms * 1e6);
        GMK_HIP_CHECK(hipMemcpy(h.data() + 4, d_timeline, timeline_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        (void)hipFree(d_timeline); (void)hipEventDestroy(tl_from); (void)hipEventDestroy(tl_to);
        if (std::FILE* f = std::fopen(timeline_path, "wb")) { std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f); std::fclose(f); }
    }
    if (stamps) {                                               // (profile build only) cycles per phase and board, mean over the wavefronts
        unsigned long long h[16];
        GMK_HIP_CHECK(hipDeviceSynchronize());
        GMK_HIP_CHECK(hipMemcpy(h, d_prof, sizeof h, hipMemcpyDeviceToHost));
        (void)hipFree(d_prof);
        const char* names[12] = {"staging", "phase0", "scan", "deposits", "phase3", "phase3b", "rescans", "wait-planes", "phaseD", "phase5", "-", "loop-head"};
        const double boards = static_cast<double>(n), waves = static_cast<double>(h[15] ? h[15] : 1);
        double total = 0;
        for (int k = 0; k < 12; ++k) total += static_cast<double>(h[k]);
        std::fprintf(stderr, "[GMK_EVAL_PROFILE] s_memtime cycles per board (wavefront time; %.0f wavefronts, %.0f cycles each):", waves, total / waves);
        for (int k = 0; k < 12; ++k) if (k != 10) std::fprintf(stderr, " %s %.0f", names[k], static_cast<double>(h[k]) / boards);
        std::fprintf(stderr, "\n");
    }
    return GMK_OK;
}

extern "C" int gmk_eval_launch_info(int n, int* grid, int* block, int* lds_bytes) {
    gmk::DeviceState& st = gmk::device_state();
    if (!st.ready) { gmk::set_error("gmk_init has not succeeded"); return GMK_ERR_STATE; }
    const Launch l = plan_launch(std::max(n, 1), st);
    if (grid) *grid = l.grid;
    if (block) *block = kThreads;
    if (lds_bytes) *lds_bytes = static_cast<int>(l.lds);
    return GMK_OK;
}

extern "C" int gmk_eval_lane_records(uint32_t* records) {
    if (!records) { gmk::set_error("gmk_eval_lane_records: bad arguments"); return GMK_ERR_ARG; }
    uint32_t pads[kLineWords];
    return lane_tables(pads, records);
}

extern "C" int gmk_eval_batch_host(const uint16_t* h_planes, int n, int32_t* h_scores, int32_t* h_density,
                                   uint32_t* h_totals, int32_t* h_status) {
    GMK_NEED_INIT();
    if (n < 0 || (n > 0 && !h_planes)) { gmk::set_error("gmk_eval_batch_host: bad arguments"); return GMK_ERR_ARG; }
    if (n == 0) return GMK_OK;
    // one block, planes | scores | density | totals | status, from the driver and back to it: the library's pool does not keep it.  The kernel
    // writes every output, asked for or not.
    const size_t nb = static_cast<size_t>(n);
    gmk::Staging st("gmk_eval_batch_host", 0, false);
    uint16_t* d_planes;
    int32_t *d_scores, *d_density, *d_status;
    uint32_t* d_totals;
    st.in(d_planes, h_planes, nb * 32);
    st.out(d_scores, h_scores, nb * 900, true); st.out(d_density, h_density, nb * 900, true); st.out(d_totals, h_totals, nb * 11, true);
    st.out(d_status, h_status, nb, true);
    int rc = st.take();
    if (rc == GMK_OK) rc = gmk_eval_batch(d_planes, n, d_scores, d_density, d_totals, d_status, nullptr);
    if (rc != GMK_OK) return rc;
    GMK_STAGED(st, hipDeviceSynchronize());
    return st.download();
}
