// host_staging_check.cpp -- the layout of the staging block (the plain-C++ part of gomokuai_amd/csrc/host_staging.h) as a stand-alone program, for
// a run under the address and undefined-behaviour sanitizers on a machine without a GPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/host_staging_check.cpp -o tools/bin/host_staging_check && tools/bin/host_staging_check
// It checks alignment, that parts neither overlap nor leave the block, absent and empty parts, the refusal of a size that overflows, and that the
// five batch host forms get the offsets their hand-written chains gave them before they moved onto the block.  Exits non-zero on the first
// thing that is wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define GMK_STAGING_LAYOUT_ONLY
#include "../gomokuai_amd/csrc/host_staging.h"

using gmk::StagePart;

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "host_staging_check: %s failed (line %d)\n", #cond, __LINE__); return 1; } } while (0)

static size_t up16(size_t b) { return (b + 15) & ~size_t(15); }

// Lays the parts out, then holds the layout to its rules on a real block: every present part is written end to end (the sanitizer sees a
// byte outside the block) with its own index, and read back (an overlap would have changed it).
static int laid_out(std::vector<StagePart>& parts, size_t* total) {
    REQUIRE(gmk::stage_layout(parts.data(), parts.size(), total));
    REQUIRE(*total % 16 == 0);
    std::vector<char> block(*total);
    char* last = nullptr;
    for (size_t i = 0; i < parts.size(); ++i) {
        char* p = gmk::stage_pointer(block.data(), parts[i]);
        if (!parts[i].present) { REQUIRE(p == nullptr); continue; }
        REQUIRE(p != nullptr && parts[i].offset % 16 == 0);
        REQUIRE(last == nullptr || p > last);                           // distinct, in order
        const size_t bytes = parts[i].count * parts[i].size;
        REQUIRE(parts[i].offset + (bytes ? bytes : 1) <= *total);
        std::memset(p, static_cast<int>(i + 1), bytes);
        last = p + (bytes ? bytes - 1 : 0);
    }
    for (size_t i = 0; i < parts.size(); ++i)
        if (parts[i].present)
            for (size_t b = 0; b < parts[i].count * parts[i].size; ++b) REQUIRE(block[parts[i].offset + b] == static_cast<char>(i + 1));
    return 0;
}

// The parts of a batch host form: the move lists, the lengths, then the outputs as (count, element bytes).
static std::vector<StagePart> form(size_t n, size_t stride, std::initializer_list<StagePart> outputs) {
    std::vector<StagePart> parts{{n * stride, 1, true, 0}, {n, 4, true, 0}};
    parts.insert(parts.end(), outputs);
    return parts;
}

int main() {
    size_t total = 0;
    // ---- absent parts, empty parts ----
    {
        std::vector<StagePart> parts{{3, 1, true, 0}, {5, 4, false, 0}, {0, 4, true, 0}, {0, 8, true, 0}, {7, 2, false, 0}, {1, 1, true, 0}};
        REQUIRE(laid_out(parts, &total) == 0);
        REQUIRE(total == 64);                                           // 3 -> 16, absent, empty -> 16, empty -> 16, absent, 1 -> 16
        REQUIRE(parts[2].offset == 16 && parts[3].offset == 32 && parts[5].offset == 48);
        std::vector<StagePart> without{{3, 1, true, 0}, {0, 4, true, 0}, {0, 8, true, 0}, {1, 1, true, 0}};
        size_t same = 0;
        REQUIRE(laid_out(without, &same) == 0 && same == total);        // an absent part takes no bytes
        std::vector<StagePart> none{{9, 4, false, 0}};
        REQUIRE(laid_out(none, &total) == 0 && total == 0);
    }
    // ---- sizes that do not fit ----
    {
        StagePart big[2] = {{SIZE_MAX / 4 + 1, 4, true, 0}, {1, 1, true, 0}};
        REQUIRE(!gmk::stage_layout(big, 2, &total));                    // count * size wraps
        StagePart sum[2] = {{SIZE_MAX - 40, 1, true, 0}, {64, 1, true, 0}};
        REQUIRE(!gmk::stage_layout(sum, 2, &total));                    // the second part passes the end
        StagePart pad[1] = {{SIZE_MAX - 7, 1, true, 0}};
        REQUIRE(!gmk::stage_layout(pad, 1, &total));                    // the rounding up wraps
        StagePart absent[2] = {{SIZE_MAX, 8, false, 0}, {4, 4, true, 0}};
        REQUIRE(gmk::stage_layout(absent, 2, &total) && total == 16);   // what is absent is not counted
        StagePart fits[1] = {{SIZE_MAX - 15, 1, true, 0}};
        REQUIRE(gmk::stage_layout(fits, 1, &total) && total == SIZE_MAX - 15);
    }
    // ---- the five batch host forms: the chains as the entries spelled them out before, every output present ----
    const size_t kVcfPv = 64, kVctPv = 80, kCells = 225;                // GMK_VCF_PV, GMK_VCT_PV
    for (size_t n : {size_t(1), size_t(3), size_t(5)})
        for (size_t stride : {size_t(1), size_t(7), size_t(225)}) {
            const size_t un = n, cells = un * 225;
            {   // gmk_vcf_solve_host: moves | lens | status | move | length | nodes | pv
                const size_t o_lens = up16(un * stride), o_status = o_lens + up16(un * 4), o_move = o_status + up16(un * 4), o_length = o_move + up16(un * 4),
                             o_nodes = o_length + up16(un * 4), o_pv = o_nodes + up16(un * 4), want = o_pv + up16(un * kVcfPv);
                std::vector<StagePart> p = form(n, stride, {{un, 4, true, 0}, {un, 4, true, 0}, {un, 4, true, 0}, {un, 4, true, 0}, {un * kVcfPv, 1, true, 0}});
                REQUIRE(laid_out(p, &total) == 0 && total == want);
                const size_t chain[] = {0, o_lens, o_status, o_move, o_length, o_nodes, o_pv};
                for (size_t i = 0; i < p.size(); ++i) REQUIRE(p[i].offset == chain[i]);
            }
            {   // gmk_vcf_defend_host: moves | lens | threat status | length | nodes | pv | verdict | cell length | cell nodes
                const size_t o_lens = up16(un * stride), o_status = o_lens + up16(un * 4), o_length = o_status + up16(un * 4), o_nodes = o_length + up16(un * 4),
                             o_pv = o_nodes + up16(un * 4), o_verdict = o_pv + up16(un * kVcfPv), o_cell_length = o_verdict + up16(cells),
                             o_cell_nodes = o_cell_length + up16(cells), want = o_cell_nodes + up16(cells * 4);
                std::vector<StagePart> p = form(n, stride, {{un, 4, true, 0}, {un, 4, true, 0}, {un, 4, true, 0}, {un * kVcfPv, 1, true, 0}, {cells, 1, true, 0},
                                                            {cells, 1, true, 0}, {cells, 4, true, 0}});
                REQUIRE(laid_out(p, &total) == 0 && total == want);
                const size_t chain[] = {0, o_lens, o_status, o_length, o_nodes, o_pv, o_verdict, o_cell_length, o_cell_nodes};
                for (size_t i = 0; i < p.size(); ++i) REQUIRE(p[i].offset == chain[i]);
            }
            {   // gmk_vcf_threats_host: moves | lens | own status | move | length | nodes | pv | verdict | cell length | cell nodes
                const size_t o_lens = up16(un * stride), o_status = o_lens + up16(un * 4), o_move = o_status + up16(un * 4), o_length = o_move + up16(un * 4),
                             o_nodes = o_length + up16(un * 4), o_pv = o_nodes + up16(un * 4), o_verdict = o_pv + up16(un * kVcfPv),
                             o_cell_length = o_verdict + up16(cells), o_cell_nodes = o_cell_length + up16(cells), want = o_cell_nodes + up16(cells * 4);
                std::vector<StagePart> p = form(n, stride, {{un, 4, true, 0}, {un, 4, true, 0}, {un, 4, true, 0}, {un, 4, true, 0}, {un * kVcfPv, 1, true, 0},
                                                            {cells, 1, true, 0}, {cells, 1, true, 0}, {cells, 4, true, 0}});
                REQUIRE(laid_out(p, &total) == 0 && total == want);
                const size_t chain[] = {0, o_lens, o_status, o_move, o_length, o_nodes, o_pv, o_verdict, o_cell_length, o_cell_nodes};
                for (size_t i = 0; i < p.size(); ++i) REQUIRE(p[i].offset == chain[i]);
            }
            {   // gmk_vct_solve_host: moves | lens | status | move | threats | positions | pv
                const size_t o_lens = up16(un * stride), o_status = o_lens + up16(un * 4), o_move = o_status + up16(un * 4), o_threats = o_move + up16(un * 4),
                             o_positions = o_threats + up16(un * 4), o_pv = o_positions + up16(un * 4), want = o_pv + up16(un * kVctPv);
                std::vector<StagePart> p = form(n, stride, {{un, 4, true, 0}, {un, 4, true, 0}, {un, 4, true, 0}, {un, 4, true, 0}, {un * kVctPv, 1, true, 0}});
                REQUIRE(laid_out(p, &total) == 0 && total == want);
                const size_t chain[] = {0, o_lens, o_status, o_move, o_threats, o_positions, o_pv};
                for (size_t i = 0; i < p.size(); ++i) REQUIRE(p[i].offset == chain[i]);
            }
            {   // gmk_pattern_policy_host: moves | lens | probs | value | best | status (the block itself is asked for at 16 MB at least)
                const size_t o_lens = up16(un * stride), o_probs = o_lens + up16(un * 4), o_value = o_probs + up16(un * kCells * 4), o_best = o_value + up16(un * 4),
                             o_status = o_best + up16(un * 4), want = o_status + up16(un * 4);
                std::vector<StagePart> p = form(n, stride, {{un * kCells, 4, true, 0}, {un, 4, true, 0}, {un, 4, true, 0}, {un, 4, true, 0}});
                REQUIRE(laid_out(p, &total) == 0 && total == want);
                const size_t chain[] = {0, o_lens, o_probs, o_value, o_best, o_status};
                for (size_t i = 0; i < p.size(); ++i) REQUIRE(p[i].offset == chain[i]);
                // an optional output that is NULL: the parts behind it move up, nothing else changes
                p[3].present = false;
                REQUIRE(laid_out(p, &total) == 0 && total == want - up16(un * 4) && p[4].offset == o_value && p[5].offset == o_best);
            }
        }
    std::printf("host_staging_check: ok\n");
    return 0;
}
