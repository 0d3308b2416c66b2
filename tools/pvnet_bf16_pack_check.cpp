// pvnet_bf16_pack_check.cpp -- the host side of "K9 in bf16" (gomokuai_amd/csrc/pvnet_bf16_pack.h on top of pvnet_pack.h) as a stand-alone
// program, for a run under the address and undefined-behaviour sanitizers on a machine without a GPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/pvnet_bf16_pack_check.cpp -o tools/bin/pvnet_bf16_pack_check && tools/bin/pvnet_bf16_pack_check
// It packs float32 buffers exactly as gmk_pvnet_create does, derives the bf16 buffer from them as gmk_pvnet_set_precision does, and checks
// every element against the layout stated from the weights directly (which tap, channel and row a lane's element is), that every source index
// stays inside its buffer, and the rounding on its edge cases.  Exits non-zero on the first thing that is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gomokuai_amd/csrc/pvnet_pack.h"
#include "../gomokuai_amd/csrc/pvnet_bf16_pack.h"

namespace Q = gmk::bf16pack;

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "pvnet_bf16_pack_check: %s failed (line %d)\n", #cond, __LINE__); return 1; } } while (0)

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

int main() {
    // ---- the rounding ----
    REQUIRE(Q::rne(1.0f) == 0x3F80 && Q::rne(-2.0f) == 0xC000 && Q::rne(0.0f) == 0 && Q::rne(-0.0f) == 0x8000);
    REQUIRE(Q::rne(from_bits(0x3F808000)) == 0x3F80 && Q::rne(from_bits(0x3F818000)) == 0x3F82);        // ties go to even
    REQUIRE(Q::rne(from_bits(0x3F807FFF)) == 0x3F80 && Q::rne(from_bits(0x3F808001)) == 0x3F81);
    REQUIRE(Q::rne(from_bits(0x7F7F7FFF)) == 0x7F7F && Q::rne(from_bits(0x7F7F8000)) == 0x7F80 && Q::rne(from_bits(0xFF7FFFFF)) == 0xFF80);
    REQUIRE(Q::rne(from_bits(0x7F800000)) == 0x7F80 && Q::rne(from_bits(0xFF800000)) == 0xFF80);
    REQUIRE(Q::rne(from_bits(0x7F800001)) == 0x7FC0 && Q::rne(from_bits(0xFFFFFFFF)) == 0x7FC0 && Q::rne(from_bits(0x7FC00000)) == 0x7FC0);
    REQUIRE(Q::rne(from_bits(0x00008000)) == 0x0000 && Q::rne(from_bits(0x00008001)) == 0x0001 && Q::rne(from_bits(0x00018000)) == 0x0002);
    for (uint32_t b = 0; b < 0x10000u; ++b) {                                 // every bf16 is its own rounding (NaNs go to the one quiet NaN)
        const bool nan = (b & 0x7FFFu) > 0x7F80u;
        REQUIRE(Q::rne_bits(b << 16) == (nan ? 0x7FC0u : b));
        if (!nan) REQUIRE(Q::rne(Q::widen(static_cast<uint16_t>(b))) == b);
    }

    // ---- the layout: weights that are all different and all exact in bf16 within a tensor's reach are not possible (73 728 of them), so
    //      the check compares against the rounding of the weight the layout names ----
    std::vector<float> w1(32 * 6 * 9), w2(64 * 32 * 9), w3(128 * 64 * 9), wp(4 * 128), wv(2 * 128);
    uint32_t s = 12345u;
    auto fill = [&](std::vector<float>& v) { for (float& x : v) { s = s * 1664525u + 1013904223u; x = (static_cast<float>(s >> 8) - 8388608.0f) * 1.1920929e-7f; } };
    fill(w1); fill(w2); fill(w3); fill(wp); fill(wv);
    std::vector<float> p1, p2, p3, ph;
    gmk::pvpack::pack_layer(w1.data(), 6, 32, p1);
    gmk::pvpack::pack_layer(w2.data(), 32, 64, p2);
    gmk::pvpack::pack_layer(w3.data(), 64, 128, p3);
    gmk::pvpack::pack_heads(wp.data(), wv.data(), ph);
    REQUIRE(ph.size() == static_cast<size_t>(gmk::pvpack::kHeadFloats));
    REQUIRE(p1.size() == 9 * 256 && p2.size() == 77 * 256 && p3.size() == 293 * 256);      // what gmk_pvnet_set_precision reads back
    const size_t sizes[4] = {p1.size(), p2.size(), p3.size(), ph.size()};
    for (int i = 0; i < Q::kElements; ++i) {
        int b = -1;
        const int at = Q::source(i, b);
        REQUIRE(b >= 0 && b < 4 && at >= -1 && (at < 0 || static_cast<size_t>(at) < sizes[b]));
    }
    // exactly sized copies, so that a read past a buffer's end is the sanitizer's to see
    std::vector<uint16_t> q(Q::kElements, 0xFFFF);
    Q::pack(p1.data(), p2.data(), p3.data(), ph.data(), q.data());
    auto frag = [&](int seg, int step, int lane, int e) { return q[seg + (step * 64 + lane) * 8 + e]; };
    for (int step = 0; step < 5; ++step)
        for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 8; ++e) {
                const int tap = 2 * step + (lane >> 5), co = lane & 31;
                const uint16_t want = e < 6 && tap < 9 ? Q::rne(w1[(co * 6 + e) * 9 + tap]) : 0;
                REQUIRE(frag(Q::kQ1, step, lane, e) == want);
            }
    for (int layer = 2; layer <= 3; ++layer) {
        const int cin = layer == 2 ? 32 : 64, per_tap = cin / 16, tiles = layer == 2 ? 2 : 4, seg = layer == 2 ? Q::kQ2 : Q::kQ3;
        const std::vector<float>& w = layer == 2 ? w2 : w3;
        for (int tile = 0; tile < tiles; ++tile)
            for (int step = 0; step < 9 * per_tap; ++step)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int tap = step / per_tap, ci = 16 * (step % per_tap) + 8 * (lane >> 5) + e, co = 32 * tile + (lane & 31);
                        REQUIRE(frag(seg, tile * 9 * per_tap + step, lane, e) == Q::rne(w[(static_cast<size_t>(co) * cin + ci) * 9 + tap]));
                    }
    }
    std::vector<int> seen(6 * 128, 0);
    for (int wave = 0; wave < 4; ++wave)
        for (int step = 0; step < 2; ++step)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    // the row of a 32 x 32 accumulator tile that register 8 step + e of this lane half holds, as a channel of the wave's 32
                    const int r = 8 * step + e, c = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), j = lane & 31;
                    const uint16_t want = j < 4 ? Q::rne(wp[j * 128 + c]) : j < 6 ? Q::rne(wv[(j - 4) * 128 + c]) : 0;
                    REQUIRE(frag(Q::kQh, wave * 2 + step, lane, e) == want);
                    if (j < 6) ++seen[j * 128 + c];
                }
    for (int v : seen) REQUIRE(v == 1);                                       // every head weight exactly once
    REQUIRE(Q::kQh + 4 * 2 * 512 == Q::kElements && Q::kElements % 8 == 0 && Q::kQ2 % 8 == 0 && Q::kQ3 % 8 == 0 && Q::kQh % 8 == 0);
    std::printf("pvnet_bf16_pack_check: ok (%d bf16 elements)\n", Q::kElements);
    return 0;
}
