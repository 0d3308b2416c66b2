// replay_image_check.cpp -- the replay buffer's image rules (gomokuai_amd/csrc/replay_image.h) as a stand-alone program, for a run under the
// address and undefined-behaviour sanitizers on a machine without a GPU:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined tools/replay_image_check.cpp -o tools/bin/replay_image_check && tools/bin/replay_image_check
// It builds valid images in memory (the empty one, a small one, the wrapped-ring case of tests/test_replay_image_gpu.py), runs the host
// check on each, on every single-byte corruption of the header and the descriptors and on every truncation.  Every image is allocated to
// exactly its size, so a check that reads past `bytes` is a sanitizer report.  Exits non-zero on the first thing that is wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gomokuai_amd/csrc/replay_image.h"

using namespace gmk;

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "replay_image_check: %s failed (line %d)\n", #cond, __LINE__); return 1; } } while (0)

struct Game { int len, first, winner; };

// an image on the heap, exactly `bytes` long
struct Image {
    uint8_t* p = nullptr;
    uint64_t bytes = 0;
    Image(const uint8_t* src, uint64_t n) : p(static_cast<uint8_t*>(std::malloc(n ? n : 1))), bytes(n) { std::memcpy(p, src, n); }
    Image(const Image&) = delete;
    ~Image() { std::free(p); }
    int check(ReplayImageHeader* h = nullptr) const { ReplayImageHeader tmp; return replay_image_check(p, bytes, h ? h : &tmp); }
};

static std::vector<uint8_t> build(const std::vector<Game>& games, uint64_t head) {
    uint64_t T = 0, S = 0;
    for (const Game& g : games) { T += g.len; S += image_sampled(g.len, g.first); }
    std::vector<uint8_t> img(replay_image_size(games.size(), T, S), 0);
    std::memcpy(img.data(), "GMKRPLY1", 8);
    image_put_u64(img.data() + 8, games.size());
    image_put_u64(img.data() + 16, T);
    image_put_u64(img.data() + 24, S);
    image_put_u64(img.data() + 32, head);
    image_put_u64(img.data() + 40, img.size());
    for (size_t g = 0; g < games.size(); ++g) replay_image_put_desc(img.data() + 64 + 8 * g, games[g].len, games[g].first, games[g].winner);
    uint8_t* moves = img.data() + 64 + 8 * games.size();
    for (uint64_t i = 0; i < T; ++i) moves[i] = static_cast<uint8_t>((i * 37 + 11) % 225);
    uint8_t* visits = moves + image_roundup8(T);
    for (uint64_t i = 0; i < kImageRowBytes * S; ++i) visits[i] = static_cast<uint8_t>(i * 131 + 7);
    return img;
}

// every single-byte corruption of the header and the descriptors: rejected, unless the byte is one the rules leave free
static int corruptions(const std::vector<uint8_t>& good, const std::vector<Game>& games, long* rejected) {
    const uint64_t head_end = 64 + 8 * games.size();
    for (uint64_t at = 0; at < head_end; ++at)
        for (int flip : {0x01, 0x80, 0xFF}) {
            std::vector<uint8_t> bad = good;
            bad[at] = static_cast<uint8_t>(bad[at] ^ flip);
            const Image img(bad.data(), bad.size());
            ReplayImageHeader h;
            const int fault = img.check(&h);
            bool may_pass = false;
            if (at >= 32 && at < 40) may_pass = image_u64(bad.data() + 32) <= kImageMaxHead;             // another head is another valid image
            if (at >= 64) {
                const Game& g = games[(at - 64) / 8];
                const uint64_t field = (at - 64) % 8;
                const int first = bad[(at & ~7ull) + 2] | (bad[(at & ~7ull) + 3] << 8);
                if (field == 4) may_pass = true;                                                          // the winner is copied, not judged
                if (field == 2 || field == 3) may_pass = first <= 225 && image_sampled(g.len, first) == image_sampled(g.len, g.first);
            }
            REQUIRE((fault == kImageOk) == may_pass);
            if (fault) ++*rejected;
        }
    return 0;
}

// a truncation to `keep` bytes, as it is and with the bytes field mended to match: both rejected
static int truncation(const std::vector<uint8_t>& good, uint64_t keep, long* rejected) {
    std::vector<uint8_t> cut(good.begin(), good.begin() + keep);
    REQUIRE(Image(cut.data(), cut.size()).check() == kImageBytesField);
    image_put_u64(cut.data() + 40, keep);
    REQUIRE(Image(cut.data(), cut.size()).check() == kImageBytesFormula);
    *rejected += 2;
    return 0;
}

int main() {
    long rejected = 0;
    ReplayImageHeader h;

    // ---- the empty buffer: the 64-byte header ----
    const std::vector<uint8_t> empty = build({}, 9);
    REQUIRE(empty.size() == 64);
    REQUIRE(Image(empty.data(), empty.size()).check(&h) == kImageOk && h.n == 0 && h.T == 0 && h.S == 0 && h.head == 9 && h.bytes == 64);
    if (corruptions(empty, {}, &rejected)) return 1;

    // ---- a small image: a game with len <= first, an empty game, odd section sizes; every truncation ----
    const std::vector<Game> small = {{3, 5, -1}, {0, 0, 0}, {7, 2, 1}, {225, 224, 1}};
    const std::vector<uint8_t> simg = build(small, 1);
    REQUIRE(simg.size() == 64 + 32 + 240 + image_roundup8(450 * 6));
    REQUIRE(Image(simg.data(), simg.size()).check(&h) == kImageOk && h.n == 4 && h.T == 235 && h.S == 6 && h.head == 1);
    if (corruptions(simg, small, &rejected)) return 1;
    for (uint64_t keep = 64; keep < simg.size(); ++keep)
        if (truncation(simg, keep, &rejected)) return 1;
    {   // one byte too many, with and without the field mended
        std::vector<uint8_t> longer = simg;
        longer.push_back(0);
        REQUIRE(Image(longer.data(), longer.size()).check() == kImageBytesField);
        image_put_u64(longer.data() + 40, longer.size());
        REQUIRE(Image(longer.data(), longer.size()).check() == kImageBytesFormula);
    }
    {   // what only the host checks: a move of 225, a non-zero pad byte in either section
        std::vector<uint8_t> bad = simg;
        bad[64 + 32 + 100] = 225;
        REQUIRE(Image(bad.data(), bad.size()).check() == kImageMove);
        bad = simg;
        bad[64 + 32 + 235] = 1;
        REQUIRE(Image(bad.data(), bad.size()).check() == kImageSectionPad);
        bad = simg;
        bad[bad.size() - 1] = 1;
        REQUIRE(Image(bad.data(), bad.size()).check() == kImageSectionPad);
        bad = simg;                                                             // T and S off by one where the size cannot tell
        image_put_u64(bad.data() + 16, 236);
        REQUIRE(Image(bad.data(), bad.size()).check() == kImagePlySum);
        rejected += 4;
    }
    {   // sums that lie, with a size that agrees with them: n = 1, T = 8 claimed for a game of 7
        std::vector<uint8_t> bad = build({{7, 0, 0}}, 0);
        std::vector<uint8_t> lie = build({{8, 1, 0}}, 0);                       // the same size: T = 8, S = 7
        REQUIRE(bad.size() == lie.size());
        replay_image_put_desc(lie.data() + 64, 7, 0, 0);
        REQUIRE(Image(lie.data(), lie.size()).check() == kImagePlySum);
        replay_image_put_desc(lie.data() + 64, 8, 0, 0);
        REQUIRE(Image(lie.data(), lie.size()).check() == kImageSampleSum);
        rejected += 2;
    }
    {   // a header that asks for more descriptors than the image has bytes: refused before one is read
        std::vector<uint8_t> bad = empty;
        image_put_u64(bad.data() + 8, kImageMaxGames);
        REQUIRE(Image(bad.data(), bad.size()).check() == kImageBytesFormula);
        image_put_u64(bad.data() + 8, kImageMaxGames + 1);
        REQUIRE(Image(bad.data(), bad.size()).check() == kImageGames);
        image_put_u64(bad.data() + 8, ~0ull);
        REQUIRE(Image(bad.data(), bad.size()).check() == kImageGames);
        bad = empty;
        image_put_u64(bad.data() + 16, ~0ull - 6);                              // roundup8 would wrap to 0
        REQUIRE(Image(bad.data(), bad.size()).check() == kImageBytesFormula);
        bad = empty;
        image_put_u64(bad.data() + 32, kImageMaxHead + 1);
        REQUIRE(Image(bad.data(), bad.size()).check() == kImageHead);
        rejected += 5;
    }

    // ---- the wrapped-ring case of the GPU test: five games of 1, 100, 150, 30 and 225 plies, head 7 ----
    const std::vector<Game> wrapped = {{1, 4, 0}, {100, 4, 1}, {150, 0, -1}, {30, 0, 1}, {225, 0, 0}};
    const std::vector<uint8_t> wimg = build(wrapped, 7);
    REQUIRE(wimg.size() == 64 + 40 + 512 + 225456);                            // T = 506 -> 512, S = 501 -> 450 * 501 = 225450 -> 225456
    REQUIRE(Image(wimg.data(), wimg.size()).check(&h) == kImageOk && h.n == 5 && h.T == 506 && h.S == 501 && h.head == 7);
    if (corruptions(wimg, wrapped, &rejected)) return 1;
    for (uint64_t keep = 64; keep < wimg.size(); keep += (keep < 64 + 40 + 512 + 900 || keep + 900 > wimg.size()) ? 1 : 449)
        if (truncation(wimg, keep, &rejected)) return 1;

    std::printf("replay_image_check: ok (%ld damaged images rejected, largest image %zu bytes)\n", rejected, wimg.size());
    return 0;
}
