// replay_image.h -- the byte image of a replay buffer (gmk_replay_snapshot / gmk_replay_restore) and the rules that make one valid.
// One definition for the device (replay_kernel.hip checks an image before it reads a move or a visit row) and the host
// (gmk_replay_image_check_host, tools/replay_image_check.cpp); the format is stated in full in include/gomoku_hip.h ("replay buffer").
// Every read goes through bytes, so an image needs no alignment here and is little-endian on any host.
#pragma once
#include <cstdint>

#include "philox.h"      // GMK_HD

namespace gmk {

constexpr uint64_t kImageHeaderBytes = 64, kImageDescBytes = 8, kImageRowBytes = 450;
constexpr int kImageCells = 225;
constexpr uint64_t kImageMaxGames = static_cast<uint64_t>(1) << 40, kImageMaxHead = static_cast<uint64_t>(1) << 62;

// what a check returns: 0 or the first rule that the image breaks
enum ReplayImageFault {
    kImageOk = 0, kImageMagic, kImageReserved, kImageGames, kImageHead, kImageBytesField, kImageBytesFormula, kImageLen, kImageFirst, kImageDescPad,
    kImagePlySum, kImageSampleSum, kImageMove, kImageSectionPad
};

GMK_HD const char* replay_image_fault_text(int fault) {
    switch (fault) {
        case kImageOk: return "valid";
        case kImageMagic: return "the magic is not GMKRPLY1";
        case kImageReserved: return "a reserved word is not zero";
        case kImageGames: return "n is above 2^40";
        case kImageHead: return "head is above 2^62";
        case kImageBytesField: return "the bytes field is not the size given";
        case kImageBytesFormula: return "the size is not 64 + 8 n + roundup8(T) + roundup8(450 S)";
        case kImageLen: return "a game length is above 225";
        case kImageFirst: return "a first sampled ply is above 225";
        case kImageDescPad: return "a descriptor's pad bytes are not zero";
        case kImagePlySum: return "the lengths do not add up to T";
        case kImageSampleSum: return "the sampled plies do not add up to S";
        case kImageMove: return "a move is above 224";
        case kImageSectionPad: return "a section's padding is not zero";
    }
    return "unknown";
}

struct ReplayImageHeader { uint64_t n, T, S, head, bytes; };

GMK_HD uint64_t image_u64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
    return v;
}

GMK_HD void image_put_u64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = static_cast<uint8_t>(v >> (8 * i));
}

GMK_HD uint64_t image_roundup8(uint64_t x) { return (x + 7) & ~static_cast<uint64_t>(7); }

// the size of the image of n games, T stored and S sampled plies (n <= 2^40, T and S <= 225 n: no overflow)
GMK_HD uint64_t replay_image_size(uint64_t n, uint64_t T, uint64_t S) {
    return kImageHeaderBytes + kImageDescBytes * n + image_roundup8(T) + image_roundup8(kImageRowBytes * S);
}

// The 64 header bytes of an image of `bytes` bytes (bytes >= 64).  Passing it means that the n descriptors lie inside the image and that
// the two big sections are where the formula puts them; nothing past the header has been read.
GMK_HD int replay_image_check_header(const uint8_t* image, uint64_t bytes, ReplayImageHeader* out) {
    const char magic[9] = "GMKRPLY1";
    for (int i = 0; i < 8; ++i)
        if (image[i] != static_cast<uint8_t>(magic[i])) return kImageMagic;
    ReplayImageHeader h;
    h.n = image_u64(image + 8);
    h.T = image_u64(image + 16);
    h.S = image_u64(image + 24);
    h.head = image_u64(image + 32);
    h.bytes = image_u64(image + 40);
    if (image_u64(image + 48) != 0 || image_u64(image + 56) != 0) return kImageReserved;
    if (h.n > kImageMaxGames) return kImageGames;
    if (h.head > kImageMaxHead) return kImageHead;
    if (h.bytes != bytes) return kImageBytesField;
    if (h.T > kImageCells * h.n || h.S > kImageCells * h.n || replay_image_size(h.n, h.T, h.S) != bytes) return kImageBytesFormula;
    *out = h;
    return kImageOk;
}

// one 8-byte descriptor: uint16 len, uint16 first, int8 winner (copied, not judged), three zero bytes
GMK_HD int replay_image_check_desc(const uint8_t* d, int* len, int* first, int* winner) {
    const int l = d[0] | (d[1] << 8), f = d[2] | (d[3] << 8);
    if (l > kImageCells) return kImageLen;
    if (f > kImageCells) return kImageFirst;
    if (d[5] | d[6] | d[7]) return kImageDescPad;
    *len = l;
    *first = f;
    *winner = static_cast<int8_t>(d[4]);
    return kImageOk;
}

GMK_HD void replay_image_put_desc(uint8_t* d, int len, int first, int winner) {
    d[0] = static_cast<uint8_t>(len);
    d[1] = static_cast<uint8_t>(len >> 8);
    d[2] = static_cast<uint8_t>(first);
    d[3] = static_cast<uint8_t>(first >> 8);
    d[4] = static_cast<uint8_t>(winner);
    d[5] = d[6] = d[7] = 0;
}

GMK_HD int image_sampled(int len, int first) { return len > first ? len - first : 0; }

// Everything: the header, every descriptor, the sums, and -- what only the host checks -- every move byte and the sections' padding.
// The device runs the same header and descriptor rules with its own parallel sums (replay_restore_kernel).
GMK_HD int replay_image_check(const uint8_t* image, uint64_t bytes, ReplayImageHeader* out) {
    ReplayImageHeader h;
    const int fault = replay_image_check_header(image, bytes, &h);
    if (fault) return fault;
    uint64_t T = 0, S = 0;
    for (uint64_t g = 0; g < h.n; ++g) {
        int len, first, winner;
        const int bad = replay_image_check_desc(image + kImageHeaderBytes + kImageDescBytes * g, &len, &first, &winner);
        if (bad) return bad;
        T += static_cast<uint64_t>(len);
        S += static_cast<uint64_t>(image_sampled(len, first));
    }
    if (T != h.T) return kImagePlySum;
    if (S != h.S) return kImageSampleSum;
    const uint8_t* moves = image + kImageHeaderBytes + kImageDescBytes * h.n;
    for (uint64_t i = 0; i < h.T; ++i)
        if (moves[i] >= kImageCells) return kImageMove;
    for (uint64_t i = h.T; i < image_roundup8(h.T); ++i)
        if (moves[i]) return kImageSectionPad;
    const uint8_t* visits = moves + image_roundup8(h.T);
    for (uint64_t i = kImageRowBytes * h.S; i < image_roundup8(kImageRowBytes * h.S); ++i)
        if (visits[i]) return kImageSectionPad;
    *out = h;
    return kImageOk;
}

}  // namespace gmk
