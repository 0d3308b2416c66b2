// host_staging.h -- the one device block behind a host-form entry or a root read-out: lay the parts out, allocate once, copy the inputs up,
// copy back the outputs the caller asked for, free on every path.  The layout is plain C++ (tools/host_staging_check.cpp runs it under the
// sanitizers with GMK_STAGING_LAYOUT_ONLY defined); Blocks and Staging below it are the HIP side.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gmk {

struct StagePart {
    size_t count, size;                                         // elements, and the bytes of one
    bool present;                                               // an optional output that was not asked for is absent: no bytes, a null pointer
    size_t offset;                                              // stage_layout's: where the part begins in the block
};

// The parts in order at 16-byte-aligned offsets, and the block's size.  A present part of count 0 still takes 16 bytes, so that its address is
// its own.  False when the size does not fit a size_t.
inline bool stage_layout(StagePart* parts, size_t n, size_t* total) {
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        StagePart& p = parts[i];
        p.offset = at;
        if (!p.present) continue;
        const size_t count = p.count ? p.count : 1;
        if (p.size == 0 || count > (SIZE_MAX - 15 - at) / p.size) return false;
        at += (count * p.size + 15) & ~size_t(15);
    }
    *total = at;
    return true;
}
inline char* stage_pointer(char* block, const StagePart& p) { return p.present ? block + p.offset : nullptr; }

}  // namespace gmk

#ifndef GMK_STAGING_LAYOUT_ONLY
#include <algorithm>
#include <cstring>
#include <vector>

#include "capi_common.h"

namespace gmk {

// A few device blocks, each carved into the arrays that were asked for since the last take(); all are freed when the object goes, whichever way.
struct Blocks {
    size_t min_bytes = 0;                                       // a block is asked for at this size at least
    bool pooled = true;                                         // false: plain hipMalloc, for blocks that the library's pool should not keep
    std::vector<void*> held;
    std::vector<void*> where;                                   // of the block to come: where each array's pointer goes ...
    std::vector<StagePart> parts;                               // ... and its part
    template <class T>
    void want(T*& p, size_t count, bool present = true) {
        p = nullptr;
        where.push_back(static_cast<void*>(&p));
        parts.push_back(StagePart{count, sizeof(T), present, 0});
    }
    bool take() {                                               // one allocation for everything wanted since the last one
        size_t total = 0;
        void* block = nullptr;
        const bool ok = stage_layout(parts.data(), parts.size(), &total) &&
                        (pooled ? device_malloc_bytes(&block, std::max(total, min_bytes)) : hipMalloc(&block, std::max(total, min_bytes))) == hipSuccess;
        if (ok) held.push_back(block);
        for (size_t i = 0; ok && i < parts.size(); ++i) {
            char* at = stage_pointer(static_cast<char*>(block), parts[i]);
            std::memcpy(where[i], &at, sizeof(at));             // every T* has the representation of a char* here
        }
        where.clear(); parts.clear();
        return ok;
    }
    void release() {
        for (void* p : held) (void)device_free(p);              // (a block that is not the pool's goes to hipFree there)
        held.clear();
    }
    ~Blocks() { release(); }
};

// A block asked for at this size at least is the library's pool's (capi.hip): an entry that is called over and over gets it back without a trip to the
// driver, which costs ~150 us from 2 MB on where smaller requests cost ~1 us.  A pooled block comes back uncleared.
constexpr size_t kPoolKeeps = size_t(16) << 20;

// One block that pairs host buffers with device pointers: register the parts, take() once, run, download().  A failing HIP call gives GMK_ERR_HIP
// and a text that names the entry and the call; a code that the wrapped device form returned is the site's to pass on, with the device form's text.
class Staging {
  public:
    explicit Staging(const char* who, size_t min_bytes = 0, bool pooled = true) : who_(who) { blocks_.min_bytes = min_bytes; blocks_.pooled = pooled; }
    template <class T>
    void in(T*& p, const T* h, size_t count) {                   // uploaded by take()
        blocks_.want(p, count);
        copies_.push_back(Copy{&p, const_cast<T*>(h), count * sizeof(T), true});
    }
    template <class T>
    void out(T*& p, T* h, size_t count, bool always = false) {   // present when h is not NULL, and then copied back by download(); `always`: the
        blocks_.want(p, count, h || always);                     // kernel writes the part whether or not the caller reads it, so it is there anyway
        if (h) copies_.push_back(Copy{&p, h, count * sizeof(T), false});
    }
    template <class T>
    void scratch(T*& p, size_t count) { blocks_.want(p, count); }      // the device's alone: never copied
    int take() {
        if (!blocks_.take()) { set_error("%s: the staging block does not fit in device memory", who_); return GMK_ERR_HIP; }
        return copy(true);
    }
    int download() { return copy(false); }
    int check(hipError_t e, const char* call) {
        if (e == hipSuccess) return GMK_OK;
        set_error("%s: %s failed: %s", who_, call, hipGetErrorString(e));
        return GMK_ERR_HIP;
    }

  private:
    struct Copy { void* where; void* host; size_t bytes; bool up; };
    int copy(bool up) {
        for (const Copy& c : copies_) {
            void* d;
            std::memcpy(&d, c.where, sizeof(d));
            if (c.up != up || c.bytes == 0) continue;
            const int rc = up ? check(hipMemcpy(d, c.host, c.bytes, hipMemcpyHostToDevice), "hipMemcpy of an input")
                              : check(hipMemcpy(c.host, d, c.bytes, hipMemcpyDeviceToHost), "hipMemcpy of an output");
            if (rc != GMK_OK) return rc;
        }
        return GMK_OK;
    }
    const char* who_;
    Blocks blocks_;
    std::vector<Copy> copies_;
};

// A HIP call of a site that holds a Staging: on failure the entry returns what check() made of it (the block goes with the object).
#define GMK_STAGED(st, expr) do { if (const int rc_ = (st).check((expr), #expr)) return rc_; } while (0)

}  // namespace gmk
#endif
