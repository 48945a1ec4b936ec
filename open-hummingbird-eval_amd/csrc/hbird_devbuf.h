// One move-only owner of a device allocation: a pointer, its size in bytes, nothing else.  Every allocation an index owns is a member of this
// type (hbird_internal.h, hbird_f16_centre.h), every temporary a local: a failing call frees what it had, and no free list is kept by hand.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

// The seam to the device (hbird_capi.hip: hipMalloc / hipFree / hipMemcpyAsync; the CPU test of this header: malloc / free / memcpy).
// alloc and copy return nullptr or the reason they failed (alloc: *p == nullptr, and no device error is left pending); alloc and free keep
// the counts of hb_debug_live_allocations.  copy_sync: `bytes` from src to dst on `stream` (none for bytes == 0), then the stream's end.
const char* hb_dev_alloc(void** p, size_t bytes);
void hb_dev_free(void* p, size_t bytes);
const char* hb_dev_copy_sync(void* dst, const void* src, size_t bytes, void* stream);

int hb_fail(const std::string& msg);

static inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }      // every carve-up of a workspace

// how a buffer that is too small grows: to the size asked for, or a quarter beyond it (workspaces sized by a search's query count)
enum hb_grow { HB_GROW_EXACT = 0, HB_GROW_QUARTER = 1 };

struct hb_devbuf {
    void* p = nullptr;
    size_t bytes = 0;

    hb_devbuf() = default;
    hb_devbuf(const hb_devbuf&) = delete;
    hb_devbuf& operator=(const hb_devbuf&) = delete;
    hb_devbuf(hb_devbuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    hb_devbuf& operator=(hb_devbuf&& o) noexcept {
        if (this != &o) { drop(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~hb_devbuf() { drop(); }

    void drop() {
        if (p) hb_dev_free(p, bytes);
        p = nullptr; bytes = 0;
    }
    explicit operator bool() const { return p != nullptr; }
    template <class T> T* as(size_t byte_offset = 0) const { return reinterpret_cast<T*>(static_cast<char*>(p) + byte_offset); }

    // At least `need` bytes; the contents do not survive a growth.  A no-op while bytes >= need, else free, then allocate.  On failure the
    // buffer is left empty; try_ensure returns the reason (nullptr: fine) and reports nothing, ensure returns -1 through hb_fail.
    const char* try_ensure(size_t need, hb_grow g) {
        if (bytes >= need) return nullptr;
        drop();
        const size_t sz = g == HB_GROW_QUARTER ? need + need / 4 : need;
        if (const char* why = hb_dev_alloc(&p, sz)) { p = nullptr; return why; }
        bytes = sz;
        return nullptr;
    }
    int ensure(size_t need, hb_grow g) {
        const char* why = try_ensure(need, g);
        return why ? hb_fail("device allocation of " + std::to_string(need) + " bytes: " + why) : 0;
    }
    // ... and the form that keeps the first `keep` bytes: allocate new, copy on `stream`, wait for the stream, free old.  On failure the
    // buffer is as it was.
    int ensure_keep(size_t need, hb_grow g, size_t keep, void* stream) {
        if (bytes >= need) return 0;
        hb_devbuf nb;
        if (nb.ensure(need, g)) return -1;
        if (const char* why = hb_dev_copy_sync(nb.p, p, keep, stream)) return hb_fail(std::string("device copy into a grown buffer: ") + why);
        *this = static_cast<hb_devbuf&&>(nb);
        return 0;
    }
};

// a buffer read as an array of T: converts to T* where a launcher or a kernel's argument block takes the pointer
template <class T> struct hb_dev : hb_devbuf {
    operator T*() const { return static_cast<T*>(p); }
};
