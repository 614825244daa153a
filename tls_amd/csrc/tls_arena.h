// tls_arena.h -- host only, no HIP: who owns device memory and how one allocation is cut into typed regions
// (DESIGN.md "Device memory").
//
// BufPool / DevBuf: a DevBuf is constructed against a pool, with its name and kind, so the pool knows every buffer there is:
// it releases them all, sums their bytes, and walks them by kind.  The pool is declared in front of its buffers and so
// outlives them; a buffer frees itself where its scope ends.  Arena: a stage names the regions of one allocation once, in
// order, as typed pointers with element counts; bind() reserves the backing DevBuf and sets every pointer.
#pragma once

#include <cassert>
#include <cstddef>

namespace tlsmem {

// The two calls behind every DevBuf, defined by the including program (hipMalloc / hipFree in the library, malloc / free in
// the host test); they return 0 for success, else the allocator's own error code, which reserve() hands on.
int device_alloc(void** out, size_t bytes);
int device_free(void* p);

enum class Kind {
    scratch,   // the next call writes all that it reads from it: tls_debug_poison_lds may smear it
    state,     // held between calls by design (the reason stands where the buffer is declared): never smeared
};

struct BufPool;

// the untyped part of a DevBuf: what the pool walks
struct PoolBuf {
    const char* name;
    Kind kind;
    size_t elem;             // bytes of one element
    size_t cap = 0;          // elements
    PoolBuf* next = nullptr;
    void* base() const { return *slot; }
    size_t bytes() const { return cap * elem; }
    void release() { if (*slot) (void)device_free(*slot); *slot = nullptr; cap = 0; }
    PoolBuf(const PoolBuf&) = delete;
    PoolBuf& operator=(const PoolBuf&) = delete;
protected:
    PoolBuf(BufPool& pool, const char* name, Kind kind, size_t elem, void** slot);
    ~PoolBuf() { release(); }   // (a buffer frees itself where its scope ends)
    void** slot;             // the typed pointer of the DevBuf around this
};

struct BufPool {
    PoolBuf* first = nullptr;
    PoolBuf* last = nullptr;
    BufPool() = default;
    BufPool(const BufPool&) = delete;
    BufPool& operator=(const BufPool&) = delete;
    void release_all() { for (PoolBuf* b = first; b; b = b->next) b->release(); }
    size_t bytes() const { size_t sum = 0; for (const PoolBuf* b = first; b; b = b->next) sum += b->bytes(); return sum; }
};

inline PoolBuf::PoolBuf(BufPool& pool, const char* name_, Kind kind_, size_t elem_, void** slot_)
    : name(name_), kind(kind_), elem(elem_), slot(slot_) {
    (pool.last ? pool.last->next : pool.first) = this;
    pool.last = this;
}

// Grows only, frees before it allocates, and leaves cap and ptr consistent on failure.
template <typename T>
struct DevBuf : PoolBuf {
    T* ptr = nullptr;
    DevBuf(BufPool& pool, const char* name, Kind kind) : PoolBuf(pool, name, kind, sizeof(T), reinterpret_cast<void**>(&ptr)) {}
    int reserve(size_t n_elem) {
        if (n_elem <= cap) return 0;
        if (ptr) { const int e = device_free(ptr); ptr = nullptr; cap = 0; if (e) return e; }
        const int e = device_alloc(reinterpret_cast<void**>(&ptr), (n_elem ? n_elem : 1) * sizeof(T));
        if (e == 0) cap = n_elem;
        return e;
    }
};

// One allocation cut into typed regions.  A region starts at its element type's alignment (the allocation itself is aligned
// for every type) and takes count * sizeof(T) bytes; a region of count 0 takes no space and its pointer is null.  A block
// of k contiguous columns is one region of k * rows elements.  No heap: at most kMaxRegions regions.
struct Arena {
    static constexpr int kMaxRegions = 32;
    template <typename T>
    void add(T*& dst, size_t count) {
        dst = nullptr;
        if (count == 0) return;
        assert(used < kMaxRegions);
        total = (total + alignof(T) - 1) / alignof(T) * alignof(T);
        region[used++] = Region{&dst, total, [](void* d, unsigned char* at) { *static_cast<T**>(d) = reinterpret_cast<T*>(at); }};
        total += count * sizeof(T);
    }
    size_t bytes() const { return total; }
    // reserves the backing buffer (the total rounded up to its element) and sets every pointer; on failure they stay null
    template <typename B>
    int bind(DevBuf<B>& buf) const {
        if (const int e = buf.reserve((total + sizeof(B) - 1) / sizeof(B))) return e;
        unsigned char* base = reinterpret_cast<unsigned char*>(buf.ptr);
        for (int i = 0; i < used; ++i) region[i].set(region[i].dst, base + region[i].offset);
        return 0;
    }
private:
    struct Region { void* dst; size_t offset; void (*set)(void*, unsigned char*); };
    Region region[kMaxRegions];
    int used = 0;
    size_t total = 0;
};

}  // namespace tlsmem
