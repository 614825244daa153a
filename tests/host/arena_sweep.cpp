// arena_sweep.cpp -- tls_amd/csrc/tls_arena.h on the host, under the address and undefined-behaviour sanitizers: the arena
// over element mixes taken from the survey stages, the closed-form sizes of three of their layouts, and the buffer pool with
// malloc / free behind it.  No device, nothing preloaded; tests/test_arena_host.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../tls_amd/csrc/tls_arena.h"

using tlsmem::Arena;
using tlsmem::BufPool;
using tlsmem::DevBuf;
using tlsmem::Kind;

namespace {
long long g_live = 0;          // allocations not yet freed
bool g_fail_next = false;      // the next allocation fails (as a full device would)
}  // namespace

int tlsmem::device_alloc(void** out, size_t bytes) {
    if (g_fail_next) { g_fail_next = false; *out = nullptr; return 2; }
    *out = std::malloc(bytes);
    if (!*out) return 2;
    ++g_live;
    return 0;
}
int tlsmem::device_free(void* p) { std::free(p); --g_live; return 0; }

namespace {

#define REQUIRE(cond)                                                                   \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

struct alignas(16) Pair { double x, y; };                   // double2
struct Row16 { int width, offset; double span_max; };       // a SingleRow
struct Fit24 { double period; int dur, roll, n_epochs, pad_; };   // a T0FitParams
static_assert(sizeof(Pair) == 16 && alignof(Pair) == 16 && sizeof(Row16) == 16 && alignof(Row16) == 8 && sizeof(Fit24) == 24, "");

// an arena that remembers what it was given, to be checked against what bind() made of it
struct Sweep {
    struct Seen { size_t align, size, count; const void* dst; unsigned char* (*get)(const void*); };
    Arena L;
    Seen seen[Arena::kMaxRegions + 8];
    int n = 0;
    template <typename T>
    void add(T*& p, size_t count) {
        p = reinterpret_cast<T*>(uintptr_t(1));                  // (a count of 0 must overwrite this with null)
        L.add(p, count);
        seen[n++] = Seen{alignof(T), sizeof(T), count, &p,
                         [](const void* q) { return reinterpret_cast<unsigned char*>(*static_cast<T* const*>(q)); }};
    }
    // binds to a fresh buffer of B, checks every property, writes every element; returns the arena's bytes
    template <typename B>
    size_t bind_and_check() {
        size_t expect = 0;
        for (int i = 0; i < n; ++i)
            if (seen[i].count) expect = (expect + seen[i].align - 1) / seen[i].align * seen[i].align + seen[i].count * seen[i].size;
        REQUIRE(L.bytes() == expect);                            // the total is the sum of the padded regions
        BufPool pool;
        DevBuf<B> buf(pool, "backing", Kind::scratch);
        REQUIRE(L.bind(buf) == 0);
        REQUIRE(buf.cap == (expect + sizeof(B) - 1) / sizeof(B));
        unsigned char* base = reinterpret_cast<unsigned char*>(buf.ptr);
        unsigned char* end = base;
        for (int i = 0; i < n; ++i) {
            unsigned char* at = seen[i].get(seen[i].dst);
            if (seen[i].count == 0) { REQUIRE(at == nullptr); continue; }
            REQUIRE(at != nullptr);
            REQUIRE(reinterpret_cast<uintptr_t>(at) % seen[i].align == 0);   // starts at its type's alignment
            REQUIRE(at >= end);                                              // disjoint, in declaration order
            REQUIRE(size_t(at - end) < seen[i].align);                       // ... with nothing but the padding between
            end = at + seen[i].count * seen[i].size;
            REQUIRE(end <= base + buf.cap * sizeof(B));                      // within the bound capacity
        }
        REQUIRE(size_t(end - base) == expect);
        for (int i = 0; i < n; ++i)                                          // ASan judges every byte of every region
            if (seen[i].count) std::memset(seen[i].get(seen[i].dst), 0xA5, seen[i].count * seen[i].size);
        return expect;
    }
};

// one mix of every element kind the stages use; k int columns of sl rows; `opt` switches the optional regions on
template <typename B>
void mix(size_t cs, size_t n, size_t sl, size_t k, size_t rows, size_t bytes, bool opt) {
    Pair *pairs, *held;
    double *y, *dy, *out, *period, *secondary, *t, *taps, *scratch;
    int *ints, *slot;
    Row16* row;
    Fit24* fit;
    unsigned char *mask, *status;
    long long* counts;
    unsigned long long* words;
    Sweep s;
    s.add(pairs, cs * n);
    s.add(held, opt ? sl * 3 : 0);
    s.add(y, cs * n);
    s.add(dy, opt ? cs * n : 0);
    s.add(out, sl * 5);
    s.add(period, sl);
    s.add(secondary, opt ? sl : 0);
    s.add(ints, k * sl);             // a block of k contiguous int columns: one region
    s.add(t, n);                     // (the realignment behind the ints)
    s.add(row, rows);
    s.add(taps, 2 * rows);
    s.add(fit, sl);
    s.add(slot, sl);
    s.add(mask, bytes);
    s.add(status, opt ? bytes : 0);
    s.add(counts, sl);               // (the realignment behind the bytes)
    s.add(words, opt ? 0 : n);
    s.add(scratch, 3 * n);
    s.bind_and_check<B>();
}

size_t sweep_mixes() {
    const size_t counts[] = {0, 1, 2, 3, 7, 64, 1001, 4097};
    size_t checked = 0;
    for (size_t n : counts)
        for (size_t sl : counts)
            for (size_t k : {size_t(1), size_t(3), size_t(5)})
                for (int opt = 0; opt < 2; ++opt) {
                    const size_t cs = sl > 64 ? 3 : sl, rows = (n % 5) + (sl % 3), bytes = n * 3 + sl;
                    mix<double>(cs, n, sl, k, rows, bytes, opt != 0);
                    mix<unsigned char>(cs, n, sl, k, rows, bytes, opt != 0);
                    mix<int>(cs, n, sl, k, rows, bytes, opt != 0);
                    checked += 3;
                }
    return checked;
}

// ---- three layouts of the library, region by region as tls_amd.hip names them, against their closed forms in doubles
size_t times_arena(size_t cs, size_t sl, size_t n, size_t E, size_t T, size_t R, size_t taps) {
    Pair* pairs; double *y, *dy, *out, *out_times, *period, *T0, *t, *d_taps, *slopes; int* ints; Row16* rows;
    Sweep s;
    s.add(pairs, cs * n); s.add(y, cs * n); s.add(dy, cs * n); s.add(out, sl * E); s.add(out_times, sl * T);
    s.add(period, sl); s.add(T0, sl); s.add(ints, 3 * sl); s.add(t, n); s.add(rows, R); s.add(d_taps, 2 * taps);
    s.add(slopes, 3 * taps);
    const size_t bytes = s.bind_and_check<double>();
    return (bytes + 7) / 8;
}

size_t views_arena(size_t cs, size_t sl, size_t n, size_t W, size_t ng, size_t nl, size_t scratch) {
    double *y, *out, *period, *T0, *duration, *secondary, *gmed, *lmed, *t, *d_scratch; int *slot, *gcnt, *lcnt;
    Sweep s;
    s.add(y, cs * n); s.add(out, sl * W); s.add(period, sl); s.add(T0, sl); s.add(duration, sl); s.add(secondary, sl);
    s.add(gmed, sl * ng); s.add(lmed, sl * nl); s.add(slot, sl); s.add(gcnt, sl * ng); s.add(lcnt, sl * nl); s.add(t, n);
    s.add(d_scratch, scratch);
    const size_t bytes = s.bind_and_check<double>();
    return (bytes + 7) / 8;
}

size_t peak_fits_arena(size_t s_, size_t rows, size_t max_len) {
    double *pick, *per_transit, *signal; Fit24* fit; int *n_epochs, *curve;
    Sweep s;
    s.add(pick, 8 * s_); s.add(per_transit, rows * s_); s.add(signal, max_len * s_); s.add(fit, s_);
    s.add(n_epochs, 2 * s_); s.add(curve, 2 * s_);
    const size_t bytes = s.bind_and_check<double>();
    return (bytes + 7) / 8;
}

size_t closed_forms() {
    size_t checked = 0;
    const size_t sls[] = {1, 2, 3, 7, 64, 1023, 1024};
    for (size_t sl : sls)
        for (size_t n : {size_t(1), size_t(50), size_t(1001)}) {
            const size_t cs = sl > 7 ? 5 : sl;
            for (size_t me : {size_t(1), size_t(9)}) {
                const size_t E = 8, T = 6 * me, R = 1 + n % 7, taps = 11 + sl % 4;
                REQUIRE(times_arena(cs, sl, n, E, T, R, taps)
                        == 4 * cs * n + sl * (E + T + 2) + (3 * sl + 1) / 2 + n + 2 * R + 5 * taps);
                ++checked;
            }
            for (size_t ng : {size_t(2), size_t(201)}) {
                const size_t W = 16, nl = 2 * (ng / 2 + 1), scratch = n > 50 ? 3 * 2 * n : 0;
                REQUIRE(views_arena(cs, sl, n, W, ng, nl, scratch)
                        == cs * n + sl * (W + 4 + ng + nl) + (sl * (1 + ng + nl) + 1) / 2 + n + scratch);
                ++checked;
            }
            for (size_t max_len : {size_t(1), size_t(37)}) {
                const size_t rows = 6 * (1 + n % 4);
                REQUIRE(peak_fits_arena(sl, rows, max_len) == 8 * sl + rows * sl + max_len * sl + 3 * sl + sl + sl);
                ++checked;
            }
        }
    return checked;
}

// ---- the owner: register, reserve, grow, count, walk by kind, a failed allocation, release, scope exit
void pool_checks() {
    REQUIRE(g_live == 0);
    {
        BufPool pool;
        DevBuf<double> a(pool, "a", Kind::scratch);
        DevBuf<int> b(pool, "b", Kind::state);
        DevBuf<unsigned char> c(pool, "c", Kind::scratch);
        REQUIRE(pool.bytes() == 0 && pool.first == &a && a.next == &b && b.next == &c && c.next == nullptr && pool.last == &c);
        REQUIRE(a.reserve(10) == 0 && a.cap == 10 && a.ptr);
        double* first = a.ptr;
        REQUIRE(a.reserve(4) == 0 && a.ptr == first && a.cap == 10);          // grows only
        REQUIRE(a.reserve(1000) == 0 && a.cap == 1000);
        for (size_t i = 0; i < a.cap; ++i) a.ptr[i] = 1.0;
        REQUIRE(b.reserve(0) == 0 && b.cap == 0 && b.ptr == nullptr);
        REQUIRE(b.reserve(33) == 0 && c.reserve(7) == 0);
        REQUIRE(pool.bytes() == 1000 * 8 + 33 * 4 + 7);
        REQUIRE(g_live == 3);
        size_t scratch = 0, state = 0;
        for (const tlsmem::PoolBuf* p = pool.first; p; p = p->next) {
            REQUIRE(p->base() != nullptr && p->bytes() == p->cap * p->elem);
            std::memset(p->base(), 0xFF, p->bytes());                         // (what the poison entry does to scratch)
            (p->kind == Kind::scratch ? scratch : state) += p->bytes();
        }
        REQUIRE(scratch == 1000 * 8 + 7 && state == 33 * 4);
        g_fail_next = true;                                                   // frees before it allocates; consistent on failure
        REQUIRE(b.reserve(100) != 0 && b.ptr == nullptr && b.cap == 0 && g_live == 2);
        REQUIRE(pool.bytes() == 1000 * 8 + 7);
        REQUIRE(b.reserve(100) == 0 && b.cap == 100 && g_live == 3);
        Arena L;                                                              // a failed bind leaves the pointers null
        double* x; int* y;
        L.add(x, 5000); L.add(y, 3);
        g_fail_next = true;
        REQUIRE(L.bind(a) != 0 && x == nullptr && y == nullptr && a.ptr == nullptr && a.cap == 0);
        REQUIRE(L.bind(a) == 0 && x == a.ptr && a.cap == 5002);
        pool.release_all();
        REQUIRE(g_live == 0 && pool.bytes() == 0 && a.ptr == nullptr && b.ptr == nullptr && c.ptr == nullptr);
        REQUIRE(c.reserve(3) == 0 && g_live == 1);                            // (left to the buffer's scope exit)
    }
    REQUIRE(g_live == 0);
}

}  // namespace

int main() {
    const size_t mixes = sweep_mixes();
    const size_t forms = closed_forms();
    pool_checks();
    std::printf("%zu arenas checked, %zu closed forms equal, pool clean\n", mixes, forms);
    return 0;
}
