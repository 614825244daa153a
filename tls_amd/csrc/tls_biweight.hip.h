// tls_biweight.hip.h -- time-windowed biweight detrending for survey mode (tls_biweight_detrend): for every row y of points
// at the shared time stamps t, trend[i] = Tukey's biweight location of the window of i, and flat[i] = y[i] / trend[i].
//
// The window of point i is the index range [lo_i, hi_i) of the points of i's segment (a new one starts behind every gap
// > break_tolerance) with |t[j] - t[i]| <= window_length / 2.  The windows depend on t alone, so the host forms them once per
// call (tls_biweight_detrend) and every row reads the same lo / hi.  Inside its window the location is iterated from the
// median (include/tls_amd.h):
//     loc = median(v);  repeat up to TLS_BIWEIGHT_MAX_ITER times:
//         mad = median(|v - loc|);  stop if mad == 0
//         u = (v - loc) / (C mad);  w = (1 - u^2)^2 where |u| < 1, else 0
//         new = sum(w v) / sum(w), both sums sequential in ascending index;  stop after this step if |new - loc| <= FTOL |new|
// Every step is one IEEE double operation (no contraction: the pragma in the kernel; the library builds with -fno-fast-math), the
// medians are selections and the sums run in a fixed order, so the result is bit-equal to a numpy restatement of these lines.
//
// A workgroup takes a tile of T consecutive outputs [first, first + T) of one row.  Their windows all lie inside the span
// [lo_first, hi_last) of S slots; it is staged into LDS twice by detrend_stage_sort (tls_detrend.hip.h): in index order (the
// sums) and as (bit-pattern key, slot) pairs sorted once (the medians).  The values are positive doubles, so their bit patterns
// order as integers.  Per output lane:
//   - the first median scans the sorted slots in order and counts the slots inside the window (an LDS broadcast while the
//     lanes of a wave scan together), up to the middle one or two;
//   - the MAD finds loc's place in the sorted slots (binary search) and walks outward from it, skipping slots outside the
//     window, always taking the nearer side: the distances come out in ascending order, fl(loc - v) on the left equal to
//     |fl(v - loc)|, up to the middle one or two;
//   - the two sums loop over the index-ordered copy of the window (neighbouring lanes read neighbouring words).
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_detrend.hip.h.

struct BiweightArgs {
    const double* y;              // [rows][n]
    double* flat;                 // [rows][n]
    double* trend;                // [rows][n], or nullptr
    unsigned long long* check;    // [kChecks] violated bounds (debug build; nullptr: off)
    const int* lo;                // [n] first point of each point's window
    const int* hi;                // [n] one past its last point
    long long n;                  // points per row
    int tile;                     // T outputs per workgroup
    int span;                     // P: sorted slots, a power of two in [64, kDetrendMaxSpan], >= every tile's S
    int smax;                     // the largest S of the call's tiles (the index-ordered copy's LDS slots)
};

// tls_biweight_detrend_masked (include/tls_amd.h): the same tiles with protected points left out of every window.
struct BiweightMaskedArgs : BiweightArgs {
    const unsigned char* mask;    // [rows][n] != 0: protected
    unsigned char* status;        // [rows][n] masked pass: 0 or kBiweightOpen out; fallback pass: in, the outputs with 2 are formed
    int min_points;               // a window with fewer unprotected points (and fewer than it holds) is open
};

// The two instantiations of the masked call's tile, tls_biweight_detrend's steps (the kernel below) with the members in place of
// the window: the masked one leaves protected slots out; the fallback one is the plain biweight for the outputs of status 2 only.
constexpr int kBiweightMasked = 1, kBiweightFallback = 2;
constexpr unsigned int kBiweightProtected = 0x80000000u;   // the spare top bit of a slot word: slot numbers stay below kDetrendMaxSpan
constexpr unsigned char kBiweightOpen = 255;               // the masked pass's mark on an output that tls_biweight_fill has to form

// LDS: keys [P] (uint64) | values in index order [smax] (double) | slot numbers [P] (uint32), 12 P + 8 smax bytes.
// Grid (ceil(n / T), rows).
//
// Masked: the largest span already fills the LDS (12 P + 8 smax = 160 KB at P = smax = 8192), so the mask takes no room of
// its own: behind the sort a protected slot gets the top bit of its slot word, which puts it outside every window for the
// median scan and the MAD walk by the very test that skips the other windows' slots (slot - ua >= the window's length), and
// the sign bit of its value in the index-ordered copy (the values are > 0), which the sums and the member count test.
template <int MODE, class A>
__device__ __forceinline__ void biweight_tile(const A& a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned long long biweight_lds[];
    const int P = a.span, T = a.tile;
    unsigned long long* keys = biweight_lds;
    double* vals = reinterpret_cast<double*>(keys + P);
    unsigned int* slot = reinterpret_cast<unsigned int*>(vals + a.smax);
    const long long row = blockIdx.y;
    const long long first = (long long)blockIdx.x * T;
    const long long n_out = a.n - first < (long long)T ? a.n - first : (long long)T;
    if constexpr (MODE == kBiweightFallback) {
        // a tile without an output of status 2 (nearly every tile of nearly every call) ends here, before it stages anything
        if (threadIdx.x == 0) slot[0] = 0u;
        wg_sync();
        for (int i = threadIdx.x; i < n_out; i += kDetrendThreads)
            if (a.status[row * a.n + first + i] == 2) slot[0] = 1u;
        wg_sync();
        const bool any = slot[0] != 0u;
        wg_sync();                // (the staging below overwrites the word)
        if (!any) return;
    }
    const long long base = a.lo[first];
    const int S = (int)(a.hi[first + n_out - 1] - base);
    TLS_CHECK(a, S >= 1 && S <= a.smax && S <= P, kChkBiweight);
    const double* y = a.y + row * a.n;

    detrend_stage_sort(a, y, base, a.n, S, P, keys, slot, vals, kChkBiweight);

    if constexpr (MODE == kBiweightMasked) {
        const unsigned char* mk = a.mask + row * a.n + base;   // (the span lies inside the row: base + s < n for s < S)
        for (int j = threadIdx.x; j < P; j += kDetrendThreads) {
            const unsigned int s = slot[j];
            if (s < (unsigned int)S && mk[s]) slot[j] = s | kBiweightProtected;
        }
        for (int s = threadIdx.x; s < S; s += kDetrendThreads)
            if (mk[s]) vals[s] = -vals[s];
        wg_sync();
    }

    for (int i = threadIdx.x; i < n_out; i += kDetrendThreads) {
        const long long g = first + i;
        const long long o = row * a.n + g;
        if constexpr (MODE == kBiweightFallback) {
            if (a.status[o] != 2) continue;
        }
        const int wa = (int)(a.lo[g] - base), wb = (int)(a.hi[g] - base);   // the window's slots [wa, wb)
        TLS_CHECK(a, wa >= 0 && wa < wb && wb <= S, kChkBiweight);
        const unsigned int ua = (unsigned int)wa, wn = (unsigned int)(wb - wa);
        unsigned int m = wn;      // the window's members: all of its slots, or the unprotected ones
        if constexpr (MODE == kBiweightMasked) {
            m = 0u;
            for (int j = wa; j < wb; ++j) m += (unsigned int)(vals[j] > 0.0);
            // (a window of fewer than min_points points is short of nothing the mask took: it is asked for all of its own)
            const unsigned int low = (unsigned int)a.min_points < wn ? (unsigned int)a.min_points : wn;
            if (m < low) { a.status[o] = kBiweightOpen; continue; }
            a.status[o] = 0;
        }
        // the ranks of the middle value(s): need1 == need2 for odd m
        const unsigned int need1 = (m + 1u) >> 1, need2 = (m >> 1) + 1u;

        // the median: the sorted slots in order, counting those inside the window
        int f1 = 0, f2 = 0;
        {
            unsigned int c = 0u;
            for (int j = 0; j < S; ++j) {
                if (slot[j] - ua < wn) {
                    ++c;
                    if (c == need1) f1 = j;
                    if (c == need2) { f2 = j; break; }
                }
            }
        }
        TLS_CHECK(a, f1 < S && f2 < S, kChkBiweight);
        const double v1 = __longlong_as_double((long long)keys[f1]), v2 = __longlong_as_double((long long)keys[f2]);
        double loc = (m & 1u) ? v2 : (v1 + v2) / 2.0;

        for (int it = 0; it < TLS_BIWEIGHT_MAX_ITER; ++it) {
            // the MAD: p = the sorted slots with a key <= loc's (loc > 0: its bit pattern orders among the keys)
            const unsigned long long kl = (unsigned long long)__double_as_longlong(loc);
            int p0 = 0, p1 = S;
            while (p0 < p1) {
                const int mid = (p0 + p1) >> 1;
                if (keys[mid] <= kl) p0 = mid + 1; else p1 = mid;
            }
            int l = p0 - 1, r = p0;
            double d1 = 0.0, d2 = 0.0;
            unsigned int c = 0u;
            while (true) {
                while (l >= 0 && slot[l] - ua >= wn) --l;
                while (r < S && slot[r] - ua >= wn) ++r;
                TLS_CHECK(a, l >= 0 || r < S, kChkBiweight);   // (the window holds m >= need2 members: never both ends)
                double d;
                if (r >= S || (l >= 0 && loc - __longlong_as_double((long long)keys[l]) <=
                                             __longlong_as_double((long long)keys[r]) - loc)) {
                    d = loc - __longlong_as_double((long long)keys[l]);
                    --l;
                } else {
                    d = __longlong_as_double((long long)keys[r]) - loc;
                    ++r;
                }
                ++c;
                if (c == need1) d1 = d;
                if (c == need2) { d2 = d; break; }
            }
            const double mad = (m & 1u) ? d2 : (d1 + d2) / 2.0;
            if (mad == 0.0) break;   // (more than half the window sits on loc: keep it)
            const double s = TLS_BIWEIGHT_C * mad;
            double sw = 0.0, swv = 0.0;
            for (int j = wa; j < wb; ++j) {
                const double v = vals[j];
                if constexpr (MODE == kBiweightMasked) {
                    if (v < 0.0) continue;
                }
                const double u = (v - loc) / s;
                const double q = 1.0 - u * u;
                const double w = __builtin_fabs(u) < 1.0 ? q * q : 0.0;
                sw = sw + w;
                swv = swv + w * v;
            }
            const double nw = swv / sw;
            const bool done = __builtin_fabs(nw - loc) <= TLS_BIWEIGHT_FTOL * __builtin_fabs(nw);
            loc = nw;
            if (done) break;
        }
        a.flat[o] = y[g] / loc;
        if (a.trend) a.trend[o] = loc;
    }
}

// The unmasked kernel stays the text it was (not an instantiation of the tile above), so that its code and its time cannot
// move with the masked forms: a trace of an instantiation of the template ran 2 to 3 % behind the parent's kernel.
__global__ void __launch_bounds__(kDetrendThreads) tls_biweight_detrend(const BiweightArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned long long biweight_lds[];
    const int P = a.span, T = a.tile;
    unsigned long long* keys = biweight_lds;
    double* vals = reinterpret_cast<double*>(keys + P);
    unsigned int* slot = reinterpret_cast<unsigned int*>(vals + a.smax);
    const long long row = blockIdx.y;
    const long long first = (long long)blockIdx.x * T;
    const long long n_out = a.n - first < (long long)T ? a.n - first : (long long)T;
    const long long base = a.lo[first];
    const int S = (int)(a.hi[first + n_out - 1] - base);
    TLS_CHECK(a, S >= 1 && S <= a.smax && S <= P, kChkBiweight);
    const double* y = a.y + row * a.n;

    detrend_stage_sort(a, y, base, a.n, S, P, keys, slot, vals, kChkBiweight);

    for (int i = threadIdx.x; i < n_out; i += kDetrendThreads) {
        const long long g = first + i;
        const int wa = (int)(a.lo[g] - base), wb = (int)(a.hi[g] - base);   // the window's slots [wa, wb)
        TLS_CHECK(a, wa >= 0 && wa < wb && wb <= S, kChkBiweight);
        const unsigned int ua = (unsigned int)wa, m = (unsigned int)(wb - wa);
        // the ranks of the middle value(s): need1 == need2 for odd m
        const unsigned int need1 = (m + 1u) >> 1, need2 = (m >> 1) + 1u;

        // the median: the sorted slots in order, counting those inside the window
        int f1 = 0, f2 = 0;
        {
            unsigned int c = 0u;
            for (int j = 0; j < S; ++j) {
                if (slot[j] - ua < m) {
                    ++c;
                    if (c == need1) f1 = j;
                    if (c == need2) { f2 = j; break; }
                }
            }
        }
        TLS_CHECK(a, f1 < S && f2 < S, kChkBiweight);
        const double v1 = __longlong_as_double((long long)keys[f1]), v2 = __longlong_as_double((long long)keys[f2]);
        double loc = (m & 1u) ? v2 : (v1 + v2) / 2.0;

        for (int it = 0; it < TLS_BIWEIGHT_MAX_ITER; ++it) {
            // the MAD: p = the sorted slots with a key <= loc's (loc > 0: its bit pattern orders among the keys)
            const unsigned long long kl = (unsigned long long)__double_as_longlong(loc);
            int p0 = 0, p1 = S;
            while (p0 < p1) {
                const int mid = (p0 + p1) >> 1;
                if (keys[mid] <= kl) p0 = mid + 1; else p1 = mid;
            }
            int l = p0 - 1, r = p0;
            double d1 = 0.0, d2 = 0.0;
            unsigned int c = 0u;
            while (true) {
                while (l >= 0 && slot[l] - ua >= m) --l;
                while (r < S && slot[r] - ua >= m) ++r;
                TLS_CHECK(a, l >= 0 || r < S, kChkBiweight);   // (the window holds m >= need2 slots: never both ends)
                double d;
                if (r >= S || (l >= 0 && loc - __longlong_as_double((long long)keys[l]) <=
                                             __longlong_as_double((long long)keys[r]) - loc)) {
                    d = loc - __longlong_as_double((long long)keys[l]);
                    --l;
                } else {
                    d = __longlong_as_double((long long)keys[r]) - loc;
                    ++r;
                }
                ++c;
                if (c == need1) d1 = d;
                if (c == need2) { d2 = d; break; }
            }
            const double mad = (m & 1u) ? d2 : (d1 + d2) / 2.0;
            if (mad == 0.0) break;   // (more than half the window sits on loc: keep it)
            const double s = TLS_BIWEIGHT_C * mad;
            double sw = 0.0, swv = 0.0;
            for (int j = wa; j < wb; ++j) {
                const double v = vals[j];
                const double u = (v - loc) / s;
                const double q = 1.0 - u * u;
                const double w = __builtin_fabs(u) < 1.0 ? q * q : 0.0;
                sw = sw + w;
                swv = swv + w * v;
            }
            const double nw = swv / sw;
            const bool done = __builtin_fabs(nw - loc) <= TLS_BIWEIGHT_FTOL * __builtin_fabs(nw);
            loc = nw;
            if (done) break;
        }
        const long long o = row * a.n + g;
        a.flat[o] = y[g] / loc;
        if (a.trend) a.trend[o] = loc;
    }
}

__global__ void __launch_bounds__(kDetrendThreads) tls_biweight_detrend_masked(const BiweightMaskedArgs a) {
    biweight_tile<kBiweightMasked>(a);
}

__global__ void __launch_bounds__(kDetrendThreads) tls_biweight_detrend_fallback(const BiweightMaskedArgs a) {
    biweight_tile<kBiweightFallback>(a);
}

// The open points of the masked pass (status kBiweightOpen in `open`), one thread a point: a and b = the nearest points of
// status 0 to the left and right inside the point's segment (a new one starts at every j with t[j] - t[j-1] > break_tolerance).
// Both: trend = ta + (tb - ta) * ((t[i] - t[a]) / (t[b] - t[a])), ta where t[b] == t[a]; one: its value; status 1.  None: status
// 2, and tls_biweight_detrend_fallback forms trend and flat.  The runs of open points are short (a transit's length), so the
// walk is; `open` is only read and `status` only written here.
struct BiweightFillArgs {
    const double* t;              // [n]
    const double* y;              // [rows][n]
    double* flat;                 // [rows][n]
    double* trend;                // [rows][n]
    const unsigned char* open;    // [rows][n] the masked pass's status
    unsigned char* status;        // [rows][n] 0, 1 or 2
    long long n, count;           // count = rows * n
    double break_tolerance;
};

__global__ void __launch_bounds__(kDetrendThreads) tls_biweight_fill(const BiweightFillArgs a) {
#pragma clang fp contract(off)
    for (long long e = (long long)blockIdx.x * kDetrendThreads + threadIdx.x; e < a.count; e += (long long)gridDim.x * kDetrendThreads) {
        if (a.open[e] == 0) { a.status[e] = 0; continue; }
        const long long at = (e / a.n) * a.n, i = e - at;
        const unsigned char* open = a.open + at;
        long long l = i - 1, r = i + 1;
        bool left = false, right = false;
        for (; l >= 0 && !(a.t[l + 1] - a.t[l] > a.break_tolerance); --l)
            if (open[l] == 0) { left = true; break; }
        for (; r < a.n && !(a.t[r] - a.t[r - 1] > a.break_tolerance); ++r)
            if (open[r] == 0) { right = true; break; }
        if (!left && !right) { a.status[e] = 2; continue; }
        double tr;
        if (left && right) {
            const double ta = a.trend[at + l], tb = a.trend[at + r];
            const double den = a.t[r] - a.t[l];
            tr = ta;
            if (den != 0.0) {
                const double rise = tb - ta;
                const double num = a.t[i] - a.t[l];
                const double q = num / den;
                const double step = rise * q;
                tr = ta + step;
            }
        } else {
            tr = a.trend[at + (left ? l : r)];
        }
        a.trend[e] = tr;
        a.flat[e] = a.y[e] / tr;
        a.status[e] = 1;
    }
}
