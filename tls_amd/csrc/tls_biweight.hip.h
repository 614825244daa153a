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

// LDS: keys [P] (uint64) | values in index order [smax] (double) | slot numbers [P] (uint32), 12 P + 8 smax bytes.
// Grid (ceil(n / T), rows).
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
