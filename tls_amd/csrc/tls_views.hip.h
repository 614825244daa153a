// tls_views.hip.h -- the phase-folded, median-binned views of a candidate (tls_folded_views): the global and local views of
// Shallue & Vanderburg (2018), the odd, even and secondary local views of Valizadegan et al. (2022).
//
// The statement (tests/folded_views_spec.py is the same in Python; include/tls_amd.h, DESIGN.md "Folded views"), for a
// candidate (P, T0, d in days, phi_s) on a curve's row y over t, and a view (phi_c, x_min, x_max, w, B, parity):
//   points, i ascending:  x = (t[i] - T0) / P;  u = x - phi_c;  e = floor(u + 0.5);  tau = (u - e) * P
//   bin b:  s = ((x_max - x_min) - w) / (B - 1);  lo = b * s + x_min;  hi = lo + w;  member iff lo <= tau and tau < hi
//           (and, with a parity, e - 2.0 * floor(e / 2.0) == parity)
//   count[b] = the members;  median[b] = the middle member by value, (a + b) / 2 of the two middle ones, NaN without one
//   n_members = the points that are a member of at least one bin
//   global (0, -0.5 P, 0.5 P, P / n_global, n_global, -);  local (0, -k d, k d, width d, n_local, -), local_even and
//   local_odd the same with parity 0 and 1, secondary the same about phi_c = phi_s
//   status 1 (every median NaN, every count 0) unless P, T0, d finite, P > 0, d > 0;  the secondary view alone is NaN / 0
//   where phi_s is not finite (or there is none)
// Every step is one IEEE double operation (contraction off); a median is a selection, so the record and the arrays equal the
// host statement bit for bit.
//
// tls_folded_views_kernel: one workgroup of kViewsThreads threads a candidate (a launch of fewer workgroups than candidates
// strides over them, so the scratch below is one stretch a WORKGROUP).  Per centre (0, then phi_s):
// (1) The points: (tau, y, class) of every point, a thread a point, the class 0 for an even e and 1 for an odd one (about phi_s
// every point is class 0); a tau that is NaN (u overflowed) is kept as +inf, which no bin holds.  Up to kViewsLdsPoints points
// live in the LDS (17 bytes each: two workgroups a CU); a longer series lives in the workgroup's stretch of device scratch,
// and the same code runs on it.
// (2) The order: a bitonic network whose comparators all put the smaller (class, tau) at the lower index, so the places at
// and beyond n count as +inf and a comparator that reaches them is skipped -- any n, no padding.  Behind it the even points
// stand in front of the odd ones, each part ascending in tau, so the members of a bin are ONE contiguous range of a part:
// [first place with lo <= tau, first place with not tau < hi) -- the statement's own two comparisons, in a binary search that
// they keep monotone -- and a view without a parity takes the ranges of both parts.  lo and hi do not fall with b, so the
// points of a part that some bin holds are counted range by range, each behind the end of the range before it.
// (3) The medians: a wave takes 64 bins at a time, a lane a bin for the ranges.  A bin of up to kViewsLaneMembers members is
// selected by its lane alone; a larger one by the whole wave, the lanes striding over its members: the rank of a member is
// the number of smaller ones plus the equal ones at lower places, every lane reading the same member in the same step (one
// LDS address a wave: a broadcast), and the members of ranks (c - 1) / 2 and c / 2 are the middle.  Ranks need no order among
// the members, so no bin is ever sorted by value and no bin population has a path of its own.
// Included by tls_kernels.hip.h (namespace tlsdev).

constexpr int kViewsThreads = 256;
constexpr int kViewsWaves = kViewsThreads / kWave;
constexpr int kViewsLdsPoints = 4608;                // points the LDS holds: 17 bytes each, two workgroups a CU
constexpr int kViewsLaneMembers = 8;                 // a bin of up to this many members is selected by one lane
constexpr int kViewsMaxPoints = 1 << 20;
constexpr int kViewsMaxBins = 1 << 16;
constexpr int kViewsSlab = 1024;                     // candidates of a launch at most
constexpr int kViewsMaxGroups = 1024;                // workgroups of a launch at most (each owns a stretch of scratch)
constexpr int kViewsWords = 7;                       // tls_views_record
constexpr int kViewsLocal = 4;                       // local, local_even, local_odd, secondary

struct ViewsArgs {
    const double* t;                                 // [n]
    const double* y;                                 // [slots][n]
    const int* slot;                                 // [fits] of the slab
    const double* period; const double* T0; const double* duration;   // [fits]
    const double* secondary;                         // [fits] phi_s (nullptr: no secondary view)
    double* scratch;                                 // [workgroups][views_scratch_words(n)]: tau | y | class, where n > kViewsLdsPoints
    double* out;                                     // [fits][kViewsWords]
    double* global_median; int* global_count;        // [fits][n_global]
    double* local_median; int* local_count;          // [fits][kViewsLocal][n_local]
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    double k, width;
    int n, fits, n_global, n_local;
};

// doubles of a workgroup's stretch of scratch: tau [n], y [n] and a byte a point
__host__ __device__ inline size_t views_scratch_words(size_t n) { return 2 * n + (n + 7) / 8; }

// first place of [from, to) whose tau is not below lo (lower) or not below hi as the statement asks it: not (tau < hi)
__device__ __forceinline__ int views_lower(const double* tau, int from, int to, double lo) {
    while (from < to) {
        const int mid = from + ((to - from) >> 1);
        if (lo <= tau[mid]) to = mid; else from = mid + 1;
    }
    return from;
}

__device__ __forceinline__ int views_upper(const double* tau, int from, int to, double hi) {
    while (from < to) {
        const int mid = from + ((to - from) >> 1);
        if (tau[mid] < hi) from = mid + 1; else to = mid;
    }
    return from;
}

// the rank of (v, place) among the members y[a1, e1) and y[a2, e2): the smaller ones and the equal ones at lower places
__device__ __forceinline__ int views_rank(const double* y, int a1, int e1, int a2, int e2, double v, int place) {
    int rank = 0;
    for (int j = a1; j < e1; ++j) { const double o = y[j]; rank += (o < v || (o == v && j < place)) ? 1 : 0; }
    for (int j = a2; j < e2; ++j) { const double o = y[j]; rank += (o < v || (o == v && j < place)) ? 1 : 0; }
    return rank;
}

// One view of the ordered points: parts [b1, n1) and [b2, n2) (the second empty for a view with a parity), the table
// (x_min, x_max, w, B); medians and counts to med, cnt [B]; the points some bin holds are added to *members (an LDS word).
__device__ __forceinline__ void views_bin(const ViewsArgs& a, const double* tau, const double* y, int b1, int n1, int b2, int n2,
                                          double x_min, double x_max, double w, int B, double* med, int* cnt, int* members) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const double nan = (double)NAN;
    const double range = x_max - x_min;
    const double room = range - w;
    const double s = room / (double)(B - 1);
    int held = 0;
    for (int b0 = wave * kWave; b0 < B; b0 += kViewsThreads) {
        const int b = b0 + lane;
        int a1 = b1, e1 = b1, a2 = b2, e2 = b2;
        if (b < B) {
            const double step = (double)b * s;
            const double lo = step + x_min;
            const double hi = lo + w;
            a1 = views_lower(tau, b1, n1, lo);
            e1 = views_upper(tau, b1, n1, hi);
            a2 = views_lower(tau, b2, n2, lo);
            e2 = views_upper(tau, b2, n2, hi);
            if (e1 < a1) e1 = a1;
            if (e2 < a2) e2 = a2;
            int p1 = b1, p2 = b2;                    // the ends of the bin before
            if (b > 0) {
                const double step_p = (double)(b - 1) * s;
                const double lo_p = step_p + x_min;
                const double hi_p = lo_p + w;
                p1 = views_upper(tau, b1, n1, hi_p);
                p2 = views_upper(tau, b2, n2, hi_p);
            }
            const int f1 = a1 > p1 ? a1 : p1, f2 = a2 > p2 ? a2 : p2;
            held += (e1 > f1 ? e1 - f1 : 0) + (e2 > f2 ? e2 - f2 : 0);
            TLS_CHECK(a, a1 >= b1 && e1 <= n1 && a2 >= b2 && e2 <= n2, kChkViews);
        }
        const int c = (e1 - a1) + (e2 - a2);
        if (b < B && c <= kViewsLaneMembers) {       // the lane's own bin
            double m_lo = nan, m_hi = nan;
            const int k_lo = (c - 1) >> 1, k_hi = c >> 1;
            for (int m = 0; m < c; ++m) {
                const int place = m < e1 - a1 ? a1 + m : a2 + (m - (e1 - a1));
                const double v = y[place];
                const int rank = views_rank(y, a1, e1, a2, e2, v, place);
                if (rank == k_lo) m_lo = v;
                if (rank == k_hi) m_hi = v;
            }
            double median = nan;
            if (c > 0) {
                const double sum = m_lo + m_hi;
                median = (c & 1) ? m_lo : sum / 2.0;
            }
            med[b] = median;
            cnt[b] = c;
        }
        // the larger bins of the 64, one after the other, by the whole wave
        unsigned long long large = __ballot(b < B && c > kViewsLaneMembers);
        while (large) {
            const int src = __ffsll((long long)large) - 1;
            large &= large - 1ull;
            const int wa1 = __shfl(a1, src), we1 = __shfl(e1, src), wa2 = __shfl(a2, src), we2 = __shfl(e2, src);
            const int c1 = we1 - wa1, wc = c1 + (we2 - wa2);
            const int k_lo = (wc - 1) >> 1, k_hi = wc >> 1;
            double m_lo = 0.0, m_hi = 0.0;
            bool has_lo = false, has_hi = false;
            for (int m = lane; m < wc; m += kWave) {
                const int place = m < c1 ? wa1 + m : wa2 + (m - c1);
                TLS_CHECK(a, place >= 0 && place < a.n, kChkViews);
                const double v = y[place];
                const int rank = views_rank(y, wa1, we1, wa2, we2, v, place);
                if (rank == k_lo) { m_lo = v; has_lo = true; }
                if (rank == k_hi) { m_hi = v; has_hi = true; }
            }
            const unsigned long long at_lo = __ballot(has_lo), at_hi = __ballot(has_hi);
            TLS_CHECK(a, __popcll(at_lo) == 1 && __popcll(at_hi) == 1, kChkViews);
            const double v_lo = __shfl(m_lo, __ffsll((long long)at_lo) - 1);
            const double v_hi = __shfl(m_hi, __ffsll((long long)at_hi) - 1);
            if (lane == src) {
                const double sum = v_lo + v_hi;
                med[b] = (wc & 1) ? v_lo : sum / 2.0;
                cnt[b] = wc;
            }
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) held += __shfl_down(held, off);
    if (lane == 0 && held) atomicAdd(members, held);
}

// The candidate on the points' arrays (the LDS, or the workgroup's scratch): tau, y [n], cls [n]; words: LDS ints
// [0] and [6] the even points of the two centres, [1 .. 5] the members of the five views.
__device__ __forceinline__ void views_candidate(const ViewsArgs& a, long long f, double* tau, double* yy, unsigned char* cls,
                                                int* words, double P, double T0, double d, double phi_s, bool secondary) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, n = a.n;
    const double* row = a.y + (long long)a.slot[f] * n;
    const double kd = a.k * d;
    const double w_local = a.width * d;
    const double half = 0.5 * P;
    const double w_global = P / (double)a.n_global;
    double* l_med = a.local_median + f * kViewsLocal * a.n_local;
    int* l_cnt = a.local_count + f * kViewsLocal * a.n_local;
    for (int centre = 0; centre < (secondary ? 2 : 1); ++centre) {
        const double phi_c = centre ? phi_s : 0.0;
        // (1) the points
        int even = 0;
        for (int i = tid; i < n; i += kViewsThreads) {
            const double lead = a.t[i] - T0;
            const double x = lead / P;
            const double u = x - phi_c;
            const double uh = u + 0.5;
            const double e = floor(uh);
            const double ph = u - e;
            const double ta = ph * P;
            const double eh = e / 2.0;
            const double fl = floor(eh);
            const double twice = 2.0 * fl;
            const double parity = e - twice;
            const bool odd = centre == 0 && parity == 1.0;
            // (a point of neither parity -- e overflowed -- has a NaN tau: no bin holds it, in whichever part it stands)
            tau[i] = ta != ta ? (double)INFINITY : ta;
            yy[i] = row[i];
            cls[i] = odd ? 1 : 0;
            even += odd ? 0 : 1;
        }
        for (int off = kWave / 2; off > 0; off >>= 1) even += __shfl_down(even, off);
        if ((tid & (kWave - 1)) == 0 && even) atomicAdd(&words[centre ? 6 : 0], even);
        wg_sync();
        // (2) the order: every comparator puts the smaller (class, tau) at the lower place
        for (int k = 2; (k >> 1) < n; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                const int mask = (j == (k >> 1)) ? k - 1 : j;
                for (int i = tid; i < n; i += kViewsThreads) {
                    const int l = i ^ mask;
                    if (l > i && l < n) {
                        const unsigned char ci = cls[i], cl = cls[l];
                        const double ti = tau[i], tl = tau[l];
                        if (cl < ci || (cl == ci && tl < ti)) {
                            const double yi = yy[i], yl = yy[l];
                            tau[i] = tl; tau[l] = ti; yy[i] = yl; yy[l] = yi; cls[i] = cl; cls[l] = ci;
                        }
                    }
                }
                wg_sync();
            }
        }
        const int n_even = words[centre ? 6 : 0];
        TLS_CHECK(a, n_even >= 0 && n_even <= n, kChkViews);
        // (3) the views
        if (centre == 0) {
            views_bin(a, tau, yy, 0, n_even, n_even, n, -half, half, w_global, a.n_global, a.global_median + f * a.n_global,
                      a.global_count + f * a.n_global, &words[1]);
            views_bin(a, tau, yy, 0, n_even, n_even, n, -kd, kd, w_local, a.n_local, l_med, l_cnt, &words[2]);
            views_bin(a, tau, yy, 0, n_even, n_even, n_even, -kd, kd, w_local, a.n_local, l_med + a.n_local, l_cnt + a.n_local,
                      &words[3]);
            views_bin(a, tau, yy, n_even, n, n, n, -kd, kd, w_local, a.n_local, l_med + 2 * a.n_local, l_cnt + 2 * a.n_local,
                      &words[4]);
        } else {
            views_bin(a, tau, yy, 0, n, n, n, -kd, kd, w_local, a.n_local, l_med + 3 * a.n_local, l_cnt + 3 * a.n_local, &words[5]);
        }
        wg_sync();                                   // (the points have been read; the counts are in)
    }
}

__global__ void __launch_bounds__(kViewsThreads) tls_folded_views_kernel(const ViewsArgs a) {
#pragma clang fp contract(off)
    __shared__ double m_tau[kViewsLdsPoints];
    __shared__ double m_y[kViewsLdsPoints];
    __shared__ unsigned char m_cls[kViewsLdsPoints];
    __shared__ int words[8];
    const int tid = threadIdx.x, n = a.n;
    const double nan = (double)NAN;
    double* s_tau = a.scratch + (size_t)blockIdx.x * views_scratch_words((size_t)n);
    double* s_y = s_tau + n;
    unsigned char* s_cls = reinterpret_cast<unsigned char*>(s_y + n);
    TLS_CHECK(a, a.n_global >= 2 && a.n_local >= 2 && n >= 1, kChkViews);
    for (long long f = blockIdx.x; f < a.fits; f += gridDim.x) {
        double* o = a.out + f * kViewsWords;
        const double P = a.period[f], T0 = a.T0[f], d = a.duration[f];
        const double phi_s = a.secondary ? a.secondary[f] : nan;
        const bool good = isfinite(P) && isfinite(T0) && isfinite(d) && P > 0.0 && d > 0.0;   // (the whole workgroup)
        const bool secondary = good && isfinite(phi_s);
        if (tid < 8) words[tid] = 0;
        // what is not binned: NaN and 0
        if (!good) {
            for (int b = tid; b < a.n_global; b += kViewsThreads) { a.global_median[f * a.n_global + b] = nan; a.global_count[f * a.n_global + b] = 0; }
        }
        for (int v = good ? kViewsLocal - 1 : 0; v < (secondary ? 0 : kViewsLocal); ++v) {
            for (int b = tid; b < a.n_local; b += kViewsThreads) {
                a.local_median[(f * kViewsLocal + v) * a.n_local + b] = nan;
                a.local_count[(f * kViewsLocal + v) * a.n_local + b] = 0;
            }
        }
        wg_sync();
        if (good) {
            if (n <= kViewsLdsPoints) views_candidate(a, f, m_tau, m_y, m_cls, words, P, T0, d, phi_s, secondary);
            else views_candidate(a, f, s_tau, s_y, s_cls, words, P, T0, d, phi_s, secondary);
        }
        if (tid == 0) {
            o[0] = good ? 0.0 : 1.0;
            o[1] = secondary ? 0.0 : 1.0;
            for (int v = 0; v < 5; ++v) o[2 + v] = (double)words[1 + v];
        }
        wg_sync();                                   // (the next candidate overwrites the LDS, its words and the scratch)
    }
}
