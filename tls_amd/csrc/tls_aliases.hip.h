// tls_aliases.hip.h -- the period aliases of a pair of single-transit events (tls_event_periods).
//
// The statement (tests/event_periods_spec.py is the same in Python; include/tls_amd.h, DESIGN.md "Event periods"), for a pair
// (ca < cb, row r of width L and shape b, reach S, offset) on a curve's pairs (xw, w) = ((1 - y) w, 1 / (dy dy)):
//   window(c): h = (L - 1) / 2;  lo = c - h;  hi = lo + L - 1;  invalid if lo < 0 or hi > n - 1 or not (t[hi] - t[lo] <= span_max)
//              N = sum_j xw[lo+j] b[j];  D = sum_j w[lo+j] bb[j]                                     (ascending, from 0)
//   look(tc):  j = the sample nearest tc (the lower one on a tie);  shifts s = -S .. S ascending:  c = j + s
//              skip if c < 0 or c > n - 1, window(c) invalid, not (fabs(t[c] - tc) <= offset) or not (D > 0)
//              q = N / sqrt(D);  hold (q, N, D) if nothing is held or q > held q;  nothing held: uncovered
//   ta = t[ca];  tb = t[cb];  dT = tb - ta;  status 1 unless dT > 0;  A = look(ta);  B = look(tb)
//   status 2 unless both covered and pN = N_A + N_B > 0;  pD = D_A + D_B;  pair_depth = pN / pD;  pair_mes = pN / sqrt(pD)
//   k_hi = floor(dT / period_min);  status 3 if k_hi < 1;  n_evaluated = min(k_hi, max_aliases)
//   alias k:  P = dT / k;  e_first = ceil((t[0] - ta) / P);  e_last = floor((t[n-1] - ta) / P);  n_epochs = (e_last - e_first) + 1.0
//       every epoch e = e_first + i ascending:  tc = ta + e * P;  look(tc);  covered:  n_covered += 1;  SN = SN + N;  SD = SD + D
//           n_seen += 1 if q >= min_ses;  if e != 0 and e != k:  z = (pair_depth - N / D) * sqrt(D), the largest is worst_sigma
//       mes = SN / sqrt(SD);  depth = SN / SD;  allowed = not (worst_sigma > veto_sigma)
//   best = the allowed alias of the largest non-NaN mes (the smallest k on ties); longest / shortest = the smallest / largest allowed k
// Every step is one IEEE double operation (contraction off) and every sum runs in the stated order in ONE thread, so both records
// equal the host statement bit for bit.
//
// (1) tls_times_pairs_kernel (tls_times.hip.h) forms the pairs (xw, w) of every curve a slab of event pairs reads.
// (2) tls_alias_plane_kernel: all aliases of an event pair -- of every event pair of one (curve, row) group -- read the same
// windows, so (N(c), D(c)) is formed ONCE for every centre of the group, a double2 a centre with NaN in both halves where the
// window is invalid, and every (alias, epoch, shift) becomes a lookup.  It is the statistic loop of tls_single.hip.h for one
// row: a workgroup takes one group and a tile of kAliasTile centres, one a thread, stages the tile and the row's halo --
// (L - 1) / 2 slots in front, L / 2 behind, zero outside the series -- as pairs in the LDS, and step j of the row is one
// ds_read_b128 a lane at consecutive slots and two multiplies and two adds.  The chain is the statement's, so the bits are those
// of a direct walk.
// (3) tls_event_aliases_kernel: one workgroup of kAliasThreads threads an event pair.  Where n <= kAliasLdsPoints the time
// stamps and the group's plane lie in the LDS (24 n bytes; LDS = true); longer series are read from device memory, where the
// 24 n bytes stay in the L2 (LDS = false).  Every thread forms the pair's own two looks (the same values in every thread);
// thread i owns alias k = 256 p + i + 1 in pass p and walks its epochs in ascending order -- the bisection for the nearest
// sample, the shifts, the lookups, the ordered sums -- so no sum is ever split.  A thread keeps the best, the smallest and the
// largest allowed k and the count of its own aliases (its k ascend, so a strict > keeps the smallest k of equal mes); thread 0
// reduces the 256 partial results in thread order under the same rule, and the thread that owns the best alias writes its
// fields.  No floating-point atomics; the stores are plain vector stores.
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_times.hip.h.

constexpr int kAliasThreads = 256;
constexpr int kAliasTile = 256;                      // centres of a workgroup of the plane kernel, one a thread
constexpr int kAliasMax = 4096;                      // TLS_ALIAS_MAX
constexpr int kAliasMaxPoints = 1 << 20;
constexpr int kAliasPairWords = 16;                  // tls_event_pair
constexpr int kAliasWords = 8;                       // tls_event_alias
constexpr int kAliasLdsPoints = 6400;                // 24 bytes a point: 150 KiB of the 160, the rest for the reduction
static_assert(kAliasTile == kAliasThreads, "one centre a thread");

struct AliasPlaneArgs {
    const double* t;                                 // [n]
    const double2* pairs;                            // [slots][n] (xw, w)
    const SingleRow* rows;                           // [n_rows]
    const double* taps;                              // pairs (b[j], b[j] * b[j]), row after row
    const int* group_slot; const int* group_row;     // [groups] of the slab
    double2* plane;                                  // [groups][n] (N, D), NaN where the window is invalid
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    int n;
};

inline size_t alias_plane_lds_bytes(int max_width) { return (size_t)(kAliasTile + max_width - 1) * 16; }

__global__ void __launch_bounds__(kAliasThreads) tls_alias_plane_kernel(const AliasPlaneArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char alias_plane_lds[];
    double2* s = reinterpret_cast<double2*>(alias_plane_lds);      // [kAliasTile + L - 1] pairs (xw, w)
    const int tid = threadIdx.x, n = a.n;
    const int base = (int)blockIdx.x * kAliasTile;
    const long long g = blockIdx.y;
    const const_single_row_ptr rows = (const_single_row_ptr)a.rows;
    const int r = a.group_row[g];
    const int L = rows[r].width, h = (L - 1) / 2;
    const double span = rows[r].span_max;
    const double2* pw = a.pairs + (long long)a.group_slot[g] * n;
    const int slots = kAliasTile + L - 1;
    const int first = base - h;
    for (int k = tid; k < slots; k += kAliasThreads) {
        const int p = first + k;
        double2 v; v.x = 0.0; v.y = 0.0;
        if (p >= 0 && p < n) v = pw[p];
        s[k] = v;
    }
    wg_sync();
    const int c = base + tid;
    const int lo = c - h, hi = lo + L - 1;
    bool ok = lo >= 0 && hi <= n - 1;                // (hi <= n - 1 implies c < n)
    if (ok) {
        const double dt = a.t[hi] - a.t[lo];
        ok = dt <= span;
    }
    double2 out; out.x = (double)NAN; out.y = (double)NAN;
    if (ballot64(ok) != 0ull) {                      // (wave-uniform: some window of this wave is whole)
        TLS_CHECK(a, tid + L <= slots && L >= kSingleMinWidth && L <= kSingleMaxWidth, kChkTimes);
        const double2* win = s + tid;                // slot tid is sample c - h
        const const_f64_ptr q = (const_f64_ptr)a.taps + 2ll * rows[r].offset;
        double N = 0.0, D = 0.0;
#pragma unroll 8
        for (int j = 0; j < L; ++j) {
            const double2 v = win[j];
            const double nb = v.x * q[2 * j];
            const double db = v.y * q[2 * j + 1];
            N = N + nb;
            D = D + db;
        }
        if (ok) { out.x = N; out.y = D; }
    }
    if (c < n) a.plane[g * n + c] = out;
}

struct AliasArgs {
    const double* t;                                 // [n]
    const double2* plane;                            // [groups][n]
    const int* group; const int* reach;              // [pairs] of the slab
    const int* index_a; const int* index_b;          // [pairs]
    const double* offset;                            // [pairs]
    double* out;                                     // [pairs][kAliasPairWords]
    double* out_aliases;                             // [pairs][max_aliases][kAliasWords], or nullptr
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    double period_min, min_ses, veto_sigma;
    int n, max_aliases;
};

inline size_t alias_lds_bytes(int n) { return n <= kAliasLdsPoints ? (size_t)n * 24 : 0; }

struct AliasLook { bool held; double q, N, D; };

// look(tc) of the statement on the time stamps and the plane of the pair's group
__device__ __forceinline__ AliasLook alias_look(const double* t, const double2* plane, int n, int S, double offset, double tc) {
#pragma clang fp contract(off)
    int lo = 0, hi = n;                              // the first index with t[j] >= tc
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (t[mid] < tc) lo = mid + 1; else hi = mid;
    }
    int j = lo < n ? lo : n - 1;
    if (j > 0) {
        const double below = tc - t[j - 1], above = t[j] - tc;
        if (below <= above) --j;
    }
    AliasLook r; r.held = false; r.q = (double)NAN; r.N = (double)NAN; r.D = (double)NAN;
    const int c0 = j - S < 0 ? 0 : j - S, c1 = j + S > n - 1 ? n - 1 : j + S;
    for (int c = c0; c <= c1; ++c) {
        const double away = fabs(t[c] - tc);
        if (!(away <= offset)) continue;
        const double2 v = plane[c];
        if (!(v.y > 0.0)) continue;                  // (an invalid window holds NaN)
        const double q = v.x / sqrt(v.y);
        if (!r.held || q > r.q) { r.held = true; r.q = q; r.N = v.x; r.D = v.y; }
    }
    return r;
}

template <bool LDS>
__global__ void __launch_bounds__(kAliasThreads) tls_event_aliases_kernel(const AliasArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char alias_lds[];
    __shared__ double red_mes[kAliasThreads];
    __shared__ int red_best[kAliasThreads], red_low[kAliasThreads], red_high[kAliasThreads], red_count[kAliasThreads];
    __shared__ int red_owner;
    const int tid = threadIdx.x, n = a.n;
    const long long f = blockIdx.x;
    double* rec = a.out + f * kAliasPairWords;
    double* table = a.out_aliases ? a.out_aliases + f * (long long)a.max_aliases * kAliasWords : nullptr;
    const double nan = (double)NAN;
    const double2* gplane = a.plane + (long long)a.group[f] * n;
    const double* t = a.t;
    const double2* plane = gplane;
    if constexpr (LDS) {
        double2* lp = reinterpret_cast<double2*>(alias_lds);       // [n] pairs, then [n] time stamps
        double* lt = reinterpret_cast<double*>(alias_lds + (size_t)n * 16);
        TLS_CHECK(a, n <= kAliasLdsPoints, kChkTimes);
        for (int k = tid; k < n; k += kAliasThreads) { lp[k] = gplane[k]; lt[k] = a.t[k]; }
        wg_sync();
        t = lt; plane = lp;
    }
    const int S = a.reach[f], ca = a.index_a[f], cb = a.index_b[f];
    const double offset = a.offset[f];
    TLS_CHECK(a, S >= 1 && S <= kTimesMaxReach && ca >= 0 && ca < cb && cb < n, kChkTimes);
    // the pair (the same values in every thread)
    const double ta = t[ca], tb = t[cb];
    const double dT = tb - ta;
    int status = 1, n_eval = 0;
    double pair_mes = nan, pair_depth = nan, k_hi = nan;
    if (dT > 0.0) {
        status = 2;
        const AliasLook A = alias_look(t, plane, n, S, offset, ta), B = alias_look(t, plane, n, S, offset, tb);
        if (A.held && B.held) {
            const double pN = A.N + B.N, pD = A.D + B.D;
            pair_depth = pN / pD;
            pair_mes = pN / sqrt(pD);
            if (pN > 0.0) {
                k_hi = floor(dT / a.period_min);
                status = 3;
                if (k_hi >= 1.0) {
                    status = 0;
                    n_eval = k_hi < (double)a.max_aliases ? (int)k_hi : a.max_aliases;
                }
            }
        }
    }
    if (table)
        for (long long k = (long long)n_eval * kAliasWords + tid; k < (long long)a.max_aliases * kAliasWords; k += kAliasThreads)
            table[k] = nan;
    if (status != 0) {                               // (the whole workgroup leaves)
        if (tid < kAliasPairWords) {
            double v = nan;
            if (tid == 0) v = (double)status;
            else if (tid == 1) v = dT;
            else if (tid == 5) v = pair_mes;
            else if (tid == 6) v = pair_depth;
            else if (status == 3 && tid == 2) v = k_hi;
            else if (status == 3 && (tid == 3 || tid == 4)) v = 0.0;
            rec[tid] = v;
        }
        return;
    }
    const double lead = t[0] - ta, tail = t[n - 1] - ta;
    // this thread's aliases, k ascending
    double my_mes = nan, my_period = nan, my_covered = nan, my_seen = nan;
    int my_best = 0, my_low = 0, my_high = 0, my_count = 0;
    for (int k = tid + 1; k <= n_eval; k += kAliasThreads) {
        const double kd = (double)k;
        const double P = dT / kd;
        const double e_first = ceil(lead / P);
        const double e_last = floor(tail / P);
        const double n_epochs = (e_last - e_first) + 1.0;
        const int ne = n_epochs >= 1.0 ? (int)n_epochs : 0;
        TLS_CHECK(a, n_epochs >= 1.0 && n_epochs <= (double)kTimesMaxEpochs, kChkTimes);
        double SN = 0.0, SD = 0.0, worst_sigma = nan, worst_epoch = nan;
        int n_covered = 0, n_seen = 0;
        for (int i = 0; i < ne; ++i) {
            const double e = e_first + (double)i;
            const double ahead = e * P;
            const double tc = ta + ahead;
            const AliasLook r = alias_look(t, plane, n, S, offset, tc);
            if (!r.held) continue;
            ++n_covered;
            SN = SN + r.N;
            SD = SD + r.D;
            if (r.q >= a.min_ses) ++n_seen;
            if (e != 0.0 && e != kd) {
                const double d = r.N / r.D;
                const double short_of = pair_depth - d;
                const double z = short_of * sqrt(r.D);
                if (isnan(worst_sigma) || z > worst_sigma) { worst_sigma = z; worst_epoch = e; }
            }
        }
        const double mes = SN / sqrt(SD);
        const double depth = SN / SD;
        if (table) {
            double* o = table + (long long)(k - 1) * kAliasWords;
            o[0] = P; o[1] = n_epochs; o[2] = (double)n_covered; o[3] = (double)n_seen;
            o[4] = mes; o[5] = depth; o[6] = worst_sigma; o[7] = worst_epoch;
        }
        if (worst_sigma > a.veto_sigma) continue;    // (NaN: allowed)
        ++my_count;
        if (my_low == 0) my_low = k;
        my_high = k;
        if (!isnan(mes) && (my_best == 0 || mes > my_mes)) {
            my_best = k; my_mes = mes; my_period = P; my_covered = (double)n_covered; my_seen = (double)n_seen;
        }
    }
    red_mes[tid] = my_mes; red_best[tid] = my_best; red_low[tid] = my_low; red_high[tid] = my_high; red_count[tid] = my_count;
    wg_sync();
    if (tid == 0) {
        int owner = -1, best = 0, low = 0, high = 0, count = 0;
        double mes = nan;
        for (int i = 0; i < kAliasThreads; ++i) {
            count += red_count[i];
            if (red_low[i] != 0 && (low == 0 || red_low[i] < low)) low = red_low[i];
            if (red_high[i] > high) high = red_high[i];
            const int k = red_best[i];
            if (k != 0 && (best == 0 || red_mes[i] > mes || (red_mes[i] == mes && k < best))) { best = k; mes = red_mes[i]; owner = i; }
        }
        red_owner = owner;
        rec[0] = 0.0; rec[1] = dT; rec[2] = k_hi; rec[3] = (double)n_eval; rec[4] = (double)count;
        rec[5] = pair_mes; rec[6] = pair_depth;
        if (owner < 0) { rec[7] = nan; rec[8] = nan; rec[9] = nan; rec[10] = nan; rec[11] = nan; }
        rec[12] = low ? (double)low : nan;
        rec[13] = low ? dT / (double)low : nan;
        rec[14] = high ? (double)high : nan;
        rec[15] = high ? dT / (double)high : nan;
    }
    wg_sync();
    if (tid == red_owner) { rec[7] = (double)my_best; rec[8] = my_period; rec[9] = my_mes; rec[10] = my_covered; rec[11] = my_seen; }
}
