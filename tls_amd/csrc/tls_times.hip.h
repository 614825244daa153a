// tls_times.hip.h -- individual transit times and the refitted ephemeris of a candidate (tls_transit_times).
//
// The statement (tests/transit_times_spec.py is the same in Python; include/tls_amd.h, DESIGN.md "Transit times"), for a
// candidate (P, T0, row r of width L and shape b, reach S) on a curve's pairs (xw, w) = ((1 - y) w, 1 / (dy dy)):
//   status 1 unless P, T0 finite and P > 0;  e_first = ceil((t[0] - T0) / P);  e_last = floor((t[n-1] - T0) / P)
//   n_epochs = (e_last - e_first) + 1.0;  status 2 unless 1 <= n_epochs <= max_epochs
//   every epoch e = e_first + i:  tc = T0 + e * P;  j = the sample nearest tc (the lower one on a tie)
//       shifts s = -S .. S ascending:  c = j + s;  h = (L - 1) / 2;  lo = c - h;  hi = lo + L - 1
//           skip if lo < 0 or hi > n - 1 or not (t[hi] - t[lo] <= span_max)
//           N = sum_k xw[lo+k] b[k];  D = sum_k w[lo+k] bb[k];  d = N / D;  skip if not (d > depth_min)
//           q = N / sqrt(D);  hold (q, d, c, lo) if nothing is held or q > held q
//       status 1 (nothing held), 3 (not q >= min_ses), 2 (c at an end of the series), else one Gauss-Newton step of the shift:
//           H = sum_k xw[lo+k] g[k];  Bg = sum_k w[lo+k] bg[k];  G = sum_k w[lo+k] gg[k];  delta = (d Bg - H) / (d G)
//           step = 0.5 (t[c+1] - t[c-1]);  status 2 if not (fabs(delta) <= 1);  time = tm + delta step;  time_err = step / (d sqrt(G))
//   the weighted straight line through (e, time - T0) of the status-0 epochs, ascending, and its residuals.
// Every step is one IEEE double operation (contraction off) and every sum runs in index order in ONE thread, so both records
// equal the host statement bit for bit.
//
// (1) tls_times_pairs_kernel forms the pairs (xw, w) of every curve a slab of candidates reads, once a curve, 16 bytes a
// point -- the layout the single-transit kernel stages in its LDS.
// (2) tls_transit_times_kernel: one workgroup of kTimesThreads threads a candidate.  The epochs are taken in chunks whose
// (epoch, shift) units fit the LDS: kTimesLdsUnits = 2 * 4096 + 1 doubles hold the widest reach of one epoch, so no chunk
// needs scratch in device memory whatever n_epochs * (2S+1) is.  A chunk is three passes between barriers: (a) a thread an
// epoch finds the nearest sample by bisection; (b) the units are dealt to the threads, unit u = epoch * (2S+1) + shift to
// thread u mod kTimesThreads -- neighbouring lanes walk neighbouring windows, so step k of a wave reads consecutive pairs,
// one global_load_dwordx4 a lane, served by the L2 after the first touch -- and a thread walks its window in index order and
// leaves q in the LDS (NaN: skipped; a held q is never NaN, since d > depth_min >= 0 needs N > 0 and D >= 0 without a NaN);
// (c) a thread an epoch picks over its shifts in ascending order, walks the picked window once more for N, D (the same chain,
// the same bits) and H, Bg, G, and writes the epoch's record.  The taps (b, bb) and (g, bg, gg) of the row are the same for
// the whole workgroup and come through the constant address space into scalar registers.  Behind the last chunk thread 0
// reads the records back (wg_sync's release and acquire fences order the other threads' stores in front of it) and forms the
// ephemeris.
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_single.hip.h (SingleRow).

constexpr int kTimesThreads = 256;
constexpr int kTimesMaxReach = 4096;
constexpr int kTimesMaxEpochs = 65536;
constexpr int kTimesMaxPoints = 1 << 30;
constexpr int kTimesEphemerisWords = 12;             // tls_ephemeris
constexpr int kTimesTimeWords = 8;                   // tls_transit_time
constexpr int kTimesLdsUnits = 2 * kTimesMaxReach + 1;   // q values of a chunk: one epoch of the widest reach at least
constexpr int kTimesChunkEpochs = 1024;              // epochs of a chunk at most (their nearest samples lie in the LDS)

struct TimesPairsArgs {
    const double* y; const double* dy;               // [slots][n]
    double2* pairs;                                  // [slots][n]
    long long count;                                 // slots * n
};

__global__ void __launch_bounds__(kTimesThreads) tls_times_pairs_kernel(const TimesPairsArgs a) {
#pragma clang fp contract(off)
    const long long stride = (long long)gridDim.x * kTimesThreads;
    for (long long p = (long long)blockIdx.x * kTimesThreads + threadIdx.x; p < a.count; p += stride) {
        const double e = a.dy[p];
        const double w = 1.0 / (e * e);
        double2 v;
        v.x = (1.0 - a.y[p]) * w;
        v.y = w;
        a.pairs[p] = v;
    }
}

struct TimesArgs {
    const double* t;                                 // [n]
    const double2* pairs;                            // [slots][n] (xw, w)
    const SingleRow* rows;                           // [n_rows]
    const double* taps;                              // pairs (b[j], b[j] * b[j]), row after row
    const double* slopes;                            // triples (g[j], b[j] * g[j], g[j] * g[j]), row after row
    const int* slot; const int* row; const int* reach;   // [fits] of the slab
    const double* period; const double* T0;          // [fits]
    double* out;                                     // [fits][kTimesEphemerisWords]
    double* out_times;                               // [fits][max_epochs][kTimesTimeWords]
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    double depth_min, min_ses;
    int n, max_epochs;
};

// the epochs of a chunk for reach S, and the LDS of a launch whose widest reach is S
__host__ __device__ inline int times_chunk_epochs(int reach) {
    const int fit = kTimesLdsUnits / (2 * reach + 1);
    return fit < 1 ? 1 : fit < kTimesChunkEpochs ? fit : kTimesChunkEpochs;
}
inline size_t times_lds_bytes(int reach, int max_epochs) {
    return (size_t)std::min(times_chunk_epochs(reach), max_epochs) * (size_t)(2 * reach + 1) * 8;
}

__global__ void __launch_bounds__(kTimesThreads) tls_transit_times_kernel(const TimesArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char times_lds[];
    __shared__ int centre[kTimesChunkEpochs];
    double* qs = reinterpret_cast<double*>(times_lds);             // [epochs of the chunk][2S+1]
    const int tid = threadIdx.x, n = a.n;
    const long long f = blockIdx.x;
    double* eph = a.out + f * kTimesEphemerisWords;
    double* rec = a.out_times + f * (long long)a.max_epochs * kTimesTimeWords;
    const double P = a.period[f], T0 = a.T0[f];
    const double nan = (double)NAN;
    // the candidate's epochs (the same values in every thread)
    int status = 1;
    double first = nan, count = nan;
    if (isfinite(P) && isfinite(T0) && P > 0.0) {
        const double lead = a.t[0] - T0, tail = a.t[n - 1] - T0;
        first = ceil(lead / P);
        const double last = floor(tail / P);
        count = (last - first) + 1.0;
        status = (count >= 1.0 && count <= (double)a.max_epochs) ? 0 : 2;
    }
    const int ne = status == 0 ? (int)count : 0;
    for (long long k = (long long)ne * kTimesTimeWords + tid; k < (long long)a.max_epochs * kTimesTimeWords; k += kTimesThreads)
        rec[k] = nan;
    if (status != 0) {                               // (the whole workgroup leaves)
        if (tid < kTimesEphemerisWords) eph[tid] = tid == 0 ? (double)status : (tid == 1 && status == 2) ? count : nan;
        return;
    }
    const const_single_row_ptr rows = (const_single_row_ptr)a.rows;
    const int r = a.row[f];
    const int L = rows[r].width, h = (L - 1) / 2;
    const double span = rows[r].span_max;
    const int S = a.reach[f], U = 2 * S + 1;
    const const_f64_ptr taps = (const_f64_ptr)a.taps + 2ll * rows[r].offset;
    const const_f64_ptr slopes = (const_f64_ptr)a.slopes + 3ll * rows[r].offset;
    const double2* pw = a.pairs + (long long)a.slot[f] * n;
    const int chunk = times_chunk_epochs(S);
    TLS_CHECK(a, S >= 1 && S <= kTimesMaxReach && L >= kSingleMinWidth && L <= kSingleMaxWidth, kChkTimes);
    for (int e0 = 0; e0 < ne; e0 += chunk) {
        const int ec = ne - e0 < chunk ? ne - e0 : chunk;
        // (a) the nearest sample of every epoch of the chunk
        for (int i = tid; i < ec; i += kTimesThreads) {
            const double e = first + (double)(e0 + i);
            const double ahead = e * P;
            const double tc = T0 + ahead;
            int lo = 0, hi = n;                      // the first index with t[j] >= tc
            while (lo < hi) {
                const int mid = lo + (hi - lo) / 2;
                if (a.t[mid] < tc) lo = mid + 1; else hi = mid;
            }
            int j = lo < n ? lo : n - 1;
            if (j > 0) {
                const double below = tc - a.t[j - 1], above = a.t[j] - tc;
                if (below <= above) --j;
            }
            centre[i] = j;
        }
        wg_sync();
        // (b) q of every (epoch, shift) unit of the chunk
        const int units = ec * U;
        for (int u = tid; u < units; u += kTimesThreads) {
            const int i = u / U, s = u - i * U;
            const int c = centre[i] + (s - S);
            const int lo = c - h, hi = lo + L - 1;
            double q = nan;
            bool whole = lo >= 0 && hi <= n - 1;
            if (whole) {
                const double dt = a.t[hi] - a.t[lo];
                whole = dt <= span;
            }
            if (whole) {
                const double2* win = pw + lo;
                double N = 0.0, D = 0.0;
#pragma unroll 4
                for (int k = 0; k < L; ++k) {
                    const double2 v = win[k];
                    const double nb = v.x * taps[2 * k];
                    const double db = v.y * taps[2 * k + 1];
                    N = N + nb;
                    D = D + db;
                }
                const double d = N / D;
                if (d > a.depth_min) q = N / sqrt(D);
            }
            qs[u] = q;
        }
        wg_sync();
        // (c) the pick over the shifts and the record of every epoch of the chunk
        for (int i = tid; i < ec; i += kTimesThreads) {
            const double e = first + (double)(e0 + i);
            const double ahead = e * P;
            const double tc = T0 + ahead;
            double* o = rec + (long long)(e0 + i) * kTimesTimeWords;
            int best = -1;
            double q = nan;
            for (int s = 0; s < U; ++s) {
                const double v = qs[i * U + s];
                if (!isnan(v) && (best < 0 || v > q)) { q = v; best = s; }
            }
            double state = 1.0, time = nan, time_err = nan, d = nan, index = nan;
            if (best >= 0) {
                const int c = centre[i] + (best - S);
                const int lo = c - h;
                TLS_CHECK(a, lo >= 0 && lo + L - 1 <= n - 1, kChkTimes);
                const double2* win = pw + lo;
                double N = 0.0, D = 0.0, H = 0.0, Bg = 0.0, G = 0.0;
                for (int k = 0; k < L; ++k) {
                    const double2 v = win[k];
                    const double nb = v.x * taps[2 * k];
                    const double db = v.y * taps[2 * k + 1];
                    const double hb = v.x * slopes[3 * k];
                    const double bgb = v.y * slopes[3 * k + 1];
                    const double gb = v.y * slopes[3 * k + 2];
                    N = N + nb;
                    D = D + db;
                    H = H + hb;
                    Bg = Bg + bgb;
                    G = G + gb;
                }
                d = N / D;
                index = (double)c;
                const double centre_sum = a.t[lo + h] + a.t[lo + L - 1 - h];
                const double tm = 0.5 * centre_sum;
                if (!(q >= a.min_ses)) {
                    state = 3.0;
                } else if (c - 1 < 0 || c + 1 > n - 1) {
                    // (the statement's check; never taken: a whole window has (L - 1) / 2 >= 1 samples in front of c and L / 2 >= 1 behind)
                    state = 2.0;
                } else {
                    const double dBg = d * Bg;
                    const double num = dBg - H;
                    const double den = d * G;
                    const double delta = num / den;
                    const double around = a.t[c + 1] - a.t[c - 1];
                    const double step = 0.5 * around;
                    if (!(fabs(delta) <= 1.0)) {
                        state = 2.0;
                    } else {
                        state = 0.0;
                        const double moved = delta * step;
                        time = tm + moved;
                        const double scale = d * sqrt(G);
                        time_err = step / scale;
                    }
                }
            }
            o[0] = e; o[1] = state; o[2] = tc; o[3] = time; o[4] = time_err; o[5] = q; o[6] = d; o[7] = index;
        }
        wg_sync();                                   // (the next chunk overwrites centre and qs; thread 0 reads the records)
    }
    if (tid != 0) return;
    // the ephemeris: the weighted line through (e, time - T0) of the timed epochs, ascending
    int timed = 0;
    double Sw = 0.0, Se = 0.0, See = 0.0, St = 0.0, Set = 0.0;
    for (int i = 0; i < ne; ++i) {
        const double* o = rec + (long long)i * kTimesTimeWords;
        if (o[1] != 0.0) continue;
        ++timed;
        const double err = o[4], x = o[0];
        const double err2 = err * err;
        const double wgt = 1.0 / err2;
        const double tau = o[3] - T0;
        const double wx = wgt * x;
        const double wxx = wx * x, wt = wgt * tau, wxt = wx * tau;
        Sw = Sw + wgt; Se = Se + wx; See = See + wxx; St = St + wt; Set = Set + wxt;
    }
    const double a1 = Sw * See, a2 = Se * Se;
    const double Dl = a1 - a2;
    double period = nan, period_err = nan, T0_fit = nan, T0_err = nan, chi2_out = nan, rms = nan, max_sigma = nan, max_epoch = nan;
    if (timed >= 2 && Dl > 0.0) {
        const double b1 = Sw * Set, b2 = Se * St, c1 = See * St, c2 = Se * Set;
        const double slope = (b1 - b2) / Dl;
        const double icpt = (c1 - c2) / Dl;
        period = slope;
        T0_fit = T0 + icpt;
        period_err = sqrt(Sw / Dl);
        T0_err = sqrt(See / Dl);
        if (timed >= 3) {
            double chi2 = 0.0, ss = 0.0;
            bool held = false;
            for (int i = 0; i < ne; ++i) {
                const double* o = rec + (long long)i * kTimesTimeWords;
                if (o[1] != 0.0) continue;
                const double x = o[0];
                const double tau = o[3] - T0;
                const double along = slope * x;
                const double line = icpt + along;
                const double oc = tau - line;
                const double rr = oc / o[4];
                const double rr2 = rr * rr, oc2 = oc * oc;
                chi2 = chi2 + rr2;
                ss = ss + oc2;
                if (!held || fabs(rr) > max_sigma) { held = true; max_sigma = fabs(rr); max_epoch = x; }
            }
            chi2_out = chi2;
            rms = sqrt(ss / (double)timed);
        }
    }
    eph[0] = 0.0; eph[1] = count; eph[2] = (double)timed; eph[3] = first;
    eph[4] = period; eph[5] = period_err; eph[6] = T0_fit; eph[7] = T0_err;
    eph[8] = chi2_out; eph[9] = rms; eph[10] = max_sigma; eph[11] = max_epoch;
}
