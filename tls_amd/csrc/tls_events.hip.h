// tls_events.hip.h -- per-transit event vetting of a candidate (tls_event_vetting).
//
// The statement (tests/event_vetting_spec.py is the same in Python; include/tls_amd.h, DESIGN.md "Event vetting"), for a
// candidate (P, T0, row r of width L and shape b, reach S, chase reach R, guard Gd, chase_span) on a curve's pairs
// (xw, w) = ((1 - y) w, 1 / (dy dy)):
//   the epochs and every epoch's held window (q, d, c, lo) as tls_transit_times has them (tls_times.hip.h), N and D kept
//   point_share = max_k xw[lo+k] b[k] / N;  before, after = (sum xw / sum w) / d over the L samples on either side of the window
//   chase: every window centred m = Gd+1 .. R samples to either side of c that lies whole inside the series and runs over no
//       gap counts; one whose |q'| >= chase_fraction q is comparable; chase_dt = the least |t[c'] - t[c]| of the comparable ones
//   chases = min(chase_dt / chase_span, 1) (1 without a comparable window, NaN without a window);  flags;  the summary.
// Every step is one IEEE double operation (contraction off) and every sum runs in index order in ONE thread; chase_dt is a
// minimum of non-negative doubles and n_chased a count, so the order the chase windows are taken in does not show.  Both
// records equal the host statement bit for bit.
//
// tls_times_pairs_kernel (tls_times.hip.h) forms the pairs.  tls_event_vetting_kernel: one workgroup of kEventsThreads threads
// a candidate, the epochs in chunks as in tls_transit_times_kernel -- passes (a) the nearest samples and (b) q of every
// (epoch, shift) unit are that kernel's, chain for chain; they are written out here once more so that kernel's code stays as
// it is -- then (c) a thread an epoch picks over the shifts, walks the held window for N, D and the largest term, sums the
// two side windows, writes the first ten fields of the record and leaves N, D in the candidate's scratch in device memory
// (two doubles an epoch) and c, q in the LDS; (d) the chase: the (epoch, side, m) units of the chunk are dealt to the threads,
// unit u to thread u mod kEventsThreads, a side's centres ascending, so neighbouring lanes walk neighbouring windows and step k
// of a wave reads consecutive pairs, one 16-byte load a lane, served by the L2 after the first touch.  A thread walks its
// window in index order and keeps (count, least dtc) of the epoch it is in, in registers; when its next unit belongs to
// another epoch it hands them to the epoch's slot in the LDS: an add and, where a comparable window was seen, a minimum on
// the bit pattern (dtc >= 0, so the patterns order as the values do).  Nothing per unit is stored anywhere.  (A form that
// staged a tile of centres and its halo in the LDS, as tls_single.hip.h does, gave the same bits and took twice the time at
// Kepler length and thirty times the time of this pass on k2-length candidates -- two barriers a tile of one (epoch, side)
// segment -- and was dropped: PERF_LOG.md, "Event vetting: the chase pass".)  (e) a thread an
// epoch forms chases and the flags and writes the last four fields.  Behind the last chunk thread 0 reads the records and the
// scratch back (wg_sync's release and acquire fences order the other threads' stores in front of it) and forms the summary.
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_times.hip.h.

constexpr int kEventsThreads = 256;
constexpr int kEventsMaxChase = 8192;
constexpr int kEventsSummaryWords = 15;              // tls_event_summary
constexpr int kEventsRecordWords = 14;               // tls_event_record

struct EventsArgs {
    const double* t;                                 // [n]
    const double2* pairs;                            // [slots][n] (xw, w)
    const SingleRow* rows;                           // [n_rows]
    const double* taps;                              // pairs (b[j], b[j] * b[j]), row after row
    const int* slot; const int* row; const int* reach;   // [fits] of the slab
    const int* chase; const int* guard;              // [fits]: R, and min(Gd, R)
    const double* period; const double* T0; const double* chase_span;   // [fits]
    double* out;                                     // [fits][kEventsSummaryWords]
    double* out_events;                              // [fits][max_epochs][kEventsRecordWords]
    double2* held;                                   // [fits][max_epochs] (N, D) of the held windows: scratch
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    double depth_min, min_ses, chase_fraction, chase_min, point_fraction, step_fraction;
    int n, max_epochs;
};

// (sum xw / sum w) / d over the L samples from a, NaN where they leave the series or run over a gap
__device__ __forceinline__ double events_side(const double* t, const double2* pw, int a, int L, int n, double span, double d) {
#pragma clang fp contract(off)
    const int z = a + L - 1;
    if (a < 0 || z > n - 1) return (double)NAN;
    const double dt = t[z] - t[a];
    if (!(dt <= span)) return (double)NAN;
    double Ns = 0.0, Ws = 0.0;
    for (int k = 0; k < L; ++k) {
        const double2 v = pw[a + k];
        Ns = Ns + v.x;
        Ws = Ws + v.y;
    }
    const double level = Ns / Ws;
    return level / d;
}

__global__ void __launch_bounds__(kEventsThreads) tls_event_vetting_kernel(const EventsArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char events_lds[];
    __shared__ int centre[kTimesChunkEpochs];                      // (a) the nearest sample; from (c) on the held c, -1: none
    __shared__ double held_q[kTimesChunkEpochs];
    __shared__ unsigned long long chase_least[kTimesChunkEpochs];  // bits of the least dtc; all ones: no comparable window
    __shared__ int chase_count[kTimesChunkEpochs];
    double* qs = reinterpret_cast<double*>(events_lds);            // [epochs of the chunk][2S+1]
    const int tid = threadIdx.x, n = a.n;
    const long long f = blockIdx.x;
    double* sum = a.out + f * kEventsSummaryWords;
    double* rec = a.out_events + f * (long long)a.max_epochs * kEventsRecordWords;
    double2* nd = a.held + f * (long long)a.max_epochs;
    const double P = a.period[f], T0 = a.T0[f];
    const double nan = (double)NAN;
    const unsigned long long none = ~0ull;
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
    for (long long k = (long long)ne * kEventsRecordWords + tid; k < (long long)a.max_epochs * kEventsRecordWords; k += kEventsThreads)
        rec[k] = nan;
    if (status != 0) {                               // (the whole workgroup leaves)
        if (tid < kEventsSummaryWords) sum[tid] = tid == 0 ? (double)status : (tid == 1 && status == 2) ? count : nan;
        return;
    }
    const const_single_row_ptr rows = (const_single_row_ptr)a.rows;
    const int r = a.row[f];
    const int L = rows[r].width, h = (L - 1) / 2;
    const double span = rows[r].span_max;
    const int S = a.reach[f], U = 2 * S + 1;
    const int R = a.chase[f], Gd = a.guard[f], side_units = R - Gd;      // (Gd <= R: the host clamps it)
    const double chase_span = a.chase_span[f];
    const const_f64_ptr taps = (const_f64_ptr)a.taps + 2ll * rows[r].offset;
    const double2* pw = a.pairs + (long long)a.slot[f] * n;
    const int chunk = times_chunk_epochs(S);
    TLS_CHECK(a, S >= 1 && S <= kTimesMaxReach && L >= kSingleMinWidth && L <= kSingleMaxWidth, kChkTimes);
    TLS_CHECK(a, R >= 0 && R <= kEventsMaxChase && Gd >= 0 && Gd <= R, kChkTimes);
    for (int e0 = 0; e0 < ne; e0 += chunk) {
        const int ec = ne - e0 < chunk ? ne - e0 : chunk;
        // (a) the nearest sample of every epoch of the chunk
        for (int i = tid; i < ec; i += kEventsThreads) {
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
        for (int u = tid; u < units; u += kEventsThreads) {
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
        // (c) the pick over the shifts, the held window once more, the largest term and the two sides of every epoch
        for (int i = tid; i < ec; i += kEventsThreads) {
            const double e = first + (double)(e0 + i);
            const double ahead = e * P;
            const double tc = T0 + ahead;
            double* o = rec + (long long)(e0 + i) * kEventsRecordWords;
            int best = -1;
            double q = nan;
            for (int s = 0; s < U; ++s) {
                const double v = qs[i * U + s];
                if (!isnan(v) && (best < 0 || v > q)) { q = v; best = s; }
            }
            double state = 1.0, d = nan, depth_err = nan, index = nan, share = nan, before = nan, after = nan;
            double2 kept;
            kept.x = nan; kept.y = nan;
            int c = -1;
            if (best >= 0) {
                c = centre[i] + (best - S);
                const int lo = c - h;
                TLS_CHECK(a, lo >= 0 && lo + L - 1 <= n - 1, kChkTimes);
                const double2* win = pw + lo;
                double N = 0.0, D = 0.0, pm = nan;
                for (int k = 0; k < L; ++k) {
                    const double2 v = win[k];
                    const double nb = v.x * taps[2 * k];
                    const double db = v.y * taps[2 * k + 1];
                    N = N + nb;
                    D = D + db;
                    if (k == 0 || nb > pm) pm = nb;
                }
                state = 0.0;
                d = N / D;
                const double root = sqrt(D);
                depth_err = 1.0 / root;
                index = (double)c;
                share = pm / N;
                before = events_side(a.t, pw, lo - L, L, n, span, d);
                after = events_side(a.t, pw, lo + L, L, n, span, d);
                kept.x = N; kept.y = D;
            }
            nd[e0 + i] = kept;
            o[0] = e; o[1] = state; o[2] = tc; o[3] = q; o[4] = d; o[5] = depth_err; o[6] = index;
            o[7] = share; o[8] = before; o[9] = after;
            centre[i] = c;                           // (only this thread read the epoch's nearest sample)
            held_q[i] = q;
            chase_least[i] = none;
            chase_count[i] = 0;
        }
        wg_sync();
        // (d) the chase: unit u = (epoch * 2 + side) * side_units + rank, a side's centres ascending
        if (side_units > 0) {
            const int per_epoch = 2 * side_units;
            const int chase_units = ec * per_epoch;  // (at most 1024 * 16384)
            int mine = -1, seen = 0;                 // the epoch this thread is in, and what it has of it
            unsigned long long least = none;
            for (int u = tid; u < chase_units; u += kEventsThreads) {
                const int i = u / per_epoch, v = u - i * per_epoch;
                if (i != mine) {
                    if (seen) atomicAdd(&chase_count[mine], seen);
                    if (least != none) atomicMin(&chase_least[mine], least);
                    mine = i; seen = 0; least = none;
                }
                const int c = centre[i];
                if (c < 0) continue;
                // the left side: c - R .. c - Gd - 1; the right side: c + Gd + 1 .. c + R
                const int c2 = v < side_units ? c - R + v : c + Gd + 1 + (v - side_units);
                const int lo = c2 - h, hi = lo + L - 1;
                if (lo < 0 || hi > n - 1) continue;
                const double dt = a.t[hi] - a.t[lo];
                if (!(dt <= span)) continue;
                ++seen;
                const double2* win = pw + lo;
                double N = 0.0, D = 0.0;
#pragma unroll 4
                for (int k = 0; k < L; ++k) {
                    const double2 x = win[k];
                    const double nb = x.x * taps[2 * k];
                    const double db = x.y * taps[2 * k + 1];
                    N = N + nb;
                    D = D + db;
                }
                const double q2 = N / sqrt(D);
                const double bar = a.chase_fraction * held_q[i];
                if (fabs(q2) >= bar) {
                    const double apart = a.t[c2] - a.t[c];
                    const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(apart));
                    if (bits < least) least = bits;
                }
            }
            if (seen) atomicAdd(&chase_count[mine], seen);
            if (least != none) atomicMin(&chase_least[mine], least);
        }
        wg_sync();
        // (e) chases and the flags of every epoch of the chunk
        for (int i = tid; i < ec; i += kEventsThreads) {
            double* o = rec + (long long)(e0 + i) * kEventsRecordWords;
            double chases = nan, chase_dt = nan, n_chased = nan, flag_sum = nan;    // (nothing held: NaN behind time_linear)
            if (centre[i] >= 0) {
                const double q = held_q[i], share = o[7], before = o[8], after = o[9];   // (this thread's own stores)
                const int chased = chase_count[i];
                const unsigned long long least = chase_least[i];
                if (chased > 0) {
                    chases = 1.0;
                    if (least != none) {
                        chase_dt = __longlong_as_double((long long)least);
                        const double x = chase_dt / chase_span;
                        if (x < 1.0) chases = x;
                    }
                }
                const int flags = (!(q >= a.min_ses) ? 1 : 0) + (share > a.point_fraction ? 2 : 0)
                                + ((before > a.step_fraction || after > a.step_fraction) ? 4 : 0) + (chases < a.chase_min ? 8 : 0);
                n_chased = (double)chased;
                flag_sum = (double)flags;
            }
            o[10] = chases; o[11] = chase_dt; o[12] = n_chased; o[13] = flag_sum;
        }
        wg_sync();                                   // (the next chunk overwrites the LDS; thread 0 reads the records)
    }
    if (tid != 0) return;
    // the summary over the held events, ascending.  The sums without the strongest event: when a new strongest event turns up,
    // the sums in front of it are those over every earlier event, in order -- the running sums as they stand.
    int n_held = 0, n_good = 0, chased = 0;
    double SN = 0.0, SD = 0.0, GN = 0.0, GD = 0.0, RN = 0.0, RD = 0.0;
    double ses_max = nan, ses_max_epoch = nan, chases_min = nan, chases_sum = 0.0;
    for (int i = 0; i < ne; ++i) {
        const double* o = rec + (long long)i * kEventsRecordWords;
        if (o[1] != 0.0) continue;
        const double2 v = nd[i];
        if (n_held == 0 || o[3] > ses_max) {
            ses_max = o[3]; ses_max_epoch = o[0];
            RN = SN; RD = SD;
        } else {
            RN = RN + v.x; RD = RD + v.y;
        }
        SN = SN + v.x; SD = SD + v.y;
        ++n_held;
        if (o[13] == 0.0) { GN = GN + v.x; GD = GD + v.y; ++n_good; }
        const double x = o[10];
        if (!isnan(x)) {
            if (chased == 0 || x < chases_min) chases_min = x;
            chases_sum = chases_sum + x;
            ++chased;
        }
    }
    double mes = nan, mes_good = nan, mes_rest = nan, dominance = nan, depth_mean = nan, chi2_out = nan, chases_mean = nan;
    if (n_held > 0) {
        mes = SN / sqrt(SD);
        depth_mean = SN / SD;
        dominance = ses_max / mes;
        if (n_good > 0) mes_good = GN / sqrt(GD);
        if (n_held >= 2) mes_rest = RN / sqrt(RD);
        double chi2 = 0.0;
        for (int i = 0; i < ne; ++i) {
            const double* o = rec + (long long)i * kEventsRecordWords;
            if (o[1] != 0.0) continue;
            const double rr = o[4] - depth_mean;
            const double r2 = rr * rr;
            const double term = r2 * nd[i].y;
            chi2 = chi2 + term;
        }
        chi2_out = chi2;
        if (chased > 0) chases_mean = chases_sum / (double)chased;
    }
    sum[0] = 0.0; sum[1] = count; sum[2] = first; sum[3] = (double)n_held; sum[4] = (double)n_good;
    sum[5] = mes; sum[6] = mes_good; sum[7] = mes_rest; sum[8] = ses_max; sum[9] = ses_max_epoch; sum[10] = dominance;
    sum[11] = depth_mean; sum[12] = chi2_out; sum[13] = chases_min; sum[14] = chases_mean;
}
