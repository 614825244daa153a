// tls_transit_fit.hip.h -- the limb-darkened transit fit of a candidate (tls_transit_fit): planet size, impact parameter and
// T14 from the dip itself, with the exposure time in the model.
//
// The statement (tests/transit_fit_spec.py is the same in Python; include/tls_amd.h, DESIGN.md "Transit fit"), for a candidate
// (P, T0, d in days, seed row j0) on a curve's pairs (xw, w) = ((1 - y) w, 1 / (dy dy)), the profile table k_rows[nK],
// profile[nK][M + 1] and the tables impact[nB], ratio[nT], shift[nS], sub[S]:
//   status 1 unless P, T0, d finite, P > 0, d > 0 and wd = window * d < 0.5 * P
//   members, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P;  member iff fabs(tau) <= wd
//   x2 = x2 + (xw * xw) / w over the members in index order
//   one pass with row j, p = profile[j]:  e1 = 1.0 + k_rows[j];  e2 = e1 * e1;  sM = M / e1
//     unit (ib, a, c) = index (ib * nT + a) * nS + c:
//       b = impact[ib] * e1;  bb = b * b;  cc = e2 - bb;  T = d * ratio[a];  rh = 1.0 / (0.5 * T);  c0 = d * shift[c]
//       over the members in index order:  acc = 0.0;  for s in order:  ts = tau + sub[s];  v = (ts - c0) * rh;  vv = v * v
//           zz = bb + cc * vv;  sample = 0.0 unless zz < e2, else  z = sqrt(zz);  q = z * sM;  m = min(floor(q), M - 1)
//           fr = q - m;  sample = p[m] + (p[m + 1] - p[m]) * fr;  acc = acc + sample
//         mval = acc / S;  counts iff mval > 0:  cnt += 1;  N = N + xw * mval;  D = D + w * (mval * mval)
//       valid iff cnt >= min_count and D > 0 and A = N / D > 0;  q = N / sqrt(D)
//     the pick = the valid unit of the largest q, the first in unit order among equals
//   pass 1 with row j0;  k1 = k_rows[j0] * sqrt(A);  j1 = the row of the least fabs(k_rows[j] - k1), the lowest on ties;
//   pass 2 with row j1 (pass 1 itself where j1 == j0);  status 2 where a pass has no valid unit
//   intervals: least and largest k_rows[j1] * sqrt(A_u), b_u, T_u, c0_u over pass 2's valid units with q_u q_u >= q q - delta
// Every step is one IEEE double operation (contraction off) and every sum runs in index order in ONE thread, so the record
// equals the host statement bit for bit.
//
// tls_transit_fit_kernel: one workgroup of kShapeThreads threads a candidate (a launch of fewer workgroups than candidates
// strides over them, so the scratch is one stretch a WORKGROUP).
// (1) The members, ranked and compacted exactly as tls_shape_fit_kernel does: ranks below kShapeLdsMembers in the LDS (48 KB),
// higher ranks in the workgroup's device scratch, and where there are any the LDS part follows them there.
// (2) A pass: the row's M + 1 doubles go to the dynamic LDS (8 KB at M = 1024; with the members two workgroups a CU).  Unit u
// belongs to thread u mod kShapeThreads, kTransitUnitsPerThread at a time with (bb, cc, rh, c0) and (cnt, N, D) in registers.
// Every lane reads the same member in the same step -- a broadcast --; the S sub-samples of a member run in registers, and
// the two profile reads of a sub-sample are the only divergent LDS reads.  A wave none of whose units the member touches
// skips the division.  No branch depends on a single lane's data.  Thread 0 adds x2 beside its first round of pass 1.
// (3) The picks: a thread's best over its ascending units (strict >), then a tree over the workgroup ordered by (larger q,
// lower unit).  Every unit's (q, A) also goes to the workgroup's scratch -- written and read back by the same thread -- so
// that the intervals, which need the best q first, are one more walk over the units and a min/max tree (wave shuffles, then
// the four waves in the LDS).
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_shape.hip.h (its constants and shape_better).

constexpr int kTransitUnitsPerThread = 4;            // units a thread carries against one read of a member
constexpr int kTransitMaxUnits = 65536;
constexpr int kTransitMaxM = 4096;
constexpr int kTransitMaxSub = 16;
constexpr int kTransitMaxRows = 4096;
constexpr int kTransitWords = 24;                    // tls_transit_fit_record
constexpr int kTransitSlab = 512;                    // candidates (and curves) of one slab at most

struct TransitFitArgs {
    const double* t;                                 // [n]
    const double2* pairs;                            // [slots][n] (xw, w)
    const int* slot;                                 // [fits] of the slab
    const int* row_first;                            // [fits] of the slab
    const double* period; const double* T0; const double* duration;   // [fits]
    const double* k_rows; const double* profile;     // [nK], [nK][M + 1]
    const double* impact; const double* ratio; const double* shift; const double* sub;   // [nB], [nT], [nS], [S]
    double* scratch;                                 // [workgroups][3 n + 2 units]: tau | xw | w of the members; q | A of the units
    double* out;                                     // [fits][kTransitWords]
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    double window, delta;
    int n, fits, nK, M, nB, nT, nS, S, min_count;
};

__global__ void __launch_bounds__(kShapeThreads) tls_transit_fit_kernel(const TransitFitArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double row_p[];                // [M + 1] the pass's profile row
    __shared__ double m_tau[kShapeLdsMembers];
    __shared__ double m_xw[kShapeLdsMembers];
    __shared__ double m_w[kShapeLdsMembers];
    __shared__ double red_q[kShapeThreads];
    __shared__ int red_u[kShapeThreads];
    __shared__ double red_span[kShapeWaves][8];
    __shared__ double best_A;
    __shared__ int best_cnt;
    __shared__ int wave_count[2][kShapeWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, n = a.n;
    const int nT = a.nT, nS = a.nS, per_b = nT * nS, units = a.nB * per_b, M = a.M, S = a.S;
    const double nan = (double)NAN, inf = (double)INFINITY;
    const double dS = (double)S, dM = (double)M, top = (double)(M - 1);
    double* s_tau = a.scratch + (long long)blockIdx.x * (3ll * n + 2ll * units);
    double* s_xw = s_tau + n;
    double* s_w = s_xw + n;
    double* u_q = s_w + n;
    double* u_A = u_q + units;
    TLS_CHECK(a, units >= 1 && units <= kTransitMaxUnits && M >= 1 && M <= kTransitMaxM && S >= 1 && S <= kTransitMaxSub, kChkShape);
    const int rounds = (units + kShapeThreads * kTransitUnitsPerThread - 1) / (kShapeThreads * kTransitUnitsPerThread);
    for (long long f = blockIdx.x; f < a.fits; f += gridDim.x) {
        double* o = a.out + f * kTransitWords;
        const double P = a.period[f], T0 = a.T0[f], d = a.duration[f];
        const double wd = a.window * d;
        const double half = 0.5 * P;
        if (!(isfinite(P) && isfinite(T0) && isfinite(d) && P > 0.0 && d > 0.0 && wd < half)) {   // (the whole workgroup)
            if (tid < kTransitWords) o[tid] = tid == 0 ? 1.0 : tid == kTransitWords - 1 ? 0.0 : nan;
            continue;
        }
        const double2* pw = a.pairs + (long long)a.slot[f] * n;
        const int j0 = a.row_first[f];
        TLS_CHECK(a, j0 >= 0 && j0 < a.nK, kChkShape);
        // (1) the members, ranked in index order
        int total = 0;
        for (int base = 0, k = 0; base < n; base += kShapeThreads, ++k) {
            const int i = base + tid;
            bool member = false;
            double tau = 0.0;
            if (i < n) {
                const double lead = a.t[i] - T0;
                const double x = lead / P;
                const double xh = x + 0.5;
                const double e = floor(xh);
                const double ph = x - e;
                tau = ph * P;
                member = fabs(tau) <= wd;
            }
            const unsigned long long mask = __ballot(member);
            if (lane == 0) wave_count[k & 1][wave] = __popcll(mask);
            wg_sync();
            int rank = total + __popcll(mask & ((1ull << lane) - 1ull));
            for (int v = 0; v < kShapeWaves; ++v) {
                const int c = wave_count[k & 1][v];
                if (v < wave) rank += c;
                total += c;
            }
            if (member) {
                const double2 v = pw[i];
                TLS_CHECK(a, rank >= 0 && rank < n, kChkShape);
                if (rank < kShapeLdsMembers) { m_tau[rank] = tau; m_xw[rank] = v.x; m_w[rank] = v.y; }
                else { s_tau[rank] = tau; s_xw[rank] = v.x; s_w[rank] = v.y; }
            }
        }
        wg_sync();
        const int tiles = (total + kShapeLdsMembers - 1) / kShapeLdsMembers;
        if (tiles > 1) {                             // (the scratch holds every tile)
            for (int m = tid; m < kShapeLdsMembers; m += kShapeThreads) { s_tau[m] = m_tau[m]; s_xw[m] = m_xw[m]; s_w[m] = m_w[m]; }
        }
        // (2) the passes
        double x2 = 0.0;
        double q_best = nan, A_best = nan, e1 = nan, kj = nan;
        int u_best = -1, cnt_best = 0, row = j0;
        for (int pass = 0; pass < 2; ++pass) {
            kj = a.k_rows[row];
            e1 = 1.0 + kj;
            const double e2 = e1 * e1;
            const double sM = dM / e1;
            wg_sync();                               // (the last pass has read its row)
            for (int m = tid; m <= M; m += kShapeThreads) row_p[m] = a.profile[(long long)row * (M + 1) + m];
            wg_sync();
            double my_q = nan, my_A = nan;
            int my_u = -1, my_cnt = 0;
            for (int round = 0; round < rounds; ++round) {
                double bb[kTransitUnitsPerThread], cc[kTransitUnitsPerThread], rh[kTransitUnitsPerThread], c0[kTransitUnitsPerThread];
                double N[kTransitUnitsPerThread], D[kTransitUnitsPerThread];
                int cnt[kTransitUnitsPerThread];
#pragma unroll
                for (int j = 0; j < kTransitUnitsPerThread; ++j) {
                    const int u = (round * kTransitUnitsPerThread + j) * kShapeThreads + tid;
                    N[j] = 0.0; D[j] = 0.0; cnt[j] = 0;
                    bb[j] = e2; cc[j] = 0.0; rh[j] = 0.0; c0[j] = 0.0;      // (no unit: zz == e2 is outside everywhere)
                    if (u < units) {
                        const int ib = u / per_b, rest = u - ib * per_b;
                        const int ia = rest / nS, ic = rest - ia * nS;
                        TLS_CHECK(a, ib >= 0 && ib < a.nB && ia >= 0 && ia < nT && ic >= 0 && ic < nS, kChkShape);
                        const double b = a.impact[ib] * e1;
                        const double T = d * a.ratio[ia];
                        const double hT = 0.5 * T;
                        bb[j] = b * b;
                        cc[j] = e2 - bb[j];
                        rh[j] = 1.0 / hT;
                        c0[j] = d * a.shift[ic];
                    }
                }
                const bool adds_x2 = tid == 0 && pass == 0 && round == 0;
                for (int tile = 0; tile < tiles; ++tile) {
                    const int m0 = tile * kShapeLdsMembers;
                    const int mc = total - m0 < kShapeLdsMembers ? total - m0 : kShapeLdsMembers;
                    if (tiles > 1) {
                        wg_sync();                   // (the last tile has been read; the scratch is written)
                        for (int m = tid; m < mc; m += kShapeThreads) {
                            TLS_CHECK(a, m0 + m < n, kChkShape);
                            m_tau[m] = s_tau[m0 + m]; m_xw[m] = s_xw[m0 + m]; m_w[m] = s_w[m0 + m];
                        }
                        wg_sync();
                    }
                    for (int m = 0; m < mc; ++m) {
                        const double tau = m_tau[m], xw = m_xw[m], w = m_w[m];
                        if (adds_x2) {
                            const double sq = xw * xw;
                            const double term = sq / w;
                            x2 = x2 + term;
                        }
                        double acc[kTransitUnitsPerThread];
#pragma unroll
                        for (int j = 0; j < kTransitUnitsPerThread; ++j) acc[j] = 0.0;
                        for (int s = 0; s < S; ++s) {
                            const double ts = tau + a.sub[s];
#pragma unroll
                            for (int j = 0; j < kTransitUnitsPerThread; ++j) {
                                const double off = ts - c0[j];
                                const double v = off * rh[j];
                                const double vv = v * v;
                                const double sc = cc[j] * vv;
                                const double zz = bb[j] + sc;
                                const bool inside = zz < e2;
                                const double z = sqrt(inside ? zz : 0.0);
                                const double q = z * sM;
                                const double fl = fmin(floor(q), top);
                                const double fr = q - fl;
                                int at = (int)fl;
                                TLS_CHECK(a, at >= 0 && at < M, kChkShape);
                                at = at < 0 ? 0 : at > M - 1 ? M - 1 : at;
                                const double p0 = row_p[at], p1 = row_p[at + 1];
                                const double rise = p1 - p0;
                                const double part = rise * fr;
                                const double value = p0 + part;
                                const double sample = inside ? value : 0.0;
                                acc[j] = acc[j] + sample;
                            }
                        }
                        bool any = false;
#pragma unroll
                        for (int j = 0; j < kTransitUnitsPerThread; ++j) any = any || acc[j] > 0.0;
                        if (__ballot(any) == 0ull) continue;             // (the whole wave: no unit counts this member)
#pragma unroll
                        for (int j = 0; j < kTransitUnitsPerThread; ++j) {
                            const double mval = acc[j] / dS;
                            const bool counts = mval > 0.0;
                            const double ns = xw * mval;
                            const double m2 = mval * mval;
                            const double ds = w * m2;
                            const double Nn = N[j] + ns;
                            const double Dn = D[j] + ds;
                            N[j] = counts ? Nn : N[j];
                            D[j] = counts ? Dn : D[j];
                            cnt[j] += counts ? 1 : 0;
                        }
                    }
                }
                // a thread's units ascend with j and with the round: strict > keeps the first among equals
#pragma unroll
                for (int j = 0; j < kTransitUnitsPerThread; ++j) {
                    const int u = (round * kTransitUnitsPerThread + j) * kShapeThreads + tid;
                    if (u >= units) continue;
                    double q = nan, A = nan;
                    if (cnt[j] >= a.min_count && D[j] > 0.0) {
                        A = N[j] / D[j];
                        if (A > 0.0) q = N[j] / sqrt(D[j]);
                    }
                    u_q[u] = q; u_A[u] = A;          // (q is NaN where the unit is not valid)
                    if (q == q && (my_u < 0 || q > my_q)) { my_q = q; my_u = u; my_A = A; my_cnt = cnt[j]; }
                }
            }
            // (3) the pick of the workgroup
            red_q[tid] = my_q; red_u[tid] = my_u;
            for (int s = kShapeThreads / 2; s > 0; s >>= 1) {
                wg_sync();
                if (tid < s && shape_better(red_q[tid + s], red_u[tid + s], red_q[tid], red_u[tid])) {
                    red_q[tid] = red_q[tid + s]; red_u[tid] = red_u[tid + s];
                }
            }
            wg_sync();
            u_best = red_u[0];
            q_best = red_q[0];
            if (u_best >= 0 && (u_best & (kShapeThreads - 1)) == tid) {      // the thread that holds the pick's sums
                TLS_CHECK(a, my_u == u_best && u_best < units, kChkShape);
                best_A = my_A; best_cnt = my_cnt;
            }
            wg_sync();                               // (red_q, red_u are read; best_A, best_cnt are written)
            if (u_best < 0) break;
            A_best = best_A; cnt_best = best_cnt;
            if (pass == 1) break;
            const double k1 = kj * sqrt(A_best);
            int j1 = 0;
            double gap_best = fabs(a.k_rows[0] - k1);
            for (int j = 1; j < a.nK; ++j) {
                const double gap = fabs(a.k_rows[j] - k1);
                if (gap < gap_best) { gap_best = gap; j1 = j; }
            }
            if (j1 == row) break;
            row = j1;
        }
        if (u_best < 0) {
            if (tid < kTransitWords) o[tid] = tid == 0 ? 2.0 : tid == 1 ? (double)total : tid == kTransitWords - 1 ? 0.0 : nan;
            wg_sync();
            continue;
        }
        // the intervals over the last pass's units (each thread its own)
        double lo[4] = {inf, inf, inf, inf}, hi[4] = {-inf, -inf, -inf, -inf};
        {
            const double qq = q_best * q_best;
            const double least = qq - a.delta;
            for (int u = tid; u < units; u += kShapeThreads) {
                const double q = u_q[u];
                const double q2 = q * q;
                if (!(q2 >= least)) continue;        // (a NaN: not valid)
                const int ib = u / per_b, rest = u - ib * per_b;
                const int ia = rest / nS, ic = rest - ia * nS;
                const double v[4] = {kj * sqrt(u_A[u]), a.impact[ib] * e1, d * a.ratio[ia], d * a.shift[ic]};
#pragma unroll
                for (int k = 0; k < 4; ++k) { lo[k] = fmin(lo[k], v[k]); hi[k] = fmax(hi[k], v[k]); }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            for (int dlt = kWave / 2; dlt > 0; dlt >>= 1) {
                lo[k] = fmin(lo[k], __shfl_down(lo[k], dlt, kWave));
                hi[k] = fmax(hi[k], __shfl_down(hi[k], dlt, kWave));
            }
        if (lane == 0)
            for (int k = 0; k < 4; ++k) { red_span[wave][2 * k] = lo[k]; red_span[wave][2 * k + 1] = hi[k]; }
        wg_sync();
        if (tid < 8) {
            double v = red_span[0][tid];
            for (int wv = 1; wv < kShapeWaves; ++wv) v = (tid & 1) ? fmax(v, red_span[wv][tid]) : fmin(v, red_span[wv][tid]);
            o[15 + tid] = v;
        }
        if (tid == 0) {
            const int ib = u_best / per_b, rest = u_best - ib * per_b;
            const int ia = rest / nS, ic = rest - ia * nS;
            o[0] = 0.0; o[1] = (double)total; o[2] = (double)cnt_best; o[3] = (double)j0; o[4] = (double)row;
            o[5] = q_best; o[6] = A_best; o[7] = kj * sqrt(A_best); o[8] = a.impact[ib] * e1;
            o[9] = d * a.ratio[ia]; o[10] = d * a.shift[ic];
            o[11] = (double)ib; o[12] = (double)ia; o[13] = (double)ic; o[14] = x2; o[23] = 0.0;
        }
        wg_sync();                                   // (the next candidate overwrites the LDS and the scratch)
    }
}
