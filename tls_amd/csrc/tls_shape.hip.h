// tls_shape.hip.h -- the trapezoid shape fit of a candidate (tls_shape_fit): is the dip flat-bottomed or V-shaped.
//
// The statement (tests/shape_fit_spec.py is the same in Python; include/tls_amd.h, DESIGN.md "Shape fit"), for a candidate
// (P, T0, d in days) on a curve's pairs (xw, w) = ((1 - y) w, 1 / (dy dy)) and the tables ratio[nT], ingress[nQ], shift[nS]:
//   status 1 unless P, T0, d finite, P > 0, d > 0 and wd = window * d < 0.5 * P
//   members, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P;  member iff fabs(tau) <= wd
//   unit (a, b, c) = index (a * nQ + b) * nS + c:
//       T = d * ratio[a];  ho = 0.5 * T;  hb = ho * (1.0 - 2.0 * ingress[b]);  r = 1.0 / (ho - hb) where hb < ho;  c0 = d * shift[c]
//       over the members in index order:  u = fabs(tau - c0);  s = 1.0 if u <= hb, (ho - u) * r if u < ho, else no count
//           cnt += 1;  N = N + xw * s;  D = D + w * (s * s)
//       valid iff cnt >= min_count and D > 0 and N / D > depth_min;  q = N / sqrt(D)
//   best, box, vee = the valid unit of the largest q (the first in unit order among equals) of all units, of those with
//   b == 0 and of those with b == nQ - 1;  status 2 where no unit is valid.
// Every step is one IEEE double operation (contraction off) and every sum runs in index order in ONE thread, so the record
// equals the host statement bit for bit.
//
// tls_shape_fit_kernel: one workgroup of kShapeThreads threads a candidate (a launch of fewer workgroups than candidates
// strides over them, so the scratch below is one stretch a WORKGROUP).
// (1) The members: the series is walked in tiles of kShapeThreads points, a thread a point; a wave's ballot and the four
// wave counts (two sets taking turns, so a tile costs one barrier) give every member its rank in index order.  Ranks below
// kShapeLdsMembers go to the LDS as three arrays (tau, xw, w), 48 KB, three workgroups a CU; higher ranks go to the
// workgroup's stretch of device scratch, and where there are any the LDS part follows them there, so that the tiles of (2)
// all come from one place.
// (2) The units: unit u belongs to thread u mod kShapeThreads, kShapeUnitsPerThread of them at a time with (ho, hb, r, c0)
// and (cnt, N, D) in registers.  Every lane reads the same member in the same step -- one LDS address a wave, a broadcast
// without bank conflicts -- and the three reads of a member serve kShapeUnitsPerThread units.  Members beyond the LDS are
// staged through it tile by tile, once per round of units.  No branch depends on the member: the two comparisons select.
// (3) The picks: a thread's best over its ascending units (strict >), then a tree over the workgroup ordered by (larger q,
// lower unit), for the three classes at once, in the LDS the members have left.  The thread that owns the best unit writes
// its fields; thread 0 the rest.
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_times.hip.h (tls_times_pairs_kernel forms the pairs).

constexpr int kShapeThreads = 256;
constexpr int kShapeWaves = kShapeThreads / kWave;
constexpr int kShapeLdsMembers = 2048;               // members the LDS holds: 3 * 8 bytes each
constexpr int kShapeUnitsPerThread = 4;              // units a thread carries against one read of a member
constexpr int kShapeMaxUnits = 65536;
constexpr int kShapeMaxPoints = 1 << 22;
constexpr int kShapeMaxGroups = 1024;                // workgroups of a launch at most (each owns 3 * n doubles of scratch)
constexpr int kShapeWords = 16;                      // tls_shape_record

struct ShapeArgs {
    const double* t;                                 // [n]
    const double2* pairs;                            // [slots][n] (xw, w)
    const int* slot;                                 // [fits] of the slab
    const double* period; const double* T0; const double* duration;   // [fits]
    const double* ratio; const double* ingress; const double* shift;  // [nT], [nQ], [nS]
    double* scratch;                                 // [workgroups][3][n]: tau | xw | w of the members the LDS does not hold
    double* out;                                     // [fits][kShapeWords]
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    double window, depth_min;
    int n, fits, nT, nQ, nS, min_count;
};

// a is the better pick: a valid unit beats none, a larger q a smaller one, the lower unit its equal
__device__ __forceinline__ bool shape_better(double qa, int ua, double qb, int ub) {
    if (ua < 0) return false;
    if (ub < 0) return true;
    return qa > qb || (qa == qb && ua < ub);
}

__global__ void __launch_bounds__(kShapeThreads) tls_shape_fit_kernel(const ShapeArgs a) {
#pragma clang fp contract(off)
    __shared__ double m_tau[kShapeLdsMembers];
    __shared__ double m_xw[kShapeLdsMembers];
    __shared__ double m_w[kShapeLdsMembers];
    __shared__ int wave_count[2][kShapeWaves];
    static_assert(3 * kShapeThreads <= kShapeLdsMembers, "the picks' tree lives in the members' LDS");
    double* red_q = m_tau;                           // [3][kShapeThreads], behind the units
    int* red_u = reinterpret_cast<int*>(m_xw);       // [3][kShapeThreads]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, n = a.n;
    const int nQ = a.nQ, nS = a.nS, per_a = nQ * nS, units = a.nT * per_a;
    const double nan = (double)NAN;
    double* s_tau = a.scratch + (long long)blockIdx.x * 3 * n;
    double* s_xw = s_tau + n;
    double* s_w = s_xw + n;
    TLS_CHECK(a, units >= 1 && units <= kShapeMaxUnits && nQ >= 2, kChkShape);
    for (long long f = blockIdx.x; f < a.fits; f += gridDim.x) {
        double* o = a.out + f * kShapeWords;
        const double P = a.period[f], T0 = a.T0[f], d = a.duration[f];
        const double wd = a.window * d;
        const double half = 0.5 * P;
        if (!(isfinite(P) && isfinite(T0) && isfinite(d) && P > 0.0 && d > 0.0 && wd < half)) {   // (the whole workgroup)
            if (tid < kShapeWords) o[tid] = tid == 0 ? 1.0 : nan;
            continue;
        }
        const double2* pw = a.pairs + (long long)a.slot[f] * n;
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
        // (2) the units, kShapeUnitsPerThread a thread and round
        double best_q[3] = {nan, nan, nan};
        int best_u[3] = {-1, -1, -1};
        int best_cnt = 0;
        double best_dep = nan, best_D = nan;
        const int rounds = (units + kShapeThreads * kShapeUnitsPerThread - 1) / (kShapeThreads * kShapeUnitsPerThread);
        for (int round = 0; round < rounds; ++round) {
            double ho[kShapeUnitsPerThread], hb[kShapeUnitsPerThread], rr[kShapeUnitsPerThread], c0[kShapeUnitsPerThread];
            double N[kShapeUnitsPerThread], D[kShapeUnitsPerThread];
            int cnt[kShapeUnitsPerThread];
#pragma unroll
            for (int j = 0; j < kShapeUnitsPerThread; ++j) {
                const int u = (round * kShapeUnitsPerThread + j) * kShapeThreads + tid;
                N[j] = 0.0; D[j] = 0.0; cnt[j] = 0;
                ho[j] = -1.0; hb[j] = -1.0; rr[j] = 0.0; c0[j] = 0.0;      // (no unit: u >= 0 counts nowhere)
                if (u < units) {
                    const int ia = u / per_a, rest = u - ia * per_a;
                    const int ib = rest / nS, ic = rest - ib * nS;
                    TLS_CHECK(a, ia >= 0 && ia < a.nT && ib >= 0 && ib < nQ && ic >= 0 && ic < nS, kChkShape);
                    const double T = d * a.ratio[ia];
                    const double g2 = 2.0 * a.ingress[ib];
                    const double flat = 1.0 - g2;
                    ho[j] = 0.5 * T;
                    hb[j] = ho[j] * flat;
                    if (hb[j] < ho[j]) {
                        const double ramp = ho[j] - hb[j];
                        rr[j] = 1.0 / ramp;
                    }
                    c0[j] = d * a.shift[ic];
                }
            }
            for (int tile = 0; tile < tiles; ++tile) {
                const int m0 = tile * kShapeLdsMembers;
                const int mc = total - m0 < kShapeLdsMembers ? total - m0 : kShapeLdsMembers;
                if (tiles > 1) {
                    wg_sync();                       // (the last tile has been read; the scratch is written)
                    for (int m = tid; m < mc; m += kShapeThreads) {
                        TLS_CHECK(a, m0 + m < n, kChkShape);
                        m_tau[m] = s_tau[m0 + m]; m_xw[m] = s_xw[m0 + m]; m_w[m] = s_w[m0 + m];
                    }
                    wg_sync();
                }
                for (int m = 0; m < mc; ++m) {
                    const double tau = m_tau[m], xw = m_xw[m], w = m_w[m];
#pragma unroll
                    for (int j = 0; j < kShapeUnitsPerThread; ++j) {
                        const double off = tau - c0[j];
                        const double u = fabs(off);
                        const double left = ho[j] - u;
                        const double slope = left * rr[j];
                        const bool inner = u <= hb[j];
                        const bool counts = inner || u < ho[j];
                        const double s = inner ? 1.0 : slope;
                        const double ns = xw * s;
                        const double s2 = s * s;
                        const double ds = w * s2;
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
            for (int j = 0; j < kShapeUnitsPerThread; ++j) {
                const int u = (round * kShapeUnitsPerThread + j) * kShapeThreads + tid;
                if (u >= units || cnt[j] < a.min_count || !(D[j] > 0.0)) continue;
                const double dep = N[j] / D[j];
                if (!(dep > a.depth_min)) continue;
                const double q = N[j] / sqrt(D[j]);
                const int ib = (u % per_a) / nS;
                if (best_u[0] < 0 || q > best_q[0]) { best_q[0] = q; best_u[0] = u; best_cnt = cnt[j]; best_dep = dep; best_D = D[j]; }
                if (ib == 0 && (best_u[1] < 0 || q > best_q[1])) { best_q[1] = q; best_u[1] = u; }
                if (ib == nQ - 1 && (best_u[2] < 0 || q > best_q[2])) { best_q[2] = q; best_u[2] = u; }
            }
        }
        // (3) the picks of the workgroup
        wg_sync();                                   // (the members have been read)
        for (int c = 0; c < 3; ++c) { red_q[c * kShapeThreads + tid] = best_q[c]; red_u[c * kShapeThreads + tid] = best_u[c]; }
        for (int s = kShapeThreads / 2; s > 0; s >>= 1) {
            wg_sync();
            if (tid < s) {
                for (int c = 0; c < 3; ++c) {
                    const int me = c * kShapeThreads + tid;
                    if (shape_better(red_q[me + s], red_u[me + s], red_q[me], red_u[me])) { red_q[me] = red_q[me + s]; red_u[me] = red_u[me + s]; }
                }
            }
        }
        wg_sync();
        const int u_all = red_u[0], u_box = red_u[kShapeThreads], u_vee = red_u[2 * kShapeThreads];
        if (tid == 0) {
            o[0] = u_all < 0 ? 2.0 : 0.0;
            o[1] = (double)total;
            if (u_all < 0) for (int k = 2; k < 12; ++k) o[k] = nan;
            double q_box = nan, T_box = nan, q_vee = nan, T_vee = nan;
            if (u_box >= 0) { q_box = red_q[kShapeThreads]; T_box = d * a.ratio[u_box / per_a]; }
            if (u_vee >= 0) { q_vee = red_q[2 * kShapeThreads]; T_vee = d * a.ratio[u_vee / per_a]; }
            o[12] = q_box; o[13] = T_box; o[14] = q_vee; o[15] = T_vee;
        }
        if (u_all >= 0 && (u_all & (kShapeThreads - 1)) == tid) {     // the thread that holds the best unit's sums
            TLS_CHECK(a, best_u[0] == u_all && u_all < units, kChkShape);
            const int ia = u_all / per_a, rest = u_all - ia * per_a;
            const int ib = rest / nS, ic = rest - ib * nS;
            const double root = sqrt(best_D);
            o[2] = (double)best_cnt; o[3] = best_q[0]; o[4] = best_dep; o[5] = 1.0 / root;
            o[6] = d * a.ratio[ia]; o[7] = a.ingress[ib]; o[8] = d * a.shift[ic];
            o[9] = (double)ia; o[10] = (double)ib; o[11] = (double)ic;
        }
        wg_sync();                                   // (the next candidate overwrites the LDS and the scratch)
    }
}
