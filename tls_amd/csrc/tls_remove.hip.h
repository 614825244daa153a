// tls_remove.hip.h -- the multi-planet search of survey mode: the fitted transits of a batch divided out (tls_remove_transits).
// DESIGN.md "Multi-planet search"; tests/remove_transits_spec.py is the statement in numpy.
//
// Candidate f of curve c carries the period and T0 of a peak and the row j, amplitude A, impact b, duration T and shift c0 of
// its transit fit (tls_transit_fit_record).  Its constants, one IEEE double operation a step and no contraction, formed on
// the host:  e1 = 1.0 + k_rows[j];  e2 = e1 * e1;  sM = M / e1;  bb = b * b;  cc = e2 - bb;  rh = 1.0 / (0.5 * T).
// For point i of curve c, the candidates of c in their order:
//     x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P
//     acc = 0.0;  for s in order:  ts = tau + sub[s];  v = (ts - c0) * rh;  vv = v * v;  zz = bb + cc * vv
//         sample = 0.0 unless zz < e2, else  z = sqrt(zz);  q = z * sM;  m = min(floor(q), M - 1);  fr = q - m
//         sample = p[m] + (p[m + 1] - p[m]) * fr;  acc = acc + sample
//     mval = acc / S;  where mval > 0:  mod = 1.0 - A * mval;  y = y / mod;  model = model * mod
// -- the sub-samples of tls_transit_fit_kernel, operation for operation, with its square root and floor, so that mval at a
// fit's members is that fit's own.  The host leaves out the candidates that take no part and groups the others by curve with
// a stable sort: candidate list [offset[c], offset[c + 1]) belongs to curve c.
//
// tls_remove_transits_kernel: one workgroup of kRemoveThreads threads a tile of kRemoveThreads neighbouring points of ONE
// curve (a launch of fewer workgroups than tiles strides over them), one thread a point, so a curve's list is the same for
// every lane and its constants are broadcasts.  y and model stay in registers across the list: one read and one write a
// point.  Under 2 % of the points are in transit, so a lane first forms zz of every sub-exposure WITHOUT the table; the
// waves vote, and only a tile one of whose lanes is inside brings the candidate's profile row (M + 1 doubles, at most 32 KB)
// into the LDS -- it stays there while the next candidates of the list read the same row -- and forms the samples.  The vote
// is one barrier a candidate; it also orders the last candidate's reads of the row in front of the next fill.  No branch
// around a barrier depends on a single lane's data.
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_transit_fit.hip.h (its limits).

constexpr int kRemoveThreads = 256;
constexpr int kRemoveWaves = kRemoveThreads / kWave;
constexpr int kRemoveWords = 10;                     // doubles of a grouped candidate (RemoveCandidate)

struct RemoveCandidate {                             // of a candidate that takes part, formed by the host
    double P, T0, A, c0, bb, cc, rh, e2, sM, row;    // row: the profile row, a whole number in [0, nK)
};

struct RemoveArgs {
    const double* t;                                 // [n]
    const RemoveCandidate* cand;                     // [m] grouped by curve
    const long long* offset;                         // [curves + 1] of this launch's curves, into cand
    const double* profile;                           // [nK][M + 1]
    const double* sub;                               // [S]
    double* rows;                                    // [curves][n] in: the flux; out: the quotient
    double* model;                                   // [curves][n] out (nullptr: not wanted)
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    long long n, tiles_per_curve, tiles;             // tiles = curves * tiles_per_curve
    int nK, M, S;
};

__global__ void __launch_bounds__(kRemoveThreads) tls_remove_transits_kernel(const RemoveArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double remove_row[];           // [M + 1] the profile row the tile holds
    __shared__ int wave_inside[2][kRemoveWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, M = a.M, S = a.S;
    const double dS = (double)S, top = (double)(M - 1);
    TLS_CHECK(a, M >= 1 && M <= kTransitMaxM && S >= 1 && S <= kTransitMaxSub, kChkShape);
    int held = -1;                                   // the row in the LDS (the whole workgroup)
    unsigned turn = 0;                               // votes so far: the vote's two slots take turns
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long c = tile / a.tiles_per_curve;
        const long long i = (tile - c * a.tiles_per_curve) * kRemoveThreads + tid;
        const bool live = i < a.n;
        const long long at_point = c * a.n + i;
        double y = 1.0, model = 1.0, ti = 0.0;
        if (live) { y = a.rows[at_point]; ti = a.t[i]; }
        for (long long f = a.offset[c]; f < a.offset[c + 1]; ++f, ++turn) {
            const RemoveCandidate k = a.cand[f];
            const double lead = ti - k.T0;
            const double x = lead / k.P;
            const double xh = x + 0.5;
            const double e = floor(xh);
            const double ph = x - e;
            const double tau = ph * k.P;
            bool mine = false;
            if (live)
                for (int s = 0; s < S; ++s) {
                    const double ts = tau + a.sub[s];
                    const double off = ts - k.c0;
                    const double v = off * k.rh;
                    const double vv = v * v;
                    const double sc = k.cc * vv;
                    const double zz = k.bb + sc;
                    mine = mine || zz < k.e2;
                }
            const unsigned long long votes = __ballot(mine);
            if (lane == 0) wave_inside[turn & 1][wave] = votes != 0ull;
            wg_sync();                               // (the votes are in; the last candidate's reads of the row are done)
            bool any = false;
            for (int v = 0; v < kRemoveWaves; ++v) any = any || wave_inside[turn & 1][v] != 0;
            if (!any) continue;                      // (the whole workgroup)
            const int row = (int)k.row;
            TLS_CHECK(a, row >= 0 && row < a.nK, kChkShape);
            if (row != held) {
                for (int m = tid; m <= M; m += kRemoveThreads) remove_row[m] = a.profile[(long long)row * (M + 1) + m];
                held = row;
                wg_sync();
            }
            if (!mine) continue;
            double acc = 0.0;
            for (int s = 0; s < S; ++s) {
                const double ts = tau + a.sub[s];
                const double off = ts - k.c0;
                const double v = off * k.rh;
                const double vv = v * v;
                const double sc = k.cc * vv;
                const double zz = k.bb + sc;
                const bool inside = zz < k.e2;
                const double z = sqrt(inside ? zz : 0.0);
                const double q = z * k.sM;
                const double fl = fmin(floor(q), top);
                const double fr = q - fl;
                int at = (int)fl;
                TLS_CHECK(a, at >= 0 && at < M, kChkShape);
                at = at < 0 ? 0 : at > M - 1 ? M - 1 : at;
                const double p0 = remove_row[at], p1 = remove_row[at + 1];
                const double rise = p1 - p0;
                const double part = rise * fr;
                const double value = p0 + part;
                const double sample = inside ? value : 0.0;
                acc = acc + sample;
            }
            const double mval = acc / dS;
            if (mval > 0.0) {
                const double am = k.A * mval;
                const double mod = 1.0 - am;
                y = y / mod;
                model = model * mod;
            }
        }
        if (live) {
            a.rows[at_point] = y;
            if (a.model) a.model[at_point] = model;
        }
    }
}
