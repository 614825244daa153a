// tls_match.hip.h -- the ephemeris match across the candidates of a batch (tls_ephemeris_match).
//
// The statement (include/tls_amd.h; tests/ephemeris_match_spec.py is the same in numpy; DESIGN.md "Ephemeris match").
// Candidate f is (star, P, T0, d in days, strength); it is good when P, T0, d, strength are finite, P > 0 and d > 0.  For
// a good f and every good g of another star, with (l, s) the member of the longer / the shorter period:
//   m = rint(P_l / P_s);  e = m * P_s;  dP = fabs(P_l - e);  c = span / P_l;  drift = dP * c
//   dmax = fmax(d_f, d_g);  plim = drift_tolerance * dmax;  elim = epoch_tolerance * dmax
//   period_match = m <= max_ratio and drift <= plim
//   x = (T0_l - T0_s) / P_s;  r = rint(x);  u = x - r;  dt = fabs(u) * P_s;  match = period_match and dt <= elim
// The record of f counts the g with period_match and m == 1, with period_match and with match, and holds the match of the
// largest strength (the lowest index among equals).  Every step is one IEEE double operation (contraction off: P_l - m * P_s
// as an FMA would lose the bits), counts are integers and the maximum takes no arithmetic, so the pairs may be split and
// combined in any order and the record still equals the host statement bit for bit.
//
// tls_match_pairs_kernel: one thread a candidate f, kMatchTile threads a workgroup, blockIdx.y one chunk of the g range.
// The g side passes through the LDS in tiles of kMatchTile candidates, six 8-byte words each (P, T0, d, strength, c_g =
// span / P_g, star: 12 KB); every lane of a wave reads the same g, a broadcast without bank conflict.  A g that is bad, or
// past n, is staged with P = NaN: m is NaN then and every comparison false, so it is invisible without a test of its own;
// g == f fails the star test, and a bad f is given P = NaN as well.  c is chosen between c_f and c_g by the same P_f >= P_g
// that chooses l, so span / P_l is one division per staged candidate, not one a pair.  Most pairs end at m <= max_ratio or
// drift <= plim behind the one division P_l / P_s; the epoch arithmetic, with its second division, is behind that test.
// The chunks cut the tile range into near-equal runs (match_chunks below) so that a few thousand candidates already give
// every CU a workgroup; a chunk's result is a partial record, 48 bytes.
// tls_match_combine_kernel: one thread a candidate: the counts of its partial records added, the best match taken over
// the chunks in ascending order with a strict comparison -- chunks ascend in g, so the lowest index among equals stays --
// and the record written.  No atomics, no sum of doubles.
//
// Included by tls_kernels.hip.h (namespace tlsdev).

constexpr int kMatchTile = 256;                      // candidates a workgroup, and staged at a time
constexpr int kMatchTargetGroups = 1024;             // workgroups the chunking aims at: four a CU
constexpr int kMatchMaxChunks = 16;
constexpr int kMatchWords = 10;                      // tls_match_record
constexpr long long kMatchMaxCandidates = 1ll << 20;
constexpr int kMatchMaxRatio = 64;

struct MatchStaged {                                 // a candidate of the g side in the LDS
    double P, T0, d, strength, c;
    long long star;
};
static_assert(sizeof(MatchStaged) == 48, "six 8-byte words");

struct MatchPartial {                                // a candidate's record over one chunk of the g range
    int n_same, n_period, n_match, best;             // best: -1 without a match
    double strength, ratio, dt, drift;               // of the best match
};
static_assert(sizeof(MatchPartial) == 48, "four ints and four doubles");

struct MatchArgs {
    const long long* star;                           // [n]
    const double* period; const double* T0; const double* duration; const double* strength;   // [n]
    MatchPartial* partial;                           // [chunks][n]
    double* out;                                     // [n][kMatchWords]
    double span, drift_tolerance, epoch_tolerance, max_ratio;
    int n, tiles, chunks;
};

// the chunks of the g range for n candidates (tiles = ceil(n / kMatchTile) > 0): enough of them to reach
// kMatchTargetGroups workgroups, at most kMatchMaxChunks and at most one a tile; chunk c holds the tiles
// [c * tiles / chunks, (c + 1) * tiles / chunks)
inline int match_chunks(int tiles) {
    const int want = (kMatchTargetGroups + tiles - 1) / tiles;     // (the f side has `tiles` workgroups a chunk; >= 1)
    const int most = tiles < kMatchMaxChunks ? tiles : kMatchMaxChunks;
    return want < most ? want : most;
}

__device__ __forceinline__ bool match_good(double P, double T0, double d, double s) {
    return isfinite(P) && isfinite(T0) && isfinite(d) && isfinite(s) && P > 0.0 && d > 0.0;
}

__global__ void __launch_bounds__(kMatchTile) tls_match_pairs_kernel(const MatchArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) MatchStaged staged[kMatchTile];
    const int tid = threadIdx.x;
    const int f = blockIdx.x * kMatchTile + tid;
    const double nan = (double)NAN;
    double Pf = nan, T0f = 0.0, df = 0.0, sf = 0.0;
    long long star_f = 0;
    if (f < a.n) {
        const double P = a.period[f];
        T0f = a.T0[f]; df = a.duration[f]; sf = a.strength[f]; star_f = a.star[f];
        if (match_good(P, T0f, df, sf)) Pf = P;
    }
    const double cf = a.span / Pf;
    const int tile_lo = (int)((long long)blockIdx.y * a.tiles / a.chunks);
    const int tile_hi = (int)((long long)(blockIdx.y + 1) * a.tiles / a.chunks);
    int n_same = 0, n_period = 0, n_match = 0, best = -1;
    double best_s = nan, best_ratio = nan, best_dt = nan, best_drift = nan;
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        const int g0 = tile * kMatchTile;
        wg_sync();                                   // (the last tile has been read)
        {
            const int g = g0 + tid;
            MatchStaged s;
            s.P = nan; s.T0 = 0.0; s.d = 0.0; s.strength = 0.0; s.star = 0;
            if (g < a.n) {
                const double P = a.period[g];
                s.T0 = a.T0[g]; s.d = a.duration[g]; s.strength = a.strength[g]; s.star = a.star[g];
                if (match_good(P, s.T0, s.d, s.strength)) s.P = P;
            }
            s.c = a.span / s.P;
            staged[tid] = s;
        }
        wg_sync();
#pragma unroll 4
        for (int j = 0; j < kMatchTile; ++j) {
            const MatchStaged s = staged[j];         // (the same word in every lane)
            const bool f_long = Pf >= s.P;           // (false for a NaN on either side: m is NaN below)
            const double Pl = f_long ? Pf : s.P, Ps = f_long ? s.P : Pf;
            const double c = f_long ? cf : s.c;
            const double m = rint(Pl / Ps);
            const double e = m * Ps;
            const double dP = fabs(Pl - e);
            const double drift = dP * c;
            const double dmax = fmax(df, s.d);
            const double plim = a.drift_tolerance * dmax;
            if (s.star != star_f && m <= a.max_ratio && drift <= plim) {
                n_period += 1;
                n_same += m == 1.0 ? 1 : 0;
                const double T0l = f_long ? T0f : s.T0, T0s = f_long ? s.T0 : T0f;
                const double x = (T0l - T0s) / Ps;
                const double r = rint(x);
                const double u = x - r;
                const double dt = fabs(u) * Ps;
                const double elim = a.epoch_tolerance * dmax;
                if (dt <= elim) {
                    n_match += 1;
                    if (best < 0 || s.strength > best_s) {   // (g ascends: the lowest index among equals stays)
                        best = g0 + j; best_s = s.strength;
                        best_ratio = s.P >= Pf ? m : -m;
                        best_dt = dt; best_drift = drift;
                    }
                }
            }
        }
    }
    if (f < a.n) {
        MatchPartial p;
        p.n_same = n_same; p.n_period = n_period; p.n_match = n_match; p.best = best;
        p.strength = best_s; p.ratio = best_ratio; p.dt = best_dt; p.drift = best_drift;
        a.partial[(size_t)blockIdx.y * a.n + f] = p;
    }
}

__global__ void __launch_bounds__(kMatchTile) tls_match_combine_kernel(const MatchArgs a) {
    const int f = blockIdx.x * kMatchTile + threadIdx.x;
    if (f >= a.n) return;
    const double nan = (double)NAN;
    double* out = a.out + (size_t)f * kMatchWords;
    const double sf = a.strength[f];
    if (!match_good(a.period[f], a.T0[f], a.duration[f], sf)) {
        out[0] = 1.0;
#pragma unroll
        for (int k = 1; k < kMatchWords; ++k) out[k] = nan;
        return;
    }
    MatchPartial best = a.partial[f];
    int n_same = best.n_same, n_period = best.n_period, n_match = best.n_match;
    for (int c = 1; c < a.chunks; ++c) {
        const MatchPartial p = a.partial[(size_t)c * a.n + f];
        n_same += p.n_same; n_period += p.n_period; n_match += p.n_match;
        if (p.best >= 0 && (best.best < 0 || p.strength > best.strength)) best = p;
    }
    const bool found = best.best >= 0;
    out[0] = 0.0;
    out[1] = (double)n_same; out[2] = (double)n_period; out[3] = (double)n_match;
    out[4] = (double)best.best;
    out[5] = found ? best.ratio : nan; out[6] = found ? best.dt : nan; out[7] = found ? best.drift : nan;
    out[8] = found ? best.strength : nan;
    out[9] = found ? (best.strength > sf ? 1.0 : 0.0) : nan;
}
