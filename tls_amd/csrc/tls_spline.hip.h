// tls_spline.hip.h -- robust B-spline detrending with a BIC-chosen knot spacing (tls_spline_detrend).  DESIGN.md "Spline
// detrending"; the statement is in include/tls_amd.h and, in Python, in tests/spline_spec.py.
//
// tls_spline_fit_kernel<LDS>: one workgroup of 256 threads a (segment, spacing, curve).  The segment's y, w and trend (24 bytes
// a point) and its membership bytes lie in the LDS up to kSplineLdsPoints points; a launch with a longer segment runs the same
// passes with w, the trend and the membership in device scratch and y read from the row.  A fit:
//   A  thread 0 owns W (the members' weights in index order).  Thread j owns interval j: its members are the contiguous range
//      [istart[j], iend[j]), and the thread adds their 10 + 4 products in index order in registers.  The band (4 doubles a
//      coefficient) and the right-hand side (1) lie in the LDS; they take the interval sums in four steps k = 3, 2, 1, 0 with a
//      barrier between them: in step k thread j adds to row j + k, so every row has one writer a step and receives its
//      intervals in ascending order.  More than 256 intervals run in chunks of 256, which keeps that order.  No atomics on
//      doubles, no reduction whose order depends on the launch.
//   B  thread 0 factors the band in place and substitutes: the statement's order is sequential.  The other workgroups of the
//      launch (curves x spacings x segments of them) hide that tail.
//   C  one thread a point evaluates the trend.
//   clip: the two medians of a round are tls_noise.hip.h's MSB-first radix selection on order-preserving keys (noise_median).
// The host forms the segment bounds and, for every (spacing, segment), q and h: the device takes no decision about the knots.
// tls_spline_pick_kernel: one workgroup a curve: the point-to-point sigma (two medians), the BIC of every spacing from its
// segment records, and the choice.  With several spacings a first launch of the fit kernel keeps the records alone; the pick
// follows; a second launch of the same fit at the chosen spacing writes trend, flat and the records that go out.
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_noise.hip.h.

constexpr int kSplineThreads = kNoiseThreads;        // (noise_select strides by kNoiseThreads)
constexpr int kSplineMaxSpacings = 16;
constexpr int kSplineMaxIter = 16;
constexpr int kSplineMaxCoef = 512;
constexpr int kSplineLdsPoints = 5120;               // 25 bytes a point: 125 KB beside 20 KB of band, 4 KB of ranges, 3 KB of words
constexpr int kSplineSegWords = 10;                  // tls_spline_segment
constexpr int kSplineCurveWords = 3 + kSplineMaxSpacings;   // tls_spline_curve
constexpr double kSplinePivot = 1e-10;
constexpr double kSplineK = 1.4826;

struct SplineShared {
    NoiseShared noise;                               // the selections' words
    double dword[4];                                 // 0 W; 1 sum w y; 2 sum (w r) r
    int iword[8];                                    // 0 |F|; 1 first member; 2 last member; 3 solved; 4 bad trend; 5 out this round
};
static_assert(sizeof(SplineShared) % 16 == 0, "the arrays behind the shared words are 16-byte aligned");

// band [4 mcap] | rhs [mcap] | istart [mcap] | iend [mcap] | (LDS) y [pcap] | w [pcap] | r [pcap] | member [pcap]; mcap, pcap even
constexpr size_t spline_lds_bytes(int mcap, int pcap, bool lds) {
    return sizeof(SplineShared) + (size_t)mcap * 48 + (lds ? (size_t)pcap * 25 : 0);
}

struct SplineArgs {
    const double* t;                                 // [n]
    const double* y;                                 // [R][n]
    const double* dy;                                // [R][n], or nullptr: w = 1.0
    const unsigned char* mask;                       // [R][n], or nullptr: nothing protected
    const long long* seg;                            // [G + 1]
    const int* q;                                    // [S_all][G] intervals of (spacing, segment); 0: T == 0
    const double* h;                                 // [S_all][G]
    const double* choice;                            // [R][kSplineCurveWords] (word 0: the spacing to fit), or nullptr: spacing blockIdx.y
    double* flat;                                    // [R][n], or nullptr: records only
    double* trend;                                   // [R][n]
    double* records;                                 // [R][S][G][kSplineSegWords]
    double* gw;                                      // [R * S][n] scratch of a launch with a long segment
    double* gr;
    unsigned char* gmember;
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    double penalty, sigma_upper, sigma_lower;
    long long n;
    int G, S, n_iter, mcap, pcap;                    // S: the spacings of this launch (gridDim.y)
};

struct SplineBasis { double b[4]; };

__device__ __forceinline__ SplineBasis spline_basis(double u) {
#pragma clang fp contract(off)
    SplineBasis o;
    const double u2 = u * u;
    const double u3 = u2 * u;
    const double om = 1.0 - u;
    const double om2 = om * om;
    const double om3 = om2 * om;
    const double t3 = 3.0 * u3;
    const double t2 = 3.0 * u2;
    const double t1 = 3.0 * u;
    const double s2 = 6.0 * u2;
    o.b[0] = om3 / 6.0;
    const double a1 = t3 - s2;
    const double a2 = a1 + 4.0;
    o.b[1] = a2 / 6.0;
    const double c1 = -t3 + t2;
    const double c2 = c1 + t1;
    const double c3 = c2 + 1.0;
    o.b[2] = c3 / 6.0;
    o.b[3] = u3 / 6.0;
    return o;
}

// the ten sums S[k][l], k <= l, of an interval: 0 1 2 3 | 4 5 6 | 7 8 | 9
__device__ __forceinline__ constexpr int spline_pair(int k, int l) { return k == 0 ? l : k == 1 ? 3 + l : k == 2 ? 5 + l : 9; }

template <bool LDS>
__global__ void __launch_bounds__(kSplineThreads) tls_spline_fit_kernel(const SplineArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char spline_lds[];
    SplineShared* sh = reinterpret_cast<SplineShared*>(spline_lds);
    const int tid = threadIdx.x;
    const int g = blockIdx.x;
    const long long c = blockIdx.z;
    const int slot = blockIdx.y;                     // where the record goes
    const int sp = a.choice ? (int)a.choice[c * kSplineCurveWords] : slot;
    const long long lo = a.seg[g], hi = a.seg[g + 1];
    const int L = (int)(hi - lo);
    const int q = a.q[(long long)sp * a.G + g];
    const double h = a.h[(long long)sp * a.G + g];
    const int m = q ? q + 3 : 0;
    TLS_CHECK(a, L >= 1 && m <= a.mcap && m <= kSplineMaxCoef && (!LDS || L <= a.pcap) && g < a.G && slot < a.S, kChkNoise);
    double* band = reinterpret_cast<double*>(spline_lds + sizeof(SplineShared));
    double* rhs = band + 4 * (size_t)a.mcap;
    int* istart = reinterpret_cast<int*>(rhs + a.mcap);
    int* iend = istart + a.mcap;
    double* l_y = reinterpret_cast<double*>(iend + a.mcap);
    const long long row = c * a.n + lo;
    const long long scratch = (c * a.S + slot) * a.n + lo;
    const double* t = a.t + lo;
    const double* g_y = a.y + row;
    const double* y_ = LDS ? l_y : g_y;
    double* w_ = LDS ? l_y + a.pcap : a.gw + scratch;
    double* r_ = LDS ? l_y + 2 * (size_t)a.pcap : a.gr + scratch;
    unsigned char* mem = LDS ? reinterpret_cast<unsigned char*>(l_y + 3 * (size_t)a.pcap) : a.gmember + scratch;
    const double t0 = t[0];
    auto place = [&](int i, double& u) -> int {
#pragma clang fp contract(off)
        const double d = t[i] - t0;
        const double x = d / h;
        int j = (int)x;
        if (j > q - 1) j = q - 1;
        u = x - (double)j;
        TLS_CHECK(a, j >= 0 && j < q, kChkNoise);
        return j < 0 ? 0 : j;
    };
    // the row, the weights and the first members
    for (int i = tid; i < L; i += kSplineThreads) {
        if (LDS) l_y[i] = g_y[i];
        double w = 1.0;
        if (a.dy) { const double e = a.dy[row + i]; const double ee = e * e; w = 1.0 / ee; }
        w_[i] = w;
        mem[i] = (a.mask && a.mask[row + i]) ? 0 : 1;
    }
    for (int j = tid; j < q; j += kSplineThreads) { istart[j] = 0; iend[j] = 0; }
    wg_sync();
    if (q) {
        for (int i = tid; i < L; i += kSplineThreads) {
            double u;
            const int j = place(i, u);
            if (i == 0 || place(i - 1, u) != j) istart[j] = i;
            if (i == L - 1 || place(i + 1, u) != j) iend[j] = i + 1;
        }
    }
    int rounds = 0, dropped = 0, status = 0, nF = 0;
    double sigma = (double)NAN;
    for (;;) {
        // ---- the members: their count, the first and the last
        if (tid == 0) { sh->iword[0] = 0; sh->iword[1] = 0x7fffffff; sh->iword[2] = -1; sh->iword[3] = 1; sh->iword[4] = 0; sh->iword[5] = 0; }
        wg_sync();
        {
            int mine = 0, first = 0x7fffffff, last = -1;
            for (int i = tid; i < L; i += kSplineThreads)
                if (mem[i]) { ++mine; if (i < first) first = i; last = i; }
            if (mine) { atomicAdd(&sh->iword[0], mine); atomicMin(&sh->iword[1], first); atomicMax(&sh->iword[2], last); }
        }
        wg_sync();
        nF = sh->iword[0];
        if (nF == 0 || q == 0 || !(t[sh->iword[2]] > t[sh->iword[1]])) { status = 1; break; }     // (the whole workgroup)
        // ---- A: W, the interval sums, the band
        for (int k = tid; k < m; k += kSplineThreads) { band[4 * k] = 0.0; band[4 * k + 1] = 0.0; band[4 * k + 2] = 0.0; band[4 * k + 3] = 0.0; rhs[k] = 0.0; }
        if (tid == 0) {
            double s = 0.0;
            for (int i = 0; i < L; ++i) if (mem[i]) s = s + w_[i];
            sh->dword[0] = s;
        }
        wg_sync();
        for (int j0 = 0; j0 < q; j0 += kSplineThreads) {
            const int j = j0 + tid;
            const bool active = j < q;
            double S[14];
#pragma unroll
            for (int e = 0; e < 14; ++e) S[e] = 0.0;
            if (active) {
                const int from = istart[j], to = iend[j];
                TLS_CHECK(a, from >= 0 && from <= to && to <= L, kChkNoise);
                for (int i = from; i < to; ++i) {
                    if (!mem[i]) continue;
                    double u;
                    place(i, u);
                    const SplineBasis B = spline_basis(u);
                    const double w = w_[i], yv = y_[i];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double wb = w * B.b[k];
#pragma unroll
                        for (int l = k; l < 4; ++l) { const double p = wb * B.b[l]; S[spline_pair(k, l)] = S[spline_pair(k, l)] + p; }
                        const double p = wb * yv;
                        S[10 + k] = S[10 + k] + p;
                    }
                }
            }
#pragma unroll
            for (int k = 3; k >= 0; --k) {
                if (active) {
                    const int cc = j + k;
                    TLS_CHECK(a, cc < m, kChkNoise);
#pragma unroll
                    for (int d = 0; k + d <= 3; ++d) band[4 * cc + d] = band[4 * cc + d] + S[spline_pair(k, k + d)];
                    rhs[cc] = rhs[cc] + S[10 + k];
                }
                wg_sync();
            }
        }
        {
            const double W = sh->dword[0];
            const double pw = W / (double)q;
            const double lam = a.penalty * pw;
            for (int cc = tid; cc < m; cc += kSplineThreads) {
                for (int d = 0; d < 3 && cc + d < m; ++d) {
                    int P = 0;                       // (D2^T D2)[cc][cc + d]
                    const int r0 = cc + d - 2 > 0 ? cc + d - 2 : 0, r1 = cc < m - 3 ? cc : m - 3;
                    for (int r = r0; r <= r1; ++r) { const int x = cc - r, z = cc + d - r; P += (x == 1 ? -2 : 1) * (z == 1 ? -2 : 1); }
                    const double add = lam * (double)P;
                    band[4 * cc + d] = band[4 * cc + d] + add;
                }
            }
        }
        wg_sync();
        // ---- B: thread 0 factors and substitutes; band[4 k + (i - k)] holds A[k][i], then L[i][k]
        if (tid == 0) {
            bool ok = true;
            for (int j = 0; j < m && ok; ++j) {
                const double ajj = band[4 * j];
                double s = ajj;
                for (int k = j - 3 > 0 ? j - 3 : 0; k < j; ++k) { const double l = band[4 * k + (j - k)]; const double p = l * l; s = s - p; }
                const double least = kSplinePivot * ajj;
                if (!(s > least)) { ok = false; break; }
                const double ljj = sqrt(s);
                band[4 * j] = ljj;
                const int top = j + 3 < m - 1 ? j + 3 : m - 1;
                for (int i = j + 1; i <= top; ++i) {
                    double v = band[4 * j + (i - j)];
                    for (int k = i - 3 > 0 ? i - 3 : 0; k < j; ++k) { const double p = band[4 * k + (i - k)] * band[4 * k + (j - k)]; v = v - p; }
                    band[4 * j + (i - j)] = v / ljj;
                }
            }
            if (ok) {
                for (int j = 0; j < m; ++j) {        // forward: z in rhs
                    double s = rhs[j];
                    for (int k = j - 3 > 0 ? j - 3 : 0; k < j; ++k) { const double p = band[4 * k + (j - k)] * rhs[k]; s = s - p; }
                    rhs[j] = s / band[4 * j];
                }
                for (int j = m - 1; j >= 0; --j) {   // back: c in rhs
                    double s = rhs[j];
                    const int top = j + 3 < m - 1 ? j + 3 : m - 1;
                    for (int k = j + 1; k <= top; ++k) { const double p = band[4 * j + (k - j)] * rhs[k]; s = s - p; }
                    rhs[j] = s / band[4 * j];
                }
            }
            sh->iword[3] = ok ? 1 : 0;
        }
        wg_sync();
        if (!sh->iword[3]) { status = 2; break; }
        // ---- C: the trend at every point
        {
            int bad = 0;
            for (int i = tid; i < L; i += kSplineThreads) {
                double u;
                const int j = place(i, u);
                const SplineBasis B = spline_basis(u);
                TLS_CHECK(a, j + 3 < m, kChkNoise);
                double p = rhs[j] * B.b[0];
                const double p1 = rhs[j + 1] * B.b[1];
                p = p + p1;
                const double p2 = rhs[j + 2] * B.b[2];
                p = p + p2;
                const double p3 = rhs[j + 3] * B.b[3];
                p = p + p3;
                r_[i] = p;
                if (!(p > 0.0 && p < (double)INFINITY)) bad = 1;
            }
            if (bad) atomicOr(&sh->iword[4], 1);
        }
        wg_sync();
        if (sh->iword[4]) { status = 2; break; }
        status = 0;
        if (rounds == a.n_iter) break;
        // ---- a clip round
        const double med = noise_median(a, &sh->noise, [&](int i, unsigned long long& k) {
            if (!mem[i]) return false;
            k = noise_key(y_[i] - r_[i]);
            return true;
        }, L, (unsigned int)nF);
        const double mad = noise_median(a, &sh->noise, [&](int i, unsigned long long& k) {
            if (!mem[i]) return false;
            const double r = y_[i] - r_[i];
            k = noise_key(fabs(r - med));
            return true;
        }, L, (unsigned int)nF);
        sigma = kSplineK * mad;
        if (sigma == 0.0) break;
        const double up = a.sigma_upper * sigma;
        const double dn = a.sigma_lower * sigma;
        const double down = -dn;
        auto out = [&](int i) -> bool { const double r = y_[i] - r_[i]; return mem[i] && (r > up || r < down); };
        {
            int mine = 0;
            for (int i = tid; i < L; i += kSplineThreads) mine += (int)out(i);
            if (mine) atomicAdd(&sh->iword[5], mine);
        }
        wg_sync();
        const int left = sh->iword[5];
        ++rounds;
        if (left == 0 || nF - left < 2) break;
        for (int i = tid; i < L; i += kSplineThreads) if (out(i)) mem[i] = 0;       // (a point belongs to one thread)
        dropped += left;
        wg_sync();
    }
    // (every thread took the same way out: the decisions above read LDS words behind a barrier)
    wg_sync();
    if (status != 0) {
        const bool everyone = nF == 0;
        if (tid == 0) {
            double s = 0.0;
            for (int i = 0; i < L; ++i) if (everyone || mem[i]) s = s + w_[i];
            sh->dword[0] = s;
        }
        if (tid == kWave) {
            double s = 0.0;
            for (int i = 0; i < L; ++i) if (everyone || mem[i]) { const double p = w_[i] * y_[i]; s = s + p; }
            sh->dword[1] = s;
        }
        wg_sync();
        const double mu = sh->dword[1] / sh->dword[0];
        for (int i = tid; i < L; i += kSplineThreads) r_[i] = mu;
        wg_sync();
    }
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < L; ++i) if (mem[i]) { const double r = y_[i] - r_[i]; const double p = w_[i] * r; const double pp = p * r; s = s + pp; }
        double* o = a.records + (((c * a.S + slot) * a.G) + g) * kSplineSegWords;
        o[0] = (double)status; o[1] = (double)q; o[2] = (double)m; o[3] = (double)L; o[4] = (double)nF; o[5] = (double)rounds;
        o[6] = (double)dropped; o[7] = sigma; o[8] = s; o[9] = nF ? sh->dword[0] : 0.0;
    }
    if (a.flat) {
        for (int i = tid; i < L; i += kSplineThreads) {
            const double tr = r_[i];
            a.trend[row + i] = tr;
            a.flat[row + i] = y_[i] / tr;
        }
    }
}

struct SplinePickArgs {
    const double* t;                                 // [n]
    const double* y;                                 // [R][n]
    const unsigned char* mask;                       // [R][n] or nullptr
    const double* records;                           // [R][S][G][kSplineSegWords]
    double* curves;                                  // [R][kSplineCurveWords]
    unsigned long long* check;
    double break_tolerance;
    int n, G, S;
};

// LDS: NoiseShared.  Grid (curves).
__global__ void __launch_bounds__(kSplineThreads) tls_spline_pick_kernel(const SplinePickArgs a) {
#pragma clang fp contract(off)
    __shared__ NoiseShared sh;
    const int tid = threadIdx.x, n = a.n;
    const long long c = blockIdx.x;
    const double* y = a.y + c * n;
    const unsigned char* mask = a.mask ? a.mask + c * n : nullptr;
    const double* t = a.t;
    const double tol = a.break_tolerance;
    auto pair = [&](int j) -> bool { return !(mask && (mask[j] || mask[j + 1])) && !(t[j + 1] - t[j] > tol); };
    if (tid == 0) sh.cnt[3] = 0u;
    wg_sync();
    unsigned int mine = 0u;
    for (int j = tid; j < n - 1; j += kSplineThreads) mine += (unsigned int)pair(j);
    atomicAdd(&sh.cnt[3], mine);
    wg_sync();
    const unsigned int pairs = sh.cnt[3];
    wg_sync();
    double pp = (double)NAN;
    if (pairs) {                                     // (the whole workgroup)
        const double med = noise_median(a, &sh, [&](int j, unsigned long long& k) {
            if (!pair(j)) return false;
            k = noise_key(y[j + 1] - y[j]);
            return true;
        }, n - 1, pairs);
        const double mad = noise_median(a, &sh, [&](int j, unsigned long long& k) {
            if (!pair(j)) return false;
            const double d = y[j + 1] - y[j];
            k = noise_key(fabs(d - med));
            return true;
        }, n - 1, pairs);
        const double scaled = kSplineK * mad;
        pp = scaled / kNoiseRoot2;
    }
    if (tid == 0) {
        double* o = a.curves + c * kSplineCurveWords;
        const double var = pp * pp;
        int best = -1;
        double least = 0.0;
        for (int s = 0; s < kSplineMaxSpacings; ++s) {
            double bic = (double)NAN;
            if (s < a.S) {
                double K = 0.0, N = 0.0, Q = 0.0, V = 0.0;           // (K and N: whole numbers, exact)
                for (int g = 0; g < a.G; ++g) {
                    const double* rec = a.records + ((c * a.S + s) * a.G + g) * kSplineSegWords;
                    if (rec[0] == 0.0) { K = K + rec[2]; N = N + rec[4]; Q = Q + rec[8]; V = V + rec[9]; }
                }
                const double lg = log(N);
                const double first = K * lg;
                const double mw = V / N;
                const double ssr = Q / mw;
                const double second = ssr / var;
                bic = first + second;
                if (bic > -(double)INFINITY && bic < (double)INFINITY && (best < 0 || bic < least)) { best = s; least = bic; }
            }
            o[3 + s] = bic;
        }
        const bool chosen = pp > 0.0 && best >= 0;
        o[0] = chosen ? (double)best : 0.0;
        o[1] = pp;
        o[2] = chosen ? 0.0 : 1.0;
    }
}
