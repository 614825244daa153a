// tls_prewhiten.hip.h -- iterative sinusoid pre-whitening (tls_prewhiten): the step kernel that follows every periodogram of
// the loop, and the kernel that closes a call.  DESIGN.md "Pre-whitening"; tests/prewhiten_spec.py is the statement in Python.
//
// The statement, for a curve y [n] (weights from dy [n], or uniform) over the shared time stamps t [n] and the grid f [F];
// r starts as y, trend as 0.0.  Iteration j = 0 .. K - 1, while the curve runs:
//   spectrum: the periodogram of r on the grid (tls_gls.hip.h: the prologue in index order, the dense product, the epilogue;
//       the sums of the weights are formed once a call); ybar_0 = the mean of the first prologue
//   pick: k = the first index of the largest finite power; none: status 2, the curve stops; power[k] < min_power: status 1,
//       the curve stops
//   refine: with 0 < k < F - 1, both neighbours finite and den = p[k-1] - 2.0 * p[k] + p[k+1] < 0:
//       half = 0.5 * (f[k+1] - f[k-1]);  f* = f[k] + 0.5 * half * (p[k-1] - p[k+1]) / den;        otherwise f* = f[k]
//   for h = 1 .. H, each on the row the harmonic before left:  fh = h * f*;  the sine test's statement without a mask
//       (ordered 256-lane sums: W, ybar, YY; the six sums at fh and 2.0 * fh of the rounded products; the epilogue with
//       ca and sa); NaN: the harmonic is skipped (term status 1); otherwise, for every i,
//       u = cos phi_i - C;  v = sin phi_i - S;  q = ca * u + sa * v;  r_i = r_i - q;  trend_i = trend_i + q
// At the end trend_i = ybar_0 + trend_i and flat_i = y_i / trend_i.  One IEEE double operation a step, contraction off.
//
// tls_prewhiten_step_kernel<LDS>: one workgroup of 256 threads a curve.  Thread j keeps the best (power, index) of the
// frequencies j, j + 256, ... (a later one wins only when strictly larger); thread 0 merges the 256 in lane order with the
// same rule plus "the lower index of equals", so the pick is the first index of the maximum whatever the order.  Thread 0
// decides and refines.  With LDS the row (n doubles) and the (cos, sin) pairs of the current harmonic (n double2, 16-byte
// aligned behind the row) sit in the LDS: 24 bytes a point behind the 12.4 KB of partial sums, up to kPrewhitenLdsPoints
// points.  Thread tid owns the points tid, tid + 256, ...: in every pass the 64 lanes of a wave read 512 contiguous bytes of
// the row and 1 KB of the pairs, one access an instruction: no bank conflicts.  The pairs are written by the pass of the six
// sums and read again by the subtraction, which so needs no trigonometry of its own.  A longer row takes the same passes
// through global memory and evaluates the pairs twice (the same instructions on the same inputs: the same bits).
// Included by tls_kernels.hip.h (namespace tlsdev) behind tls_gls.hip.h.

constexpr int kPrewhitenThreads = 256;
constexpr int kPrewhitenWords = 16;                  // tls_prewhiten_term
constexpr int kPrewhitenMaxTerms = 32;
constexpr int kPrewhitenLdsPoints = 6144;            // 24 bytes a point: 144 KB of the 160 KB behind the partial sums
constexpr int kPrewhitenFixedDoubles = 6 * kPrewhitenThreads + 16;   // partial sums [6][256] | totals and broadcast words

constexpr size_t prewhiten_lds_bytes(int n, bool lds) {
    return (size_t)kPrewhitenFixedDoubles * 8 + (lds ? ((size_t)(n + (n & 1)) * 8 + (size_t)n * 16) : 0);
}

// the epilogue with the coefficients of the fit: gls_epilogue's steps, ca and sa kept
__device__ __forceinline__ void gls_epilogue_fit(double YC, double YS, double C, double S, double C2, double S2, double YY,
                                                 double* power, double* amplitude, double* phase, double* ca_out, double* sa_out) {
#pragma clang fp contract(off)
    const double hp = 1.0 + C2, hm = 1.0 - C2;
    const double c2 = C * C, s2 = S * S, cs = C * S;
    const double CC = 0.5 * hp - c2;
    const double SS = 0.5 * hm - s2;
    const double CS = 0.5 * S2 - cs;
    const double D = CC * SS - CS * CS;
    if (!(D > 0.0) || !(YY > 0.0)) {
        *power = (double)NAN; *amplitude = (double)NAN; *phase = (double)NAN; *ca_out = (double)NAN; *sa_out = (double)NAN;
        return;
    }
    const double p1 = SS * YC * YC;
    const double p2 = CC * YS * YS;
    const double p3 = 2.0 * CS * YC * YS;
    const double num = p1 + p2 - p3;
    const double den = YY * D;
    *power = num / den;
    const double ca = (YC * SS - YS * CS) / D;
    const double sa = (YS * CC - YC * CS) / D;
    *amplitude = sqrt(ca * ca + sa * sa);
    *phase = atan2(sa, ca) / kGlsTwoPi;
    *ca_out = ca; *sa_out = sa;
}

struct PrewhitenArgs {
    const double* t;                                 // [n]
    const double* f;                                 // [F]
    const double* dy;                                // [R][n], or nullptr: uniform weights
    const double* power;                             // [R][F] of this iteration
    double* r;                                       // [R][n] the rows, resident for the call
    double* trend;                                   // [R][n] the sum of what was subtracted
    double* terms;                                   // [R][K][H][kPrewhitenWords]
    double* sums;                                    // [R][K][H][6] YC YS C S C2 S2
    double* steps;                                   // [K * H + 1][R][n] the row entering every (iteration, harmonic), or nullptr
    int* active;                                     // [R] 1 while the curve runs
    long long* n_iterations;                         // [R]
    double* status;                                  // [R]
    unsigned long long* counts;                      // [K] the curves that go on behind iteration j
    double min_power;
    int n, F, R, K, H, j;
};

// MASKED (tls_prewhiten_masked; mask_rows [R][n], != 0: protected): the weights of the fit are v_i / W with v_i = 0.0 at a
// protected point and 1.0 / (dy_i * dy_i) or, without dy, 1.0 elsewhere, W their ordered lane sum; the subtraction and the trend
// cover every point.  (A row with fewer than 3 unprotected points never gets here: every power of it is NaN.)
template <bool LDS, bool MASKED>
__device__ __forceinline__ void prewhiten_step(const PrewhitenArgs& a, const unsigned char* mask_rows) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double prewhiten_lds[];
    double (*part)[kPrewhitenThreads] = reinterpret_cast<double (*)[kPrewhitenThreads]>(prewhiten_lds);
    double* total = prewhiten_lds + 6 * kPrewhitenThreads;           // [16]: 0-5 sums, 6 go, 7 f*, 8-11 ca sa C S, 12 fitted
    const int tid = threadIdx.x, n = a.n, F = a.F, H = a.H, j = a.j;
    const long long c = blockIdx.x;
    const long long at = c * n;
    const double nan = (double)NAN;
    double* g_row = a.r + at;
    double* row = LDS ? total + 16 : g_row;
    double2* pair = LDS ? reinterpret_cast<double2*>(row + n + (n & 1)) : nullptr;
    const long long plane = (long long)a.R * n;
    auto snapshot = [&](int h, const double* from) {
        if (!a.steps) return;
        double* to = a.steps + ((long long)j * H + h) * plane + at;
        for (int i = tid; i < n; i += kPrewhitenThreads) to[i] = from[i];
    };
    if (!a.active[c]) {                              // (the whole workgroup) a stopped curve: its row is final
        for (int h = 0; h < H; ++h) snapshot(h, g_row);
        return;
    }
    // ---- pick: the first index of the largest finite power
    const double* p = a.power + c * F;
    double best = -1.0;
    int best_k = -1;
    for (int k = tid; k < F; k += kPrewhitenThreads) {
        const double v = p[k];
        if (isfinite(v) && (best_k < 0 || v > best)) { best = v; best_k = k; }
    }
    part[0][tid] = best;
    part[1][tid] = (double)best_k;
    wg_sync();
    double* term = a.terms + ((c * a.K + j) * H) * kPrewhitenWords;
    if (tid == 0) {
        double top = 0.0;
        int k = -1;
        for (int m = 0; m < kPrewhitenThreads; ++m) {
            const int km = (int)part[1][m];
            const double v = part[0][m];
            if (km >= 0 && (k < 0 || v > top || (v == top && km < k))) { top = v; k = km; }
        }
        double go = 1.0, fstar = nan;
        if (k < 0) { go = 0.0; a.status[c] = 2.0; }
        else if (top < a.min_power) { go = 0.0; a.status[c] = 1.0; }
        else {
            const double fk = a.f[k];
            const double left = k > 0 ? p[k - 1] : nan, right = k < F - 1 ? p[k + 1] : nan;
            fstar = fk;
            if (k > 0 && k < F - 1 && isfinite(left) && isfinite(right)) {
                const double twice = 2.0 * top;
                const double d1 = left - twice;
                const double den = d1 + right;
                if (den < 0.0) {
                    const double span = a.f[k + 1] - a.f[k - 1];
                    const double half = 0.5 * span;
                    const double hh = 0.5 * half;
                    const double diff = left - right;
                    const double mv = hh * diff;
                    const double shift = mv / den;
                    fstar = fk + shift;
                }
            }
            for (int h = 0; h < H; ++h) {
                double* o = term + h * kPrewhitenWords;
                o[1] = (double)k; o[2] = fk; o[3] = left; o[4] = top; o[5] = right;
            }
        }
        total[6] = go; total[7] = fstar;
        if (go == 0.0) a.active[c] = 0;
    }
    wg_sync();
    const bool go = total[6] != 0.0;
    const double fstar = total[7];
    if (!go) {
        for (int h = 0; h < H; ++h) snapshot(h, g_row);
        return;
    }
    if (LDS) {
        for (int i = tid; i < n; i += kPrewhitenThreads) row[i] = g_row[i];
        // (every thread reads back only what it wrote: no barrier)
    }
    const double* dy = a.dy ? a.dy + at : nullptr;
    const unsigned char* mask = MASKED ? mask_rows + at : nullptr;
    [[maybe_unused]] auto inverse_variance = [&](int i) -> double {   // (MASKED only)
#pragma clang fp contract(off)
        if (mask[i]) return 0.0;
        if (!dy) return 1.0;
        const double e = dy[i]; const double pp = e * e;
        return 1.0 / pp;
    };
    const double t0 = a.t[0];
    // the lanes of a sum are added by one thread in lane order
    auto lanes = [&](double mine) -> double {
#pragma clang fp contract(off)
        part[0][tid] = mine;
        wg_sync();
        if (tid == 0) { double s = part[0][0]; for (int m = 1; m < kPrewhitenThreads; ++m) s = s + part[0][m]; total[0] = s; }
        wg_sync();
        const double s = total[0];
        wg_sync();
        return s;
    };
    double W = 1.0;
    if constexpr (MASKED) {
        double sv = 0.0;
        for (int i = tid; i < n; i += kPrewhitenThreads) { const double v = inverse_variance(i); sv = sv + v; }
        W = lanes(sv);
    } else if (dy) {
        double sv = 0.0;
        for (int i = tid; i < n; i += kPrewhitenThreads) { const double e = dy[i]; const double pp = e * e; const double v = 1.0 / pp; sv = sv + v; }
        W = lanes(sv);
    }
    const double uniform = 1.0 / (double)n;
    auto weight = [&](int i) -> double {
#pragma clang fp contract(off)
        if constexpr (MASKED) { const double v = inverse_variance(i); return v / W; }
        if (!dy) return uniform;
        const double e = dy[i]; const double pp = e * e; const double v = 1.0 / pp;
        return v / W;
    };
    double* trend = a.trend + at;
    for (int h = 0; h < H; ++h) {
        snapshot(h, row);
        double sy = 0.0;
        for (int i = tid; i < n; i += kPrewhitenThreads) { const double q = weight(i) * row[i]; sy = sy + q; }
        const double ybar = lanes(sy);
        double syy = 0.0;
        for (int i = tid; i < n; i += kPrewhitenThreads) {
            const double dd = row[i] - ybar;
            const double av = weight(i) * dd;
            const double q = av * dd;
            syy = syy + q;
        }
        const double YY = lanes(syy);
        const double fh = (double)(h + 1) * fstar;
        const double fh2 = 2.0 * fh;
        double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += kPrewhitenThreads) {
            const double w = weight(i);
            const double dd = row[i] - ybar;
            const double av = w * dd;
            const double lead = a.t[i] - t0;
            double s1, c1, s2, c2;
            sincos(gls_phase(fh, lead), &s1, &c1);
            sincos(gls_phase(fh2, lead), &s2, &c2);
            if (LDS) pair[i] = make_double2(c1, s1);
            const double q0 = av * c1, q1 = av * s1, q2 = w * c1, q3 = w * s1, q4 = w * c2, q5 = w * s2;
            s6[0] = s6[0] + q0; s6[1] = s6[1] + q1; s6[2] = s6[2] + q2;
            s6[3] = s6[3] + q3; s6[4] = s6[4] + q4; s6[5] = s6[5] + q5;
        }
#pragma unroll
        for (int s = 0; s < 6; ++s) part[s][tid] = s6[s];
        wg_sync();
        if (tid < 6) { double s = part[tid][0]; for (int m = 1; m < kPrewhitenThreads; ++m) s = s + part[tid][m]; total[tid] = s; }
        wg_sync();
        if (tid == 0) {
            double power, amplitude, phase, ca, sa;
            gls_epilogue_fit(total[0], total[1], total[2], total[3], total[4], total[5], YY, &power, &amplitude, &phase, &ca, &sa);
            const bool fitted = !isnan(power);
            double* o = term + h * kPrewhitenWords;
            o[0] = fitted ? 0.0 : 1.0; o[6] = fh; o[7] = ybar; o[8] = YY; o[9] = ca; o[10] = sa; o[11] = total[2]; o[12] = total[3];
            o[13] = power; o[14] = amplitude; o[15] = phase;
            double* os = a.sums + ((c * a.K + j) * H + h) * 6;
            for (int s = 0; s < 6; ++s) os[s] = total[s];
            total[8] = ca; total[9] = sa; total[10] = total[2]; total[11] = total[3]; total[12] = fitted ? 1.0 : 0.0;
        }
        wg_sync();
        const double ca = total[8], sa = total[9], C = total[10], S = total[11];
        const bool fitted = total[12] != 0.0;
        if (fitted) {
            for (int i = tid; i < n; i += kPrewhitenThreads) {
                double c1, s1;
                if (LDS) { const double2 cs = pair[i]; c1 = cs.x; s1 = cs.y; }
                else sincos(gls_phase(fh, a.t[i] - t0), &s1, &c1);
                const double u = c1 - C;
                const double v = s1 - S;
                const double m1 = ca * u;
                const double m2 = sa * v;
                const double q = m1 + m2;
                row[i] = row[i] - q;
                trend[i] = trend[i] + q;
            }
        }
        wg_sync();                                   // (the next harmonic overwrites the partials and the totals)
    }
    if (LDS) for (int i = tid; i < n; i += kPrewhitenThreads) g_row[i] = row[i];
    if (tid == 0) {
        a.n_iterations[c] = j + 1;
        if (j + 1 < a.K) atomicAdd(&a.counts[j], 1ull);
        else a.active[c] = 0;
    }
}

template <bool LDS>
__global__ void __launch_bounds__(kPrewhitenThreads) tls_prewhiten_step_kernel(const PrewhitenArgs a) {
    prewhiten_step<LDS, false>(a, nullptr);
}

template <bool LDS>
__global__ void __launch_bounds__(kPrewhitenThreads) tls_prewhiten_step_masked_kernel(const PrewhitenArgs a, const unsigned char* mask) {
    prewhiten_step<LDS, true>(a, mask);
}

struct PrewhitenFinishArgs {
    const double* y;                                 // [R][n]
    const double* mean0;                             // [R] ybar_0
    double* trend;                                   // [R][n] in: the sum; out: the trend
    double* flat;                                    // [R][n]
    long long count;                                 // R * n
    int n;
};

__global__ void __launch_bounds__(kPrewhitenThreads) tls_prewhiten_finish_kernel(const PrewhitenFinishArgs a) {
#pragma clang fp contract(off)
    for (long long e = (long long)blockIdx.x * kPrewhitenThreads + threadIdx.x; e < a.count; e += (long long)gridDim.x * kPrewhitenThreads) {
        const double tr = a.mean0[e / a.n] + a.trend[e];
        a.trend[e] = tr;
        a.flat[e] = a.y[e] / tr;
    }
}
