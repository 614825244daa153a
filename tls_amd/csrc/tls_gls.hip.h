// tls_gls.hip.h -- the generalised (floating-mean, weighted) Lomb-Scargle periodogram of Zechmeister & Kuerster 2009
// (tls_nudft, tls_lomb_scargle) and the per-candidate sine test (tls_sine_test).  DESIGN.md "Variability periodogram";
// tests/gls_spec.py is the statement in Python.
//
// The statement, for a curve y [n] (weights from dy [n], or uniform) over the shared time stamps t [n], t_0 = t[0]:
//   prologue, every sum in index order:
//       v_i = 1.0 / (dy_i * dy_i);  W = sum v_i;  w_i = v_i / W        (without dy: w_i = 1.0 / n)
//       ybar = sum (w_i * y_i);  d_i = y_i - ybar;  a_i = w_i * d_i;  YY = sum (a_i * d_i)
//   phase of (frequency f, point i):  e = t_i - t_0;  x = f * e;  r = x - floor(x);  phi = 6.283185307179586 * r
//   six sums:  YC, YS = sum a_i cos phi, sum a_i sin phi;  C, S = sum w_i cos phi, sum w_i sin phi;
//              C2, S2 = the same two of w at the frequency 2.0 * f
//   epilogue (gls_epilogue below), one IEEE operation a step.
//
// tls_nudft_kernel<RJ> is the dense product behind the six sums: out[r][k] = (sum_i A[r][i] cos phi_ki, sum_i A[r][i] sin phi_ki).
// One workgroup of 256 threads owns a tile of 32 * RJ rows x 64 frequencies and walks the time axis in chunks of 32 points.
// A chunk of A (32 x 32 RJ doubles, a point's rows contiguous) and the chunk's (cos, sin) pairs (32 x 64 double2) are staged
// in the LDS; a pair is generated ONCE per workgroup and chunk (8 sincos a thread) and serves every row of the tile, so the
// trigonometry is amortised over the row tile.  Thread (tx, ty) = (tid % 16, tid / 16) keeps 2 RJ rows x 4 frequencies x
// (cos, sin) accumulators in registers: rows 32 j + 2 tx + {0, 1}, frequencies 16 m + ty.  A point costs it RJ + 4
// ds_read_b128 -- the 16 tx of a 16-lane group read 256 contiguous bytes, the ty of a wave 64 contiguous bytes, everything
// else is a broadcast: no bank conflicts -- against 16 RJ fp64 FMAs.  The sum of an output runs over i ascending in one
// thread, so a result does not depend on the launch.  RJ = 4 (128 rows) is the product; RJ = 1 (32 rows) serves the one
// shared weight row and batches of at most 32 rows.
//
// tls_gls_prologue_kernel: one workgroup a curve; the terms of a sum are formed by all threads into the LDS, tile by tile,
// and added by thread 0 in index order.  tls_gls_epilogue_kernel: one thread a (curve, frequency).
// tls_sine_test_kernel: one workgroup a candidate (a launch of fewer workgroups strides over them); see there.
// Included by tls_kernels.hip.h (namespace tlsdev).

constexpr int kGlsThreads = 256;
constexpr int kGlsFreqTile = 64;                     // frequencies of a workgroup's tile
constexpr int kGlsChunk = 32;                        // points of a chunk
constexpr int kGlsRowsPerJ = 32;                     // rows of a tile = kGlsRowsPerJ * RJ
constexpr int kGlsRowTile = 128;                     // RJ = 4
constexpr int kGlsSmallRows = 32;                    // RJ = 1: batches of at most this many rows
constexpr int kGlsMaxPoints = 1 << 22;
constexpr int kGlsTile = 2048;                       // terms of the prologue's LDS tile
constexpr int kSineThreads = 256;
constexpr int kSineMaxHarmonics = 8;
constexpr int kSineWords = 4;                        // tls_sine_record
constexpr int kSineHarmonicWords = 5;                // tls_sine_harmonic
constexpr double kGlsTwoPi = 6.283185307179586;      // numpy's 2 * pi

// phi of (frequency f, lead e = t_i - t_0): the phase is reduced in cycles before it is scaled
__device__ __forceinline__ double gls_phase(double f, double e) {
#pragma clang fp contract(off)
    const double x = f * e;
    const double r = x - floor(x);
    return kGlsTwoPi * r;
}

// the epilogue of one (curve, frequency), one IEEE operation a step in the order of the statement
__device__ __forceinline__ void gls_epilogue(double YC, double YS, double C, double S, double C2, double S2, double YY,
                                             double* power, double* amplitude, double* phase) {
#pragma clang fp contract(off)
    const double hp = 1.0 + C2, hm = 1.0 - C2;
    const double c2 = C * C, s2 = S * S, cs = C * S;
    const double CC = 0.5 * hp - c2;
    const double SS = 0.5 * hm - s2;
    const double CS = 0.5 * S2 - cs;
    const double D = CC * SS - CS * CS;
    if (!(D > 0.0) || !(YY > 0.0)) { *power = (double)NAN; *amplitude = (double)NAN; *phase = (double)NAN; return; }
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
}

struct NudftArgs {
    const double* A;                                 // [R][lda]
    const double* t;                                 // [n]
    const double* f;                                 // [F]
    double2* out;                                    // [R][F] (cos sum, sin sum)
    long long lda;
    int R, n, F;
};

template <int RJ>
__global__ void __launch_bounds__(kGlsThreads) tls_nudft_kernel(const NudftArgs a) {
#pragma clang fp contract(off)
    constexpr int kRows = kGlsRowsPerJ * RJ;
    constexpr int kStride = kRows + 2;               // (a point's rows, padded by one 16-byte slot: the staging writes spread)
    __shared__ __attribute__((aligned(16))) double s_a[kGlsChunk * kStride];
    __shared__ double2 s_trig[kGlsChunk * kGlsFreqTile];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int f0 = blockIdx.x * kGlsFreqTile, r0 = blockIdx.y * kRows;
    const int n = a.n;
    const double t0 = a.t[0];
    double acc_c[2 * RJ][4], acc_s[2 * RJ][4];
#pragma unroll
    for (int j = 0; j < 2 * RJ; ++j)
#pragma unroll
        for (int m = 0; m < 4; ++m) { acc_c[j][m] = 0.0; acc_s[j][m] = 0.0; }
    for (int i0 = 0; i0 < n; i0 += kGlsChunk) {
        // the chunk of A: element e = (row e / 32, point e % 32); rows and points past the end are zeros
#pragma unroll
        for (int q = 0; q < kRows * kGlsChunk / kGlsThreads; ++q) {
            const int e = q * kGlsThreads + tid;
            const int row = e / kGlsChunk, k = e % kGlsChunk;
            const int r = r0 + row, i = i0 + k;
            s_a[k * kStride + row] = (r < a.R && i < n) ? a.A[(long long)r * a.lda + i] : 0.0;
        }
        // the chunk's pairs: entry e = (point e / 64, frequency e % 64); a point past the end meets zeros of A
#pragma unroll
        for (int q = 0; q < kGlsChunk * kGlsFreqTile / kGlsThreads; ++q) {
            const int e = q * kGlsThreads + tid;
            const int k = e / kGlsFreqTile, fl = e % kGlsFreqTile;
            const int i = i0 + k < n ? i0 + k : n - 1;
            const double f = f0 + fl < a.F ? a.f[f0 + fl] : 0.0;
            const double lead = a.t[i] - t0;
            double s, c;
            sincos(gls_phase(f, lead), &s, &c);
            s_trig[e] = make_double2(c, s);
        }
        wg_sync();
#pragma unroll 4
        for (int k = 0; k < kGlsChunk; ++k) {
            double2 av[RJ], tv[4];
#pragma unroll
            for (int j = 0; j < RJ; ++j) av[j] = *reinterpret_cast<const double2*>(&s_a[k * kStride + kGlsRowsPerJ * j + 2 * tx]);
#pragma unroll
            for (int m = 0; m < 4; ++m) tv[m] = s_trig[k * kGlsFreqTile + 16 * m + ty];
#pragma unroll
            for (int j = 0; j < RJ; ++j)
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    acc_c[2 * j][m] = __builtin_fma(av[j].x, tv[m].x, acc_c[2 * j][m]);
                    acc_s[2 * j][m] = __builtin_fma(av[j].x, tv[m].y, acc_s[2 * j][m]);
                    acc_c[2 * j + 1][m] = __builtin_fma(av[j].y, tv[m].x, acc_c[2 * j + 1][m]);
                    acc_s[2 * j + 1][m] = __builtin_fma(av[j].y, tv[m].y, acc_s[2 * j + 1][m]);
                }
        }
        wg_sync();                                   // (the next chunk overwrites the LDS)
    }
#pragma unroll
    for (int j = 0; j < 2 * RJ; ++j) {
        const int r = r0 + kGlsRowsPerJ * (j >> 1) + 2 * tx + (j & 1);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int k = f0 + 16 * m + ty;
            if (r < a.R && k < a.F) a.out[(long long)r * a.F + k] = make_double2(acc_c[j][m], acc_s[j][m]);
        }
    }
}

struct GlsPrologueArgs {
    const double* y;                                 // [R][n]
    const double* dy;                                // [R][n], or nullptr: uniform weights
    double* rows;                                    // [R][n] a_i
    double* weights;                                 // [R][n] w_i with dy; [n] without (every workgroup writes the same values)
    double* mean; double* variance;                  // [R]
    int n;
};

// thread 0 adds the `count` terms of the tile to *sum in index order (between two barriers of the caller)
__device__ __forceinline__ double gls_add_tile(const double* term, int count, double sum) {
#pragma clang fp contract(off)
    for (int m = 0; m < count; ++m) sum = sum + term[m];
    return sum;
}

// MASKED (tls_prewhiten_masked): v_i = 0.0 where mask[i] != 0, elsewhere 1.0 / (dy_i * dy_i) or, without dy, 1.0; W = the sum
// of the v_i in index order and w_i = v_i / W -- the per-curve weight rows of the dy case, with or without a dy.  A row with
// fewer than 3 unprotected points is not fitted: its weights and mean ignore the mask and its variance is reported as 0.0, so
// that every power of the row is NaN (gls_epilogue) as a constant row's is.
template <bool MASKED>
__device__ __forceinline__ void gls_prologue(const GlsPrologueArgs& a, const unsigned char* mask_rows) {
#pragma clang fp contract(off)
    __shared__ double term[kGlsTile];
    __shared__ double total;
    const int tid = threadIdx.x, n = a.n;
    const long long at = (long long)blockIdx.x * n;
    const double* y = a.y + at;
    const double* dy = a.dy ? a.dy + at : nullptr;
    const bool own = MASKED || a.dy;                 // a weight row of the curve's own
    double* w_out = own ? a.weights + at : a.weights;
    const double uniform = 1.0 / (double)n;
    const unsigned char* mask = nullptr;
    bool fitted = true;
    if constexpr (MASKED) {
        __shared__ int members[kGlsThreads];
        int mine = 0;
        for (int i = tid; i < n; i += kGlsThreads) mine += mask_rows[at + i] == 0;
        members[tid] = mine;
        wg_sync();
        if (tid == 0) { int c = 0; for (int m = 0; m < kGlsThreads; ++m) c += members[m]; members[0] = c; }
        wg_sync();
        fitted = members[0] >= 3;
        if (fitted) mask = mask_rows + at;
        wg_sync();
    }
    [[maybe_unused]] auto inverse_variance = [&](int i) -> double {
#pragma clang fp contract(off)
        if (MASKED && mask && mask[i]) return 0.0;
        if (!dy) return 1.0;
        const double d = dy[i]; const double p = d * d;
        return 1.0 / p;
    };
    double W = 1.0;
    if (own) {
        double sum = 0.0;
        for (int base = 0; base < n; base += kGlsTile) {
            const int count = n - base < kGlsTile ? n - base : kGlsTile;
            for (int m = tid; m < count; m += kGlsThreads) {
                if constexpr (MASKED) term[m] = inverse_variance(base + m);
                else { const double d = dy[base + m]; const double p = d * d; term[m] = 1.0 / p; }
            }
            wg_sync();
            if (tid == 0) sum = gls_add_tile(term, count, sum);
            wg_sync();
        }
        if (tid == 0) total = sum;
        wg_sync();
        W = total;
        wg_sync();
    }
    double sum = 0.0;
    for (int base = 0; base < n; base += kGlsTile) {
        const int count = n - base < kGlsTile ? n - base : kGlsTile;
        for (int m = tid; m < count; m += kGlsThreads) {
            double w = uniform;
            if constexpr (MASKED) { const double v = inverse_variance(base + m); w = v / W; }
            else if (dy) { const double d = dy[base + m]; const double p = d * d; const double v = 1.0 / p; w = v / W; }
            w_out[base + m] = w;
            term[m] = w * y[base + m];
        }
        wg_sync();
        if (tid == 0) sum = gls_add_tile(term, count, sum);
        wg_sync();
    }
    if (tid == 0) total = sum;
    wg_sync();
    const double ybar = total;
    wg_sync();
    sum = 0.0;
    for (int base = 0; base < n; base += kGlsTile) {
        const int count = n - base < kGlsTile ? n - base : kGlsTile;
        for (int m = tid; m < count; m += kGlsThreads) {
            const double d = y[base + m] - ybar;
            const double v = w_out[base + m] * d;    // (this thread wrote it)
            a.rows[at + base + m] = v;
            term[m] = v * d;
        }
        wg_sync();
        if (tid == 0) sum = gls_add_tile(term, count, sum);
        wg_sync();
    }
    if (tid == 0) { a.mean[blockIdx.x] = ybar; a.variance[blockIdx.x] = fitted ? sum : 0.0; }
}

__global__ void __launch_bounds__(kGlsThreads) tls_gls_prologue_kernel(const GlsPrologueArgs a) {
    gls_prologue<false>(a, nullptr);
}

// weights [R][n] always; mask [R][n]
__global__ void __launch_bounds__(kGlsThreads) tls_gls_prologue_masked_kernel(const GlsPrologueArgs a, const unsigned char* mask) {
    gls_prologue<true>(a, mask);
}

struct GlsEpilogueArgs {
    const double2* yc;                               // [R][F] (YC, YS)
    const double2* cs;                               // [Rw][F] (C, S): Rw = R with per-curve weights, else 1
    const double2* cs2;                              // [Rw][F] (C2, S2)
    const double* variance;                          // [R]
    double* power; double* amplitude; double* phase; // [R][F]
    long long count;                                 // R * F
    int F, shared_weights;
};

__global__ void __launch_bounds__(kGlsThreads) tls_gls_epilogue_kernel(const GlsEpilogueArgs a) {
    for (long long e = (long long)blockIdx.x * kGlsThreads + threadIdx.x; e < a.count; e += (long long)gridDim.x * kGlsThreads) {
        const long long r = e / a.F;
        const long long w = a.shared_weights ? e - r * a.F : e;
        const double2 y = a.yc[e], c = a.cs[w], c2 = a.cs2[w];
        gls_epilogue(y.x, y.y, c.x, c.y, c2.x, c2.y, a.variance[r], &a.power[e], &a.amplitude[e], &a.phase[e]);
    }
}

// ---- the sine test of a candidate (after the SWEET test of the Kepler Robovetter): is the curve a sinusoid at h * P
// The statement (tests/gls_spec.py sine_test), for a candidate (P, T0, d) on a curve and the harmonics h[nH]:
//   status 1 (NaN elsewhere) unless P finite and > 0 and, with a mask, T0 finite, d finite and > 0
//   with a mask, hw = 0.5 * mask * d:  x = (t_i - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P;  point i is out iff fabs(tau) <= hw
//   n_used = the points left;  status 2 (n_used reported, NaN elsewhere) if n_used < 4
//   an ordered sum of terms q_i:  lane j = i mod 256 adds q_i (0.0 for a point that is out) over its i ascending, starting
//   from 0.0; the sum is lane 0's plus lane 1's ... plus lane 255's, in that order
//   v_i = 1.0 / (dy_i * dy_i);  W = ordered sum v_i;  w_i = v_i / W           (without dy: w_i = 1.0 / n_used)
//   ybar = ordered sum (w_i * y_i);  d_i = y_i - ybar;  a_i = w_i * d_i;  YY = ordered sum (a_i * d_i)
//   for every harmonic:  Ph = h * P;  f = 1.0 / Ph;  f2 = 2.0 * f;  the six sums as ordered sums of a_i cos phi, ... (the
//   product rounded, then added), phi from gls_phase;  power, amplitude, phase = the epilogue
//   err = sqrt(2.0 * YY * (1.0 - power) / (n_used - 3.0));  significance = amplitude / err
// One thread owns one lane's partial sum; thread s < 6 adds the 256 partials of sum s in lane order.
struct SineArgs {
    const double* t;                                 // [n]
    const double* y; const double* dy;               // [slots][n]; dy nullptr: uniform weights
    const int* slot;                                 // [fits] of the slab
    const double* period; const double* T0; const double* duration;   // [fits]; T0 and duration nullptr: no mask
    const double* harmonics;                         // [nH]
    double* out;                                     // [fits][kSineWords]
    double* out_h;                                   // [fits][nH][kSineHarmonicWords]
    double* out_sums;                                // [fits][nH][6] YC YS C S C2 S2, or nullptr
    double mask;
    int n, fits, nH;
};

__global__ void __launch_bounds__(kSineThreads) tls_sine_test_kernel(const SineArgs a) {
#pragma clang fp contract(off)
    __shared__ double part[6][kSineThreads];
    __shared__ double total[6];
    __shared__ int part_n[kSineThreads];
    const int tid = threadIdx.x, n = a.n, nH = a.nH;
    const double nan = (double)NAN;
    const double t0 = a.t[0];
    const bool masked = a.T0 != nullptr;
    for (long long f = blockIdx.x; f < a.fits; f += gridDim.x) {
        double* o = a.out + f * kSineWords;
        double* oh = a.out_h + f * nH * kSineHarmonicWords;
        double* os = a.out_sums ? a.out_sums + f * nH * 6 : nullptr;
        const double P = a.period[f];
        const double T0 = masked ? a.T0[f] : 0.0, d = masked ? a.duration[f] : 1.0;
        const bool good = isfinite(P) && P > 0.0 && isfinite(T0) && isfinite(d) && d > 0.0;       // (the whole workgroup)
        if (!good) {
            if (tid < kSineWords) o[tid] = tid == 0 ? 1.0 : nan;
            for (int m = tid; m < nH * kSineHarmonicWords; m += kSineThreads) oh[m] = nan;
            if (os) for (int m = tid; m < nH * 6; m += kSineThreads) os[m] = nan;
            continue;
        }
        const double hw = 0.5 * a.mask * d;
        const double* y = a.y + (long long)a.slot[f] * n;
        const double* dy = a.dy ? a.dy + (long long)a.slot[f] * n : nullptr;
        auto used = [&](int i) -> bool {
#pragma clang fp contract(off)
            if (!masked) return true;
            const double lead = a.t[i] - T0;
            const double x = lead / P;
            const double xh = x + 0.5;
            const double e = floor(xh);
            const double ph = x - e;
            const double tau = ph * P;
            return !(fabs(tau) <= hw);
        };
        // the points left, and W
        int cnt = 0;
        double sv = 0.0;
        for (int i = tid; i < n; i += kSineThreads) {
            const bool u = used(i);
            cnt += u ? 1 : 0;
            if (dy) { const double e = dy[i]; const double p = e * e; const double v = 1.0 / p; sv = sv + (u ? v : 0.0); }
        }
        part_n[tid] = cnt;
        part[0][tid] = sv;
        wg_sync();
        if (tid == 0) {
            int c = 0;
            double s = 0.0;
            for (int j = 0; j < kSineThreads; ++j) { c += part_n[j]; s = j == 0 ? part[0][0] : s + part[0][j]; }
            part_n[0] = c;
            total[0] = s;
        }
        wg_sync();
        const int n_used = part_n[0];
        const double W = total[0];
        wg_sync();
        if (n_used < 4) {
            if (tid == 0) { o[0] = 2.0; o[1] = (double)n_used; o[2] = nan; o[3] = nan; }
            for (int m = tid; m < nH * kSineHarmonicWords; m += kSineThreads) oh[m] = nan;
            if (os) for (int m = tid; m < nH * 6; m += kSineThreads) os[m] = nan;
            continue;
        }
        const double uniform = 1.0 / (double)n_used;
        auto weight = [&](int i) -> double {
#pragma clang fp contract(off)
            if (!dy) return uniform;
            const double e = dy[i]; const double p = e * e; const double v = 1.0 / p;
            return v / W;
        };
        // ybar
        double sy = 0.0;
        for (int i = tid; i < n; i += kSineThreads) { const double q = weight(i) * y[i]; sy = sy + (used(i) ? q : 0.0); }
        part[0][tid] = sy;
        wg_sync();
        if (tid == 0) { double s = part[0][0]; for (int j = 1; j < kSineThreads; ++j) s = s + part[0][j]; total[0] = s; }
        wg_sync();
        const double ybar = total[0];
        wg_sync();
        // YY
        double syy = 0.0;
        for (int i = tid; i < n; i += kSineThreads) {
            const double dd = y[i] - ybar;
            const double av = weight(i) * dd;
            const double q = av * dd;
            syy = syy + (used(i) ? q : 0.0);
        }
        part[0][tid] = syy;
        wg_sync();
        if (tid == 0) { double s = part[0][0]; for (int j = 1; j < kSineThreads; ++j) s = s + part[0][j]; total[0] = s; }
        wg_sync();
        const double YY = total[0];
        wg_sync();
        if (tid == 0) { o[0] = 0.0; o[1] = (double)n_used; o[2] = ybar; o[3] = YY; }
        for (int h = 0; h < nH; ++h) {
            const double Ph = a.harmonics[h] * P;
            const double fr = 1.0 / Ph;
            const double fr2 = 2.0 * fr;
            double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int i = tid; i < n; i += kSineThreads) {
                const bool u = used(i);
                const double w = weight(i);
                const double dd = y[i] - ybar;
                const double av = w * dd;
                const double lead = a.t[i] - t0;
                double s1, c1, s2, c2;
                sincos(gls_phase(fr, lead), &s1, &c1);
                sincos(gls_phase(fr2, lead), &s2, &c2);
                const double q0 = av * c1, q1 = av * s1, q2 = w * c1, q3 = w * s1, q4 = w * c2, q5 = w * s2;
                s6[0] = s6[0] + (u ? q0 : 0.0); s6[1] = s6[1] + (u ? q1 : 0.0); s6[2] = s6[2] + (u ? q2 : 0.0);
                s6[3] = s6[3] + (u ? q3 : 0.0); s6[4] = s6[4] + (u ? q4 : 0.0); s6[5] = s6[5] + (u ? q5 : 0.0);
            }
#pragma unroll
            for (int s = 0; s < 6; ++s) part[s][tid] = s6[s];
            wg_sync();
            if (tid < 6) { double s = part[tid][0]; for (int j = 1; j < kSineThreads; ++j) s = s + part[tid][j]; total[tid] = s; }
            wg_sync();
            if (tid == 0) {
                double power, amplitude, phase;
                gls_epilogue(total[0], total[1], total[2], total[3], total[4], total[5], YY, &power, &amplitude, &phase);
                const double left = 1.0 - power;
                const double dof = (double)n_used - 3.0;
                const double err = sqrt(2.0 * YY * left / dof);
                double* r = oh + h * kSineHarmonicWords;
                r[0] = power; r[1] = amplitude; r[2] = phase; r[3] = err; r[4] = amplitude / err;
                if (os) for (int s = 0; s < 6; ++s) os[h * 6 + s] = total[s];
            }
            wg_sync();                               // (the next harmonic overwrites the partials)
        }
    }
}
