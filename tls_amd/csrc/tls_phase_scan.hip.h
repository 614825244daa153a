// tls_phase_scan.hip.h -- the secondary-eclipse phase scan of a candidate (tls_phase_scan, tls_power_batch_phase_scan).
//
// The scan, per fit (light curve y over t, period P, T0, duration d in days; tests/phase_scan_spec.py is the same in Python;
// DESIGN.md "Phase scan"):
//   status 1 and NaN everywhere else unless P, T0, d are finite, P > 0, d > 0 and q = 2.0 * P / d >= 16
//   B = int(min(floor(q), max_bins))
//   for i ascending:  x = (t[i] - T0) / P;  phi = x - floor(x);  b = min(int(phi * B), B - 1);  S[b] += y[i];  N[b] += 1
//   window j = bins j and (j+1) % B:  W[j] = S[j] + S[(j+1)%B],  M[j] = N[j] + N[(j+1)%B];  primary p = B-1
//   baseline Sb, Nb = bins 2 .. B-3 summed ascending;  inside windows 2 <= j <= B-4
//   delta[j] = (Sb - W[j]) / (Nb - M[j]) - W[j] / M[j]   inside, where M[j] >= min_count and Nb - M[j] >= 1
//   delta[p] = Sb / Nb - W[p] / M[p]                     where M[p] >= min_count and Nb >= 1;  every other delta NaN
//   js / jb = the first inside j of the largest / smallest delta that is no NaN;  rest = those with |j - js| > 2
//   scan_mean, scan_std = mean and root mean square deviation of delta over rest, summed ascending, where len(rest) >= 8
// Every step is one IEEE double operation (contraction off) and every sum runs in the stated order, so the record equals the
// host statement bit for bit.
//
// One workgroup of kPhaseThreads threads per fit.  The points pass through the LDS in chunks of kPhaseChunk, ascending: a
// chunk's flux (8 bytes a point) and bin (16 bits: B <= 4096) are staged by all threads, then EVERY thread walks the staged
// bins in index order -- all lanes read the same LDS word, a broadcast without bank conflict, four bins a ds_read_b64 -- and
// the one thread that owns bin b (b mod kPhaseThreads) adds the point to S[b] and N[b] in the LDS.  One owner per bin and
// one order per owner fix the bits: no floating-point atomic, no tree over points.  O(n) LDS reads per thread whatever B
// is.  (The other form -- ceil(B / kPhaseThreads) passes, a thread's one bin of the pass in registers, every point added
// by a select -- has no store in its walk and no divergent lane, but walks the points once a pass: it measured 1.5 times
// this one's kernel time on the k2_90d peaks, whose slowest fit of a launch has seven passes; DESIGN.md "Phase scan".)
// The window pass writes delta over S and M over N, kPhaseThreads windows a step: a step reads its bins into registers
// before a barrier and stores behind it (bin j + 1 of a step's last window belongs to the next step; bin 0, which the primary
// window reads last, is saved first).  Baseline, mean and scatter are serial loops of thread 0 in the stated order; the two
// extremes are (value, lowest index) reductions, wave64 shuffles and then wave 0 over the per-wave results.
//
// LDS: 10 bytes a staged point + 12 bytes a bin of the launch's max_bins (S, N) + 128 bytes of scalars: 68.1 KB at
// max_bins = 4096, two workgroups a CU (160 KB); 32.1 KB at max_bins = 1024, four.  Included by tls_kernels.hip.h (namespace
// tlsdev), behind tls_peak_fits.hip.h.

constexpr int kPhaseThreads = 256;
constexpr int kPhaseChunk = 2048;                    // points staged at a time (a multiple of 4)
constexpr int kPhaseWords = 12;                      // tls_phase_record
constexpr int kPhaseMinBins = 16, kPhaseMaxBins = 4096;
constexpr int kPhaseMinWindows = 8;                  // fewer windows in `rest`: no scan_mean, no scan_std
constexpr double kPhaseScanned = 0.0, kPhaseNothing = 1.0;   // tls_phase_record.status

struct PhaseScanArgs {
    const double* t; const double* y;                // [n], [curves][n]
    const int* curve;                                // [fits]: fit f reads y + curve[f] * n
    // fit f reads period[f * period_stride], T0[f], duration[f * duration_stride] (the peak-fit stage: the period out of
    // the pick records, the duration out of the statistics records)
    const double* period; const double* T0; const double* duration;
    int period_stride, duration_stride;
    const double* status;                            // nullptr, or [fits]: a fit whose status is not 0 is not scanned
    double* out;                                     // [fits][kPhaseWords]
    int n, max_bins, min_count;
};

inline size_t phase_scan_lds_bytes(int max_bins) {
    return (size_t)max_bins * 12 + (size_t)kPhaseChunk * 10;
}

// (value, index) a over b in the search for the largest or the smallest value (index -1: nothing held): b holds nothing, or
// a wins, or a ties at a lower index
__device__ __forceinline__ bool phase_before(double av, int ai, double bv, int bi, bool largest) {
    if (ai < 0) return false;
    if (bi < 0) return true;
    return (largest ? av > bv : av < bv) || (av == bv && ai < bi);
}

__global__ void __launch_bounds__(kPhaseThreads) tls_phase_scan_kernel(const PhaseScanArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char phase_lds[];
    __shared__ double sh_d[2];                       // Sb, S[0]
    __shared__ int sh_i[2];                          // Nb, N[0]
    __shared__ double red_v[2][kPhaseThreads / kWave];
    __shared__ int red_i[2][kPhaseThreads / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long f = blockIdx.x;
    double* out = a.out + f * kPhaseWords;
    const double P = a.period[f * a.period_stride], T0 = a.T0[f], d = a.duration[f * a.duration_stride];
    const bool wanted = !a.status || a.status[f] == 0.0;
    // (the same decision in every thread: nothing below is reached by a part of the workgroup)
    const double q = 2.0 * P / d;
    if (!(wanted && isfinite(P) && isfinite(T0) && isfinite(d) && P > 0.0 && d > 0.0 && q >= (double)kPhaseMinBins)) {
        if (tid < kPhaseWords) out[tid] = tid == 0 ? kPhaseNothing : (double)NAN;
        return;
    }
    const int B = (int)fmin(floor(q), (double)a.max_bins);
    const double Bd = (double)B;
    double* sy = reinterpret_cast<double*>(phase_lds);                         // [kPhaseChunk]
    unsigned short* sb = reinterpret_cast<unsigned short*>(sy + kPhaseChunk);  // [kPhaseChunk], read four at a time
    double* S = reinterpret_cast<double*>(sb + kPhaseChunk);                   // [max_bins]
    int* N = reinterpret_cast<int*>(S + a.max_bins);                           // [max_bins]
    for (int b = tid; b < B; b += kPhaseThreads) { S[b] = 0.0; N[b] = 0; }
    const double* y = a.y + (long long)a.curve[f] * a.n;
    for (int base = 0; base < a.n; base += kPhaseChunk) {
        const int len = min(kPhaseChunk, a.n - base);
        wg_sync();                                   // (the bins are zero; the last chunk has been read)
        for (int i = tid; i < len; i += kPhaseThreads) {
            const double x = (a.t[base + i] - T0) / P;
            const double phi = x - floor(x);
            const int b = (int)(phi * Bd);           // (saturating; 0 for a NaN)
            sy[i] = y[base + i];
            sb[i] = (unsigned short)max(0, min(b, B - 1));
        }
        wg_sync();
        const int quads = len / 4;
        const unsigned long long* sb4 = reinterpret_cast<const unsigned long long*>(sb);
        unsigned long long next = sb4[0];            // (the read of the next four bins is under way while these are added)
        for (int g = 0; g < quads; ++g) {
            const unsigned long long four = next;
            next = sb4[min(g + 1, kPhaseChunk / 4 - 1)];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int b = (int)((four >> (16 * k)) & 0xffffull);
                if ((b & (kPhaseThreads - 1)) == tid) { S[b] = S[b] + sy[4 * g + k]; N[b] += 1; }
            }
        }
        for (int i = 4 * quads; i < len; ++i) {
            const int b = sb[i];
            if ((b & (kPhaseThreads - 1)) == tid) { S[b] = S[b] + sy[i]; N[b] += 1; }
        }
    }
    wg_sync();
    // the baseline, bins 2 .. B-3 ascending (B >= 16), and bin 0 for the primary window
    if (tid == 0) {
        double Sb = 0.0; int Nb = 0;
#pragma unroll 8
        for (int b = 2; b < B - 2; ++b) { Sb = Sb + S[b]; Nb += N[b]; }
        sh_d[0] = Sb; sh_i[0] = Nb; sh_d[1] = S[0]; sh_i[1] = N[0];
    }
    wg_sync();
    const double Sb = sh_d[0], S0 = sh_d[1];
    const int Nb = sh_i[0], N0 = sh_i[1];
    // the windows: delta over S, M over N; the extremes of the inside windows on the way
    double hi_v = 0.0, lo_v = 0.0; int hi_j = -1, lo_j = -1;
    for (int j0 = 0; j0 < B; j0 += kPhaseThreads) {
        const int j = j0 + tid;
        double w = 0.0; int m = 0;
        if (j < B) {
            w = S[j] + (j + 1 == B ? S0 : S[j + 1]);
            m = N[j] + (j + 1 == B ? N0 : N[j + 1]);
        }
        wg_sync();
        if (j < B) {
            double delta = (double)NAN;
            if (j >= 2 && j <= B - 4) {
                if (m >= a.min_count && Nb - m >= 1) {
                    const double rest = (Sb - w) / (double)(Nb - m);
                    const double in = w / (double)m;
                    delta = rest - in;
                }
                if (!isnan(delta)) {
                    if (phase_before(delta, j, hi_v, hi_j, true)) { hi_v = delta; hi_j = j; }
                    if (phase_before(delta, j, lo_v, lo_j, false)) { lo_v = delta; lo_j = j; }
                }
            } else if (j == B - 1 && m >= a.min_count && Nb >= 1) {
                const double rest = Sb / (double)Nb;
                const double in = w / (double)m;
                delta = rest - in;
            }
            S[j] = delta; N[j] = m;
        }
    }
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) {
        double ov = __shfl_down(hi_v, s, kWave); int oj = __shfl_down(hi_j, s, kWave);
        if (phase_before(ov, oj, hi_v, hi_j, true)) { hi_v = ov; hi_j = oj; }
        ov = __shfl_down(lo_v, s, kWave); oj = __shfl_down(lo_j, s, kWave);
        if (phase_before(ov, oj, lo_v, lo_j, false)) { lo_v = ov; lo_j = oj; }
    }
    if (lane == 0) { red_v[0][wave] = hi_v; red_i[0][wave] = hi_j; red_v[1][wave] = lo_v; red_i[1][wave] = lo_j; }
    wg_sync();
    if (tid != 0) return;
    for (int w = 1; w < kPhaseThreads / kWave; ++w) {
        if (phase_before(red_v[0][w], red_i[0][w], hi_v, hi_j, true)) { hi_v = red_v[0][w]; hi_j = red_i[0][w]; }
        if (phase_before(red_v[1][w], red_i[1][w], lo_v, lo_j, false)) { lo_v = red_v[1][w]; lo_j = red_i[1][w]; }
    }
    const double nan = (double)NAN;
    const int js = hi_j, jb = lo_j;
    out[0] = kPhaseScanned; out[1] = Bd;
    out[3] = S[B - 1]; out[4] = (double)N[B - 1];
    double n_windows = 0.0, mean = nan, sd = nan;
    if (js >= 0) {
        int count = 0;
        double total = 0.0;
        // (a select, not a branch, in both loops: the LDS reads of an unrolled step are under way together, the sum's
        // order stays)
#pragma unroll 8
        for (int j = 2; j <= B - 4; ++j) {
            const double v = S[j];
            const bool in = !isnan(v) && abs(j - js) > 2;
            const double more = total + v;
            total = in ? more : total;
            count += in ? 1 : 0;
        }
        n_windows = (double)count;
        if (count >= kPhaseMinWindows) {
            mean = total / (double)count;
            total = 0.0;
#pragma unroll 8
            for (int j = 2; j <= B - 4; ++j) {
                const double v = S[j];
                const bool in = !isnan(v) && abs(j - js) > 2;
                const double dv = v - mean;
                const double sq = dv * dv;
                const double more = total + sq;
                total = in ? more : total;
            }
            sd = sqrt(total / (double)count);
        }
    }
    out[2] = n_windows;
    out[5] = js >= 0 ? hi_v : nan; out[6] = js >= 0 ? (double)(js + 1) / Bd : nan; out[7] = js >= 0 ? (double)N[js] : nan;
    out[8] = js >= 0 ? lo_v : nan; out[9] = js >= 0 ? (double)(jb + 1) / Bd : nan;
    out[10] = mean; out[11] = sd;
}
