// tls_peaks.hip.h -- the K harmonic-aware peaks of a periodogram (tls_find_peaks, tls_power_batch_peaks).
//
// The selection, per row (tests/peaks_spec.py is the same in numpy; DESIGN.md "Periodogram peaks"):
//   cand[j] = (j == 0 or power[j] > power[j-1]) and (j == n-1 or power[j] >= power[j+1]) and power[j] >= min_power
//   alive = cand; at most k times, while an index is alive:
//       j = the lowest index of the largest power among the alive ones (numpy.argmax); take j; P = periods[j]
//       for r in (1.0,) + ratios:  c = r * P;  w = sep * c;  alive[i] = false wherever fabs(periods[i] - c) <= w
// A NaN fails every comparison: an index that holds one or lies next to one is no candidate.  c, w and periods[i] - c are
// one IEEE double operation each (contraction off: an FMA of periods[i] - r * P would flip an index on a window's edge).
// Nothing assumes an order of `periods`.  It is a selection: the peaks' values are copies, bit for bit.
//
// One workgroup of 1024 threads per row.  The alive set is a bit mask, one 64-bit word per 64 consecutive indices, formed
// by __ballot: the wave that owns indices [64 w, 64 w + 64) in the strided loops below is the same in every pass, so a word
// is read and written by one wave only.  The mask lies in the workgroup's dynamic LDS up to kPeaksLdsPeriods = 2^20 periods
// (128 KiB of the CU's 160 KiB; the Kepler grid of 182 388 periods takes 23 KB); a longer grid keeps it in HBM, one mask
// per row in the context's scratch (PeaksArgs::hbm_mask), same code.  A round is a (value, lowest index) argmax over the
// alive bits -- wave64 shuffles, then wave 0 over the per-wave results -- and a pass that clears the 1 + n_ratios windows;
// words without an alive bit are skipped by their wave in both.  Included by tls_kernels.hip.h (namespace tlsdev).

constexpr int kPeaksMaxK = 32;                       // peaks per row
constexpr int kPeaksMaxRatios = 16;                  // caller's ratios (the window at ratio 1 comes on top)
constexpr int kPeakWords = 6;                        // tls_peak: period, power, chi2, depth | index, row
constexpr long long kPeaksLdsPeriods = 1ll << 20;    // the mask of a longer grid lies in HBM
constexpr long long kPeaksMaxPeriods = 1ll << 30;
constexpr int kPeaksNone = 0x7fffffff;

struct PeaksArgs {
    const double* power; long long power_stride;                      // [rows] stride power_stride
    const double* periods;                                            // [n]
    const double* chi2; const long long* row; const double* depth;    // each nullptr or [rows][n]
    const double* pick;                                               // nullptr or [rows][8] of tls_power_pick ([6]: no fit)
    unsigned long long* hbm_mask;                                     // [rows][ceil(n / 64)] where the mask is not in LDS
    unsigned long long* out;                                          // [rows][1 + k kPeakWords]: n_peaks | k records
    double ratios[kPeaksMaxRatios + 1];                               // 1.0, then the caller's
    double sep, min_power;
    int n_ratios;                                                     // entries of `ratios`, the leading 1.0 included
    int n, k;
};

// (value, index) a over b: b holds nothing, or a is larger, or as large at a lower index
__device__ __forceinline__ bool peak_before(double av, int ai, double bv, int bi) {
    return ai != kPeaksNone && (bi == kPeaksNone || av > bv || (av == bv && ai < bi));
}

template <bool LDS>
__global__ void __launch_bounds__(1024) tls_find_peaks(const PeaksArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned long long peaks_lds[];
    __shared__ double red_v[kMaxWaves + 1];
    __shared__ int red_i[kMaxWaves + 1];
    const int tid = threadIdx.x, nt = blockDim.x, n = a.n;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nw = nt / kWave;
    const long long c = blockIdx.x;
    const long long words = ((long long)n + kWave - 1) / kWave;
    unsigned long long* mask = LDS ? peaks_lds : a.hbm_mask + c * words;
    const double* power = a.power + c * a.power_stride;
    const bool fit = !a.pick || a.pick[c * 8 + 6] == 0.0;
    // candidates: one mask word per wave and step
    for (long long base = 0; base < n; base += nt) {
        const long long j = base + tid;
        bool cand = false;
        if (fit && j < n) {
            const double p = power[j];
            cand = (j == 0 || p > power[j - 1]) && (j == n - 1 || p >= power[j + 1]) && p >= a.min_power;
        }
        const unsigned long long m = __ballot(cand);
        if (lane == 0 && base + (long long)wave * kWave < n) mask[base / kWave + wave] = m;
    }
    wg_sync();
    unsigned long long* out = a.out + c * (1 + (long long)a.k * kPeakWords);
    int taken = 0;
    for (int round = 0; round < a.k; ++round) {
        double v = -INFINITY; int i = kPeaksNone;
        for (long long base = (long long)wave * kWave; base < n; base += nt) {
            const unsigned long long m = mask[base / kWave];
            if (m == 0ull) continue;
            if ((m >> lane) & 1ull) {
                const double p = power[base + lane];
                if (peak_before(p, (int)(base + lane), v, i)) { v = p; i = (int)(base + lane); }
            }
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const double ov = __shfl_down(v, d, kWave);
            const int oi = __shfl_down(i, d, kWave);
            if (peak_before(ov, oi, v, i)) { v = ov; i = oi; }
        }
        if (lane == 0) { red_v[wave] = v; red_i[wave] = i; }
        wg_sync();
        if (wave == 0) {
            v = lane < nw ? red_v[lane] : -INFINITY; i = lane < nw ? red_i[lane] : kPeaksNone;
#pragma unroll
            for (int d = kMaxWaves / 2; d > 0; d >>= 1) {
                const double ov = __shfl_down(v, d, kWave);
                const int oi = __shfl_down(i, d, kWave);
                if (peak_before(ov, oi, v, i)) { v = ov; i = oi; }
            }
            if (lane == 0) { red_v[kMaxWaves] = v; red_i[kMaxWaves] = i; }
        }
        wg_sync();
        const int j = red_i[kMaxWaves];
        if (j == kPeaksNone) break;                                   // nothing alive (the same value in every thread)
        const double P = a.periods[j];
        if (tid == 0) {
            unsigned long long* o = out + 1 + (long long)taken * kPeakWords;
            o[0] = (unsigned long long)__double_as_longlong(P);
            o[1] = (unsigned long long)__double_as_longlong(red_v[kMaxWaves]);
            o[2] = (unsigned long long)__double_as_longlong(a.chi2 ? a.chi2[c * n + j] : (double)NAN);
            o[3] = (unsigned long long)__double_as_longlong(a.depth ? a.depth[c * n + j] : (double)NAN);
            o[4] = (unsigned long long)(long long)j;
            o[5] = (unsigned long long)(a.row ? a.row[c * n + j] : -1ll);
        }
        ++taken;
        if (round + 1 == a.k) break;
        // the windows of the taken peak: every index inside one of them leaves the alive set
        for (long long base = (long long)wave * kWave; base < n; base += nt) {
            const unsigned long long m = mask[base / kWave];
            if (m == 0ull) continue;
            bool kill = false;
            if ((m >> lane) & 1ull) {
                const double per = a.periods[base + lane];
                for (int r = 0; r < a.n_ratios; ++r) {
                    const double ctr = a.ratios[r] * P;
                    const double w = a.sep * ctr;
                    const double d = per - ctr;
                    kill = kill || fabs(d) <= w;
                }
            }
            const unsigned long long gone = __ballot(kill);
            if (lane == 0 && gone != 0ull) mask[base / kWave] = m & ~gone;
        }
        wg_sync();
    }
    // (`taken` is the same in every thread) entries past it: NaN and -1
    if (tid == 0) out[0] = (unsigned long long)(long long)taken;
    const unsigned long long nan_bits = (unsigned long long)__double_as_longlong((double)NAN);
    for (int q = taken * kPeakWords + tid; q < a.k * kPeakWords; q += nt)
        out[1 + q] = (q % kPeakWords) < 4 ? nan_bits : ~0ull;
}
