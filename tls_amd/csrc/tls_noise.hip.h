// tls_noise.hip.h -- the per-star noise profile (tls_noise_profile): a robust sigma of every curve and the scatter of its
// running means at a list of window widths, the robust CDPP.  DESIGN.md "Noise profile"; tests/noise_profile_spec.py is the
// statement in Python.
//
// The statement, for a curve y [n] (a -0.0 taken as +0.0) over the shared time stamps t [n] (or none), K = 1.4826022185056018;
// median(v [m]) is the value of rank m / 2 for odd m and 0.5 * (s[m/2 - 1] + s[m/2]) of the sorted values for even m:
//   m = median(y);  d_j = y_j - m;  sigma = K * median(|d_j|);  sigma == 0: status 1, nothing else is measured
//   keep_j = (d_j <= clip_upper * sigma) and (d_j >= -(clip_lower * sigma))                       (one pass)
//   pairs: the j with keep_j, keep_{j+1} and t_{j+1} - t_j <= pair_span;  sigma_p2p = (K * median(|y_{j+1} - y_j|)) / sqrt(2)
//   width w, window i = the samples [i, i + w), valid when all are kept and t[i + w - 1] - t[i] <= span_max[w]:
//     v_i = (((0.0 + d_i) + d_{i+1}) + ...) / w;  count = the valid windows;  count < min_count: NaN
//     mu = median(valid v);  robust = K * median(|v_i - mu|)
//     mean = lanes(v) / count;  rms = sqrt(lanes((v_i - mean) * (v_i - mean)) / count)
// lanes() is the ordered 256-lane sum of the sine test (tls_gls.hip.h): lane i mod 256 adds its terms with i ascending from
// 0.0, one thread adds the lanes in lane order.  One IEEE double operation a step, contraction off.
//
// tls_noise_curve_kernel<LDS>: one workgroup of 256 threads a curve: m, sigma, d (to device memory), the running count of
// clipped points bad[0 .. n] (bad[i] = the clipped among the first i, so a window is clean when bad[i + w] == bad[i]) and
// sigma_p2p.  tls_noise_width_kernel<LDS>: one workgroup a (width, curve): thread i mod 256 walks the w samples of window i --
// the 64 lanes of a wave read 64 neighbouring doubles a step -- and stores v_i; a wave's ballot is the 64 validity bits of
// its windows.  Every median is a selection on order-preserving 64-bit keys (the bit pattern with the sign flipped for a
// non-negative double and all bits flipped for a negative one), MSB first, 8 bits a pass: an integer histogram of 256 bins
// in the LDS filled with integer atomics, whose counts do not depend on the order of the atomics, scanned by one wave.  An
// even count takes the rank below the middle by selection and the next one as that key again or the smallest key above it
// (a count and an integer atomic minimum).  No floating-point atomic anywhere.  With LDS the curve (y, then d) and v lie in
// the LDS, 16 bytes a point behind 3.1 KB of shared words, up to kNoiseLdsPoints points; a longer row runs the same passes
// on device memory (the rows, d, and a scratch of v and validity words per (curve, width)).
// Included by tls_kernels.hip.h (namespace tlsdev).

constexpr int kNoiseThreads = 256;
constexpr int kNoiseWords = 6;                       // tls_noise_curve
constexpr int kNoiseMaxWidth = 4096;
constexpr int kNoiseMaxWidths = 64;
constexpr int kNoiseLdsPoints = 8192;                // 16 bytes a point and a validity bit a window: 132 KB of the 160 KB
constexpr double kNoiseK = 1.4826022185056018;
constexpr double kNoiseRoot2 = 1.4142135623730951;

struct NoiseShared {
    double part[kNoiseThreads];                      // the lanes of a sum
    double total[4];                                 // 0: the sum of the lanes
    unsigned long long word[4];                      // 0: the key prefix of a selection; 1: the smallest key above a key
    unsigned int hist[kNoiseThreads];                // the bins of a pass; the curve kernel's per-thread clip counts
    unsigned int cnt[4];                             // 0: the rank inside the bin; 1: keys <= a key; 2: clipped; 3: pairs / valid windows
};
static_assert(sizeof(NoiseShared) % 16 == 0, "the arrays behind the shared words are 16-byte aligned");

constexpr size_t noise_mask_words(int n) { return ((size_t)n + 63) >> 6; }
constexpr size_t noise_curve_lds_bytes(int n, bool lds) { return sizeof(NoiseShared) + (lds ? (size_t)n * 8 : 0); }
constexpr size_t noise_width_lds_bytes(int n, bool lds) {
    return sizeof(NoiseShared) + (lds ? (size_t)n * 16 + noise_mask_words(n) * 8 : 0);
}

struct NoiseArgs {
    const double* t;                                 // [n], or nullptr: no gaps
    const double* y;                                 // [R][n]
    double* d;                                       // [R][n] y - median
    unsigned int* bad;                               // [R][n + 1] the clipped points among the first i
    double* records;                                 // [R][kNoiseWords]
    const int* widths;                               // [W]
    const double* span_max;                          // [W]
    double* v;                                       // [R * W][n] the window means of a long row, or nullptr (LDS)
    unsigned long long* mask;                        // [R * W][noise_mask_words(n)] their validity bits, or nullptr (LDS)
    long long* count;                                // [R][W]
    double* robust;                                  // [R][W]
    double* rms;                                     // [R][W]
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    double pair_span, clip_upper, clip_lower;
    int n, W, min_count;
};

__device__ __forceinline__ unsigned long long noise_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double noise_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// The key of rank `rank` (0-based, ascending) among the keys key_of(i, key) == true, i < N.  Every thread of the workgroup
// calls it with the same arguments and gets the same key.
template <class A, class F>
__device__ __forceinline__ unsigned long long noise_select(const A& a, NoiseShared* sh, F key_of, int N, unsigned int rank) {
    const int tid = threadIdx.x;
    unsigned long long prefix = 0ull;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        sh->hist[tid] = 0u;
        wg_sync();
        for (int i = tid; i < N; i += kNoiseThreads) {
            unsigned long long k;
            if (key_of(i, k) && (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))))
                atomicAdd(&sh->hist[(unsigned int)(k >> shift) & 255u], 1u);
        }
        wg_sync();
        if (tid < kWave) {                           // one wave: lane l holds the bins 4 l .. 4 l + 3
            const unsigned int h0 = sh->hist[4 * tid], h1 = sh->hist[4 * tid + 1], h2 = sh->hist[4 * tid + 2], h3 = sh->hist[4 * tid + 3];
            const unsigned int own = h0 + h1 + h2 + h3;
            unsigned int incl = own;
            for (int o = 1; o < kWave; o <<= 1) {
                const unsigned int up = __shfl_up(incl, o, kWave);
                if (tid >= o) incl += up;
            }
            const unsigned long long over = __ballot(incl > rank);
            TLS_CHECK(a, over != 0ull, kChkNoise);
            const int first = over ? __ffsll((long long)over) - 1 : kWave - 1;
            if (tid == first) {
                unsigned int r = rank - (incl - own);
                unsigned int bin = 4u * (unsigned int)tid;
                if (r >= h0) { r -= h0; ++bin; if (r >= h1) { r -= h1; ++bin; if (r >= h2) { r -= h2; ++bin; } } }
                TLS_CHECK(a, bin < 256u && r < sh->hist[bin & 255u], kChkNoise);
                sh->word[0] = prefix | ((unsigned long long)(bin & 255u) << shift);
                sh->cnt[0] = r;
            }
        }
        wg_sync();
        prefix = sh->word[0];
        rank = sh->cnt[0];
    }
    wg_sync();                                       // (every thread has read the last prefix: the next selection may write)
    return prefix;
}

// median of the `count` >= 1 doubles behind the keys
template <class A, class F>
__device__ __forceinline__ double noise_median(const A& a, NoiseShared* sh, F key_of, int N, unsigned int count) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const unsigned long long lo = noise_select(a, sh, key_of, N, (count - 1u) >> 1);
    if (count & 1u) return noise_value(lo);
    if (tid == 0) { sh->cnt[1] = 0u; sh->word[1] = ~0ull; }
    wg_sync();
    unsigned int le = 0u;
    unsigned long long above = ~0ull;
    for (int i = tid; i < N; i += kNoiseThreads) {
        unsigned long long k;
        if (key_of(i, k)) {
            le += (unsigned int)(k <= lo);
            if (k > lo && k < above) above = k;
        }
    }
    atomicAdd(&sh->cnt[1], le);
    atomicMin(&sh->word[1], above);
    wg_sync();
    const unsigned long long hi = sh->cnt[1] > (count >> 1) ? lo : sh->word[1];
    wg_sync();                                       // (read by all before the next median resets the two words)
    const double sum = noise_value(lo) + noise_value(hi);
    return 0.5 * sum;
}

// the ordered sum of the 256 lanes
__device__ __forceinline__ double noise_lanes(NoiseShared* sh, double mine) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    sh->part[tid] = mine;
    wg_sync();
    if (tid == 0) { double s = sh->part[0]; for (int m = 1; m < kNoiseThreads; ++m) s = s + sh->part[m]; sh->total[0] = s; }
    wg_sync();
    const double s = sh->total[0];
    wg_sync();
    return s;
}

// LDS: NoiseShared | y [n] (LDS).  Grid (curves).
template <bool LDS>
__global__ void __launch_bounds__(kNoiseThreads) tls_noise_curve_kernel(const NoiseArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char noise_lds[];
    NoiseShared* sh = reinterpret_cast<NoiseShared*>(noise_lds);
    const int tid = threadIdx.x, n = a.n;
    const long long c = blockIdx.x;
    const double nan = (double)NAN;
    const double* g_y = a.y + c * n;
    double* l_y = reinterpret_cast<double*>(noise_lds + sizeof(NoiseShared));
    if (LDS) {
        for (int i = tid; i < n; i += kNoiseThreads) l_y[i] = g_y[i];
        wg_sync();
    }
    const double* row = LDS ? l_y : g_y;
    auto value = [&](int i) -> double { return row[i] + 0.0; };       // (-0.0 counts as +0.0)
    const double m = noise_median(a, sh, [&](int i, unsigned long long& k) { k = noise_key(value(i)); return true; }, n, (unsigned int)n);
    auto dev = [&](int i) -> double { return value(i) - m; };
    const double mad = noise_median(a, sh, [&](int i, unsigned long long& k) { k = noise_key(fabs(dev(i))); return true; }, n, (unsigned int)n);
    const double sigma = kNoiseK * mad;
    double* g_d = a.d + c * n;
    for (int i = tid; i < n; i += kNoiseThreads) g_d[i] = dev(i);
    double* rec = a.records + c * kNoiseWords;
    if (sigma == 0.0) {                              // (the whole workgroup)
        if (tid == 0) { rec[0] = 1.0; rec[1] = 0.0; rec[2] = 0.0; rec[3] = m; rec[4] = sigma; rec[5] = nan; }
        return;
    }
    const double up = a.clip_upper * sigma;
    const double low = -(a.clip_lower * sigma);
    auto keep = [&](int i) -> bool { const double d = dev(i); return d <= up && d >= low; };
    // the clipped among the first i: thread tid counts the points of its stretch, then writes their running count
    const int stretch = (n + kNoiseThreads - 1) / kNoiseThreads;
    const int lo_i = tid * stretch < n ? tid * stretch : n, hi_i = lo_i + stretch < n ? lo_i + stretch : n;
    unsigned int mine = 0u;
    for (int i = lo_i; i < hi_i; ++i) mine += (unsigned int)!keep(i);
    sh->hist[tid] = mine;
    if (tid == 0) sh->cnt[3] = 0u;
    wg_sync();
    unsigned int before = 0u;
    for (int k = 0; k < tid; ++k) before += sh->hist[k];
    unsigned int* bad = a.bad + c * ((long long)n + 1);
    unsigned int run = before;
    for (int i = lo_i; i < hi_i; ++i) { bad[i] = run; run += (unsigned int)!keep(i); }
    if (tid == kNoiseThreads - 1) { bad[n] = run; sh->cnt[2] = run; }
    // the pairs of neighbours, both kept and no gap between them
    const double* t = a.t;
    const double pair_span = a.pair_span;
    auto pair = [&](int j) -> bool { return keep(j) && keep(j + 1) && (!t || t[j + 1] - t[j] <= pair_span); };
    unsigned int pairs = 0u;
    for (int j = tid; j < n - 1; j += kNoiseThreads) pairs += (unsigned int)pair(j);
    atomicAdd(&sh->cnt[3], pairs);
    wg_sync();                                       // (also: every thread has read the clip counts: the bins are free)
    const unsigned int n_pairs = sh->cnt[3], n_clipped = sh->cnt[2];
    TLS_CHECK(a, n_clipped <= (unsigned int)n && n_pairs <= (unsigned int)(n - 1), kChkNoise);
    double p2p = nan;
    if (n_pairs) {                                   // (the whole workgroup)
        const double med = noise_median(a, sh, [&](int j, unsigned long long& k) {
            if (!pair(j)) return false;
            k = noise_key(fabs(value(j + 1) - value(j)));
            return true;
        }, n - 1, n_pairs);
        const double scaled = kNoiseK * med;
        p2p = scaled / kNoiseRoot2;
    }
    if (tid == 0) { rec[0] = 0.0; rec[1] = (double)n_clipped; rec[2] = (double)n_pairs; rec[3] = m; rec[4] = sigma; rec[5] = p2p; }
}

// LDS: NoiseShared | d [n] | v [n] | validity words (LDS).  Grid (W, curves).
template <bool LDS>
__global__ void __launch_bounds__(kNoiseThreads) tls_noise_width_kernel(const NoiseArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char noise_lds[];
    NoiseShared* sh = reinterpret_cast<NoiseShared*>(noise_lds);
    const int tid = threadIdx.x, n = a.n;
    const int kw = blockIdx.x;
    const long long c = blockIdx.y;
    const long long cw = c * a.W + kw;
    const double nan = (double)NAN;
    if (a.records[c * kNoiseWords] != 0.0) {          // (the whole workgroup) a curve without a sigma
        if (tid == 0) { a.count[cw] = 0; a.robust[cw] = nan; a.rms[cw] = nan; }
        return;
    }
    const int w = a.widths[kw];
    TLS_CHECK(a, w >= 1 && w <= n && w <= kNoiseMaxWidth && kw < a.W, kChkNoise);
    const int windows = n - w + 1;
    const double span = a.span_max[kw];
    const double* g_d = a.d + c * n;
    const unsigned int* bad = a.bad + c * ((long long)n + 1);
    double* l_d = reinterpret_cast<double*>(noise_lds + sizeof(NoiseShared));
    if (LDS) for (int i = tid; i < n; i += kNoiseThreads) l_d[i] = g_d[i];
    if (tid == 0) sh->cnt[3] = 0u;
    wg_sync();
    const double* d = LDS ? l_d : g_d;
    double* v = LDS ? l_d + n : a.v + cw * n;
    unsigned long long* mask = LDS ? reinterpret_cast<unsigned long long*>(l_d + 2 * (size_t)n) : a.mask + cw * (long long)noise_mask_words(n);
    const double* t = a.t;
    const double width = (double)w;
    unsigned int mine = 0u;
    for (int base = 0; base < windows; base += kNoiseThreads) {       // (the same trips for every lane: the ballot is a wave's)
        const int i = base + tid;
        bool valid = false;
        if (i < windows) {
            TLS_CHECK(a, i + w <= n, kChkNoise);
            valid = bad[i + w] == bad[i] && (!t || t[i + w - 1] - t[i] <= span);
            double s = 0.0;
            for (int j = 0; j < w; ++j) s = s + d[i + j];
            v[i] = s / width;
        }
        const unsigned long long bits = __ballot(valid);
        const int first = base + (tid & ~(kWave - 1));
        if ((tid & (kWave - 1)) == 0 && first < windows) mask[first >> 6] = bits;
        mine += (unsigned int)valid;
    }
    atomicAdd(&sh->cnt[3], mine);
    wg_sync();
    const unsigned int count = sh->cnt[3];
    TLS_CHECK(a, count <= (unsigned int)windows, kChkNoise);
    if (count < (unsigned int)a.min_count) {         // (the whole workgroup)
        if (tid == 0) { a.count[cw] = (long long)count; a.robust[cw] = nan; a.rms[cw] = nan; }
        return;
    }
    auto valid_at = [&](int i) -> bool { return (mask[i >> 6] >> (i & 63)) & 1ull; };
    const double mu = noise_median(a, sh, [&](int i, unsigned long long& k) {
        if (!valid_at(i)) return false;
        k = noise_key(v[i]);
        return true;
    }, windows, count);
    const double mad = noise_median(a, sh, [&](int i, unsigned long long& k) {
        if (!valid_at(i)) return false;
        k = noise_key(fabs(v[i] - mu));
        return true;
    }, windows, count);
    const double robust = kNoiseK * mad;
    const double cnt = (double)count;
    double s = 0.0;
    for (int i = tid; i < windows; i += kNoiseThreads) if (valid_at(i)) s = s + v[i];
    const double mean = noise_lanes(sh, s) / cnt;
    s = 0.0;
    for (int i = tid; i < windows; i += kNoiseThreads) {
        if (valid_at(i)) {
            const double dv = v[i] - mean;
            const double q = dv * dv;
            s = s + q;
        }
    }
    const double var = noise_lanes(sh, s) / cnt;
    if (tid == 0) { a.count[cw] = (long long)count; a.robust[cw] = robust; a.rms[cw] = sqrt(var); }
}
