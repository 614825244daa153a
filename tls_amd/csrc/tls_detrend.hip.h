// tls_detrend.hip.h -- median-filter detrending for survey mode (tls_medfilt_detrend): for every row y and an odd kernel k,
// trend = scipy.signal.medfilt(y, k) (a window of k SAMPLES, zero padding at both ends: ndimage.rank_filter(y, k // 2,
// size=k, mode="constant")) and flat = y / trend, one IEEE division per point.
//
// A workgroup takes a tile of T consecutive outputs [lo, lo + T) of one row.  It stages the span [lo - h, lo + T + h),
// h = k / 2, into LDS (S = T + k - 1 slots, 0.0 outside [0, n): the zero padding), each value with its slot number, pads
// the slots S .. P - 1 with keys above every double, and sorts the P (a power of two) pairs once (bitonic, in LDS).  Output
// lo + i has the window of slots [i, i + k); its lane walks the sorted slots in order and stops at the (h + 1)-th slot whose
// number lies in that window: the median, a selection, so bit-equal to scipy.  All active lanes of a wave read the same
// sorted slot at each step (an LDS broadcast).  Values are finite and >= 0 (the host checks y > 0), so ordering their bit
// patterns as integers orders the doubles; equal values may land in either order, the (h + 1)-th smallest value is the same.
// Included by tls_kernels.hip.h (namespace tlsdev).

constexpr int kDetrendThreads = 256;
constexpr int kDetrendMaxSpan = 8192;   // P for the largest kernel (TLS_MEDFILT_MAX_KERNEL = 4095: 2 (k - 1) = 8188)

struct DetrendArgs {
    const double* y;              // [rows][n]
    double* flat;                 // [rows][n]
    double* trend;                // [rows][n], or nullptr
    unsigned long long* check;    // [kChecks] violated bounds (debug build; nullptr: off)
    long long n;                  // points per row
    int k;                        // odd kernel size, 1 <= k <= min(n, 4095)
    int span;                     // P: sorted slots, a power of two in [64, kDetrendMaxSpan]
    int tile;                     // T = P - (k - 1) outputs per workgroup
};

// Stages the S values y[base + s], s < S (0.0 where base + s lies outside [0, n): the median filter's zero padding), as
// (bit-pattern key, slot s) pairs into keys/slot [P], the slots S .. P - 1 with a key above every double and slot ~0u (in no
// window), copies the values in index order into vals [S] unless vals is nullptr, and sorts the P pairs ascending by key
// (bitonic, in LDS).  Every thread of the workgroup calls it; it ends with a barrier.  Shared by tls_medfilt_detrend and
// tls_biweight_detrend (tls_biweight.hip.h); `chk` is the caller's check code.
template <class A>
__device__ __forceinline__ void detrend_stage_sort(const A& a, const double* y, long long base, long long n, int S, int P,
                                                   unsigned long long* keys, unsigned int* slot, double* vals, int chk) {
    for (int s = threadIdx.x; s < P; s += kDetrendThreads) {
        unsigned long long key = ~0ull;   // (above every double: the padding slots sort last)
        unsigned int p = ~0u;             // (in no window)
        if (s < S) {
            const long long g = base + s;
            key = (g >= 0 && g < n) ? (unsigned long long)__double_as_longlong(y[g]) : 0ull;   // (0ull: +0.0)
            p = (unsigned int)s;
            if (vals) vals[s] = __longlong_as_double((long long)key);
        }
        keys[s] = key;
        slot[s] = p;
    }
    wg_sync();

    // bitonic sort of the P (key, slot) pairs, ascending by key
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += kDetrendThreads) {
                const int i = 2 * t - (t & (stride - 1));
                const int j = i + stride;
                TLS_CHECK(a, j < P, chk);
                const unsigned long long ki = keys[i], kj = keys[j];
                const bool up = (i & size) == 0;
                if (up ? ki > kj : ki < kj) {
                    keys[i] = kj; keys[j] = ki;
                    const unsigned int si = slot[i];
                    slot[i] = slot[j]; slot[j] = si;
                }
            }
            wg_sync();
        }
    }
}

// LDS: keys [P] (uint64: the bit patterns) | slot numbers [P] (uint32), 12 P bytes.  Grid (ceil(n / T), rows).
__global__ void __launch_bounds__(kDetrendThreads) tls_medfilt_detrend(const DetrendArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long detrend_lds[];
    const int P = a.span, T = a.tile, k = a.k, h = k >> 1;
    const int S = T + k - 1;
    unsigned long long* keys = detrend_lds;
    unsigned int* slot = reinterpret_cast<unsigned int*>(keys + P);
    const long long row = blockIdx.y;
    const long long lo = (long long)blockIdx.x * T;
    const double* y = a.y + row * a.n;

    detrend_stage_sort(a, y, lo - h, a.n, S, P, keys, slot, nullptr, kChkDetrend);

    // selection: lane of output lo + i counts the sorted slots that fall into [i, i + k), four at a time, up to the (h+1)-th
    const uint4* slot4 = reinterpret_cast<const uint4*>(slot);
    const unsigned int need = (unsigned int)h + 1u, uk = (unsigned int)k;
    const long long n_out = a.n - lo < (long long)T ? a.n - lo : (long long)T;
    for (int i = threadIdx.x; i < n_out; i += kDetrendThreads) {
        const unsigned int ui = (unsigned int)i;
        unsigned int c = 0u;
        int j = 0;
        for (; j < P; j += 4) {
            const uint4 q = slot4[j >> 2];
            const unsigned int m = (unsigned int)(q.x - ui < uk) + (unsigned int)(q.y - ui < uk) + (unsigned int)(q.z - ui < uk)
                                   + (unsigned int)(q.w - ui < uk);
            if (c + m >= need) break;
            c += m;
        }
        TLS_CHECK(a, j < S, kChkDetrend);
        j = j < P ? j : P - 4;   // (unreachable: the window's k slots are all staged and need <= k)
        const uint4 q = slot4[j >> 2];
        int f = j;
        c += (unsigned int)(q.x - ui < uk);
        if (c < need) {
            ++f;
            c += (unsigned int)(q.y - ui < uk);
            if (c < need) {
                ++f;
                c += (unsigned int)(q.z - ui < uk);
                if (c < need) ++f;
            }
        }
        TLS_CHECK(a, f < S, kChkDetrend);
        const double trend = __longlong_as_double((long long)keys[f]);
        const long long g = row * a.n + lo + i;
        a.flat[g] = y[lo + i] / trend;   // (IEEE division: the library builds with -fno-fast-math)
        if (a.trend) a.trend[g] = trend;
    }
}
