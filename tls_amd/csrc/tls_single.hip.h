// tls_single.hip.h -- single-transit events: the template slid along the time series itself (tls_single_transits).
//
// The statement (tests/single_transit_spec.py is the same in Python; include/tls_amd.h, DESIGN.md "Single-transit events"):
//   w = 1.0 / (dy * dy);  xw = (1.0 - y) * w;  bb_r[j] = b_r[j] * b_r[j]
//   for every centre c, rows r ascending (widths L_r strictly ascending, nothing held at first):
//       h = (L_r - 1) / 2;  lo = c - h;  hi = lo + L_r - 1
//       skip if lo < 0 or hi > n - 1 or not (t[hi] - t[lo] <= span_max[r])
//       N = 0; D = 0; for j ascending: N = N + xw[lo+j] * b_r[j];  D = D + w[lo+j] * bb_r[j]
//       d = N / D;  skip if not (d > depth_min);  s = N / sqrt(D);  take (s, r, d) if nothing is held or s > held s
//   ses[c], row[c], depth[c] = held, or NaN, -1, NaN
//   events: alive = ses no NaN and >= min_ses; at most k times: take the alive centre of the largest ses (lowest index on
//   ties); g = int(separation * L) of its row; every alive centre whose window [lo', hi'] of its own best row meets
//   [lo - g, hi + g] leaves.
// Every step is one IEEE double operation (contraction off) and every sum runs in the stated order, so planes and records
// equal the host statement bit for bit.
//
// (1) tls_single_statistic_kernel: a workgroup of kSingleThreads threads takes one curve and a tile of kSingleTile centres,
// one centre a thread.  It forms (xw, w) of the tile and of a halo of the launch's widest row on either side -- (Lmax-1)/2
// slots in front, Lmax/2 behind -- as PAIRS in the LDS, 16 bytes a slot.  Lanes are consecutive centres, so step j of a row is
// one ds_read_b128 a lane at consecutive slots: each of the instruction's four 16-lane groups covers 256 contiguous bytes,
// every bank once, whatever j is.  (The pair form moves the same 16 bytes a step as two ds_read_b64 on two planes would, in
// half the instructions, and leaves nothing for the compiler to fuse into ds_read2_b64, which moves half the bytes per LDS
// cycle.)  The taps (b_r[j], bb_r[j]) are wave-uniform pairs read through the constant address space into scalar registers.
// Every thread walks every row, so all threads do the same sum of widths of steps; a thread whose window is not valid walks
// it all the same (every slot a tile can reach is staged, zero outside the series) and drops the result, and a wave without
// one valid window skips the row.  A step is four fp64 operations (no FMA: two roundings each) and 16 bytes of LDS: both
// pipes at 16 steps a clock and CU.  N <= 0 cannot pass d > depth_min >= 0 (D >= 0), so the two divisions and the root are
// taken only where N > 0.
//
// (2) tls_single_select_kernel: one workgroup of 1024 threads a curve, in the manner of tls_peaks.hip.h: the alive set is a
// bit mask in the LDS, one 64-bit word per 64 consecutive centres owned by one wave in every pass; a round is a (value,
// lowest index) argmax -- wave64 shuffles, then wave 0 over the per-wave results -- and a pass that clears the centres whose
// windows meet the taken one's.  n <= kSingleMaxPoints = 2^20: the mask takes at most 128 KiB.
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_peaks.hip.h.

constexpr int kSingleThreads = 256;
constexpr int kSingleTile = 256;                     // centres of a workgroup, one a thread
constexpr int kSingleMinWidth = 3, kSingleMaxWidth = 4096;
constexpr int kSingleMaxK = 32;
constexpr int kSingleEventWords = 8;                 // tls_single_event
constexpr int kSingleMaxPoints = 1 << 20;            // the alive mask of the selection lies in the LDS
constexpr int kSingleSelectThreads = 1024;
constexpr int kSingleNone = 0x7fffffff;
static_assert(kSingleTile == kSingleThreads, "one centre a thread");

struct SingleRow {
    int width;         // L_r
    int offset;        // the row's first pair in SingleArgs::taps
    double span_max;   // days
};
typedef const __attribute__((address_space(4))) SingleRow* const_single_row_ptr;

struct SingleArgs {
    const double* t;                                 // [n]
    const double* y; const double* dy;               // [curves][n]
    const SingleRow* rows;                           // [n_rows]
    const double* taps;                              // pairs (b_r[j], b_r[j] * b_r[j]), row after row
    double* ses; int* row; double* depth;            // [curves][n]
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    double depth_min;
    int n, n_rows;
    int halo_lo, halo_hi;                            // (Lmax - 1) / 2, Lmax / 2 of the widest row
};

inline size_t single_lds_bytes(int max_width) { return (size_t)(kSingleTile + max_width - 1) * 16; }

__global__ void __launch_bounds__(kSingleThreads) tls_single_statistic_kernel(const SingleArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char single_lds[];
    double2* s = reinterpret_cast<double2*>(single_lds);           // [kSingleTile + halo_lo + halo_hi] pairs (xw, w)
    const int tid = threadIdx.x, n = a.n;
    const int base = (int)blockIdx.x * kSingleTile;
    const long long curve = blockIdx.y;
    const double* y = a.y + curve * n;
    const double* dy = a.dy + curve * n;
    const int slots = kSingleTile + a.halo_lo + a.halo_hi;
    const int first = base - a.halo_lo;
    for (int k = tid; k < slots; k += kSingleThreads) {
        const int p = first + k;
        double2 v; v.x = 0.0; v.y = 0.0;
        if (p >= 0 && p < n) {
            const double e = dy[p];
            const double w = 1.0 / (e * e);
            v.x = (1.0 - y[p]) * w;
            v.y = w;
        }
        s[k] = v;
    }
    wg_sync();
    const int c = base + tid;
    const int at = tid + a.halo_lo;                  // the slot of centre c
    const const_single_row_ptr rows = (const_single_row_ptr)a.rows;
    const const_f64_ptr taps = (const_f64_ptr)a.taps;
    double best_s = (double)NAN, best_d = (double)NAN;
    int best_r = -1;
    for (int r = 0; r < a.n_rows; ++r) {
        const int L = rows[r].width;
        const double span = rows[r].span_max;
        const int h = (L - 1) / 2;
        const int lo = c - h, hi = lo + L - 1;
        bool ok = lo >= 0 && hi <= n - 1;            // (hi <= n - 1 implies c < n)
        if (ok) {
            const double dt = a.t[hi] - a.t[lo];
            ok = dt <= span;
        }
        if (ballot64(ok) == 0ull) continue;          // (wave-uniform: no window of this wave is whole)
        TLS_CHECK(a, at - h >= 0 && at - h + L <= slots, kChkSingle);
        const double2* win = s + (at - h);
        const const_f64_ptr q = taps + 2ll * rows[r].offset;
        double N = 0.0, D = 0.0;
#pragma unroll 8
        for (int j = 0; j < L; ++j) {
            const double2 v = win[j];
            const double nb = v.x * q[2 * j];
            const double db = v.y * q[2 * j + 1];
            N = N + nb;
            D = D + db;
        }
        if (ok && N > 0.0) {
            const double d = N / D;
            if (d > a.depth_min) {
                const double sv = N / sqrt(D);
                if (best_r < 0 || sv > best_s) { best_s = sv; best_r = r; best_d = d; }
            }
        }
    }
    if (c < n) {
        a.ses[curve * n + c] = best_s;
        a.row[curve * n + c] = best_r;
        a.depth[curve * n + c] = best_d;
    }
}

struct SingleSelectArgs {
    const double* t;                                 // [n]
    const double* ses; const int* row; const double* depth;   // [curves][n]
    const SingleRow* rows;                           // [n_rows]
    double* events;                                  // [curves][k][kSingleEventWords]
    long long* n_events;                             // [curves]
    unsigned long long* check;
    double min_ses, separation;
    int n, n_rows, k;
};

inline size_t single_select_lds_bytes(int n) { return (size_t)((n + kWave - 1) / kWave) * 8; }

// (value, index) a over b: b holds nothing, or a is larger, or as large at a lower index
__device__ __forceinline__ bool single_before(double av, int ai, double bv, int bi) {
    return ai != kSingleNone && (bi == kSingleNone || av > bv || (av == bv && ai < bi));
}

__global__ void __launch_bounds__(kSingleSelectThreads) tls_single_select_kernel(const SingleSelectArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned long long single_mask[];
    __shared__ double red_v[kMaxWaves + 1];
    __shared__ int red_i[kMaxWaves + 1];
    const int tid = threadIdx.x, nt = blockDim.x, n = a.n;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nw = nt / kWave;
    const long long curve = blockIdx.x;
    const double* ses = a.ses + curve * n;
    const int* row = a.row + curve * n;
    unsigned long long* mask = single_mask;
    // alive: one mask word per wave and step
    for (int base = 0; base < n; base += nt) {
        const int j = base + tid;
        bool alive = false;
        if (j < n) {
            const double v = ses[j];
            alive = !isnan(v) && v >= a.min_ses;
        }
        const unsigned long long m = __ballot(alive);
        if (lane == 0 && base + wave * kWave < n) mask[base / kWave + wave] = m;
    }
    wg_sync();
    double* out = a.events + curve * (long long)a.k * kSingleEventWords;
    int taken = 0;
    for (int round = 0; round < a.k; ++round) {
        double v = -INFINITY; int i = kSingleNone;
        for (int base = wave * kWave; base < n; base += nt) {
            const unsigned long long m = mask[base / kWave];
            if (m == 0ull) continue;
            if ((m >> lane) & 1ull) {
                const double p = ses[base + lane];
                if (single_before(p, base + lane, v, i)) { v = p; i = base + lane; }
            }
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const double ov = __shfl_down(v, d, kWave);
            const int oi = __shfl_down(i, d, kWave);
            if (single_before(ov, oi, v, i)) { v = ov; i = oi; }
        }
        if (lane == 0) { red_v[wave] = v; red_i[wave] = i; }
        wg_sync();
        if (wave == 0) {
            v = lane < nw ? red_v[lane] : -INFINITY; i = lane < nw ? red_i[lane] : kSingleNone;
#pragma unroll
            for (int d = kMaxWaves / 2; d > 0; d >>= 1) {
                const double ov = __shfl_down(v, d, kWave);
                const int oi = __shfl_down(i, d, kWave);
                if (single_before(ov, oi, v, i)) { v = ov; i = oi; }
            }
            if (lane == 0) { red_v[kMaxWaves] = v; red_i[kMaxWaves] = i; }
        }
        wg_sync();
        const int c = red_i[kMaxWaves];
        if (c == kSingleNone) break;                 // nothing alive (the same value in every thread)
        const int r = row[c];
        TLS_CHECK(a, c >= 0 && c < n && r >= 0 && r < a.n_rows, kChkSingle);
        const int L = a.rows[r].width;
        const int lo = c - (L - 1) / 2, hi = lo + L - 1;
        TLS_CHECK(a, lo >= 0 && hi <= n - 1, kChkSingle);
        if (tid == 0) {
            double* o = out + (long long)taken * kSingleEventWords;
            o[0] = (double)c; o[1] = a.t[c]; o[2] = red_v[kMaxWaves]; o[3] = a.depth[curve * n + c];
            o[4] = (double)r; o[5] = (double)L; o[6] = a.t[lo]; o[7] = a.t[hi];
        }
        ++taken;
        if (round + 1 == a.k) break;
        // the guard: g = int(separation * L), no larger than n (a larger one clears everything as well)
        const double gd = a.separation * (double)L;
        const int g = gd < (double)n ? (int)gd : n;
        const int first = lo - g, last = hi + g;
        for (int base = wave * kWave; base < n; base += nt) {
            const unsigned long long m = mask[base / kWave];
            if (m == 0ull) continue;
            bool kill = false;
            if ((m >> lane) & 1ull) {
                const int j = base + lane;
                const int Lj = a.rows[row[j]].width;
                const int lo_j = j - (Lj - 1) / 2, hi_j = lo_j + Lj - 1;
                kill = lo_j <= last && hi_j >= first;
            }
            const unsigned long long gone = __ballot(kill);
            if (lane == 0 && gone != 0ull) mask[base / kWave] = m & ~gone;
        }
        wg_sync();
    }
    // (`taken` is the same in every thread) ranks past it: index -1, NaN elsewhere
    if (tid == 0) a.n_events[curve] = taken;
    for (int q = taken * kSingleEventWords + tid; q < a.k * kSingleEventWords; q += nt)
        out[q] = (q % kSingleEventWords) == 0 ? -1.0 : (double)NAN;
}
