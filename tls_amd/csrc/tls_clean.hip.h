// tls_clean.hip.h -- the cleaning stage of survey mode (tls_clean_rows): the bad points of every light curve flagged (missing,
// the caller's, high and low outliers by rounds of a robust clip) and replaced with defined values, so that everything
// downstream keeps its shared time stamps.  The statement is in include/tls_amd.h and tests/clean_spec.py; DESIGN.md "Cleaning".
//
// Four kernels, all on one stream:
//   tls_clean_init     a thread a point: the flags 1 (not (isfinite(y) and y > 0)) and 2 (the caller's); a missing value is
//                      overwritten with 1.0 in the device copy of the row, so that no NaN or negative bit pattern is ever a
//                      sort key (the repair never reads a flagged value).  Sets the row's "still running" word.
//   tls_clean_tile     a round's sliding centre, the hot path: the biweight's tiles (detrend_stage_sort: a tile's span in the
//                      LDS as (key, slot) pairs sorted once; a lane an output, scanning the sorted slots inside its window).
//                      A flagged slot gets the top bit of its slot word, as a protected point does in biweight_tile<kBiweightMasked>,
//                      and the output's own slot is skipped: the leave-one-out median.  The valid members of a window are
//                      counted from a running count of the span's valid slots.  r = y - centre, NaN: no residual.
//   tls_clean_row      one workgroup a row: c0 and sigma of the residuals by the noise profile's radix selection (noise_median),
//                      the high flags, the low candidates and their runs, the guard, the flags and the row's "still running"
//                      word; the rows still running are counted in counts[round] with an integer atomic.  The row lies in the
//                      LDS up to kNoiseLdsPoints points, in device memory beyond.
//   tls_clean_repair   one workgroup a row: the nearest valid neighbours of every flagged point by a sweep over 256 stretches,
//                      the interpolation, the fills and the record.
// No floating-point atomic and no sum at all: every value is a selection or one IEEE operation of the statement, contraction
// off.  A finished row's workgroups return at once: the word they test is written by an earlier kernel.
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_biweight.hip.h and tls_noise.hip.h.

constexpr int kCleanWords = 10;                      // tls_clean_record
constexpr int kCleanMaxIter = 16;
constexpr double kCleanMad = 1.4826;
constexpr unsigned char kCleanMissing = 1, kCleanBad = 2, kCleanHigh = 4, kCleanLow = 8;

struct CleanArgs {
    const double* t;                                 // [n]
    const int* seg;                                  // [n] the segment of every point, ascending from 0
    double* y;                                       // [R][n] the rows; a missing value becomes 1.0 (tls_clean_init)
    const unsigned char* bad;                        // [R][n] != 0: the caller's flag, or nullptr
    unsigned char* flags;                            // [R][n]
    double* r;                                       // [R][n] a round's residuals, NaN: none
    unsigned char* code;                             // [R][n] a round's codes of a long row, or nullptr (LDS)
    double* out;                                     // [R][n] the repaired rows
    double* records;                                 // [R][kCleanWords]
    unsigned int* run;                               // [R] != 0: the row's rounds go on
    unsigned long long* counts;                      // [kCleanMaxIter] the rows still running behind round k
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    const int* lo;                                   // [n] first point of each point's window, or nullptr: the row's median
    const int* hi;                                   // [n] one past its last point
    double sigma_upper, sigma_lower;
    long long max_run;
    long long n, count;                              // points a row; R * n
    int n_iter, min_points, round, rounds_wanted;    // round: the rounds done before this one; rounds_wanted: 0 no round runs
    int tile, span, smax;                            // the biweight's plan (tls_clean_tile)
};

constexpr size_t clean_tile_lds_bytes(int P, int smax) { return (size_t)P * 12 + ((size_t)smax + 1 + kDetrendThreads) * 4; }
constexpr size_t clean_row_lds_bytes(int n, bool lds) { return sizeof(NoiseShared) + (lds ? (size_t)n * 9 : 0); }

__global__ void __launch_bounds__(kDetrendThreads) tls_clean_init(const CleanArgs a) {
    for (long long e = (long long)blockIdx.x * kDetrendThreads + threadIdx.x; e < a.count; e += (long long)gridDim.x * kDetrendThreads) {
        const double v = a.y[e];
        unsigned char f = (v > 0.0 && v < (double)INFINITY) ? 0 : kCleanMissing;   // (NaN fails both)
        if (a.bad && a.bad[e]) f |= kCleanBad;
        a.flags[e] = f;
        if (f & kCleanMissing) a.y[e] = 1.0;
        const long long row = e / a.n;
        if (e - row * a.n == 0) {
            a.run[row] = a.rounds_wanted ? 1u : 0u;
            double* rec = a.records + row * kCleanWords;
            rec[7] = 0.0; rec[8] = (double)NAN; rec[9] = (double)NAN;
        }
    }
}

// LDS: keys [P] (uint64) | slot numbers [P] (uint32) | valid slots in front of slot s [smax + 1] (uint32) | a thread's count
// [256] (uint32).  Grid (ceil(n / T), rows).
__global__ void __launch_bounds__(kDetrendThreads) tls_clean_tile(const CleanArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned long long clean_lds[];
    const long long row = blockIdx.y;
    if (a.run[row] == 0u) return;                    // (the whole workgroup: the word is an earlier kernel's)
    const int P = a.span, T = a.tile, tid = threadIdx.x;
    unsigned long long* keys = clean_lds;
    unsigned int* slot = reinterpret_cast<unsigned int*>(keys + P);
    unsigned int* before = slot + P;
    unsigned int* part = before + a.smax + 1;
    const long long first = (long long)blockIdx.x * T;
    const long long n_out = a.n - first < (long long)T ? a.n - first : (long long)T;
    const long long base = a.lo[first];
    const int S = (int)(a.hi[first + n_out - 1] - base);
    TLS_CHECK(a, S >= 1 && S <= a.smax && S <= P, kChkBiweight);
    const double* y = a.y + row * a.n;
    const double nan = (double)NAN;

    detrend_stage_sort(a, y, base, a.n, S, P, keys, slot, nullptr, kChkBiweight);

    const unsigned char* fl = a.flags + row * a.n + base;   // (the span lies inside the row: base + s < n for s < S)
    for (int j = tid; j < P; j += kDetrendThreads) {
        const unsigned int s = slot[j];
        if (s < (unsigned int)S && fl[s]) slot[j] = s | kBiweightProtected;
    }
    // before[s] = the valid among the slots < s: a thread counts its stretch, then writes the running count
    const int stretch = (S + kDetrendThreads - 1) / kDetrendThreads;
    const int s0 = tid * stretch < S ? tid * stretch : S, s1 = s0 + stretch < S ? s0 + stretch : S;
    unsigned int mine = 0u;
    for (int s = s0; s < s1; ++s) mine += (unsigned int)(fl[s] == 0);
    part[tid] = mine;
    wg_sync();
    unsigned int running = 0u;
    for (int k = 0; k < tid; ++k) running += part[k];
    for (int s = s0; s < s1; ++s) { before[s] = running; running += (unsigned int)(fl[s] == 0); }
    if (tid == kDetrendThreads - 1) before[S] = running;
    wg_sync();

    for (int i = tid; i < n_out; i += kDetrendThreads) {
        const long long g = first + i;
        const long long o = row * a.n + g;
        if (a.flags[o] != 0) { a.r[o] = nan; continue; }
        const int wa = (int)(a.lo[g] - base), wb = (int)(a.hi[g] - base);   // the window's slots [wa, wb)
        TLS_CHECK(a, wa >= 0 && wa < wb && wb <= S, kChkBiweight);
        const unsigned int ua = (unsigned int)wa, wn = (unsigned int)(wb - wa), own = (unsigned int)(g - base);
        TLS_CHECK(a, own - ua < wn && before[wb] > before[wa], kChkBiweight);
        const unsigned int m = before[wb] - before[wa] - 1u;   // the valid points of the window other than this one
        if ((long long)m < (long long)a.min_points) { a.r[o] = nan; continue; }
        const unsigned int need1 = (m + 1u) >> 1, need2 = (m >> 1) + 1u;
        int f1 = 0, f2 = 0;
        {
            unsigned int c = 0u;
            for (int j = 0; j < S; ++j) {
                const unsigned int s = slot[j];
                if (s - ua < wn && s != own) {
                    ++c;
                    if (c == need1) f1 = j;
                    if (c == need2) { f2 = j; break; }
                }
            }
        }
        TLS_CHECK(a, f1 < S && f2 < S, kChkBiweight);
        const double v1 = __longlong_as_double((long long)keys[f1]), v2 = __longlong_as_double((long long)keys[f2]);
        const double centre = (m & 1u) ? v2 : (v1 + v2) / 2.0;
        a.r[o] = y[g] - centre;
    }
}

// LDS: NoiseShared | r [n] | code [n] (LDS).  Grid (rows).
template <bool LDS>
__global__ void __launch_bounds__(kNoiseThreads) tls_clean_row_kernel(const CleanArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char clean_row_lds[];
    const long long row = blockIdx.x;
    if (a.run[row] == 0u) return;                    // (the whole workgroup: the word is an earlier kernel's)
    NoiseShared* sh = reinterpret_cast<NoiseShared*>(clean_row_lds);
    const int tid = threadIdx.x, n = (int)a.n;
    const bool sliding = a.lo != nullptr;
    double* r = LDS ? reinterpret_cast<double*>(clean_row_lds + sizeof(NoiseShared)) : a.r + row * a.n;
    unsigned char* code = LDS ? reinterpret_cast<unsigned char*>(r + n) : a.code + row * a.n;
    unsigned char* fl = a.flags + row * a.n;
    const double* y = a.y + row * a.n;
    const double* gr = a.r + row * a.n;
    double* rec = a.records + row * kCleanWords;
    const double nan = (double)NAN;

    // the residuals a sliding centre left (tls_clean_tile), or the valid values themselves
    if (tid == 0) { sh->cnt[2] = 0u; sh->cnt[3] = 0u; }
    wg_sync();
    unsigned int valid_mine = 0u, has_mine = 0u;
    for (int i = tid; i < n; i += kNoiseThreads) {
        const bool valid = fl[i] == 0;
        const double v = sliding ? gr[i] : (valid ? y[i] : nan);
        if (LDS || !sliding) r[i] = v;
        valid_mine += (unsigned int)valid;
        has_mine += (unsigned int)(v == v);
    }
    atomicAdd(&sh->cnt[2], valid_mine);
    atomicAdd(&sh->cnt[3], has_mine);
    wg_sync();
    const unsigned int n_valid = sh->cnt[2], n_has = sh->cnt[3];
    wg_sync();                                       // (read by all before the count of the new flags resets the word)
    TLS_CHECK(a, n_has <= n_valid && n_valid <= (unsigned int)n, kChkNoise);
    if (n_has < 2u) {                                // (the whole workgroup)
        if (tid == 0) a.run[row] = 0u;
        return;
    }
    auto residual = [&](int i, unsigned long long& k) -> bool {
        const double v = r[i];
        if (!(v == v)) return false;
        k = noise_key(v);
        return true;
    };
    double med = nan;
    if (!sliding) {
        med = noise_median(a, sh, residual, n, n_has);
        for (int i = tid; i < n; i += kNoiseThreads) {
            const double v = r[i];
            if (v == v) r[i] = v - med;
        }
        wg_sync();
    }
    const double c0 = noise_median(a, sh, residual, n, n_has);
    const double mad = noise_median(a, sh, [&](int i, unsigned long long& k) -> bool {
        const double v = r[i];
        if (!(v == v)) return false;
        k = noise_key(fabs(v - c0));
        return true;
    }, n, n_has);
    const double sigma = kCleanMad * mad;
    const int rounds = a.round + 1;
    if (tid == 0) { rec[7] = (double)rounds; rec[8] = sliding ? c0 : med; rec[9] = sigma; }
    if (!(sigma > 0.0)) {                            // (the whole workgroup)
        if (tid == 0) a.run[row] = 0u;
        return;
    }
    const double up = a.sigma_upper * sigma;
    const double down = -(a.sigma_lower * sigma);
    // a point's code: 0 not valid (a run steps over it), 1 valid and no candidate, 2 low candidate, 3 high
    for (int i = tid; i < n; i += kNoiseThreads) {
        unsigned char c = 0;
        if (fl[i] == 0) {
            c = 1;
            const double v = r[i];
            if (v == v) {
                const double d = v - c0;
                if (d > up) c = 3;
                else if (d < down) c = 2;
            }
        }
        code[i] = c;
    }
    if (tid == 0) sh->cnt[2] = 0u;
    wg_sync();
    // the run of a low candidate: its neighbours in the sequence of the valid points of its segment, to both sides, up to the
    // first that is no candidate; true when the run holds at most max_run
    const int* seg = a.seg;
    const long long max_run = a.max_run;
    auto short_run = [&](int i) -> bool {
        long long members = 1;
        for (int p = i; p > 0 && seg[p - 1] == seg[i];) {
            --p;
            const unsigned char c = code[p];
            if (c == 0) continue;
            if (c != 2) break;
            if (++members > max_run) return false;
        }
        for (int p = i; p + 1 < n && seg[p + 1] == seg[i];) {
            ++p;
            const unsigned char c = code[p];
            if (c == 0) continue;
            if (c != 2) break;
            if (++members > max_run) return false;
        }
        return true;
    };
    unsigned int fresh = 0u;
    for (int i = tid; i < n; i += kNoiseThreads) {
        const unsigned char c = code[i];
        if (c == 3 || (c == 2 && short_run(i))) ++fresh;
    }
    atomicAdd(&sh->cnt[2], fresh);
    wg_sync();
    const unsigned int n_fresh = sh->cnt[2];
    TLS_CHECK(a, n_fresh <= n_has, kChkNoise);
    if (n_fresh == 0u || n_valid < n_fresh + 2u) {   // (the whole workgroup) nobody flagged, or the round is not applied
        if (tid == 0) a.run[row] = 0u;
        return;
    }
    for (int i = tid; i < n; i += kNoiseThreads) {
        const unsigned char c = code[i];
        if (c == 3) fl[i] = fl[i] | kCleanHigh;
        else if (c == 2 && short_run(i)) fl[i] = fl[i] | kCleanLow;
    }
    if (tid == 0) {
        if (rounds >= a.n_iter) a.run[row] = 0u;
        else atomicAdd(&a.counts[a.round], 1ull);
    }
}

struct CleanRepairShared {
    int last_valid[kNoiseThreads], first_valid[kNoiseThreads];     // of a thread's stretch, -1: none
    int lead[kNoiseThreads], trail[kNoiseThreads], inner[kNoiseThreads], length[kNoiseThreads];   // its filled stretches
    unsigned int tally[5][kNoiseThreads];            // missing, bad, high, low, filled
    unsigned int filled;                             // of the row
    unsigned int need;                               // != 0: a point has no valid neighbour in its segment
};

// Grid (rows).
__global__ void __launch_bounds__(kNoiseThreads) tls_clean_repair_kernel(const CleanArgs a) {
#pragma clang fp contract(off)
    __shared__ NoiseShared noise_words;
    __shared__ CleanRepairShared rs;
    NoiseShared* sh = &noise_words;
    const long long row = blockIdx.x;
    const int tid = threadIdx.x, n = (int)a.n;
    const unsigned char* fl = a.flags + row * a.n;
    const double* y = a.y + row * a.n;
    const double* t = a.t;
    const int* seg = a.seg;
    double* out = a.out + row * a.n;
    double* rec = a.records + row * kCleanWords;
    const double nan = (double)NAN;
    const int stretch = (n + kNoiseThreads - 1) / kNoiseThreads;
    const int i0 = (long long)tid * stretch < n ? tid * stretch : n, i1 = i0 + stretch < n ? i0 + stretch : n;

    // a thread's stretch: its first and last valid point, its tallies, the filled points at its ends and its longest inside
    {
        int lastv = -1, firstv = -1, lead = 0, cur = 0, best = 0;
        unsigned int c1 = 0u, c2 = 0u, c4 = 0u, c8 = 0u, cf = 0u;
        for (int i = i0; i < i1; ++i) {
            const unsigned char f = fl[i];
            if (f == 0) {
                if (firstv < 0) { firstv = i; lead = cur; }
                lastv = i;
                cur = 0;
            } else {
                ++cur;
                best = cur > best ? cur : best;
                ++cf;
                c1 += (unsigned int)((f & kCleanMissing) != 0); c2 += (unsigned int)((f & kCleanBad) != 0);
                c4 += (unsigned int)((f & kCleanHigh) != 0); c8 += (unsigned int)((f & kCleanLow) != 0);
            }
        }
        rs.last_valid[tid] = lastv; rs.first_valid[tid] = firstv;
        rs.lead[tid] = firstv < 0 ? cur : lead; rs.trail[tid] = cur; rs.inner[tid] = best; rs.length[tid] = i1 - i0;
        rs.tally[0][tid] = c1; rs.tally[1][tid] = c2; rs.tally[2][tid] = c4; rs.tally[3][tid] = c8; rs.tally[4][tid] = cf;
    }
    if (tid == 0) rs.need = 0u;
    wg_sync();
    if (tid == 0) {
        unsigned int sum[5] = {0u, 0u, 0u, 0u, 0u};
        int cur = 0, best = 0;
        for (int k = 0; k < kNoiseThreads; ++k) {
            for (int q = 0; q < 5; ++q) sum[q] += rs.tally[q][k];
            if (rs.length[k] == 0) continue;
            if (rs.first_valid[k] < 0) {
                cur += rs.length[k];
            } else {
                cur += rs.lead[k];
                best = cur > best ? cur : best;
                best = rs.inner[k] > best ? rs.inner[k] : best;
                cur = rs.trail[k];
            }
            best = cur > best ? cur : best;
        }
        rec[1] = (double)sum[0]; rec[2] = (double)sum[1]; rec[3] = (double)sum[2]; rec[4] = (double)sum[3];
        rec[5] = (double)sum[4]; rec[6] = (double)best;
        rs.filled = sum[4];
    }
    wg_sync();
    const unsigned int n_valid = (unsigned int)n - rs.filled;
    TLS_CHECK(a, rs.filled <= (unsigned int)n, kChkNoise);
    if (n_valid == 0u) {                             // (the whole workgroup) a row without a valid point
        for (int i = tid; i < n; i += kNoiseThreads) out[i] = 1.0;
        if (tid == 0) rec[0] = 2.0;
        return;
    }
    // the nearest valid point in front of and behind the stretch
    int left = -1, right = -1;
    for (int k = tid - 1; k >= 0; --k)
        if (rs.last_valid[k] >= 0) { left = rs.last_valid[k]; break; }
    for (int k = tid + 1; k < kNoiseThreads; ++k)
        if (rs.first_valid[k] >= 0) { right = rs.first_valid[k]; break; }
    bool lonely = false;
    for (int k = i0; k < i1;) {
        if (fl[k] == 0) { left = k; out[k] = y[k]; ++k; continue; }
        int j = k + 1;
        while (j < i1 && fl[j] != 0) ++j;
        const int b = j < i1 ? j : right;
        TLS_CHECK(a, left < k && (b < 0 || (b >= j && b < n)), kChkNoise);
        for (int q = k; q < j; ++q) {
            const bool has_a = left >= 0 && seg[left] == seg[q], has_b = b >= 0 && seg[b] == seg[q];
            double v = nan;
            if (has_a && has_b) {
                const double ya = y[left], yb = y[b];
                const double den = t[b] - t[left];
                v = ya;
                if (den != 0.0) {
                    const double rise = yb - ya;
                    const double num = t[q] - t[left];
                    const double share = num / den;
                    const double step = rise * share;
                    v = ya + step;
                }
            } else if (has_a) {
                v = y[left];
            } else if (has_b) {
                v = y[b];
            } else {
                lonely = true;
            }
            out[q] = v;
        }
        k = j;
    }
    if (lonely) rs.need = 1u;
    wg_sync();
    const bool need = rs.need != 0u;
    if (need) {                                      // (the whole workgroup) a segment without a valid point: the row's median
        const double med = noise_median(a, sh, [&](int i, unsigned long long& k) -> bool {
            if (fl[i] != 0) return false;
            k = noise_key(y[i]);
            return true;
        }, n, n_valid);
        for (int i = i0; i < i1; ++i) {              // (a thread's own stretch: it wrote these words itself)
            const double v = out[i];
            if (!(v == v)) out[i] = med;
        }
    }
    if (tid == 0) rec[0] = need ? 1.0 : 0.0;
}
