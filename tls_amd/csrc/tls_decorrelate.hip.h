// tls_decorrelate.hip.h -- regression detrending against shared and per-curve series (tls_decorrelate).  DESIGN.md
// "Decorrelation"; the statement is in include/tls_amd.h and, in Python, in tests/decorrelate_spec.py.
//
// tls_decorrelate_kernel: one workgroup of 256 threads a (curve, segment).  A segment's columns do not fit the LDS (4320 points
// x 17 columns x 8 B is over 500 KB), so every pass streams the segment in tiles of 256 points: thread t loads point t of the
// tile from every column (coalesced) and writes its values into the LDS tile, and after the barrier the OWNER of a sum -- one
// thread a sum -- adds the tile's products in index order.  Every sum of the statement is so a plain left-to-right sum held in
// one register from the first tile to the last: no reduction tree, no floating-point atomic.  The passes of a fit:
//   A  W, Sy and the m column sums (m + 2 owners; the tile holds x_k, y and a column of 1.0, so every owner runs the same code)
//   B  the m sums of squares about the means (m owners)
//   C  the m (m + 1) / 2 entries of G and the m of b (at most 152 owners; the tile holds u_k and z)
//   D  thread 0: Cholesky and the substitutions, in place in the LDS
//   E  one thread a point forms r (kept in the trend row, which the same thread reads back in the clip); thread 0 owns Q
//   clip: one thread a point; F loses its bit through an integer atomic
// F is a bit mask: in the LDS for a segment of at most kDecorLdsPoints points, in device scratch (the same passes) beyond.
// The tile is [column][kDecorStride] doubles with kDecorStride = 258: the owners of one step read the same point of different
// columns, 258 * 8 B apart, which is 4 banks on -- 16 columns on 16 different bank pairs -- and the loaders write
// consecutive doubles.  Included by tls_kernels.hip.h (namespace tlsdev).

constexpr int kDecorThreads = 256;
constexpr int kDecorTile = 256;
constexpr int kDecorStride = 258;
constexpr int kDecorMaxTerms = 16;
constexpr int kDecorMaxIter = 16;
constexpr int kDecorLdsPoints = 32768;
constexpr int kDecorWords = 8;                       // tls_decor_fit
constexpr double kDecorPivot = 1e-10;

struct DecorArgs {
    const double* y;                                 // [R][n]
    const double* dy;                                // [R][n], or nullptr: w = 1.0
    const unsigned char* mask;                       // [R][n], or nullptr: nothing protected
    const double* shared;                            // [n_shared][n]
    const double* own;                               // [R][n_own][n]
    const long long* segments;                       // [S + 1]
    double* flat;                                    // [R][n]
    double* trend;                                   // [R][n] (between the passes: r)
    double* record;                                  // [R][S][kDecorWords]
    double* coef;                                    // [R][S][m]
    double* mean;                                    // [R][S][m]
    double* scale;                                   // [R][S][m]
    unsigned int* members;                           // [R * S][member_words]: F where a segment is longer than kDecorLdsPoints
    long long n, member_words;
    double ridge, sigma_upper, sigma_lower;
    int n_shared, n_own, S, n_iter;
};

__global__ void __launch_bounds__(kDecorThreads) tls_decorrelate_kernel(const DecorArgs a) {
#pragma clang fp contract(off)
    __shared__ double tile[kDecorMaxTerms + 2][kDecorStride];
    __shared__ double wt[kDecorTile];
    __shared__ unsigned int ft[kDecorTile];
    __shared__ double G[kDecorMaxTerms][kDecorMaxTerms + 1];   // the lower triangle, then L in place (17: the rows on different banks)
    __shared__ double bv[kDecorMaxTerms], cf[kDecorMaxTerms], mean[kDecorMaxTerms], scale[kDecorMaxTerms], sums[kDecorMaxTerms + 2];
    __shared__ int live[kDecorMaxTerms];
    __shared__ double sigma_word;
    __shared__ int iword[3];                                   // 0 |F|, 1 the points that left this round, 2 a bad trend value
    __shared__ unsigned int lds_members[kDecorLdsPoints / 32];
    const int tid = threadIdx.x;
    const int m = a.n_shared + a.n_own;
    const long long c = blockIdx.x / a.S;
    const int seg = (int)(blockIdx.x % a.S);
    const long long lo = a.segments[seg], hi = a.segments[seg + 1], len = hi - lo;
    const long long row = c * a.n;
    const double* y = a.y + row;
    const double* dy = a.dy ? a.dy + row : nullptr;
    const unsigned char* mask = a.mask ? a.mask + row : nullptr;
    double* trend = a.trend + row;
    double* flat = a.flat + row;
    const long long words = (len + 31) / 32;
    unsigned int* F = len <= kDecorLdsPoints ? lds_members : a.members + (long long)blockIdx.x * a.member_words;
    auto column = [&](int k) -> const double* {
        return k < a.n_shared ? a.shared + (long long)k * a.n : a.own + (c * a.n_own + (k - a.n_shared)) * a.n;
    };
    auto weight = [&](long long j) -> double {
#pragma clang fp contract(off)
        if (!dy) return 1.0;
        const double e = dy[j]; const double pp = e * e;
        return 1.0 / pp;
    };
    auto member = [&](long long j) -> bool { return (F[(j - lo) >> 5] >> ((j - lo) & 31)) & 1u; };
    // F: the unprotected points of the segment; a word belongs to one thread (bits past the segment stay 0)
    for (long long q = tid; q < words; q += kDecorThreads) {
        unsigned int bits = 0;
        for (int b = 0; b < 32; ++b) {
            const long long j = lo + q * 32 + b;
            if (j < hi && !(mask && mask[j])) bits |= 1u << b;
        }
        F[q] = bits;
    }
    if (tid < kDecorMaxTerms) { cf[tid] = 0.0; mean[tid] = 0.0; scale[tid] = 1.0; live[tid] = 0; }
    wg_sync();
    int rounds = 0, n_clipped = 0, status = 0, dropped = 0;
    double mu = 0.0, sigma = (double)NAN;
    // the entry of G or b this thread owns in pass C: (ka, la) with la <= ka, or la == m for b
    int ka = -1, la = -1;
    {
        const int pairs = m * (m + 1) / 2;
        if (tid < pairs) { int k = 0; while ((k + 1) * (k + 2) / 2 <= tid) ++k; ka = k; la = tid - k * (k + 1) / 2; }
        else if (tid < pairs + m) { ka = tid - pairs; la = m; }
    }
    for (;;) {
        // ---- count F
        if (tid == 0) iword[0] = 0;
        wg_sync();
        {
            int mine = 0;
            for (long long q = tid; q < words; q += kDecorThreads) mine += __popc(F[q]);
            if (mine) atomicAdd(&iword[0], mine);
        }
        wg_sync();
        const int nF = iword[0];
        const bool everyone = nF == 0;
        // ---- pass A: tile rows 0 .. m - 1 = x_k, m = y, m + 1 = 1.0; owner t < m + 2 adds w * tile[t]
        double s = 0.0;
        for (long long base = lo; base < hi; base += kDecorTile) {
            const long long j = base + tid;
            wg_sync();                               // (the owners are done with the tile before)
            if (j < hi) {
                for (int k = 0; k < m; ++k) tile[k][tid] = column(k)[j];
                tile[m][tid] = y[j]; tile[m + 1][tid] = 1.0;
                wt[tid] = weight(j); ft[tid] = everyone || member(j);
            }
            wg_sync();
            if (tid < m + 2) {
                const int cnt = (int)(hi - base < kDecorTile ? hi - base : kDecorTile);
                for (int q = 0; q < cnt; ++q) if (ft[q]) { const double p = wt[q] * tile[tid][q]; s = s + p; }
            }
        }
        if (tid < m + 2) sums[tid] = s;
        wg_sync();
        const double W = sums[m + 1];
        mu = sums[m] / W;
        if (everyone) { status = 1; break; }         // (the whole workgroup: nF is one word)
        if (tid < m) mean[tid] = sums[tid] / W;
        wg_sync();
        // ---- pass B: tile rows = x_k - mean_k; owner k adds (w * d) * d
        s = 0.0;
        for (long long base = lo; base < hi; base += kDecorTile) {
            const long long j = base + tid;
            wg_sync();
            if (j < hi) {
                for (int k = 0; k < m; ++k) tile[k][tid] = column(k)[j] - mean[k];
                wt[tid] = weight(j); ft[tid] = member(j);
            }
            wg_sync();
            if (tid < m) {
                const int cnt = (int)(hi - base < kDecorTile ? hi - base : kDecorTile);
                for (int q = 0; q < cnt; ++q) if (ft[q]) { const double d = tile[tid][q]; const double p = wt[q] * d; const double pp = p * d; s = s + pp; }
            }
        }
        if (tid < m) {
            const double v = s / W;
            const double sc = sqrt(v);
            scale[tid] = sc; live[tid] = (sc > 0.0 && sc < (double)INFINITY) ? 1 : 0; cf[tid] = 0.0;
        }
        wg_sync();
        int n_live = 0;
        dropped = 0;
        for (int k = 0; k < m; ++k) { if (live[k]) ++n_live; else dropped |= 1 << k; }
        if (nF < n_live + 2) { status = 1; break; }
        // ---- pass C: tile rows 0 .. m - 1 = u_k, m = z
        s = 0.0;
        for (long long base = lo; base < hi; base += kDecorTile) {
            const long long j = base + tid;
            wg_sync();
            if (j < hi) {
                for (int k = 0; k < m; ++k) {
                    double u = 0.0;
                    if (live[k]) { const double d = column(k)[j] - mean[k]; u = d / scale[k]; }
                    tile[k][tid] = u;
                }
                const double q = y[j] / mu;
                tile[m][tid] = q - 1.0;
                wt[tid] = weight(j); ft[tid] = member(j);
            }
            wg_sync();
            if (ka >= 0) {
                const int cnt = (int)(hi - base < kDecorTile ? hi - base : kDecorTile);
                for (int q = 0; q < cnt; ++q) if (ft[q]) { const double p = wt[q] * tile[ka][q]; const double pp = p * tile[la][q]; s = s + pp; }
            }
        }
        if (ka >= 0) {
            if (la == m) bv[ka] = s;
            else if (la == ka) { const double rw = a.ridge * W; G[ka][la] = s + rw; }
            else G[ka][la] = s;
        }
        wg_sync();
        // ---- D: thread 0 solves, in place: L replaces the lower triangle of G
        if (tid == 0) {
            for (int j = 0; j < m; ++j) {
                if (!live[j]) continue;
                const double gjj = G[j][j];
                double t = gjj;
                for (int k = 0; k < j; ++k) if (live[k]) { const double p = G[j][k] * G[j][k]; t = t - p; }
                const double least = kDecorPivot * gjj;
                if (!(t > least)) { live[j] = 0; continue; }
                const double ljj = sqrt(t);
                G[j][j] = ljj;
                for (int i = j + 1; i < m; ++i) {
                    if (!live[i]) continue;
                    double q = G[i][j];
                    for (int k = 0; k < j; ++k) if (live[k]) { const double p = G[i][k] * G[j][k]; q = q - p; }
                    G[i][j] = q / ljj;
                }
            }
            for (int j = 0; j < m; ++j) {            // forward: v in bv
                if (!live[j]) continue;
                double t = bv[j];
                for (int k = 0; k < j; ++k) if (live[k]) { const double p = G[j][k] * bv[k]; t = t - p; }
                bv[j] = t / G[j][j];
            }
            for (int j = m - 1; j >= 0; --j) {       // back
                cf[j] = 0.0;
                if (!live[j]) continue;
                double t = bv[j];
                for (int k = j + 1; k < m; ++k) if (live[k]) { const double p = G[k][j] * cf[k]; t = t - p; }
                cf[j] = t / G[j][j];
            }
        }
        wg_sync();
        for (int k = 0; k < m; ++k) if (!live[k]) dropped |= 1 << k;
        // ---- pass E: r of every point of the segment (into the trend row); thread 0 owns Q
        s = 0.0;
        for (long long base = lo; base < hi; base += kDecorTile) {
            const long long j = base + tid;
            wg_sync();
            if (j < hi) {
                double p = 0.0;
                for (int k = 0; k < m; ++k) if (live[k]) { const double d = column(k)[j] - mean[k]; const double u = d / scale[k]; const double cu = cf[k] * u; p = p + cu; }
                const double q = y[j] / mu;
                const double z = q - 1.0;
                const double r = z - p;
                trend[j] = r;
                tile[0][tid] = r; wt[tid] = weight(j); ft[tid] = member(j);
            }
            wg_sync();
            if (tid == 0) {
                const int cnt = (int)(hi - base < kDecorTile ? hi - base : kDecorTile);
                for (int q = 0; q < cnt; ++q) if (ft[q]) { const double r = tile[0][q]; const double p = wt[q] * r; const double pp = p * r; s = s + pp; }
            }
        }
        if (tid == 0) { const double v = s / W; sigma_word = sqrt(v); iword[1] = 0; }
        wg_sync();
        sigma = sigma_word;
        if (rounds == a.n_iter) break;
        // ---- clip: every thread reads back the r it wrote
        const double up = a.sigma_upper * sigma;
        const double dn = a.sigma_lower * sigma;
        const double down = -dn;
        for (long long j = lo + tid; j < hi; j += kDecorThreads) {
            const double r = trend[j];
            if (member(j) && (r > up || r < down)) {
                atomicAnd(&F[(j - lo) >> 5], ~(1u << ((j - lo) & 31)));
                atomicAdd(&iword[1], 1);
            }
        }
        wg_sync();
        const int left = iword[1];
        ++rounds;
        n_clipped += left;
        if (left == 0) break;
    }
    // (every thread took the same way out: the decisions above read LDS words behind a barrier)
    wg_sync();
    if (status == 1) {
        dropped = 0; sigma = (double)NAN;
        if (tid < kDecorMaxTerms) { cf[tid] = 0.0; mean[tid] = 0.0; scale[tid] = 1.0; live[tid] = 0; }
    }
    if (tid == 0) iword[2] = 0;
    wg_sync();
    // ---- the trend and the flat row at every point of the segment
    int bad = 0;
    for (long long j = lo + tid; j < hi; j += kDecorThreads) {
        double p = 0.0;
        for (int k = 0; k < m; ++k) if (live[k]) { const double d = column(k)[j] - mean[k]; const double u = d / scale[k]; const double cu = cf[k] * u; p = p + cu; }
        const double one = 1.0 + p;
        const double tr = mu * one;
        trend[j] = tr;
        flat[j] = y[j] / tr;
        if (!(tr > 0.0 && tr < (double)INFINITY)) bad = 1;
    }
    if (bad) atomicOr(&iword[2], 1);
    wg_sync();
    if (iword[2]) {
        status = 2;
        for (long long j = lo + tid; j < hi; j += kDecorThreads) { trend[j] = mu; flat[j] = y[j] / mu; }
    }
    // ---- the record and the tables
    if (tid == 0) iword[0] = 0;
    wg_sync();
    {
        int mine = 0;
        for (long long q = tid; q < words; q += kDecorThreads) mine += __popc(F[q]);
        if (mine) atomicAdd(&iword[0], mine);
    }
    wg_sync();
    if (tid == 0) {
        int n_live = 0;
        for (int k = 0; k < m; ++k) n_live += live[k];
        double* o = a.record + (long long)blockIdx.x * kDecorWords;
        o[0] = (double)status; o[1] = (double)dropped; o[2] = (double)iword[0]; o[3] = (double)n_clipped; o[4] = (double)rounds;
        o[5] = mu; o[6] = sigma; o[7] = (double)n_live;
    }
    if (tid < m) {
        const long long at = (long long)blockIdx.x * m + tid;
        a.coef[at] = cf[tid]; a.mean[at] = mean[tid]; a.scale[at] = scale[tid];
    }
}
