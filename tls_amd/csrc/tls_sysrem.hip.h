// tls_sysrem.hip.h -- SysRem (Tamuz, Mazeh & Zucker 2005) for survey mode (tls_sysrem): the shared systematics of an ensemble
// of light curves on the same time stamps, fitted ACROSS the rows as rank-1 terms c_i a_j (star coefficient times epoch
// profile) of the residual matrix x_ij = y_ij / m_i - 1 by alternating weighted least squares, and divided out:
// trend_ij = m_i (1 + sum_k C_ik A_kj), flat_ij = y_ij / trend_ij.
//
// The statement is in include/tls_amd.h.  Every step is one IEEE double operation (no contraction: the pragma in the
// kernels; the library builds with -fno-fast-math) and both reductions have their order fixed:
//   rowsum: lane l of kSysremLanes = 256 adds v[l], v[l + 256], ... in ascending order from 0.0; the 256 partials fold by the
//           tree p[l] += p[l + s], s = 128, 64, .., 1;
//   colsum: chunks of kSysremRowChunk = 32 consecutive rows summed in ascending order from 0.0; the chunk sums added in
//           ascending order from 0.0;
// so the result, the stop decision and the iteration counts included, is bit-equal to tests/sysrem_spec.py.
//
// One iteration of component k is three launches:
//   tls_sysrem_columns  grid (ceil(n / 256), chunks): a thread owns one column of one 32-row chunk and adds its rows in order
//                       (neighbouring lanes read neighbouring doubles); it writes the chunk's partial sums;
//   tls_sysrem_epochs   a thread a column: the chunk partials in order, a_j, and the two maxima max |a_j - a_prev_j| and
//                       max |a_j| (workgroup maxima in LDS, then an integer atomic max on the bit patterns: non-negative doubles
//                       order as integers);
//   tls_sysrem_rows     a workgroup a row: the lane-strided sums and the LDS tree, c_i.
// c of component k lives in row k of c [K][rows] and a in row k of a [K][n]: iteration 1 reads c as 1.0 and a_prev as 0.0
// instead of the stored values, and a_prev of every later iteration is the stored a itself, so nothing is reset between
// components.  The host enqueues max_iter iterations per component without waiting.  The stop decision of iteration t
// (from the maxima of its epochs launch, slot t & 1 of the state) is taken by the columns launch of iteration t + 1: every
// workgroup takes the same one, the first sets done[k], and every later launch of the component returns at once on it.
// tls_sysrem_subtract removes a finished component from x (not behind the last one: x is not read again), and
// tls_sysrem_apply forms trend and flat and records the first trend value that is not finite and > 0.
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_biweight.hip.h.

constexpr int kSysremLanes = TLS_SYSREM_LANES;
constexpr int kSysremRowChunk = TLS_SYSREM_ROW_CHUNK;
// the state words: maxima [2 slots][diff, amax] | the first bad trend (~index, 0: none) | done [8] | iterations run [8]
constexpr int kSysremBad = 4, kSysremDone = 8, kSysremIters = kSysremDone + TLS_SYSREM_MAX_COMPONENTS;
constexpr int kSysremState = kSysremIters + TLS_SYSREM_MAX_COMPONENTS;
static_assert(kSysremLanes == 256 && (kSysremLanes & (kSysremLanes - 1)) == 0, "the tree folds a power of two");

struct SysremArgs {
    const double* y;              // [rows][n]
    const double* dy;             // [rows][n], or nullptr: one weight a row
    double* x;                    // [rows][n] residuals
    double* w;                    // [rows][n] with dy, [rows] without
    double* m;                    // [rows] row means
    double* c;                    // [K][rows]
    double* a;                    // [K][n]
    double* pnum;                 // [chunks][n] the chunks' numerators
    double* pden;                 // [chunks][n] ... and denominators
    double* flat;                 // [rows][n]
    double* trend;                // [rows][n], or nullptr
    unsigned long long* state;    // [kSysremState]
    unsigned long long* check;    // [kChecks] violated bounds (debug build; nullptr: off)
    long long n, rows, chunks;
    double tol;
    int n_components, k, iter;
};

// p[0] of the tree over the workgroup's 256 partials (every thread gets it)
__device__ __forceinline__ double sysrem_tree(double* p, double mine) {
#pragma clang fp contract(off)
    const int l = threadIdx.x;
    p[l] = mine;
    __syncthreads();
    for (int s = kSysremLanes / 2; s >= 1; s >>= 1) {
        if (l < s) p[l] = p[l] + p[l + s];
        __syncthreads();
    }
    const double r = p[0];
    __syncthreads();   // (p is reused by the next tree)
    return r;
}

// the component is finished before this launch: a launch behind the convergence returns at once
__device__ __forceinline__ bool sysrem_done(const SysremArgs& a) {
    return __atomic_load_n(&a.state[kSysremDone + a.k], __ATOMIC_RELAXED) != 0ull;
}

// m, x and the weights.  Grid (rows), one workgroup a row.
__global__ void __launch_bounds__(kSysremLanes) tls_sysrem_prepare(const SysremArgs a) {
#pragma clang fp contract(off)
    __shared__ double p[kSysremLanes];
    const long long i = blockIdx.x;
    TLS_CHECK(a, i < a.rows, kChkSysrem);
    const double* y = a.y + i * a.n;
    double* x = a.x + i * a.n;
    double acc = 0.0;
    for (long long j = threadIdx.x; j < a.n; j += kSysremLanes) acc = acc + y[j];
    const double m = sysrem_tree(p, acc) / (double)a.n;
    acc = 0.0;
    for (long long j = threadIdx.x; j < a.n; j += kSysremLanes) {
        const double v = y[j] / m - 1.0;
        x[j] = v;
        acc = acc + v * v;
    }
    if (a.dy) {
        const double* dy = a.dy + i * a.n;
        double* w = a.w + i * a.n;
        for (long long j = threadIdx.x; j < a.n; j += kSysremLanes) {
            const double r = dy[j] / m;
            w[j] = 1.0 / (r * r);
        }
    } else {
        const double v = sysrem_tree(p, acc) / (double)a.n;
        if (threadIdx.x == 0) a.w[i] = v > 0.0 ? 1.0 / v : 0.0;
    }
    if (threadIdx.x == 0) a.m[i] = m;
}

// The chunk partials of sum_i (x_ij c_i) w_ij and sum_i (c_i c_i) w_ij.  Grid (ceil(n / 256), min(chunks, 65535)).
__global__ void __launch_bounds__(kSysremLanes) tls_sysrem_columns(const SysremArgs a) {
#pragma clang fp contract(off)
    if (sysrem_done(a)) return;
    if (a.iter > 1) {
        // the stop decision of iteration iter - 1, the same in every workgroup (nothing writes its slot during this launch)
        const unsigned long long* mx = a.state + 2 * ((a.iter - 1) & 1);
        const double diff = __longlong_as_double((long long)mx[0]), amax = __longlong_as_double((long long)mx[1]);
        if (diff <= a.tol * amax) {
            if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
                __atomic_store_n(&a.state[kSysremDone + a.k], 1ull, __ATOMIC_RELAXED);
            return;
        }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        a.state[2 * (a.iter & 1)] = 0ull;       // this iteration's maxima (+0.0)
        a.state[2 * (a.iter & 1) + 1] = 0ull;
    }
    const long long j = (long long)blockIdx.x * kSysremLanes + threadIdx.x;
    if (j >= a.n) return;
    const double* c = a.c + (long long)a.k * a.rows;
    const bool first = a.iter == 1;    // c = 1.0
    for (long long q = blockIdx.y; q < a.chunks; q += gridDim.y) {
        const long long i0 = q * kSysremRowChunk;
        const long long i1 = i0 + kSysremRowChunk < a.rows ? i0 + kSysremRowChunk : a.rows;
        TLS_CHECK(a, i0 < i1, kChkSysrem);
        double num = 0.0, den = 0.0;
        if (a.dy) {
            for (long long i = i0; i < i1; ++i) {
                const double ci = first ? 1.0 : c[i];
                const double w = a.w[i * a.n + j];
                num = num + (a.x[i * a.n + j] * ci) * w;
                den = den + (ci * ci) * w;
            }
        } else {
            for (long long i = i0; i < i1; ++i) {
                const double ci = first ? 1.0 : c[i];
                const double w = a.w[i];
                num = num + (a.x[i * a.n + j] * ci) * w;
                den = den + (ci * ci) * w;
            }
        }
        a.pnum[q * a.n + j] = num;
        a.pden[q * a.n + j] = den;
    }
}

// a_j from the chunk partials, and the iteration's two maxima.  Grid (ceil(n / 256)).
__global__ void __launch_bounds__(kSysremLanes) tls_sysrem_epochs(const SysremArgs a) {
#pragma clang fp contract(off)
    if (sysrem_done(a)) return;
    __shared__ unsigned long long mx[2][kSysremLanes];
    const long long j = (long long)blockIdx.x * kSysremLanes + threadIdx.x;
    unsigned long long diff = 0ull, mag = 0ull;
    if (j < a.n) {
        double num = 0.0, den = 0.0;
        const double* pn = a.pnum + j;
        const double* pd = a.pden + j;
        long long q = 0;
        for (; q + 4 <= a.chunks; q += 4) {   // (four chunks' loads in flight; the sums keep their order)
            const double n0 = pn[q * a.n], n1 = pn[(q + 1) * a.n], n2 = pn[(q + 2) * a.n], n3 = pn[(q + 3) * a.n];
            const double d0 = pd[q * a.n], d1 = pd[(q + 1) * a.n], d2 = pd[(q + 2) * a.n], d3 = pd[(q + 3) * a.n];
            num = num + n0; num = num + n1; num = num + n2; num = num + n3;
            den = den + d0; den = den + d1; den = den + d2; den = den + d3;
        }
        for (; q < a.chunks; ++q) {
            num = num + pn[q * a.n];
            den = den + pd[q * a.n];
        }
        double* aj = a.a + (long long)a.k * a.n + j;
        const double prev = a.iter == 1 ? 0.0 : *aj;
        const double v = den > 0.0 ? num / den : 0.0;
        *aj = v;
        diff = (unsigned long long)__double_as_longlong(__builtin_fabs(v - prev));
        mag = (unsigned long long)__double_as_longlong(__builtin_fabs(v));
    }
    const int l = threadIdx.x;
    mx[0][l] = diff;
    mx[1][l] = mag;
    __syncthreads();
    for (int s = kSysremLanes / 2; s >= 1; s >>= 1) {
        if (l < s) {
            if (mx[0][l + s] > mx[0][l]) mx[0][l] = mx[0][l + s];
            if (mx[1][l + s] > mx[1][l]) mx[1][l] = mx[1][l + s];
        }
        __syncthreads();
    }
    if (l == 0) {
        unsigned long long* out = a.state + 2 * (a.iter & 1);
        atomicMax(&out[0], mx[0][0]);
        atomicMax(&out[1], mx[1][0]);
    }
}

// c_i = rowsum((x_ij a_j) w_ij) / rowsum((a_j a_j) w_ij).  Grid (rows), one workgroup a row.
__global__ void __launch_bounds__(kSysremLanes) tls_sysrem_rows(const SysremArgs a) {
#pragma clang fp contract(off)
    if (sysrem_done(a)) return;
    __shared__ double p[kSysremLanes];
    const long long i = blockIdx.x;
    TLS_CHECK(a, i < a.rows, kChkSysrem);
    const double* x = a.x + i * a.n;
    const double* aj = a.a + (long long)a.k * a.n;
    double num = 0.0, den = 0.0;
    if (a.dy) {
        const double* w = a.w + i * a.n;
        for (long long j = threadIdx.x; j < a.n; j += kSysremLanes) {
            const double v = aj[j];
            num = num + (x[j] * v) * w[j];
            den = den + (v * v) * w[j];
        }
    } else {
        const double w = a.w[i];
        for (long long j = threadIdx.x; j < a.n; j += kSysremLanes) {
            const double v = aj[j];
            num = num + (x[j] * v) * w;
            den = den + (v * v) * w;
        }
    }
    num = sysrem_tree(p, num);
    den = sysrem_tree(p, den);
    if (threadIdx.x == 0) {
        a.c[(long long)a.k * a.rows + i] = den > 0.0 ? num / den : 0.0;
        if (i == 0) a.state[kSysremIters + a.k] = (unsigned long long)a.iter;
    }
}

// x_ij = x_ij - c_i a_j of the finished component k.  Grid (ceil(n / 256), min(rows, 65535)).
__global__ void __launch_bounds__(kSysremLanes) tls_sysrem_subtract(const SysremArgs a) {
#pragma clang fp contract(off)
    const long long j = (long long)blockIdx.x * kSysremLanes + threadIdx.x;
    if (j >= a.n) return;
    const double v = a.a[(long long)a.k * a.n + j];
    for (long long i = blockIdx.y; i < a.rows; i += gridDim.y) {
        const double ci = a.c[(long long)a.k * a.rows + i];
        a.x[i * a.n + j] = a.x[i * a.n + j] - ci * v;
    }
}

// trend_ij = m_i (1 + sum_k C_ik A_kj) and flat_ij = y_ij / trend_ij.  Grid (ceil(n / 256), min(rows, 65535)).
__global__ void __launch_bounds__(kSysremLanes) tls_sysrem_apply(const SysremArgs a) {
#pragma clang fp contract(off)
    const long long j = (long long)blockIdx.x * kSysremLanes + threadIdx.x;
    if (j >= a.n) return;
    TLS_CHECK(a, a.n_components >= 1 && a.n_components <= TLS_SYSREM_MAX_COMPONENTS, kChkSysrem);
    double ak[TLS_SYSREM_MAX_COMPONENTS];
    for (int k = 0; k < TLS_SYSREM_MAX_COMPONENTS; ++k) ak[k] = k < a.n_components ? a.a[(long long)k * a.n + j] : 0.0;
    for (long long i = blockIdx.y; i < a.rows; i += gridDim.y) {
        double s = 0.0;
        for (int k = 0; k < TLS_SYSREM_MAX_COMPONENTS; ++k)
            if (k < a.n_components) s = s + a.c[(long long)k * a.rows + i] * ak[k];
        const double trend = a.m[i] * (1.0 + s);
        const long long o = i * a.n + j;
        a.flat[o] = a.y[o] / trend;
        if (a.trend) a.trend[o] = trend;
        // (a NaN fails both comparisons)
        if (!(trend > 0.0 && trend < __builtin_inf())) atomicMax(&a.state[kSysremBad], ~(unsigned long long)o);
    }
}
