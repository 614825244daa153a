// tls_null.hip.h -- null (noise-only) light curves for survey-mode SDE false-alarm calibration (tls_null_rows).
//
// Random stream: Philox4x64-10 (Salmon et al. 2011, the Random123 constants) with key (seed, 0), word j of the stream
// being word j % 4 of the block at counter (j / 4 + 1, 0, 0, 0) -- numpy.random.Philox(key=seed).random_raw()'s order, which
// increments its counter in front of every block.  Trial R owns words [R W, R W + words), W = words rounded up to a multiple
// of 4, so its row depends on (seed, R) alone: numpy.random.Philox(key=seed, counter=R W / 4).random_raw(W) are its words.
//   mode 0 (white noise, words = 2n): u_a, u_b from words 2i, 2i + 1 as numpy's Generator.random() forms them,
//          z = sqrt(-2 log(1 - u_a)) cos(2 pi u_b), out = 1 + sigma z.
//   mode 1 (block bootstrap, words = ceil(n / L)): block b of trial R copies L points (fewer in a last, short block) of
//          source row R mod n_src from start_b = high word of w[b] (n - L + 1): integer arithmetic and copies only.
// The host checks that no counter of a launch passes 2^64 - 1, so counter words 1..3 stay 0.  Included by tls_kernels.hip.h
// (namespace tlsdev).

struct NullArgs {
    double* out;                  // [rows][n]
    const double* sigma;          // mode 0: [rows] (sigma_stride 1) or [1] (sigma_stride 0), this launch's first row first
    const double* src;            // mode 1: [n_src][n]
    unsigned long long seed;
    long long first_trial;        // global trial index of this launch's row 0
    long long blocks;             // Philox blocks per trial, W / 4
    long long sigma_stride, n_src;
    unsigned int n, L;            // points per row (<= 1e8); mode 1: points per bootstrap block
};

constexpr unsigned long long kPhiloxM0 = 0xD2E7470EE14C6C93ull;
constexpr unsigned long long kPhiloxM1 = 0xCA5A826395121157ull;
constexpr unsigned long long kPhiloxW0 = 0x9E3779B97F4A7C15ull;
constexpr unsigned long long kPhiloxW1 = 0xBB67AE8584CAA73Bull;

// Philox4x64-10 of counter (c0, 0, 0, 0) under key (k0, 0): ten rounds, the key bumped between rounds
__device__ __forceinline__ void philox4x64_10(unsigned long long c0, unsigned long long k0, unsigned long long w[4]) {
    unsigned long long c[4] = {c0, 0ull, 0ull, 0ull};
    unsigned long long k1 = 0ull;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        if (round) { k0 += kPhiloxW0; k1 += kPhiloxW1; }
        const unsigned long long hi0 = __umul64hi(kPhiloxM0, c[0]), lo0 = kPhiloxM0 * c[0];
        const unsigned long long hi1 = __umul64hi(kPhiloxM1, c[2]), lo1 = kPhiloxM1 * c[2];
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
    }
    w[0] = c[0]; w[1] = c[1]; w[2] = c[2]; w[3] = c[3];
}

// counter of Philox block j of launch row r
__device__ __forceinline__ unsigned long long null_counter(const NullArgs& a, long long r, long long j) {
    return (unsigned long long)(a.first_trial + r) * (unsigned long long)a.blocks + (unsigned long long)j + 1ull;
}

// numpy Generator.random(): the top 53 bits of a word times 2^-53
__device__ __forceinline__ double null_uniform(unsigned long long w) { return (double)(w >> 11) * 0x1.0p-53; }

__device__ __forceinline__ double null_normal(unsigned long long wa, unsigned long long wb) {
#pragma clang fp contract(off)
    const double ua = null_uniform(wa), ub = null_uniform(wb);
    return sqrt(-2.0 * log(1.0 - ua)) * cos(6.283185307179586 * ub);   // (1 - ua is exact and > 0)
}

// Mode 0.  Grid (ceil(W / 4 / 256), rows): one Philox block per thread, points 2j and 2j + 1 (the second one past the
// row's end for odd n is dropped, its words unused).
__global__ void __launch_bounds__(256) tls_null_white(const NullArgs a) {
#pragma clang fp contract(off)
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = blockIdx.y;
    if (j >= a.blocks) return;
    unsigned long long w[4];
    philox4x64_10(null_counter(a, r, j), a.seed, w);
    const double sigma = a.sigma[r * a.sigma_stride];
    double* out = a.out + r * (long long)a.n;
    const unsigned int i = 2u * (unsigned int)j;
    out[i] = 1.0 + sigma * null_normal(w[0], w[1]);
    if (i + 1u < a.n) out[i + 1u] = 1.0 + sigma * null_normal(w[2], w[3]);
}

// Mode 1.  Grid (ceil(n / 256), rows), one point per thread; the thread forms the Philox block that holds its bootstrap
// block's word (blocks of up to four bootstrap blocks, the words shared by at most 4 L neighbouring points).
__global__ void __launch_bounds__(256) tls_null_bootstrap(const NullArgs a) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = blockIdx.y;
    if (i >= a.n) return;
    const unsigned int b = i / a.L;
    unsigned long long w[4];
    philox4x64_10(null_counter(a, r, b >> 2), a.seed, w);
    const unsigned int q = b & 3u;
    const unsigned long long word = q == 0u ? w[0] : q == 1u ? w[1] : q == 2u ? w[2] : w[3];
    // start_b = floor(word (n - L + 1) / 2^64) <= n - L, so start_b + (i - b L) <= n - 1
    const unsigned long long start = __umul64hi(word, (unsigned long long)(a.n - a.L + 1u));
    const long long s = (a.first_trial + r) % a.n_src;
    a.out[r * (long long)a.n + i] = a.src[s * (long long)a.n + (long long)start + (long long)(i - b * a.L)];
}

// tls_debug_null_words: every trial's W words as the two kernels above take them.  Grid (ceil(W / 4 / 256), rows).
__global__ void __launch_bounds__(256) tls_null_words(const NullArgs a, unsigned long long* out) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = blockIdx.y;
    if (j >= a.blocks) return;
    unsigned long long w[4];
    philox4x64_10(null_counter(a, r, j), a.seed, w);
    unsigned long long* o = out + (r * a.blocks + j) * 4;
    o[0] = w[0]; o[1] = w[1]; o[2] = w[2]; o[3] = w[3];
}
