// Developer micro-benchmark: one step of the four-slot kernel's sliding dot product (phase 3b, XTH = 1: 8 ds_read_b64, 40 fp64 FMAs
// into 5 accumulators) with the template taps
//   (a) in SGPRs, loaded by s_load, one s_waitcnt lgkmcnt(0) behind taps and samples -- the shipped dot_windows<true, 1>;
//   (b) broadcast from lanes: lane l holds tap base + (l & 15) in ONE VGPR pair (a global_load_dwordx2 per step), every FMA
//       names its tap as v_fmac_f64_dpp ... row_newbcast:k; waits as in (a): vmcnt(0) lgkmcnt(0), then the 40 FMAs;
//   (c) form (b) with counted waits: lgkmcnt(7 - u) in front of the 5 FMAs of sample u;
//   (d) form (c) with the pair of step t + 2 requested before the reads of step t (three rotating pairs, vmcnt(2));
//   (e) the pair two steps ahead as in (d), ONE lgkmcnt(0) as in (b);  (f) the same, the samples waited for in two halves;
//   (g) form (d) with the pair ONE step ahead.
// Cycles per step and wave, on one CU and on all CUs, at 1, 2 and 4 waves per SIMD (one workgroup of 256 / 512 / 1024 threads
// per CU, held alone there by its LDS allocation), on random live units as pk_dot.hip; and the bare issue rate of 40 FMAs in the
// two operand forms with no memory operation at all.  The results of (b) .. (g) are compared with (a) bit by bit.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o /tmp/dpp_tap_fma tools/micro/dpp_tap_fma.hip && /tmp/dpp_tap_fma
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include <cmath>
#include <cstdlib>
typedef const __attribute__((address_space(4))) double* const_f64_ptr;
constexpr int kR = 5, kU = 8, kM = 4864, kS = kR - 1, kTapRow = 64;   // the template row starts kTapRow entries into the table

__device__ __forceinline__ void load8(unsigned addr, double (&x)[8]) {
    asm volatile("ds_read_b64 %0, %8\n\tds_read_b64 %1, %8 offset:8\n\tds_read_b64 %2, %8 offset:16\n\tds_read_b64 %3, %8 offset:24\n\t"
                 "ds_read_b64 %4, %8 offset:32\n\tds_read_b64 %5, %8 offset:40\n\tds_read_b64 %6, %8 offset:48\n\tds_read_b64 %7, %8 offset:56\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]), "=&v"(x[4]), "=&v"(x[5]), "=&v"(x[6]), "=&v"(x[7]) : "v"(addr) : "memory");
}
// (a): the shipped step
__device__ __forceinline__ void dot_sgpr(unsigned e_addr, const_f64_ptr q, int nsteps, double (&B)[kR]) {
    for (int t0 = 0; t0 < nsteps * kU; t0 += kU) {
        const const_f64_ptr qs = q + (t0 - kS);
        double taps[kU + kS];
#pragma unroll
        for (int m = 0; m < kU + kS; ++m) taps[m] = qs[m];
        double x[kU];
        load8(e_addr + 8u * (unsigned)t0, x);
#pragma unroll
        for (int u = 0; u < kU; ++u)
#pragma unroll
            for (int r = 0; r < kR; ++r) B[r] = fma(taps[u + kS - r], x[u], B[r]);
    }
}

// (b), (c), (d): three steps per trip of ONE asm loop (the pairs are written by loads the compiler does not see in flight).
// Window r takes tap u + kS - r of the pair's 16: the broadcast index.  EXEC is all ones here.
#define FD(B, T, X, K) "v_fmac_f64_dpp " B ", " T ", " X " row_newbcast:" #K " row_mask:0xf bank_mask:0xf\n\t"
#define SAMP(T, X, k0, k1, k2, k3, k4) FD("%[b0]", T, X, k0) FD("%[b1]", T, X, k1) FD("%[b2]", T, X, k2) FD("%[b3]", T, X, k3) FD("%[b4]", T, X, k4)
#define WAIT(N) "s_waitcnt lgkmcnt(" #N ")\n\t"
#define FMAS_FLAT(T) SAMP(T, "%[x0]", 4, 3, 2, 1, 0) SAMP(T, "%[x1]", 5, 4, 3, 2, 1) SAMP(T, "%[x2]", 6, 5, 4, 3, 2) SAMP(T, "%[x3]", 7, 6, 5, 4, 3) \
                     SAMP(T, "%[x4]", 8, 7, 6, 5, 4) SAMP(T, "%[x5]", 9, 8, 7, 6, 5) SAMP(T, "%[x6]", 10, 9, 8, 7, 6) SAMP(T, "%[x7]", 11, 10, 9, 8, 7)
#define FMAS_COUNTED(T) WAIT(7) SAMP(T, "%[x0]", 4, 3, 2, 1, 0) WAIT(6) SAMP(T, "%[x1]", 5, 4, 3, 2, 1) WAIT(5) SAMP(T, "%[x2]", 6, 5, 4, 3, 2) \
                        WAIT(4) SAMP(T, "%[x3]", 7, 6, 5, 4, 3) WAIT(3) SAMP(T, "%[x4]", 8, 7, 6, 5, 4) WAIT(2) SAMP(T, "%[x5]", 9, 8, 7, 6, 5) \
                        WAIT(1) SAMP(T, "%[x6]", 10, 9, 8, 7, 6) WAIT(0) SAMP(T, "%[x7]", 11, 10, 9, 8, 7)
#define FMAS_HALVES(T) WAIT(4) SAMP(T, "%[x0]", 4, 3, 2, 1, 0) SAMP(T, "%[x1]", 5, 4, 3, 2, 1) SAMP(T, "%[x2]", 6, 5, 4, 3, 2) SAMP(T, "%[x3]", 7, 6, 5, 4, 3) \
                       WAIT(0) SAMP(T, "%[x4]", 8, 7, 6, 5, 4) SAMP(T, "%[x5]", 9, 8, 7, 6, 5) SAMP(T, "%[x6]", 10, 9, 8, 7, 6) SAMP(T, "%[x7]", 11, 10, 9, 8, 7)
#define RD(o0, o1, o2, o3, o4, o5, o6, o7) \
    "ds_read_b64 %[x0], %[ea] offset:" #o0 "\n\tds_read_b64 %[x1], %[ea] offset:" #o1 "\n\tds_read_b64 %[x2], %[ea] offset:" #o2 "\n\t" \
    "ds_read_b64 %[x3], %[ea] offset:" #o3 "\n\tds_read_b64 %[x4], %[ea] offset:" #o4 "\n\tds_read_b64 %[x5], %[ea] offset:" #o5 "\n\t" \
    "ds_read_b64 %[x6], %[ea] offset:" #o6 "\n\tds_read_b64 %[x7], %[ea] offset:" #o7 "\n\t"
#define RD0 RD(0, 8, 16, 24, 32, 40, 48, 56)
#define RD1 RD(64, 72, 80, 88, 96, 104, 112, 120)
#define RD2 RD(128, 136, 144, 152, 160, 168, 176, 184)
#define LD(T, OFF) "global_load_dwordx2 " T ", %[toff], %[q] offset:" #OFF "\n\t"
// (no scalar load and no store of the surrounding code may be in flight under the counted waits; the s_nop is the distance
// between whatever wrote EXEC last and the first DPP read)
#define HEAD "s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 4\n\t"
#define TAIL(L) "v_add_u32 %[ea], 192, %[ea]\n\tv_add_u32 %[toff], 192, %[toff]\n\ts_sub_u32 %[n], %[n], 1\n\ts_cmp_lg_u32 %[n], 0\n\t" \
                "s_cbranch_scc1 " L "\n\ts_waitcnt vmcnt(0)"
#define OPERANDS \
    : [b0] "+v"(B[0]), [b1] "+v"(B[1]), [b2] "+v"(B[2]), [b3] "+v"(B[3]), [b4] "+v"(B[4]), \
      [x0] "=&v"(x0), [x1] "=&v"(x1), [x2] "=&v"(x2), [x3] "=&v"(x3), [x4] "=&v"(x4), [x5] "=&v"(x5), [x6] "=&v"(x6), [x7] "=&v"(x7), \
      [t0] "=&v"(T0), [t1] "=&v"(T1), [t2] "=&v"(T2), [ea] "+v"(e_addr), [toff] "+v"(tap_off), [n] "+s"(n) \
    : [q] "s"(q) : "memory", "scc"
template <int MODE>
__device__ __forceinline__ void dot_dpp(unsigned e_addr, const double* q, unsigned tap_off, int nsteps, double (&B)[kR]) {
    double x0, x1, x2, x3, x4, x5, x6, x7, T0, T1, T2;
    int n = nsteps / 3;
    if constexpr (MODE == 1) {
        asm volatile(HEAD ".Lb%=:\n\t"
                     LD("%[t0]", 0) RD0 "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" FMAS_FLAT("%[t0]")
                     LD("%[t1]", 64) RD1 "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" FMAS_FLAT("%[t1]")
                     LD("%[t2]", 128) RD2 "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" FMAS_FLAT("%[t2]")
                     TAIL(".Lb%=") OPERANDS);
    } else if constexpr (MODE == 2) {
        asm volatile(HEAD ".Lc%=:\n\t"
                     LD("%[t0]", 0) RD0 "s_waitcnt vmcnt(0)\n\t" FMAS_COUNTED("%[t0]")
                     LD("%[t1]", 64) RD1 "s_waitcnt vmcnt(0)\n\t" FMAS_COUNTED("%[t1]")
                     LD("%[t2]", 128) RD2 "s_waitcnt vmcnt(0)\n\t" FMAS_COUNTED("%[t2]")
                     TAIL(".Lc%=") OPERANDS);
    } else if constexpr (MODE == 3) {
        asm volatile(HEAD LD("%[t0]", 0) LD("%[t1]", 64) ".Ld%=:\n\t"
                     LD("%[t2]", 128) RD0 "s_waitcnt vmcnt(2)\n\t" FMAS_COUNTED("%[t0]")
                     LD("%[t0]", 192) RD1 "s_waitcnt vmcnt(2)\n\t" FMAS_COUNTED("%[t1]")
                     LD("%[t1]", 256) RD2 "s_waitcnt vmcnt(2)\n\t" FMAS_COUNTED("%[t2]")
                     TAIL(".Ld%=") OPERANDS);
    } else if constexpr (MODE == 4) {   // (e): the pair two steps ahead, ONE wait for the eight samples
        asm volatile(HEAD LD("%[t0]", 0) LD("%[t1]", 64) ".Le%=:\n\t"
                     LD("%[t2]", 128) RD0 "s_waitcnt vmcnt(2) lgkmcnt(0)\n\t" FMAS_FLAT("%[t0]")
                     LD("%[t0]", 192) RD1 "s_waitcnt vmcnt(2) lgkmcnt(0)\n\t" FMAS_FLAT("%[t1]")
                     LD("%[t1]", 256) RD2 "s_waitcnt vmcnt(2) lgkmcnt(0)\n\t" FMAS_FLAT("%[t2]")
                     TAIL(".Le%=") OPERANDS);
    } else if constexpr (MODE == 5) {   // (f): the pair two steps ahead, the samples waited for in two halves
        asm volatile(HEAD LD("%[t0]", 0) LD("%[t1]", 64) ".Lf%=:\n\t"
                     LD("%[t2]", 128) RD0 "s_waitcnt vmcnt(2)\n\t" FMAS_HALVES("%[t0]")
                     LD("%[t0]", 192) RD1 "s_waitcnt vmcnt(2)\n\t" FMAS_HALVES("%[t1]")
                     LD("%[t1]", 256) RD2 "s_waitcnt vmcnt(2)\n\t" FMAS_HALVES("%[t2]")
                     TAIL(".Lf%=") OPERANDS);
    } else {   // (g): form (d) with the pair ONE step ahead
        asm volatile(HEAD LD("%[t0]", 0) ".Lg%=:\n\t"
                     LD("%[t1]", 64) RD0 "s_waitcnt vmcnt(1)\n\t" FMAS_COUNTED("%[t0]")
                     LD("%[t2]", 128) RD1 "s_waitcnt vmcnt(1)\n\t" FMAS_COUNTED("%[t1]")
                     LD("%[t0]", 192) RD2 "s_waitcnt vmcnt(1)\n\t" FMAS_COUNTED("%[t2]")
                     TAIL(".Lg%=") OPERANDS);
    }
}

__device__ __forceinline__ unsigned hash(unsigned x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
template <int MODE>
__global__ __launch_bounds__(1024) void bench(const double* q, const double* e, double* out, unsigned long long* cycles, int nsteps, int iters, int n_units) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    double* ed = reinterpret_cast<double*>(sm);
    for (int i = threadIdx.x; i < kM; i += blockDim.x) ed[i] = e[i];
    __syncthreads();
    const unsigned base = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)sm;
    const unsigned wave = threadIdx.x / 64, lane = threadIdx.x & 63;
    double total[kR] = {0, 0, 0, 0, 0};
    const unsigned long long c0 = __builtin_readcyclecounter();
    for (int it = 0; it < iters; ++it) {
        // a batch: 64 live units of one row in ascending order with random gaps (~14 % live)
        unsigned u = (hash(it * 977u + wave * 131u + blockIdx.x) % 200u) + lane * 7u + (hash(it * 64u + lane + wave * 7919u) % 7u);
        u %= (unsigned)n_units;
        const unsigned addr = base + 8u * (u * kR);
        double B[kR] = {0, 0, 0, 0, 0};
        if constexpr (MODE == 0) dot_sgpr(addr, (const_f64_ptr)q + kTapRow, nsteps, B);
        else dot_dpp<MODE>(addr, q, 8u * (unsigned)(kTapRow - kS + (int)(lane & 15u)), nsteps, B);
#pragma unroll
        for (int r = 0; r < kR; ++r) total[r] += B[r];
    }
    __syncthreads();
    const unsigned long long c1 = __builtin_readcyclecounter();
    if (threadIdx.x == 0) cycles[blockIdx.x] = c1 - c0;
    double s = 0; for (int r = 0; r < kR; ++r) s += total[r] * (r + 1);
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// the bare issue rate: 40 FMAs a trip into 5 accumulators, 12 taps, nothing else
#define FS(B, T, X) "v_fmac_f64 " B ", " T ", " X "\n\t"
template <bool DPP>
__global__ __launch_bounds__(1024) void issue(const double* q, double* out, unsigned long long* cycles, int trips) {
    const_f64_ptr qs = (const_f64_ptr)q + kTapRow;
    double B[kR] = {0, 0, 0, 0, 0}, x = 1.0 + 1e-9 * threadIdx.x, T = q[kTapRow + (threadIdx.x & 15)];
    double s0 = qs[0], s1 = qs[1], s2 = qs[2], s3 = qs[3], s4 = qs[4], s5 = qs[5], s6 = qs[6], s7 = qs[7], s8 = qs[8], s9 = qs[9], s10 = qs[10], s11 = qs[11];
    int n = trips;
    __syncthreads();
    const unsigned long long c0 = __builtin_readcyclecounter();
    if constexpr (DPP) {
        asm volatile("s_nop 4\n.Li%=:\n\t"
                     SAMP("%[t]", "%[x]", 4, 3, 2, 1, 0) SAMP("%[t]", "%[x]", 5, 4, 3, 2, 1) SAMP("%[t]", "%[x]", 6, 5, 4, 3, 2) SAMP("%[t]", "%[x]", 7, 6, 5, 4, 3)
                     SAMP("%[t]", "%[x]", 8, 7, 6, 5, 4) SAMP("%[t]", "%[x]", 9, 8, 7, 6, 5) SAMP("%[t]", "%[x]", 10, 9, 8, 7, 6) SAMP("%[t]", "%[x]", 11, 10, 9, 8, 7)
                     "s_sub_u32 %[n], %[n], 1\n\ts_cmp_lg_u32 %[n], 0\n\ts_cbranch_scc1 .Li%="
                     : [b0] "+v"(B[0]), [b1] "+v"(B[1]), [b2] "+v"(B[2]), [b3] "+v"(B[3]), [b4] "+v"(B[4]), [n] "+s"(n)
                     : [t] "v"(T), [x] "v"(x) : "scc");
    } else {
#define SS(k0, k1, k2, k3, k4) FS("%[b0]", "%[s" #k0 "]", "%[x]") FS("%[b1]", "%[s" #k1 "]", "%[x]") FS("%[b2]", "%[s" #k2 "]", "%[x]") FS("%[b3]", "%[s" #k3 "]", "%[x]") FS("%[b4]", "%[s" #k4 "]", "%[x]")
        asm volatile(".Lj%=:\n\t"
                     SS(4, 3, 2, 1, 0) SS(5, 4, 3, 2, 1) SS(6, 5, 4, 3, 2) SS(7, 6, 5, 4, 3) SS(8, 7, 6, 5, 4) SS(9, 8, 7, 6, 5) SS(10, 9, 8, 7, 6) SS(11, 10, 9, 8, 7)
                     "s_sub_u32 %[n], %[n], 1\n\ts_cmp_lg_u32 %[n], 0\n\ts_cbranch_scc1 .Lj%="
                     : [b0] "+v"(B[0]), [b1] "+v"(B[1]), [b2] "+v"(B[2]), [b3] "+v"(B[3]), [b4] "+v"(B[4]), [n] "+s"(n)
                     : [s0] "s"(s0), [s1] "s"(s1), [s2] "s"(s2), [s3] "s"(s3), [s4] "s"(s4), [s5] "s"(s5), [s6] "s"(s6), [s7] "s"(s7), [s8] "s"(s8),
                       [s9] "s"(s9), [s10] "s"(s10), [s11] "s"(s11), [x] "v"(x) : "scc");
    }
    __syncthreads();
    const unsigned long long c1 = __builtin_readcyclecounter();
    if (threadIdx.x == 0) cycles[blockIdx.x] = c1 - c0;
    out[blockIdx.x * blockDim.x + threadIdx.x] = B[0] + 2 * B[1] + 3 * B[2] + 4 * B[3] + 5 * B[4];
}

#define CHECK(x) do { hipError_t err_ = (x); if (err_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(err_)); return 1; } } while (0)
constexpr int kMaxBlocks = 256, kTable = 2048, kModes = 7;
static double *d_q, *d_e, *d_out;
static unsigned long long* d_cyc;
static const size_t kLds = 96 * 1024;   // more than half a CU's: one workgroup per CU

template <int MODE>
int run(int blocks, int threads, int nsteps, int iters, int n_units, std::vector<double>& o, double& cyc_per_step, float& ms) {
    CHECK(hipFuncSetAttribute((const void*)bench<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
    hipEvent_t a, b; CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
    bench<MODE><<<blocks, threads, kLds>>>(d_q, d_e, d_out, d_cyc, nsteps, iters / 4, n_units);   // warm-up
    CHECK(hipEventRecord(a));
    bench<MODE><<<blocks, threads, kLds>>>(d_q, d_e, d_out, d_cyc, nsteps, iters, n_units);
    CHECK(hipEventRecord(b)); CHECK(hipEventSynchronize(b)); CHECK(hipEventElapsedTime(&ms, a, b));
    CHECK(hipGetLastError());
    o.resize((size_t)blocks * threads);
    CHECK(hipMemcpy(o.data(), d_out, o.size() * 8, hipMemcpyDeviceToHost));
    std::vector<unsigned long long> c(blocks);
    CHECK(hipMemcpy(c.data(), d_cyc, blocks * 8, hipMemcpyDeviceToHost));
    double mean = 0; for (auto v : c) mean += (double)v; mean /= blocks;
    cyc_per_step = mean / ((double)iters * nsteps);
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    return 0;
}
template <bool DPP>
int run_issue(int blocks, int threads, int trips, double& cyc_per_trip) {
    issue<DPP><<<blocks, threads>>>(d_q, d_out, d_cyc, trips / 4);
    issue<DPP><<<blocks, threads>>>(d_q, d_out, d_cyc, trips);
    CHECK(hipDeviceSynchronize());
    std::vector<unsigned long long> c(blocks);
    CHECK(hipMemcpy(c.data(), d_cyc, blocks * 8, hipMemcpyDeviceToHost));
    double mean = 0; for (auto v : c) mean += (double)v; mean /= blocks;
    cyc_per_trip = mean / trips;
    return 0;
}

int main() {
    const int iters = 2000, n_units = (kM - 512) / kR;
    std::vector<double> q(kTable, 0.0), e(kM);
    for (int j = 0; j < 400; ++j) q[kTapRow + j] = 0.5 + 0.5 * std::sin(3.14159 * (j + 0.5) / 400);
    srand(1); for (auto& v : e) v = 1e-4 * ((rand() % 2001) - 1000) / 1000.0;
    CHECK(hipMalloc(&d_q, kTable * 8)); CHECK(hipMalloc(&d_e, kM * 8)); CHECK(hipMalloc(&d_out, (size_t)kMaxBlocks * 1024 * 8)); CHECK(hipMalloc(&d_cyc, kMaxBlocks * 8));
    CHECK(hipMemcpy(d_q, q.data(), kTable * 8, hipMemcpyHostToDevice)); CHECK(hipMemcpy(d_e, e.data(), kM * 8, hipMemcpyHostToDevice));
    for (int blocks : {1, kMaxBlocks})
        for (int wps : {1, 2, 4}) {
            double cs, cd;
            if (run_issue<false>(blocks, 256 * wps, 20000, cs) || run_issue<true>(blocks, 256 * wps, 20000, cd)) return 1;
            printf("issue only      CUs %3d  waves/SIMD %d   40 FMAs: SGPR taps %7.1f cycles, DPP taps %7.1f cycles (x%.3f)\n", blocks, wps, cs, cd, cd / cs);
        }
    for (int nsteps : {6, 24})
        for (int blocks : {1, kMaxBlocks})
            for (int wps : {1, 2, 4}) {
                typedef int (*run_fn)(int, int, int, int, int, std::vector<double>&, double&, float&);
                const run_fn runs[kModes] = {run<0>, run<1>, run<2>, run<3>, run<4>, run<5>, run<6>};
                std::vector<double> o[kModes];
                double c[kModes]; float ms[kModes];
                bool same = true;
                for (int m = 0; m < kModes; ++m) {
                    if (runs[m](blocks, 256 * wps, nsteps, iters, n_units, o[m], c[m], ms[m])) return 1;
                    same = same && !memcmp(o[0].data(), o[m].data(), o[0].size() * 8);
                }
                printf("steps/batch %2d  CUs %3d  waves/SIMD %d   cycles per step and wave:", nsteps, blocks, wps);
                for (int m = 0; m < kModes; ++m) printf("  (%c) %6.1f", 'a' + m, c[m]);
                printf("   ms:");
                for (int m = 0; m < kModes; ++m) printf(" %.3f", ms[m]);
                printf("   bits %s\n", same ? "equal" : "DIFFER");
            }
    return 0;
}
