// tls_protect.hip.h -- transit-protected detrending for survey mode: the in-transit flags of a batch (tls_transit_mask).  The
// masked detrenders that read them live with their unmasked forms: tls_biweight.hip.h (tls_biweight_detrend_masked) and
// tls_gls.hip.h / tls_prewhiten.hip.h (tls_prewhiten_masked).  DESIGN.md "Transit-protected detrending";
// tests/transit_protect_spec.py is the statement in numpy.
//
// Point i of curve c is protected if any candidate k of curve c has, one IEEE double operation a step and no contraction,
//     d = t[i] - T0_k;  e = floor(d / P_k + 0.5);  r = d - e * P_k;  fabs(r) <= 0.5 * (factor * duration_k).
// The host leaves out the candidates that take no part (a period, T0 or duration that is not finite, a period or duration
// <= 0) and groups the others by curve with a stable sort: candidate list [offset[c], offset[c + 1]) belongs to curve c.  One
// thread owns one (curve, point) and walks its curve's list; the lanes of a wave read the same candidate (a broadcast) and
// neighbouring time stamps, and write neighbouring bytes.
// Included by tls_kernels.hip.h (namespace tlsdev).

constexpr int kProtectThreads = 256;

struct TransitMaskArgs {
    const double* t;                                 // [n]
    const double* period;                            // [m] grouped by curve
    const double* T0;                                // [m]
    const double* duration;                          // [m] days
    const long long* offset;                         // [curves + 1] of this launch's curves, into the three arrays above
    unsigned char* mask;                             // [curves][n] 1 = protected
    long long n, count;                              // count = curves * n
    double factor;
};

__global__ void __launch_bounds__(kProtectThreads) tls_transit_mask_kernel(const TransitMaskArgs a) {
#pragma clang fp contract(off)
    for (long long e = (long long)blockIdx.x * kProtectThreads + threadIdx.x; e < a.count; e += (long long)gridDim.x * kProtectThreads) {
        const long long c = e / a.n;
        const double ti = a.t[e - c * a.n];
        unsigned char prot = 0;
        for (long long k = a.offset[c]; k < a.offset[c + 1]; ++k) {
            const double P = a.period[k];
            const double d = ti - a.T0[k];
            const double x = d / P;
            const double ep = floor(x + 0.5);
            const double back = ep * P;
            const double r = d - back;
            const double width = a.factor * a.duration[k];
            const double hw = 0.5 * width;
            if (__builtin_fabs(r) <= hw) { prot = 1; break; }
        }
        a.mask[e] = prot;
    }
}
