// tls_inject.hip.h -- injection for survey-mode injection-recovery: out[k][i] = flux[k or 0][i] * model_k(t[i]).
//
// model_k is transit_model.light_curve(t, T0_k, P_k, rp_k, a_k, inc_k, ecc=0, w=90, u, law) restated operation by
// operation (numpy's order of every product and sum, no contraction): the circular branch of _true_anomaly plus
// projected_separation, then quadratic_ld_flux.  The per-injection constants (tp, period, rp, a, sin(radians(inc)),
// omega = radians(90)) come from the host, formed by numpy as those functions form them; the device does the per-point
// steps.  "linear" is u2 = 0, "uniform" u1 = u2 = 0.  Included by tls_kernels.hip.h (namespace tlsdev).

struct InjectArgs {
    const double* t;              // [n]
    const double* flux;           // [flux_rows][n]: flux_stride 0 (one shared base row) or n
    const double* consts;         // [n_inj][6]: tp, period, rp, a, sin_inc, omega (tls_injection)
    double u1, u2;
    double* out;                  // [n_inj][n]
    unsigned long long* count;    // [n_inj]: points with z < 1 + p, zeroed in front of the launch
    long long n, flux_stride;
};

constexpr double kInjTol = 1e-14;     // transit_model._TOL
constexpr double kInjBig = 1.0e10;    // transit_model._BIG
constexpr double kInjPi = 3.141592653589793;

// numpy.minimum / numpy.maximum against a constant: a NaN operand propagates
__device__ __forceinline__ double np_minimum(double a, double b) { return (a != a || a < b) ? a : b; }
__device__ __forceinline__ double np_maximum(double a, double b) { return (a != a || a > b) ? a : b; }

// Hastings K(k) and E(k) (transit_model.ellip_k / ellip_e)
__device__ __forceinline__ double inj_ellip_k(double k) {
#pragma clang fp contract(off)
    const double m1 = 1.0 - k * k;
    const double a = 1.38629436112 + m1 * (0.09666344259 + m1 * (0.03590092383 + m1 * (0.03742563713 + m1 * 0.01451196212)));
    const double b = 0.5 + m1 * (0.12498593597 + m1 * (0.06880248576 + m1 * (0.03328355346 + m1 * 0.00441787012)));
    return a - b * log(m1);
}
__device__ __forceinline__ double inj_ellip_e(double k) {
#pragma clang fp contract(off)
    const double m1 = 1.0 - k * k;
    const double a = 1.0 + m1 * (0.44325141463 + m1 * (0.06260601220 + m1 * (0.04757383546 + m1 * 0.01736506451)));
    const double b = m1 * (0.24998368310 + m1 * (0.09200180037 + m1 * (0.04069697526 + m1 * 0.00526449639)));
    return a + b * log(1.0 / m1);
}
// Bulirsch's Pi(n, k) for one element (transit_model.ellip_pi): stops on its own |1 - kc/g| <= 1e-8, at most 100 rounds
__device__ double inj_ellip_pi(double n, double k) {
#pragma clang fp contract(off)
    double kc = sqrt(1.0 - k * k);
    double p = sqrt(n + 1.0);
    double m0 = 1.0, c = 1.0, d = 1.0 / p, e = kc;
    for (int it = 0; it < 100; ++it) {
        const double f = c;
        c = d / p + c;
        double g = e / p;
        d = 2.0 * (f * g + d);
        p = g + p;
        g = m0;
        m0 = kc + m0;
        if (!(fabs(1.0 - kc / g) > 1.0e-8)) return 0.5 * kInjPi * (c * m0 + d) / (m0 * (m0 + p));
        kc = 2.0 * sqrt(e);
        e = kc * m0;
    }
    return NAN;   // (numpy leaves such an element of its numpy.empty output unset)
}

// quadratic_ld_flux at one separation z (>= 0): the four snaps, then the cases in the module's order; the first case
// that claims the point finishes it (todo); kap0, kap1 and lam_e come from the limb-crossing block, zero where it did
// not run.  The branches on p are uniform over a launch row (one injection).
__device__ double inj_quadratic_flux(double z, double p, double u1, double u2) {
#pragma clang fp contract(off)
    z = fabs(z);
    double flux = 1.0;
    const double omega = 1.0 - u1 / 3.0 - u2 / 6.0;
    const double c2 = u1 + 2.0 * u2;
    if (fabs(p - z) < kInjTol) z = p;
    if (fabs(p - 1.0 - z) < kInjTol) z = p - 1.0;
    if (fabs(1.0 - p - z) < kInjTol) z = 1.0 - p;
    if (z < kInjTol) z = 0.0;
    const double x1 = (p - z) * (p - z);
    const double x2 = (p + z) * (p + z);
    const double pp = p * p;
    const double x3 = pp - z * z;
    bool todo = z < 1.0 + p;
    double lam_e = 0.0, lam_d = 0.0, eta_d = 0.0, kap0 = 0.0, kap1 = 0.0;

    // star fully covered
    if (p >= 1.0 && todo && z <= p - 1.0) {
        flux = 1.0 - ((1.0 - c2) + c2 * (2.0 / 3.0) + u2 * 0.5) / omega;
        todo = false;
    }
    // disc crosses the stellar limb: the uniform-source term and the two angles
    if (todo && z >= fabs(1.0 - p) && z <= 1.0 + p) {
        kap1 = acos(np_minimum((1.0 - pp + z * z) / 2.0 / z, 1.0));
        kap0 = acos(np_minimum((pp + z * z - 1.0) / 2.0 / p / z, 1.0));
        const double le = pp * kap0 + kap1;
        const double r = 1.0 + z * z - pp;
        lam_e = (le - 0.5 * sqrt(np_maximum(4.0 * z * z - r * r, 0.0))) / kInjPi;
    }
    // planet edge on the stellar centre (z == p)
    if (todo && z == p) {
        if (p < 0.5) {
            const double q = 2.0 * p;
            lam_d = 1.0 / 3.0 + 2.0 / 9.0 / kInjPi * (4.0 * (2.0 * p * p - 1.0) * inj_ellip_e(q) + (1.0 - 4.0 * p * p) * inj_ellip_k(q));
            eta_d = pp / 2.0 * (pp + 2.0 * z * z);
            lam_e = pp;
        } else if (p > 0.5) {
            const double q = 0.5 / p;
            const double p4 = pow(p, 4.0);   // (Python's float power)
            lam_d = 1.0 / 3.0 + 16.0 * p / 9.0 / kInjPi * (2.0 * p * p - 1.0) * inj_ellip_e(q)
                    - (32.0 * p4 - 20.0 * p * p + 3.0) / 9.0 / kInjPi / p * inj_ellip_k(q);
            const double zsq = z * z;
            eta_d = 0.5 / kInjPi * (kap1 + pp * (pp + 2.0 * zsq) * kap0
                                    - (1.0 + 5.0 * p * p + zsq) / 4.0 * sqrt((1.0 - x1) * (x2 - 1.0)));
        } else {
            lam_d = 1.0 / 3.0 - 4.0 / kInjPi / 9.0;
            eta_d = 3.0 / 32.0;
        }
        flux = 1.0 - ((1.0 - c2) * lam_e + c2 * lam_d + u2 * eta_d) / omega;
        todo = false;
    }
    // ingress / egress: partial overlap, limb crossed
    if (todo && (((z > 0.5 + fabs(p - 0.5)) && (z < 1.0 + p)) || ((p > 0.5) && (z > fabs(1.0 - p) * 1.0001) && (z < p)))) {
        const double q = sqrt((1.0 - x1) / (x2 - x1));
        const double Kk = inj_ellip_k(q), Ek = inj_ellip_e(q);
        const double Pk = inj_ellip_pi(1.0 / x1 - 1.0, q);
        lam_d = 1.0 / 9.0 / kInjPi / sqrt(p * z) * (
            ((1.0 - x2) * (2.0 * x2 + x1 - 3.0) - 3.0 * x3 * (x2 - 2.0)) * Kk
            + 4.0 * p * z * (z * z + 7.0 * p * p - 4.0) * Ek
            - 3.0 * x3 / x1 * Pk);
        eta_d = 1.0 / 2.0 / kInjPi * (kap1 + pp * (pp + 2.0 * z * z) * kap0
                                      - (1.0 + 5.0 * p * p + z * z) / 4.0 * sqrt((1.0 - x1) * (x2 - 1.0)));
        const double ld = lam_d + (p > z ? 2.0 / 3.0 : 0.0);
        flux = 1.0 - ((1.0 - c2) * lam_e + c2 * ld + u2 * eta_d) / omega;
        todo = false;
    }
    // planet disc entirely inside the stellar disc
    if (p <= 1.0 && todo && z <= 1.0 - p) {
        eta_d = pp / 2.0 * (pp + 2.0 * z * z);
        double ld;
        if (z == 0.0) {
            ld = -2.0 / 3.0 * pow(1.0 - pp, 1.5);   // (Python's float power)
        } else if (fabs(p + z - 1.0) <= kInjTol) {   // second contact exactly
            ld = 2.0 / 3.0 / kInjPi * acos(1.0 - 2.0 * p)
                 - 4.0 / 9.0 / kInjPi * sqrt(p * (1.0 - p)) * (3.0 + 2.0 * p - 8.0 * p * p);
        } else {
            const double q = sqrt((x2 - x1) / (1.0 - x1));
            const double Kk = inj_ellip_k(q), Ek = inj_ellip_e(q);
            const double Pk = inj_ellip_pi(x2 / x1 - 1.0, q);
            ld = 2.0 / 9.0 / kInjPi / sqrt(1.0 - x1) * (
                (1.0 - 5.0 * z * z + pp + x3 * x3) * Kk
                + (1.0 - x1) * (z * z + 7.0 * p * p - 4.0) * Ek
                - 3.0 * x3 / x1 * Pk);
        }
        const double add = p > z ? 2.0 / 3.0 : 0.0;
        flux = 1.0 - ((1.0 - c2) * p * p + c2 * (ld + add) + u2 * eta_d) / omega;
        todo = false;
    }
    return flux;
}

// Grid (ceil(n / 256), n_inj), one point per thread.  A point out of contact (z >= 1 + p) has model 1 and keeps its base
// flux bit for bit; a wave with no point in contact takes that exit as a whole (time-ordered data keeps the contact points
// together).  n_in_transit: one ballot popcount and one atomic per wave.
__global__ void __launch_bounds__(256) tls_inject_transits(const InjectArgs a) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long k = blockIdx.y;
    const double* c = a.consts + 6 * k;
    const double tp = c[0], per = c[1], p = c[2], ar = c[3], sin_inc = c[4], omega = c[5];
    const bool live = i < a.n;
    double z = kInjBig, base = 0.0;
    if (live) {
        base = a.flux[k * a.flux_stride + i];
        const double x = (a.t[i] - tp) / per;                  // _true_anomaly, ecc < 1e-5
        const double f = (x - trunc(x)) * 2.0 * kInjPi;
        const double s = sin(f + omega) * sin_inc;             // projected_separation
        z = s <= 0.0 ? kInjBig : ar * sqrt(np_maximum(1.0 - s * s, 0.0));
    }
    // contact as quadratic_ld_flux decides it: its `todo`, after the four snaps (z >= 0 here)
    double zs = z;
    if (fabs(p - zs) < kInjTol) zs = p;
    if (fabs(p - 1.0 - zs) < kInjTol) zs = p - 1.0;
    if (fabs(1.0 - p - zs) < kInjTol) zs = 1.0 - p;
    if (zs < kInjTol) zs = 0.0;
    const bool contact = live && zs < 1.0 + p;
    const unsigned long long mask = __ballot(contact);
    if ((threadIdx.x & (kWave - 1)) == 0 && mask != 0ull) atomicAdd(a.count + k, (unsigned long long)__popcll(mask));
    double* out = a.out + k * a.n;
    if (mask == 0ull) {   // wave-uniform: nothing of this wave is in contact
        if (live) out[i] = base;
        return;
    }
    if (live) out[i] = contact ? base * inj_quadratic_flux(z, p, a.u1, a.u2) : base;
}
