// tls_centroid.hip.h -- the centroid-shift test of a candidate (tls_centroid_test): which star dims.
//
// The statement (tests/centroid_spec.py is the same in Python; include/tls_amd.h, DESIGN.md "Centroid test"), for a candidate
// (P, T0, d in days) on a curve's flux y and flux-weighted centroids cx, cy, and the shape b[L] (0 out of transit, 1 at the
// bottom):
//   status 1 unless P, T0, d finite, P > 0, d > 0 and wd = window * d < 0.5 * P
//   points, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P
//       member iff fabs(tau) <= wd and cx[i], cy[i] finite;  its epoch is k
//       v = tau / d + 0.5;  inside iff 0 <= v <= 1;  s = 0.0 outside, else the shape interpolated at u = v * (L - 1)
//   status 2 if the epochs holding a member are more than max_epochs
//   an epoch, its members in index order:  pass 1 the means of s and of the channels (1 - y, cx, cy);  pass 2 the sums
//       De = sum ds ds,  Ne[c] = sum ds dc,  Qe[c] = sum dc dc of the residuals;  used iff m_in >= min_in and m - m_in >= min_out
//   the used epochs ascending:  D, N[c], Q[c];  A[c] = N[c] / D;  var[c] = (Q[c] - A[c] N[c]) / dof;  the chi^2 of the epochs'
//       own amplitudes Ne[c] / De about A[c].
// Every step is one IEEE double operation (contraction off) and every sum runs in index order in ONE thread, so the record
// equals the host statement bit for bit.
//
// tls_centroid_kernel: one workgroup of kCentroidThreads threads a candidate (a launch of fewer workgroups than candidates
// strides over them, so the scratch below is one stretch a WORKGROUP).
// (1) The epochs: the series is walked in tiles of kCentroidThreads points, a thread a point, the loads of t, cx and cy
// coalesced.  t ascends, so k never falls and tau ascends inside an epoch: an epoch's members are an index range, with holes
// where a centroid is not finite.  A member is the HEAD of its epoch iff no earlier point of the same k with tau >= -wd is a
// member; the thread looks back for one, which ends at the point in front of it unless that point is a hole.  A wave's ballot
// and the four wave counts (two sets taking turns, so a tile costs one barrier) give every head its rank, the epoch's number,
// and it leaves its index there.
// (2) The sums: epoch e belongs to thread e mod kCentroidThreads, which walks forward from the head until k changes or tau
// passes wd, twice: the means, then the residuals.  It leaves the seven sums and (m, m_in).
// (3) Threads 0, 1 and 2 take a channel each: the sums over the used epochs in ascending order, the amplitude, its error, and
// the chi^2 sweep over the epochs once more.  No atomics anywhere.
// The first kCentroidLdsEpochs epochs live in the LDS (head, counts, seven sums: 17 KB); later ones in the workgroup's
// stretch of device scratch, kCentroidEpochWords doubles each (wg_sync's release and acquire fences order the stores of (1)
// and (2) in front of the reads of (2) and (3)).
// Included by tls_kernels.hip.h (namespace tlsdev).

constexpr int kCentroidThreads = 256;
constexpr int kCentroidWaves = kCentroidThreads / kWave;
constexpr int kCentroidLdsEpochs = 256;              // epochs the LDS holds
constexpr int kCentroidSums = 7;                     // De | Ne[3] | Qe[3]
constexpr int kCentroidEpochWords = 9;               // of an epoch in the scratch: the sums | (m, m_in) | head
constexpr int kCentroidMaxEpochs = 65536;
constexpr int kCentroidMaxPoints = 1 << 22;
constexpr int kCentroidMaxShape = 1 << 20;           // samples of the shape at most
constexpr int kCentroidMaxGroups = 1024;             // workgroups of a launch at most
constexpr int kCentroidWords = 16;                   // tls_centroid_record

struct CentroidArgs {
    const double* t;                                 // [n]
    const double* y; const double* cx; const double* cy;   // [slots][n]
    const int* slot;                                 // [fits] of the slab
    const double* period; const double* T0; const double* duration;   // [fits]
    const double* shape;                             // [L]
    double* scratch;                                 // [workgroups][max_epochs - kCentroidLdsEpochs][kCentroidEpochWords]
    double* out;                                     // [fits][kCentroidWords]
    unsigned long long* check;                       // [kChecks] violated bounds (debug build; nullptr: off)
    double window;
    int n, fits, L, min_in, min_out, max_epochs;
};

// (k, tau) of a time stamp
__device__ __forceinline__ void centroid_fold(double ti, double T0, double P, double& k, double& tau) {
#pragma clang fp contract(off)
    const double lead = ti - T0;
    const double x = lead / P;
    const double xh = x + 0.5;
    k = floor(xh);
    const double ph = x - k;
    tau = ph * P;
}

// s of a member at tau, and whether it lies inside the transit
__device__ __forceinline__ double centroid_shape(const double* b, int L, double top, double tau, double d, bool& inside) {
#pragma clang fp contract(off)
    const double vq = tau / d;
    const double v = vq + 0.5;
    inside = v >= 0.0 && v <= 1.0;
    if (!inside) return 0.0;
    const double u = v * top;
    int j = (int)floor(u);
    if (j > L - 2) j = L - 2;
    const double fr = u - (double)j;
    const double b0 = b[j], b1 = b[j + 1];
    const double rise = b1 - b0;
    const double part = rise * fr;
    return b0 + part;
}

__global__ void __launch_bounds__(kCentroidThreads) tls_centroid_kernel(const CentroidArgs a) {
#pragma clang fp contract(off)
    __shared__ double e_sums[kCentroidLdsEpochs][kCentroidSums];
    __shared__ int e_count[kCentroidLdsEpochs][2];
    __shared__ int e_head[kCentroidLdsEpochs];
    __shared__ int wave_count[2][2][kCentroidWaves];     // [set][members, heads][wave]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, n = a.n, L = a.L;
    const double nan = (double)NAN;
    const double top = (double)(L - 1);
    const int extra = a.max_epochs > kCentroidLdsEpochs ? a.max_epochs - kCentroidLdsEpochs : 0;
    double* far = a.scratch + (long long)blockIdx.x * extra * kCentroidEpochWords;
    // where epoch e keeps its sums, its counts and its head
    auto sums_of = [&](int e) -> double* {
        return e < kCentroidLdsEpochs ? &e_sums[e][0] : far + (long long)(e - kCentroidLdsEpochs) * kCentroidEpochWords;
    };
    auto count_of = [&](int e) -> int* {
        return e < kCentroidLdsEpochs ? &e_count[e][0]
                                      : reinterpret_cast<int*>(far + (long long)(e - kCentroidLdsEpochs) * kCentroidEpochWords + kCentroidSums);
    };
    auto head_of = [&](int e) -> int* {
        return e < kCentroidLdsEpochs ? &e_head[e]
                                      : reinterpret_cast<int*>(far + (long long)(e - kCentroidLdsEpochs) * kCentroidEpochWords + kCentroidSums + 1);
    };
    TLS_CHECK(a, L >= 2 && L <= kCentroidMaxShape && a.max_epochs >= 1 && a.max_epochs <= kCentroidMaxEpochs, kChkShape);
    for (long long f = blockIdx.x; f < a.fits; f += gridDim.x) {
        double* o = a.out + f * kCentroidWords;
        const double P = a.period[f], T0 = a.T0[f], d = a.duration[f];
        const double wd = a.window * d;
        const double half = 0.5 * P;
        if (!(isfinite(P) && isfinite(T0) && isfinite(d) && P > 0.0 && d > 0.0 && wd < half)) {   // (the whole workgroup)
            if (tid < kCentroidWords) o[tid] = tid == 0 ? 1.0 : nan;
            continue;
        }
        const long long row = (long long)a.slot[f] * n;
        const double* y = a.y + row;
        const double* cx = a.cx + row;
        const double* cy = a.cy + row;
        // (1) the members counted and the heads ranked, in index order
        int total = 0, epochs = 0;
        for (int base = 0, tile = 0; base < n; base += kCentroidThreads, ++tile) {
            const int i = base + tid;
            bool member = false, head = false;
            if (i < n) {
                double k, tau;
                centroid_fold(a.t[i], T0, P, k, tau);
                member = fabs(tau) <= wd && isfinite(cx[i]) && isfinite(cy[i]);
                if (member) {
                    head = true;
                    for (int j = i - 1; j >= 0; --j) {   // (an earlier point of the window: a hole, or the epoch has a member)
                        double kj, tj;
                        centroid_fold(a.t[j], T0, P, kj, tj);
                        if (kj != k || !(tj >= -wd)) break;
                        if (isfinite(cx[j]) && isfinite(cy[j])) { head = false; break; }
                    }
                }
            }
            const unsigned long long members = __ballot(member), heads = __ballot(head);
            if (lane == 0) { wave_count[tile & 1][0][wave] = __popcll(members); wave_count[tile & 1][1][wave] = __popcll(heads); }
            wg_sync();
            int rank = epochs + __popcll(heads & ((1ull << lane) - 1ull));
            for (int v = 0; v < kCentroidWaves; ++v) {
                const int c = wave_count[tile & 1][1][v];
                if (v < wave) rank += c;
                epochs += c;
                total += wave_count[tile & 1][0][v];
            }
            if (head && rank < a.max_epochs) *head_of(rank) = i;
        }
        wg_sync();
        if (epochs > a.max_epochs) {                 // (the whole workgroup)
            if (tid < kCentroidWords) o[tid] = tid == 0 ? 2.0 : tid == 3 ? (double)total : nan;
            wg_sync();                               // (the next candidate overwrites the LDS)
            continue;
        }
        // (2) an epoch a thread: the means, then the residuals
        for (int e = tid; e < epochs; e += kCentroidThreads) {
            const int i0 = *head_of(e);
            TLS_CHECK(a, i0 >= 0 && i0 < n, kChkShape);
            double ke, tau;
            centroid_fold(a.t[i0], T0, P, ke, tau);
            int m = 0, m_in = 0, i1 = i0;
            double Ss = 0.0, S0 = 0.0, S1 = 0.0, S2 = 0.0;
            for (int i = i0; i < n; ++i) {
                double k;
                centroid_fold(a.t[i], T0, P, k, tau);
                if (k != ke || !(tau <= wd)) break;
                const double px = cx[i], py = cy[i];
                if (!(fabs(tau) <= wd && isfinite(px) && isfinite(py))) continue;
                bool inside;
                const double s = centroid_shape(a.shape, L, top, tau, d, inside);
                const double dip = 1.0 - y[i];
                ++m;
                m_in += inside ? 1 : 0;
                Ss = Ss + s; S0 = S0 + dip; S1 = S1 + px; S2 = S2 + py;
                i1 = i + 1;
            }
            double De = 0.0, N0 = 0.0, N1 = 0.0, N2 = 0.0, Q0 = 0.0, Q1 = 0.0, Q2 = 0.0;
            if (m_in >= a.min_in && m - m_in >= a.min_out) {
                const double mf = (double)m;
                const double sbar = Ss / mf, c0 = S0 / mf, c1 = S1 / mf, c2 = S2 / mf;
                for (int i = i0; i < i1; ++i) {
                    double k;
                    centroid_fold(a.t[i], T0, P, k, tau);
                    const double px = cx[i], py = cy[i];
                    if (!(fabs(tau) <= wd && isfinite(px) && isfinite(py))) continue;
                    bool inside;
                    const double s = centroid_shape(a.shape, L, top, tau, d, inside);
                    const double dip = 1.0 - y[i];
                    const double ds = s - sbar, d0 = dip - c0, d1 = px - c1, d2 = py - c2;
                    const double ss = ds * ds, n0 = ds * d0, n1 = ds * d1, n2 = ds * d2, q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2;
                    De = De + ss;
                    N0 = N0 + n0; N1 = N1 + n1; N2 = N2 + n2;
                    Q0 = Q0 + q0; Q1 = Q1 + q1; Q2 = Q2 + q2;
                }
            }
            double* sums = sums_of(e);
            sums[0] = De; sums[1] = N0; sums[2] = N1; sums[3] = N2; sums[4] = Q0; sums[5] = Q1; sums[6] = Q2;
            int* count = count_of(e);
            count[0] = m; count[1] = m_in;
        }
        wg_sync();
        // (3) a channel a thread: the used epochs in ascending order, then the chi^2 sweep
        if (tid < 3) {
            int n_used = 0, n_skipped = 0, n_points = 0, n_in = 0;
            double D = 0.0, N = 0.0, Q = 0.0;
            for (int e = 0; e < epochs; ++e) {
                const int* count = count_of(e);
                const int m = count[0], m_in = count[1];
                if (!(m_in >= a.min_in && m - m_in >= a.min_out)) { ++n_skipped; continue; }
                const double* sums = sums_of(e);
                ++n_used;
                n_points += m;
                n_in += m_in;
                D = D + sums[0];
                N = N + sums[1 + tid];
                Q = Q + sums[4 + tid];
            }
            const bool fitted = n_used >= 1 && D > 0.0;
            if (tid == 0) {
                o[0] = fitted ? 0.0 : 2.0;
                o[1] = (double)n_used; o[2] = (double)n_skipped; o[3] = (double)n_points; o[4] = (double)n_in;
            }
            double A = nan, err = nan, rms = nan, chi2 = nan;
            if (fitted) {
                A = N / D;
                const int dof = n_points - n_used - 1;
                double var = nan;
                if (dof >= 1) {
                    const double explained = A * N;
                    const double left = Q - explained;
                    var = left / (double)dof;
                    if (!(var > 0.0)) var = nan;
                }
                const double scaled = var / D;
                err = sqrt(scaled);
                rms = sqrt(var);
                double sum = 0.0;
                for (int e = 0; e < epochs; ++e) {
                    const int* count = count_of(e);
                    const int m = count[0], m_in = count[1];
                    if (!(m_in >= a.min_in && m - m_in >= a.min_out)) continue;
                    const double* sums = sums_of(e);
                    const double De = sums[0];
                    if (!(De > 0.0)) continue;
                    const double own = sums[1 + tid] / De;
                    const double r = own - A;
                    const double rr = r * r;
                    const double term = rr * De;
                    sum = sum + term;
                }
                chi2 = sum / var;
            }
            // depth, depth_err | shift_x, shift_x_err | shift_y, shift_y_err | rms_x, rms_y | chi2_depth, chi2_x, chi2_y
            o[5 + 2 * tid] = A;
            o[6 + 2 * tid] = err;
            if (tid > 0) o[10 + tid] = rms;
            o[13 + tid] = chi2;
        }
        wg_sync();                                   // (the next candidate overwrites the LDS and the scratch)
    }
}
