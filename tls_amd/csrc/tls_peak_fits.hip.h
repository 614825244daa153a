// tls_peak_fits.hip.h -- the candidate picks of the peak-fit stage (tls_power_batch_peak_fits, tls_debug_peak_fits).
//
// The stage gives every peak of tls_find_peaks what the main chain gives the one pick of a curve: the final T0 fit and the
// tls_transit_stats record.  It runs the main chain's own kernels -- tls_power_prep, the three launches of the T0 fit,
// tls_first_min, tls_transit_stats -- on fits f = c k + r (curve c of the group, rank r) instead of curves, on arrays of its
// own, in slabs of at most kPeakFitSlab fits (DESIGN.md "Peak fits").  tls_peak_picks below opens a slab: from the group's
// peak records it forms, per fit, a pick record in tls_power_pick's layout, the curve the fit reads its flux and its detrended
// power from (T0FitArgs::curve, TransitStatsArgs::curve: a slab may begin and end inside a curve's k candidates) and the
// fit's status.
//
// A candidate's pick is NOT the main chain's pick.  tls_power_pick takes the template row from argmin(chi2) and period and
// depth from argmax(power), two indices that usually but not always agree; a candidate has ONE index, its own, and takes
// period, depth AND row from it: [0] chi2 at the index, [1] = [2] the index, [3] period, [4] depth, [5] row, [6] 1.0 where
// there is nothing to fit (rank >= n_peaks, or the search fitted nothing at the index: row < 0), [7] 0.0.  So rank 0 equals
// the summary's T0 and statistics exactly where index_best == index_power.
// Whether a row starts a template duration is tls_power_prep's to decide, here as in the main chain: it raises [7] of the
// fit's pick, tls_transit_stats then writes the record of a pick without fit (NaN behind the period uncertainty), and the
// host reports a fit of status 0 whose record holds no transit count as that error.
// Included by tls_kernels.hip.h (namespace tlsdev), behind tls_peaks.hip.h.

constexpr int kPeakFitSlab = 128;        // fits per set of launches: the T0 fit's rotation scratch is 3 n + 4 doubles a fit
constexpr int kPeakFitWords = 2 + kTransitStats;   // tls_peak_fit: T0, status | tls_transit_stats
constexpr double kPeakFitted = 0.0, kPeakNone = 1.0, kPeakUnfitted = 2.0;   // tls_peak_fit.status

struct PeakPicksArgs {
    const unsigned long long* peaks;     // [curves][1 + k kPeakWords]: n_peaks | k records (tls_find_peaks)
    double* pick;                        // [fits][8]
    int* curve;                          // [fits]
    double* status;                      // [fits]
    int k, first, fits;                  // fit l of the slab is fit first + l of the group
};

// one thread a fit
__global__ void __launch_bounds__(256) tls_peak_picks(const PeakPicksArgs a) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.fits) return;
    const int f = a.first + l, c = f / a.k, r = f % a.k;
    const unsigned long long* rec = a.peaks + (long long)c * (1 + (long long)a.k * kPeakWords);
    const long long n_peaks = (long long)rec[0];
    const unsigned long long* p = rec + 1 + (long long)r * kPeakWords;
    const long long index = (long long)p[4], row = (long long)p[5];
    const double status = r >= n_peaks ? kPeakNone : row < 0 ? kPeakUnfitted : kPeakFitted;
    const bool none = status == kPeakNone;
    double* o = a.pick + 8LL * l;
    o[0] = none ? (double)NAN : __longlong_as_double((long long)p[2]);
    o[1] = none ? -1.0 : (double)index; o[2] = o[1];
    o[3] = none ? (double)NAN : __longlong_as_double((long long)p[0]);
    o[4] = none ? (double)NAN : __longlong_as_double((long long)p[3]);
    o[5] = none ? -1.0 : (double)row;
    o[6] = status == kPeakNone || status == kPeakUnfitted ? 1.0 : 0.0;
    o[7] = 0.0;
    a.curve[l] = c;
    a.status[l] = status;
}
