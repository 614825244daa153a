"""The phase scan of survey.phase_scan / power_batch(peaks=K, peak_fits=True, phase_scan=True) (tls_phase_scan,
tls_power_batch_phase_scan), stated in plain Python and numpy: what the device is tested against bit for bit
(include/tls_amd.h tls_phase_record, DESIGN.md "Phase scan").

A candidate is (light curve y over the time stamps t, period P, T0, duration d in days).  The curve is folded into B bins
of width 1/B >= d/(2P), a window is two neighbouring bins (about one duration), and every window's depth is measured
against the baseline -- the bins away from the primary -- without it.  Unweighted.

    scan(t[n], y[n], P, T0, d, max_bins=4096, min_count=3):
      record = {status: 1, every other field NaN}
      if P, T0, d not all finite, or P <= 0, or d <= 0: return record
      q = 2.0 * P / d
      if not q >= 16: return record
      B = int(min(floor(q), max_bins))          # bin width 1/B >= d/(2P)
      for i in 0..n-1 ascending:                # S[b], N[b] start at 0
          x = (t[i] - T0) / P;  phi = x - floor(x);  b = min(int(phi * B), B - 1)
          S[b] = S[b] + y[i];  N[b] += 1
      # window j = bins j and (j+1) % B:  W[j] = S[j] + S[(j+1)%B],  M[j] = N[j] + N[(j+1)%B]
      # primary window p = B-1 (bins B-1 and 0: phase [-1/B, 1/B))
      # baseline: bins 2 .. B-3 ascending:  Sb = sum S[b], Nb = sum N[b]   (free of the primary)
      # "inside" windows: 2 <= j <= B-4 (they lie in the baseline); the others are excluded from the scan
      delta[j] = (Sb - W[j]) / (Nb - M[j]) - W[j] / M[j]   for inside j with M[j] >= min_count and Nb - M[j] >= 1
      delta[p] =  Sb / Nb - W[p] / M[p]                    if M[p] >= min_count and Nb >= 1
      every other delta is NaN
      status = 0; n_bins = B; primary_depth = delta[p]; primary_count = M[p]
      free = inside j with delta[j] not NaN;  if none: n_windows = 0, return
      js = first j of free with the largest delta;  jb = first j of free with the smallest
      secondary_depth = delta[js]; secondary_phase = (js + 1) / B; secondary_count = M[js]
      bump_depth = delta[jb]; bump_phase = (jb + 1) / B
      rest = free j with |j - js| > 2;  n_windows = len(rest)
      if n_windows >= 8:  mu = (sum of delta over rest, ascending j) / n_windows
                          scan_mean = mu;  scan_std = sqrt((sum of (delta - mu) * (delta - mu), ascending j) / n_windows)

Every sum is a left-to-right loop in the stated order and every arithmetic step is one IEEE double operation (Python floats
and numpy's element-wise operations never contract); counts enter the quotients as exact doubles.  The time stamps are
finite.  The host adds secondary_significance and primary_significance, (depth - scan_mean) / scan_std."""
import math

import numpy

FIELDS = ("status", "n_bins", "n_windows", "primary_depth", "primary_count", "secondary_depth", "secondary_phase",
          "secondary_count", "bump_depth", "bump_phase", "scan_mean", "scan_std")
SCANNED, NOTHING = 0, 1


def bins(t, P, T0, B):
    """The bin of every point."""
    x = (numpy.asarray(t, dtype=numpy.float64) - numpy.float64(T0)) / numpy.float64(P)
    phi = x - numpy.floor(x)
    return numpy.minimum((phi * numpy.float64(B)).astype(numpy.int64), B - 1)


def scan(t, y, P, T0, d, max_bins=4096, min_count=3, with_delta=False):
    """The tls_phase_record of one candidate, a dict by field (with_delta: and the window depths, NaN where excluded)."""
    nan = float("nan")
    rec = dict.fromkeys(FIELDS, nan)
    rec["status"] = float(NOTHING)
    P, T0, d = float(P), float(T0), float(d)
    if not (math.isfinite(P) and math.isfinite(T0) and math.isfinite(d)) or P <= 0 or d <= 0:
        return (rec, None) if with_delta else rec
    q = 2.0 * P / d
    if not q >= 16:
        return (rec, None) if with_delta else rec
    B = int(min(math.floor(q), max_bins))
    y = [float(v) for v in numpy.asarray(y, dtype=numpy.float64)]
    S, N = [0.0] * B, [0] * B
    for i, b in enumerate(bins(t, P, T0, B).tolist()):
        S[b] = S[b] + y[i]
        N[b] += 1
    W = [S[j] + S[(j + 1) % B] for j in range(B)]
    M = [N[j] + N[(j + 1) % B] for j in range(B)]
    p = B - 1
    Sb, Nb = 0.0, 0
    for b in range(2, B - 2):
        Sb = Sb + S[b]
        Nb += N[b]
    delta = [nan] * B
    for j in range(2, B - 3):
        if M[j] >= min_count and Nb - M[j] >= 1:
            delta[j] = (Sb - W[j]) / float(Nb - M[j]) - W[j] / float(M[j])
    if M[p] >= min_count and Nb >= 1:
        delta[p] = Sb / float(Nb) - W[p] / float(M[p])
    rec.update(status=float(SCANNED), n_bins=float(B), primary_depth=delta[p], primary_count=float(M[p]), n_windows=0.0)
    free = [j for j in range(2, B - 3) if not math.isnan(delta[j])]
    if free:
        js = jb = free[0]
        for j in free:
            if delta[j] > delta[js]:
                js = j
            if delta[j] < delta[jb]:
                jb = j
        rec.update(secondary_depth=delta[js], secondary_phase=float(js + 1) / float(B), secondary_count=float(M[js]),
                   bump_depth=delta[jb], bump_phase=float(jb + 1) / float(B))
        rest = [j for j in free if abs(j - js) > 2]
        rec["n_windows"] = float(len(rest))
        if len(rest) >= 8:
            total = 0.0
            for j in rest:
                total = total + delta[j]
            mu = total / float(len(rest))
            total = 0.0
            for j in rest:
                total = total + (delta[j] - mu) * (delta[j] - mu)
            rec.update(scan_mean=mu, scan_std=math.sqrt(total / float(len(rest))))
    return (rec, delta) if with_delta else rec


def significances(rec):
    """(secondary_significance, primary_significance) as the host forms them."""
    with numpy.errstate(all="ignore"):
        mean, std = numpy.float64(rec["scan_mean"]), numpy.float64(rec["scan_std"])
        return (float((numpy.float64(rec["secondary_depth"]) - mean) / std),
                float((numpy.float64(rec["primary_depth"]) - mean) / std))


def expected(t, y, P, T0, d, max_bins=4096, min_count=3):
    """The record with the two significances: every field survey.phase_scan returns."""
    rec = scan(t, y, P, T0, d, max_bins, min_count)
    rec["secondary_significance"], rec["primary_significance"] = significances(rec)
    return rec
