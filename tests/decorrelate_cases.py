"""The inputs test_decorrelate_host.py and test_decorrelate.py share: the K2 roll simulation, the basis-vector ensemble, and
the small shapes at which tls_decorrelate's kernel can go wrong.  GPU-free."""
import numpy

import decorrelate_spec as spec

CADENCE = 1.0 / 48.0
NOISE = 3e-4
DEPTH, DURATION, PERIOD = 0.005, 0.2, 7.3


def regressors(cx, cy):
    """survey.centroid_regressors(order=2) restated: x, y, x^2, x y, y^2 of the centroids minus their medians."""
    x, y = cx - numpy.median(cx), cy - numpy.median(cy)
    return numpy.stack([x, y, x * x, x * y, y * y])


def roll_star(seed, n=4320, period=PERIOD, outliers=0, depth=DEPTH):
    """A K2 star: n points at 48 a day; the photocentre rolls by about a fifth of a pixel in a six-hour sawtooth whose
    amplitude drifts, and the flux follows it as 1 + 0.01 cx - 0.03 cx^2 + 0.004 cy; a box of `depth` (0.5 %) and 0.2 d every
    `period` d; white noise of 3e-4; `outliers` points 12 sigma up, outside the transits.  A dict."""
    rng = numpy.random.default_rng(seed)
    t = 1.0 + numpy.arange(n) * CADENCE                     # (the search takes time stamps > 0)
    phase = (t / 0.25) % 1.0
    cx = 0.22 * (2.0 * phase - 1.0) * (1.0 + 0.2 * numpy.sin(2.0 * numpy.pi * t / 20.0)) + 0.005 * rng.standard_normal(n)
    cy = 0.3 * cx + 0.1 * numpy.sin(2.0 * numpy.pi * t / 3.1) + 0.005 * rng.standard_normal(n)
    systematics = 1.0 + 0.01 * cx - 0.03 * cx * cx + 0.004 * cy
    T0 = 2.3 + 0.37 * seed
    in_transit = numpy.abs((t - T0 + 0.5 * period) % period - 0.5 * period) <= 0.5 * DURATION
    star = numpy.where(in_transit, 1.0 - depth, 1.0)
    noise = NOISE * rng.standard_normal(n)
    spikes = numpy.zeros(n)
    if outliers:
        spikes[rng.choice(numpy.flatnonzero(~in_transit), outliers, replace=False)] = 12.0 * NOISE
    return {"t": t, "cx": cx, "cy": cy, "flux": systematics * (star + noise + spikes), "in_transit": in_transit,
            "spiked": spikes > 0.0, "own": regressors(cx, cy), "T0": T0, "period": period}


def rms_and_depth(flat, star):
    """(the rms of the flat row outside the transits and the spikes, 1 - the in-transit mean over the mean outside)."""
    out = ~star["in_transit"] & ~star["spiked"]
    level = flat[out].mean()
    return float(numpy.sqrt(numpy.mean((flat[out] / level - 1.0) ** 2))), float(1.0 - flat[star["in_transit"]].mean() / level)


def ensemble(n_stars=64, n=960, seed=11):
    """n_stars stars that share a ramp and a sawtooth, each with its own strengths and its own white noise: (flux
    [n_stars, n], the two profiles [2, n], the noise level of every star)."""
    rng = numpy.random.default_rng(seed)
    t = numpy.arange(n) * CADENCE
    profiles = numpy.stack([t / t[-1] - 0.5, 2.0 * ((t / 0.25) % 1.0) - 1.0])
    strength = rng.uniform(-0.01, 0.01, (n_stars, 2))
    sigma = rng.uniform(2e-4, 8e-4, n_stars)
    flux = (1.0 + strength @ profiles) * (1.0 + sigma[:, None] * rng.standard_normal((n_stars, n)))
    return flux, profiles, sigma


def small(n, n_shared, n_own, n_curves=1, dy=False, seed=0, strength=0.02):
    """A small batch: flux that follows its columns with white noise of 1e-3 and a few 10-sigma outliers where n allows."""
    rng = numpy.random.default_rng(1000 * n + 17 * n_shared + n_own + seed)
    shared = rng.standard_normal((n_shared, n))
    own = rng.standard_normal((n_curves, n_own, n))
    flux = 1.0 + 1e-3 * rng.standard_normal((n_curves, n))
    if n_shared:
        flux += strength * rng.uniform(-1, 1, (n_curves, n_shared)) @ shared
    if n_own:
        flux += numpy.einsum("ck,ckn->cn", strength * rng.uniform(-1, 1, (n_curves, n_own)), own)
    if n > 40:
        flux[:, rng.choice(n, 3, replace=False)] += 0.01
    out = {"y": flux, "shared": shared if n_shared else None, "own": own if n_own else None}
    out["dy"] = rng.uniform(5e-4, 2e-3, (n_curves, n)) if dy else None
    return out


def equal_bits(got, want, names=("flat", "trend", "record", "coef", "mean", "scale")):
    """Asserts the fields `names` of the two results equal bit for bit (a NaN equals a NaN)."""
    for k in names:
        a, b = numpy.asarray(got[k]), numpy.asarray(want[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        numpy.testing.assert_array_equal(a, b, err_msg=k)
        assert numpy.array_equal(numpy.signbit(a[a == 0.0]), numpy.signbit(b[b == 0.0])), k


def statement(case, **kw):
    return spec.fit(case["y"], case.get("dy"), case.get("mask"), case.get("shared"), case.get("own"), case.get("segments"), **kw)
