"""The cases of the centroid-shift test (tests/centroid_spec.py), shared by the host tests (the loop statement against the
vectorised one) and the device tests (tls_centroid_test against the statement): the edges of the statement, of the kernel
(tls_amd/csrc/tls_centroid.hip.h: tiles of 256 points, an epoch a thread, 256 epochs in the LDS) and of the call (slabs of 1024
candidates), and the scenario -- a planet on an isolated target against the same dip from a source a few pixels away.

A case is a dict: label, t [n], y, cx, cy [n_curves, n], period, T0, duration, curve [n_fits], b [L], options (window, min_in,
min_out, max_epochs) and check(records), which looks at what the case is there to show.  Time stamps are multiples of
DT = 1/32 d unless a case says otherwise, so every time difference is exact."""
import numpy

import centroid_spec as spec

DT = 1.0 / 32.0
NAMES = spec.FIELDS


def series(n, start=0.0):
    return start + numpy.arange(n) * DT


def shape_of(L=spec.SHAPE_SAMPLES):
    """A dome, 0 at both ends and 1 in the middle, with a flat part: what the statement needs of a shape."""
    x = numpy.linspace(0.0, 1.0, L)
    return numpy.minimum(1.0, 1.6 * numpy.sqrt(numpy.sin(numpy.pi * x).clip(0.0)))


def template_shape():
    """The shape survey.centroid_test takes: 1 - the reference transit of power()'s default template on 1025 samples."""
    import warnings
    from tls_amd import template
    from tls_amd.planning import search_inputs
    t = numpy.arange(480) / 48.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp = search_inputs(t, 1.0 + 1e-4 * numpy.sin(t), None, oversampling_factor=1)
    return 1.0 - template.reference_transit(spec.SHAPE_SAMPLES, **inp["shape"])


def curves(t, n_curves, seed, depth=0.0, period=1.0, T0=0.0, duration=0.125, shift=(0.0, 0.0), b=None):
    """(y, cx, cy) [n_curves, n]: noise, a slow drift of the centroids, and a dip of `depth` with the shape b whose centroids
    move by `shift` at the bottom."""
    rng = numpy.random.RandomState(seed)
    n = len(t)
    b = shape_of() if b is None else b
    x = (t - T0) / period
    tau = (x - numpy.floor(x + 0.5)) * period
    v = tau / duration + 0.5
    s = numpy.where((v >= 0) & (v <= 1), numpy.interp(v.clip(0, 1) * (len(b) - 1), numpy.arange(len(b)), b), 0.0)
    y = 1.0 - depth * s[None, :] + rng.normal(0, 3e-4, (n_curves, n))
    drift = 0.01 * numpy.sin(2 * numpy.pi * t / 6.0)
    cx = 512.0 + drift[None, :] + shift[0] * s[None, :] + rng.normal(0, 1e-3, (n_curves, n))
    cy = 77.0 - 0.5 * drift[None, :] + shift[1] * s[None, :] + rng.normal(0, 1e-3, (n_curves, n))
    return y, cx, cy


def case(label, t, rows, period, T0, duration, curve=None, b=None, check=None, **options):
    y, cx, cy = (numpy.atleast_2d(numpy.asarray(v, dtype=float)) for v in rows)
    period, T0, duration = (numpy.atleast_1d(numpy.asarray(v, dtype=float)) for v in (period, T0, duration))
    curve = numpy.arange(len(period)) % len(y) if curve is None else numpy.asarray(curve, dtype=numpy.int64)
    return dict(label=label, t=numpy.asarray(t, dtype=float), y=y, cx=cx, cy=cy, period=period, T0=T0, duration=duration,
                curve=curve, b=shape_of() if b is None else numpy.asarray(b, dtype=float), options=options,
                check=check or (lambda r: None))


def expected(c, fit=spec.centroid, which=slice(None)):
    """The statement's records of a case as a structured array."""
    raw = spec.centroid_batch(c["t"], c["y"], c["cx"], c["cy"], c["period"][which], c["T0"][which], c["duration"][which],
                              c["curve"][which], c["b"], fit=fit, **c["options"])
    out = numpy.zeros(len(raw), dtype=[(k, "f8") for k in NAMES])
    for i, k in enumerate(NAMES):
        out[k] = raw[:, i]
    return out


def rest_is_nan(r, reported):
    return all(numpy.isnan(r[k]).all() for k in NAMES if k not in reported)


# ---- the edges ------------------------------------------------------------------------------------------------------------------
def no_candidate():
    """Every cause of status 1, and one candidate that is measured, on 7 points."""
    t = series(7)
    nan, inf = numpy.nan, numpy.inf
    P = [nan, inf, -inf, 0.0, -1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    T0 = [0.1, 0.1, 0.1, 0.1, 0.1, nan, inf, -inf, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, t[3]]
    d = [0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, nan, inf, 0.0, -0.1, 0.25, 0.3, 2 * DT]    # (2 * 0.25 == 0.5 * 1.0: no window)

    def check(r):
        assert (r["status"][:-1] == 1).all() and rest_is_nan(r[:-1], ("status",))
        assert r["status"][-1] == 0 and r["n_points"][-1] == 7 and r["n_in"][-1] == 3 and r["n_epochs"][-1] == 1

    return case("status 1", t, curves(t, 1, 1, 0.01, T0=t[3], duration=2 * DT), P, T0, d, curve=numpy.zeros(15, dtype=int),
                check=check, window=2.0)


def one_point():
    """n = 1: a member inside the transit and nothing outside: the epoch is skipped, status 2."""
    t = series(1, 5.0)

    def check(r):
        assert r["status"].tolist() == [2, 2] and r["n_epochs"].tolist() == [0, 0]
        assert r["n_skipped"].tolist() == [1, 0] and r["n_points"].tolist() == [0, 0]
        assert rest_is_nan(r, ("status", "n_epochs", "n_skipped", "n_points", "n_in"))

    return case("one point", t, curves(t, 1, 2), [1.0, 1.0], [5.0, 5.4], [0.1, 0.1], curve=[0, 0], check=check)


def small_dof_windows():
    """7 points, one used epoch, a triangle of three samples for a shape: 7, 5 and -- the epoch cut by the start of the series
    -- 2 members, dof 5, 3 and 0 (one call has one window, so three cases)."""
    t = series(7)
    rows = curves(t, 1, 3, 0.01, T0=t[3], duration=2 * DT)
    out = []
    for label, T0, d, W, points, n_in in (("dof 5", t[3], 2 * DT, 1.5, 7, 3), ("dof 3", t[3], 2 * DT, 1.0, 5, 3),
                                           ("dof 0, cut by the start", t[0], DT, 1.0, 2, 1)):
        def check(r, points=points, n_in=n_in):
            assert r["status"][0] == 0 and r["n_epochs"][0] == 1 and r["n_points"][0] == points and r["n_in"][0] == n_in
            assert numpy.isfinite(r["shift_x"][0]) and numpy.isfinite(r["depth"][0])
            if points == 2:
                assert numpy.isnan(r["shift_x_err"][0]) and numpy.isnan(r["rms_y"][0]) and numpy.isnan(r["chi2_depth"][0])
            else:
                assert numpy.isfinite(r["shift_x_err"][0]) and r["chi2_x"][0] == 0    # (one epoch: its amplitude is the common one)
        out.append(case(label, t, rows, [1.0], [T0], [d], check=check, window=W, min_out=1, b=shape_of(3)))
    return out


def gaps_and_holes():
    """P = 1 on 9 d at 32 a day: epoch 0 cut by the start, epoch 8 by the end, epoch 3 inside a gap (no member: not an epoch),
    epoch 5 short of min_out, epoch 6 with NaN centroids in transit, epoch 7 NaN all over (not an epoch), epoch 2 with one hole
    behind its first member."""
    t = series(8 * 32 + 1)
    keep = ~((t > 2.6) & (t < 3.4))
    near5 = numpy.abs(t - 5.0)
    keep &= ~((near5 > 2 * DT) & (near5 <= 0.25) & (near5 != 3 * DT))
    t = t[keep]
    y, cx, cy = curves(t, 2, 4, 0.01, duration=4 * DT, shift=(0.02, -0.01))
    cx[:, numpy.abs(t - 6.0) <= DT] = numpy.nan
    cy[:, numpy.abs(t - 7.0) <= 0.25] = numpy.inf
    cy[0, numpy.abs(t - (2.0 - 7 * DT)) < 1e-9] = numpy.nan

    def check(r):
        assert (r["status"] == 0).all() and (r["n_epochs"] == 6).all() and (r["n_skipped"] == 1).all()
        assert r["n_points"].tolist() == [9 + 17 + 16 + 17 + 14 + 9, 9 + 17 + 17 + 17 + 14 + 9]
        assert (r["n_in"] == 3 + 5 + 5 + 5 + 2 + 3).all()
        assert (numpy.abs(r["shift_x"] - 0.02) < 5 * r["shift_x_err"]).all() and (r["shift_x"] > 10 * r["shift_x_err"]).all()

    return case("gaps and holes", t, (y, cx, cy), [1.0, 1.0], [0.0, 0.0], [4 * DT, 4 * DT], check=check, window=2.0)


def exact_edges():
    """P = 2, T0 = 1, d = 1/8, W = 2 on multiples of 1/32: tau hits -wd and +wd exactly (members) and v hits 0 and 1 exactly
    (inside: 5 of the 17 members of an epoch)."""
    t = series(257)

    def check(r):
        assert r["status"][0] == 0 and r["n_epochs"][0] == 4 and r["n_points"][0] == 4 * 17 and r["n_in"][0] == 4 * 5

    return case("tau at wd, v at 0 and 1", t, curves(t, 1, 5, 0.01, 2.0, 1.0, 0.125, (0.01, 0.0)), [2.0], [1.0], [0.125],
                check=check, window=2.0)


def constant_centroids():
    """Centroid rows that never move: every residual is 0, var is 0 and so not > 0: the shift is 0 and its error NaN."""
    t = series(255)
    y, cx, cy = curves(t, 1, 6, 0.01, T0=0.5, duration=0.125)
    cx[:] = 3.5
    cy[:] = -2.25

    def check(r):
        assert r["status"][0] == 0 and r["shift_x"][0] == 0 and r["shift_y"][0] == 0 and r["depth"][0] > 0.005
        assert all(numpy.isnan(r[k][0]) for k in ("shift_x_err", "shift_y_err", "rms_x", "rms_y", "chi2_x", "chi2_y"))
        assert numpy.isfinite(r["depth_err"][0]) and numpy.isfinite(r["chi2_depth"][0])

    return case("constant centroids", t, (y, cx, cy), [1.0], [0.5], [0.125], check=check)


def no_usable_epoch():
    t = series(255)

    def check(r):
        assert r["status"][0] == 2 and r["n_epochs"][0] == 0 and r["n_skipped"][0] == 8 and r["n_points"][0] == 0
        assert rest_is_nan(r, ("status", "n_epochs", "n_skipped", "n_points", "n_in"))

    return case("no usable epoch", t, curves(t, 1, 7), [1.0], [0.5], [0.125], check=check, min_in=6)


def sizes():
    """255 and 257 points (one tile of the kernel short of a point, and one point into the second), candidates off the grid."""
    out = []
    for n in (255, 257):
        t = series(n)
        rows = curves(t, 3, 8 + n, 0.008, 1.37, 0.41, 0.11, (-0.03, 0.02))

        def check(r):
            assert (r["status"] == 0).all() and (r["n_epochs"] >= 4).all()
            assert (r["shift_x"][0] < -10 * r["shift_x_err"][0]) and (r["shift_y"][0] > 10 * r["shift_y_err"][0])

        out.append(case("n = %d" % n, t, rows, [1.37, 1.37, 0.9, 2.11], [0.41, 0.41 + 1.37, 0.2, 7.9], [0.11, 0.11, 0.07, 0.2],
                        curve=[0, 1, 2, 0], check=check, window=2.5, min_in=2, min_out=4))
    return out


def many_epochs(max_epochs=65536, label="many epochs"):
    """1500 points, P = 5 samples: 300 used epochs of 5 members each -- more than the 256 threads of a workgroup and than the
    256 epochs its LDS holds -- on the grid, off it, and at a period of 6 samples."""
    t = series(1500)
    rows = curves(t, 2, 9, 0.01, 5 * DT, t[2], 0.034, (0.05, 0.0))
    # the epochs holding a member: 300; 301 (T0 two samples on, so an epoch in front of the series reaches into it with two
    # members and the last one is cut to three: both skipped); 250; 300 (off the grid a window of 4.35 samples holds 4 points)
    status = {65536: [0, 0, 0, 0], 300: [0, 2, 0, 0], 299: [2, 2, 0, 2]}[max_epochs]

    def check(r):
        assert r["status"].tolist() == status
        for f, (epochs, skipped, points) in enumerate(((300, 0, 1500), (299, 2, 1495), (250, 0, 1250), (300, 0, 1200))):
            if status[f] == 0:
                assert (r["n_epochs"][f], r["n_skipped"][f], r["n_points"][f], r["n_in"][f]) == (epochs, skipped, points, epochs)
                # (the dip and its shift of 0.05 are at the ephemeris of candidates 0 and 3)
                assert r["shift_x"][f] > 20 * r["shift_x_err"][f] if f in (0, 3) else numpy.isfinite(r["chi2_x"][f])
            else:
                assert r["n_points"][f] == (1500 if f < 2 else 1200) and rest_is_nan(r[[f]], ("status", "n_points"))

    return case(label, t, rows, [5 * DT, 5 * DT, 6 * DT, 5 * DT], [t[2], t[4], t[3], t[2] + 0.3 * DT], [0.034] * 4,
                curve=[0, 1, 0, 1], check=check, window=2.0, max_epochs=max_epochs)


def julian_dates():
    t = series(257, 2454833.0)

    def check(r):
        assert (r["status"] == 0).all() and (r["n_epochs"] >= 5).all()
        assert abs(r["shift_x"][0] - 0.04) < 5 * r["shift_x_err"][0]

    return case("Julian dates", t, curves(t, 2, 10, 0.01, 1.3, 2454833.4, 0.12, (0.04, 0.0)), [1.3, 1.3], [2454833.4, 2454834.7],
                [0.12, 0.12], check=check)


def scattered_curves():
    """Five curves, candidates on two of them, out of order and repeated."""
    t = series(255)
    rows = curves(t, 5, 11, 0.01, 1.1, 0.3, 0.1, (0.02, 0.02))

    def check(r):
        assert (r["status"] == 0).all()
        for k in NAMES:
            assert r[k][0] == r[k][2] == r[k][3] and r[k][1] == r[k][4]
        assert r["depth"][0] != r["depth"][1]

    return case("curves 3 0 3 3 0", t, rows, [1.1] * 5, [0.3] * 5, [0.1] * 5, curve=[3, 0, 3, 3, 0], check=check)


def over_a_slab():
    """1025 candidates -- one above the slab of 1024 -- on 7 points."""
    t = series(7)
    rng = numpy.random.RandomState(12)
    n_fits = 1025

    def check(r):
        assert (r["status"] == 0).sum() > 900 and r["status"][1024] == 0

    T0 = rng.uniform(t[2], t[4], n_fits)
    T0[1024] = t[3]
    return case("1025 candidates", t, curves(t, 4, 12, 0.01, T0=t[3], duration=2 * DT, shift=(0.01, 0.0)), numpy.full(n_fits, 1.0),
                T0, rng.uniform(1.5 * DT, 2.5 * DT, n_fits), curve=rng.randint(0, 4, n_fits), check=check, window=1.2, min_out=2)


def edge_cases():
    return ([no_candidate(), one_point()] + small_dof_windows() + [gaps_and_holes(), exact_edges(), constant_centroids(),
            no_usable_epoch()] + sizes() + [many_epochs(), many_epochs(300, "300 epochs allowed"),
            many_epochs(299, "299 epochs allowed"), julian_dates(), scattered_curves()])


# ---- the scenario: which star dims ----------------------------------------------------------------------------------------------
SCENARIO = dict(period=7.3, duration=0.14, depth=0.005, source=(4.0, -3.0))


def scenario(seed, blended):
    """90 d at 48 a day with a gap, flux noise 3e-4, centroid noise 1e-3 px, a pointing drift of 0.01 px (a sinusoid of 6 d
    plus a sawtooth of 3 d), a planet of depth 0.5 % at P = 7.3 d and d = 0.14 d with the limb-darkened template's shape -- on the target itself (the photocentre
    does not move), or on a source 4 px and -3 px from the out-of-transit photocentre (it moves by -r D s / (1 - D s)):
    (t, y, cx, cy, T0, b)."""
    rng = numpy.random.RandomState(seed)
    t = numpy.arange(90 * 48) / 48.0
    t = t[(t < 41.0) | (t > 44.5)]
    P, d, D = SCENARIO["period"], SCENARIO["duration"], SCENARIO["depth"]
    T0 = 2.1 + 0.37 * seed
    b = template_shape()
    x = (t - T0) / P
    tau = (x - numpy.floor(x + 0.5)) * P
    v = tau / d + 0.5
    s = numpy.where((v >= 0) & (v <= 1), numpy.interp(v.clip(0, 1) * (len(b) - 1), numpy.arange(len(b)), b), 0.0)
    y = 1.0 - D * s + rng.normal(0, 3e-4, len(t))
    drift = 0.01 * numpy.sin(2 * numpy.pi * t / 6.0) + 0.01 * ((t / 3.0) % 1.0)
    move = D * s / (1.0 - D * s) if blended else 0.0 * s
    cx = 100.0 + drift - SCENARIO["source"][0] * move + rng.normal(0, 1e-3, len(t))
    cy = 200.0 - 0.7 * drift - SCENARIO["source"][1] * move + rng.normal(0, 1e-3, len(t))
    return t, y, cx, cy, T0, b
