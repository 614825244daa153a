"""The edge cases of the event vetting, shared by tests/test_event_vetting_host.py (the statement's loops against its vectorised
form) and tests/test_event_vetting.py (the device against the statement).  Time stamps are multiples of 1/64 d, so every time
difference is exact.  A case is a dict: the arguments of event_vetting_spec.expected / Context.event_vetting, a label, and
`check(summary, events)`, which asserts what the case is there to show on whichever result it is given."""
import numpy

import event_vetting_spec as spec

WIDTHS = [3, 4, 5, 8, 37, 65]
SHAPE = dict(per=12.9, rp=0.03, a=23.1, inc=89.21, ecc=0, w=90, u=[0.4804, 0.1867], limb_dark="quadratic")
DT = 1 / 64.0
_SHAPES = {}


def shapes_of(widths):
    """The rows' shapes, computed once a width."""
    for L in widths:
        if int(L) not in _SHAPES:
            _SHAPES[int(L)] = spec.shapes_of([L], **SHAPE)[0]
    return [_SHAPES[int(L)] for L in widths]


def spans_of(widths, gap_tolerance=0.5):
    return [(int(L) - 1) * DT * (1 + gap_tolerance) for L in widths]


def series(n, gap_at=None, gap=0):
    """n time stamps at 1/64 d, `gap` cadences missing in front of index gap_at."""
    t = 1.0 + numpy.arange(n + gap) / 64.0
    return t if gap_at is None else numpy.concatenate([t[:gap_at], t[gap_at + gap:]])


def dips(t, period, T0, width, depth=4e-3, seed=0, sigma=1e-3):
    """Noise of `sigma` and a box dip of `width` samples centred on the sample nearest every T0 + e * period."""
    rng = numpy.random.RandomState(seed)
    y = 1 + rng.normal(0, sigma, len(t)) if sigma else numpy.ones(len(t))
    e = int(numpy.ceil((t[0] - T0) / period))
    while T0 + e * period <= t[-1]:
        c = int(numpy.argmin(numpy.abs(t - (T0 + e * period))))
        y[max(0, c - width // 2): max(0, c - width // 2 + width)] -= depth
        e += 1
    return y


def case(label, t, y, dy, period, T0, row, reach, chase_reach, guard, chase_span, curve=None, widths=WIDTHS, span_max=None,
         check=None, **options):
    y = numpy.atleast_2d(numpy.asarray(y, dtype=float))
    dy = numpy.array(numpy.broadcast_to(numpy.asarray(dy, dtype=float), y.shape)) if numpy.ndim(dy) < 2 else numpy.asarray(dy)
    # (scalars are repeated: one candidate a curve, or one a `curve` entry)
    n_fits = max([numpy.size(v) for v in (period, T0, row, reach, chase_reach, guard, chase_span)]
                 + [len(y) if curve is None else len(curve)])
    full = lambda v, kind: numpy.array(numpy.broadcast_to(numpy.asarray(v, dtype=kind), (n_fits,)))
    options.setdefault("max_epochs", 48)
    return dict(label=label, t=t, y=y, dy=dy, period=full(period, float), T0=full(T0, float), row=full(row, int),
                reach=full(reach, int), chase_reach=full(chase_reach, int), guard=full(guard, int),
                chase_span=full(chase_span, float), curve=numpy.arange(len(y)) if curve is None else numpy.asarray(curve),
                widths=list(widths), span_max=spans_of(widths) if span_max is None else list(span_max), options=options,
                check=check or (lambda s, e: None))


def expected(c, loops=False, which=slice(None)):
    """The statement on a case (on the candidates `which`)."""
    return spec.expected(c["t"], c["y"], c["dy"], c["curve"][which], c["period"][which], c["T0"][which], c["row"][which],
                         c["reach"][which], c["chase_reach"][which], c["guard"][which], c["chase_span"][which],
                         shapes_of(c["widths"]), c["span_max"], loops=loops, **c["options"])


def held(events, f=0):
    return events[f][events["status"][f] == 0]


def edge_cases():
    """Every edge the issue names below the slabs; small enough for the statement's loops."""
    out = []
    nan, inf = numpy.nan, numpy.inf

    # ---- the ends of the series: side windows outside it (NaN), chase windows on one side only
    for n in (257, 300, 700):
        t = series(n)
        P = (n - 1) * DT / 4
        y = numpy.array([dips(t, P, t[0], L, seed=L) for L in WIDTHS])

        def ends(s, e, n=n):
            assert (s["n_epochs"] == 5).all() and (s["epoch_first"] == 0).all()
            for f, L in enumerate(WIDTHS):
                first, last = e[f][0], e[f][4]
                assert first["status"] == 0 and last["status"] == 0, L
                assert numpy.isnan(first["before"]) and numpy.isnan(last["after"]), L        # (no L samples beside the window)
                side = max(0, 20 - L)                # (R - Gd windows a side)
                assert first["n_chased"] <= side and last["n_chased"] <= side and e[f][2]["n_chased"] == 2 * side, L
        out.append(case(("ends", n), t, y, 1e-3, P, t[0], numpy.arange(6), WIDTHS, 20, WIDTHS, 0.25, check=ends, min_ses=0.0))
        out.append(case(("ends, reach 1", n), t, y, 1e-3, P, t[0], numpy.arange(6), 1, 20, 2, 0.25))

    # ---- gaps: a gap of 20 cadences beside an event; a side window that hits span_max exactly is kept, one cadence short is not
    t = series(500, gap_at=250, gap=20)
    y = numpy.ones(500)
    y[252:257] -= 5e-3                                # the event: lo = 252, c = 254; `before` is [247, 251]: 24 / 64 d exactly
    for span, seen in ((24 * DT, True), (23 * DT, False)):
        def gap(s, e, seen=seen):
            assert e["index"][0][0] == 254 and numpy.isfinite(e["before"][0][0]) == seen and numpy.isfinite(e["after"][0][0])
            assert e["n_chased"][0][0] == 2 * 30 and (e["before"][0][0] == 0.0 or not seen)   # (the windows over the gap lie inside the guard)
        out.append(case(("gap", span), t, y, 1e-3, [1000.0], [t[254]], [0], [1], [37], [7], [1.0], widths=[5], span_max=[span],
                        check=gap))
    y37 = dips(t, 100 * DT, t[50], 37, seed=3)
    out.append(case("gap, epochs in it", t, y37, 1e-3, 100 * DT, t[50], [4, 4, 2], [1, 40, 1], [60, 60, 30], [50, 55, 7], 0.5,
                    curve=[0, 0, 0]))

    # ---- empty chases
    t = series(400)
    P, T0 = 80 * DT, t[40]
    y = dips(t, P, T0, 5, seed=5)

    def empty(s, e):
        for f in range(3):
            rows = held(e, f)
            assert len(rows) >= 4 and (rows["n_chased"] == 0).all() and numpy.isnan(rows["chases"]).all()
            assert numpy.isnan(s["chases_min"][f]) and numpy.isnan(s["chases_mean"][f]) and (rows["flags"] < 8).all()
    out.append(case("empty chases", t, y, 1e-3, P, T0, 2, 3, [10, 0, 7], [10, 0, 9000], 0.1, curve=[0, 0, 0], check=empty))

    # ---- comparable and non-comparable neighbours: exact on constant flux
    flat = numpy.ones((4, 400))
    flat[0, 98:103] -= 4e-3
    flat[0, 128:133] -= 4e-3                          # two identical box dips, 30 samples apart
    flat[1, 98:103] -= 4e-3
    flat[1, 128:133] += 4e-3                          # ... the second one a bump
    flat[2, 98:103] -= 4e-3                           # a lone dip
    flat[3, 98:103] -= 4e-3
    flat[3, 128:133] -= 2e-3                          # half as deep: not comparable at 1.0, comparable at 0.5

    def neighbours(s, e):
        assert (e["index"][:, 0] == 100).all() and (e["n_chased"][:, 0] == 2 * 32).all()
        assert e["chase_dt"][0][0] == e["chase_dt"][1][0] == 30 * DT and e["chases"][0][0] == 30 * DT
        assert numpy.isnan(e["chase_dt"][2][0]) and e["chases"][2][0] == 1.0 and numpy.isnan(e["chase_dt"][3][0])
        assert e["flags"][:, 0].tolist() == [8, 8, 0, 0] and s["n_good"].tolist() == [0, 0, 1, 1]
    out.append(case("neighbours", t, flat, 1e-3, 1000.0, t[100], 2, 2, 40, 8, 1.0, check=neighbours, chase_fraction=1.0))

    def half(s, e):
        assert e["chase_dt"][0][0] == 30 * DT and e["chases"][0][0] == 0.75 and e["flags"][0][0] == 0
    out.append(case("half as deep", t, flat[3], 1e-3, [1000.0], [t[100]], [2], [2], [40], [8], [0.625], check=half,
                    chase_fraction=0.5))

    # ---- point share: a single low sample between two high ones
    one = numpy.ones(400)
    one[100] -= 1e-2
    one[99] += 1e-3
    one[101] += 1e-3

    def point(s, e):
        assert e["point_share"][0][0] > 1 and int(e["flags"][0][0]) & 2
    out.append(case("point share", t, one, 1e-3, [1000.0], [t[100]], [2], [2], [40], [7], [1.0], check=point))

    # ---- every flag bit alone
    bits = numpy.ones((4, 400))
    bits[0, 98:103] -= 4e-3                           # 1: a clean dip under a min_ses nothing reaches (its own call below)
    bits[1, 100] -= 1e-2                              # 2: one sample
    bits[2, 98:103] -= 4e-3
    bits[2, 103:108] -= 3.2e-3                        # 4: the flux stays down behind the dip
    bits[3, 98:103] -= 4e-3
    bits[3, 118:123] -= 4e-3                          # 8: a twin 20 samples on

    def flags(s, e):
        assert e["flags"][:, 0].tolist() == [0, 2, 4, 8], e["flags"][:, 0]
        assert e["after"][2][0] > 0.5 and e["before"][2][0] == 0 and s["n_good"].tolist() == [1, 0, 0, 0]
    out.append(case("flags 2, 4, 8", t, bits, 1e-3, 1000.0, t[100], 2, 2, 40, 7, 1.0, check=flags))

    def weak(s, e):
        assert e["flags"][0][0] == 1 and s["n_held"][0] == 1 and s["n_good"][0] == 0
        assert numpy.isnan(s["mes_good"][0]) and numpy.isnan(s["mes_rest"][0]) and s["dominance"][0] == 1.0
    out.append(case("flag 1, n_good 0, n_held 1", t, bits[0], 1e-3, [1000.0], [t[100]], [2], [2], [40], [7], [1.0], check=weak,
                    min_ses=inf))

    # ---- the summary's edge counts and ties
    def nothing(s, e):
        assert s["status"][0] == 0 and s["n_epochs"][0] == 5 and s["n_held"][0] == 0 and s["n_good"][0] == 0
        assert all(numpy.isnan(s[k][0]) for k in spec.SUMMARY_FIELDS[5:]) and (e["status"][0][:5] == 1).all()
        assert numpy.isnan(e["n_chased"][0]).all() and numpy.isnan(e["flags"][0]).all()
    out.append(case("n_held 0", t, numpy.ones(400), 1e-3, [P], [T0], [2], [4], [20], [7], [0.5], check=nothing))
    twins = dips(t, P, T0, 5, depth=5e-3, sigma=0)

    def tie(s, e):
        assert s["n_held"][0] == 5 and len(set(held(e)["ses"].tolist())) == 1 and s["ses_max_epoch"][0] == 0
        assert s["depth_chi2"][0] == 0 and s["n_good"][0] == 5 and s["mes_rest"][0] < s["mes"][0] == s["mes_good"][0]
    out.append(case("a tie in ses_max", t, twins, 1e-3, [P], [T0], [2], [2], [20], [7], [0.5], check=tie))

    # ---- unit counts against the workgroup's threads, per-point dy throughout
    t = series(650)
    rng = numpy.random.RandomState(8)
    dy = rng.uniform(5e-4, 2e-3, (2, 650))
    P40, P3 = 16 * DT, 300 * DT
    y = numpy.array([dips(t, P40, t[5], 5, seed=9), dips(t, P3, t[20], 37, seed=10)])

    def units(s, e):
        assert s["n_epochs"].tolist() == [41, 3, 41, 3] and (s["n_held"] >= [30, 2, 30, 2]).all()
        assert held(e, 0)["n_chased"].max() == 650 - 4 - 2 * 2 - 1 and (held(e, 1)["n_chased"] <= 2).all()
    out.append(case("units", t, y, dy, [P40, P3, P40, P3], [t[5], t[20], t[5], t[20]], [2, 4, 0, 4], [8, 1, 100, 4096],
                    [8192, 2, 300, 8192], [2, 1, 3, 37], [0.1, 0.5, 0.1, 0.5], curve=[0, 1, 0, 1], check=units))

    # ---- the epoch limit and bad ephemerides
    t = series(300)
    P = 24 * DT
    y = dips(t, P, t[0], 5, seed=7)
    period = [P, P, nan, inf, 0.0, -1.0, P, P, P, 5000.0, 5e-324, 1e300]
    T0s = [t[0], t[0] - 24 * DT, 1.0, 1.0, 1.0, 1.0, nan, inf, -inf, 0.3, 1.0, 1.0]

    def limit(s, e):
        assert s["status"].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 2, 0]
        assert s["n_epochs"][0] == 13 and s["epoch_first"][1] == 1 and s["n_epochs"][9] == 0 and s["n_epochs"][10] == inf
        assert s["n_epochs"][11] == 1 and e["time_linear"][11][0] == 1.0
        assert numpy.isnan(e["epoch"][2:11]).all() and not numpy.isnan(e["epoch"][:2]).any()
        assert numpy.isnan(s["n_held"][2:11]).all() and numpy.isnan(s["epoch_first"][2:11]).all()
    out.append(case("limit 13", t, y, 1e-3, period, T0s, 0, 2, 10, 4, 0.1, curve=numpy.zeros(12, dtype=int), check=limit,
                    max_epochs=13))

    def over(s, e):
        assert s["status"].tolist() == [2, 2] and s["n_epochs"].tolist() == [13, 13]
        assert numpy.isnan(e["epoch"]).all() and numpy.isnan(s["n_held"]).all()
    out.append(case("limit 12", t, y, 1e-3, period[:2], T0s[:2], 0, 2, 10, 4, 0.1, curve=[0, 0], check=over, max_epochs=12))
    return out


def many_candidates():
    """1030 candidates over 5 curves: more than one slab."""
    n = 257
    t = series(n)
    rng = numpy.random.RandomState(11)
    P = 64 * DT
    y = numpy.array([dips(t, P, t[10 + 3 * i], 5, seed=20 + i) for i in range(5)])
    n_fits = 1030
    curve = rng.randint(0, 5, n_fits)
    period = numpy.where(rng.uniform(size=n_fits) < 0.1, P / 2, P)
    T0 = t[10 + 3 * curve] + rng.randint(-2, 3, n_fits) * DT / 4
    return case("slabs", t, y, 1e-3, period, T0, rng.randint(0, 4, n_fits), rng.randint(1, 6, n_fits), rng.randint(0, 25, n_fits),
                rng.randint(0, 12, n_fits), rng.uniform(0.05, 0.3, n_fits), curve=curve, max_epochs=9)
