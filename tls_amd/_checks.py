"""The argument checks of the host layer: the vocabulary every `*_arguments`, `*_options`, `*_tables` and `*_rows` function
of _lib and survey composes.  Plain functions, GPU-free, numpy only.  Each takes the heading `what` of the stage first (None:
no heading), returns the checked value in the form the library takes (float, int, contiguous float64 or int64 arrays) and
raises ValueError otherwise; the messages are formatted here and nowhere else.  A new stage names its checks from these; it
does not copy a neighbour's."""
import numbers
import operator

import numpy

INF = numpy.inf
MAX_ROW_POINTS = 100000000   # the longest row of the entries without a limit of their own; the messages write it 1e8


def refusal(what, text):
    """The ValueError of a stage: `text` headed `what`."""
    return ValueError(text if what is None else "%s: %s" % (what, text))


def _count(n):
    return "1e8" if n == MAX_ROW_POINTS else "%d" % n


# ---- scalars ---------------------------------------------------------------------------------------------------------------
def real(what, name, value, text="must be a number"):
    """value as a float: a numbers.Real and no bool."""
    if isinstance(value, (bool, numpy.bool_)) or not isinstance(value, numbers.Real):
        raise refusal(what, "%s %s, got %r" % (name, text, value))
    return float(value)


def _inside(what, name, value, inside, text):
    """value as a float where inside(it) holds; "<name> <text>, got <value>" for any other, a bool and a non-number."""
    v = real(what, name, value, text)
    if not inside(v):
        raise refusal(what, "%s %s, got %r" % (name, text, value))
    return v


def finite_at_least(what, name, value, low=0.0, text=None):
    """value as a float: low <= value < inf."""
    return _inside(what, name, value, lambda v: low <= v < INF, text or "must be finite and >= %g" % low)


def finite_positive(what, name, value, text="must be finite and > 0"):
    """value as a float: 0 < value < inf."""
    return _inside(what, name, value, lambda v: 0.0 < v < INF, text)


def finite(what, name, value):
    """value as a float: no NaN and no infinity."""
    return _inside(what, name, value, lambda v: -INF < v < INF, "must be finite")


def not_negative(what, name, value):
    """value as a float: value >= 0, +inf included."""
    return _inside(what, name, value, lambda v: v >= 0.0, "must be a number >= 0")


def positive(what, name, value, text="must be a number > 0"):
    """value as a float: value > 0, +inf included."""
    return _inside(what, name, value, lambda v: v > 0.0, text)


def within(what, name, value, low, high, low_open=False, text=None):
    """value as a float in [low, high], or in (low, high] where low_open."""
    return _inside(what, name, value, lambda v: (low < v if low_open else low <= v) and v <= high,
                   text or "must be a number in %s%g, %g]" % ("(" if low_open else "[", low, high))


def no_nan(what, name, value, text="must be a number and no NaN"):
    """value as a float: any number but a NaN, the infinities included."""
    return _inside(what, name, value, lambda v: v == v, text)


def integer(what, name, value, low=None, high=None, text=None):
    """value as an int: a numbers.Integral and no bool, in [low, high] (None: no bound on that side)."""
    if text is None:
        text = "must be an integer" + ("" if low is None else " >= %d" % low if high is None else " in [%d, %d]" % (low, high))
    if isinstance(value, (bool, numpy.bool_)) or not isinstance(value, numbers.Integral) \
            or not ((low is None or low <= int(value)) and (high is None or int(value) <= high)):
        raise refusal(what, "%s %s, got %r" % (name, text, value))
    return int(value)


def index(what, name, value, low, high, high_text):
    """value as an int in [low, high] by operator.index: anything that is an integer, a bool excepted."""
    try:
        if isinstance(value, (bool, numpy.bool_)):
            raise TypeError
        v = operator.index(value)
    except TypeError:
        raise refusal(what, "%s must be an integer, got %r" % (name, value))
    if not low <= v <= high:
        raise refusal(what, "%s must be in [%d, %s], got %d" % (name, low, high_text, v))
    return v


# ---- the time stamps and the rows over them --------------------------------------------------------------------------------
def time_values(what, t, order="non-decreasing", name="t"):
    """Refuses time stamps that are not finite or not in `order` ("non-decreasing" and "ascending" both admit ties; None:
    any order)."""
    if not numpy.all(numpy.isfinite(t)) or (order is not None and not numpy.all(t[1:] >= t[:-1])):
        raise refusal(what, "%s must be finite%s" % (name, "" if order is None else " and " + order))


def times(what, t, max_points, min_points=1, order="non-decreasing"):
    """t as contiguous float64 [n]: 1-D, n in [min_points, max_points], finite and in `order`."""
    t = numpy.asarray(t, dtype=numpy.float64)
    if t.ndim != 1 or not min_points <= len(t) <= max_points:
        raise refusal(what, "t must have shape [n] with n in [%d, %s], got %s" % (min_points, _count(max_points), t.shape))
    time_values(what, t, order)
    return numpy.ascontiguousarray(t)


def over_t(what, names, tail=""):
    """The refusal of rows that do not lie over the time stamps."""
    return refusal(what, "%s must be [n] or [n_curves, n] over the time stamps t [n]%s" % (names, tail))


def row_shapes(what, t, y, dy=None, names=None, tail=""):
    """(y, dy) as float64 [n_curves, n] over t [n] (None: any n): a row [n] becomes [1, n]; dy None stays None, another has
    y's shape."""
    y = numpy.asarray(y, dtype=numpy.float64)
    dy = None if dy is None else numpy.asarray(dy, dtype=numpy.float64)
    if y.ndim == 1:
        y = y[None, :]
    if dy is not None and dy.ndim == 1:
        dy = dy[None, :]
    if y.ndim != 2 or (t is not None and (numpy.ndim(t) != 1 or y.shape[1] != len(t))) or (dy is not None and dy.shape != y.shape):
        raise over_t(what, names or ("y" if dy is None else "y and dy"), tail)
    return y, dy


def row_values(what, y, dy=None, noun="y"):
    """(y, dy) contiguous: y finite, dy (unless None) finite and > 0.  `noun` is what the message calls y."""
    if y.size and not numpy.all(numpy.isfinite(y)):
        raise refusal(what, "%s has a NaN or an infinite value" % noun)
    # (min and max propagate a NaN, which then fails both comparisons)
    if dy is not None and dy.size and not (dy.min() > 0.0 and dy.max() < INF):
        raise refusal(what, "dy has a NaN, infinite or non-positive value")
    return numpy.ascontiguousarray(y), None if dy is None else numpy.ascontiguousarray(dy)


def rows(what, t, y, dy):
    """(y, dy) of a stage that needs both: row_shapes, then row_values; a dy of None is refused as a dy of another shape is."""
    return row_values(what, *row_shapes(what, t, y, numpy.asarray(dy, dtype=numpy.float64)))


def flux_rows(what, t, y):
    """y of a stage that takes no dy: row_shapes, then row_values."""
    return row_values(what, *row_shapes(what, t, y))[0]


def positive_values(what, rows, noun, who):
    """Refuses rows of `who`'s `noun` with a value that is not finite and > 0 (min and max propagate a NaN, which fails both
    comparisons)."""
    if rows.size and not (rows.min() > 0.0 and rows.max() < INF):
        raise refusal(what, "%s has a NaN, infinite or non-positive value: %s needs %s > 0" % (noun, who, noun))


# ---- the candidates --------------------------------------------------------------------------------------------------------
def floats(what, values, text):
    """Every one of `values` as a contiguous float64 array of at least one dimension; the refusal says `text`."""
    try:
        return [numpy.ascontiguousarray(numpy.atleast_1d(numpy.asarray(v, dtype=numpy.float64))) for v in values]
    except (TypeError, ValueError):
        raise refusal(what, text)


def columns(what, names, values):
    """The candidates' columns `values` as contiguous float64 [n_fits], any value; `names` is what the messages call them."""
    values = floats(what, values, "%s must be numbers" % names)
    if values[0].ndim != 1 or any(v.shape != values[0].shape for v in values):
        raise refusal(what, "%s must be [n_fits]" % names)
    return values


def indices(what, name, values, shape, count, noun="index"):
    """values as contiguous int64 of `shape`: one integer in [0, count) a candidate."""
    v = numpy.atleast_1d(numpy.asarray(values))
    if v.shape != shape or (v.size and (v.dtype.kind not in "iu" or v.min() < 0 or v.max() >= count)):
        raise refusal(what, "%s must hold one %s in [0, %d) a candidate" % (name, noun, count))
    return numpy.ascontiguousarray(v, dtype=numpy.int64)


def one_a_curve(what, n_fits, n_curves):
    """The refusal of curve=None where the candidates are not one a light curve."""
    return refusal(what, "curve=None takes one candidate a light curve: %d candidates, %d curves" % (n_fits, n_curves))


def curves(what, curve, n_fits, n_curves):
    """curve as contiguous int64 [n_fits] in [0, n_curves); None: one candidate a light curve, in order."""
    if curve is None:
        if n_fits != n_curves:
            raise one_a_curve(what, n_fits, n_curves)
        curve = numpy.arange(n_curves)
    return indices(what, "curve", curve, (n_fits,), n_curves)


def candidates(what, period, T0, duration, curve, n_curves):
    """(period, T0, duration, curve) of the candidates of n_curves light curves: columns and curves."""
    period, T0, duration = columns(what, "period, T0 and duration", (period, T0, duration))
    return period, T0, duration, curves(what, curve, len(period), n_curves)


def integer_columns(what, shape, columns, noun="candidate"):
    """{name: contiguous int64 of `shape`} of the (name, values, lo, hi) in `columns`: one integer in [lo, hi] a `noun` (hi
    None: any int64 from lo up)."""
    out = {}
    for name, v, lo, hi in columns:
        v = numpy.atleast_1d(numpy.asarray(v))
        if v.ndim != 1 or v.shape != shape or (v.size and v.dtype.kind not in "iu"):
            raise refusal(what, "%s must hold one integer a %s" % (name, noun))
        if v.size and (v.min() < lo or (hi is not None and v.max() > hi)):
            raise refusal(what, "%s out of range [%d, %s]" % (name, lo, "2^63)" if hi is None else "%d" % hi))
        out[name] = numpy.ascontiguousarray(v, dtype=numpy.int64)
    return out


def float_column(what, name, values, shape, noun, above=">=", not_numbers="must hold numbers"):
    """values as contiguous float64 of `shape`: one finite value >= 0 (above=">": > 0) a `noun`."""
    v, = floats(what, [values], "%s %s" % (name, not_numbers))
    if v.shape != shape or not numpy.all(numpy.isfinite(v) & ((v > 0.0) if above == ">" else (v >= 0.0))):
        raise refusal(what, "%s must hold one finite value %s 0 a %s" % (name, above, noun))
    return v


# ---- tables ----------------------------------------------------------------------------------------------------------------
def table(what, name, values, ascending=True):
    """values as a contiguous float64 table [k], k >= 1, finite and (unless not `ascending`) non-decreasing."""
    try:
        v = numpy.ascontiguousarray(numpy.asarray(values, dtype=numpy.float64))
    except (TypeError, ValueError):
        raise refusal(what, "%s must hold numbers" % name)
    if v.ndim != 1 or len(v) < 1:
        raise refusal(what, "%s must be a table [k] with k >= 1, got shape %s" % (name, v.shape))
    time_values(what, v, "ascending" if ascending else None, name)
    return v


def fit_window(what, window, ratio, shift):
    """window as a float: finite and at least 0.5 * max(ratio) + max|shift|, so that the model lies inside it."""
    finite(what, "window", window)
    least = 0.5 * float(ratio[-1]) + max(abs(float(shift[0])), abs(float(shift[-1])))
    if not float(window) >= least:
        raise refusal(what, "window %r is below 0.5 * max(ratio) + max|shift| = %r: the model must lie inside it" % (window, least))
    return float(window)


# ---- decorrelation ---------------------------------------------------------------------------------------------------------
def regressors(what, shared, own, n_curves, n, max_terms, single=False):
    """(shared [n_shared, n], own [n_curves, n_own, n]) as contiguous float64, a None becoming an array without columns: at
    least one of the two given, every value finite, n_shared + n_own in [1, max_terms].  One shared series may be [n]; with
    `single` (the flux was one row) own is [n_own, n] or one series [n]."""
    if shared is None and own is None:
        raise refusal(what, "at least one of own and shared must be given")
    try:
        shared = numpy.zeros((0, n)) if shared is None else numpy.asarray(shared, dtype=numpy.float64)
        own = numpy.zeros((n_curves, 0, n)) if own is None else numpy.asarray(own, dtype=numpy.float64)
    except (TypeError, ValueError):
        raise refusal(what, "own and shared must hold numbers")
    if shared.ndim == 1:
        shared = shared[None, :]
    if shared.ndim != 2 or shared.shape[1] != n:
        raise refusal(what, "shared must be [n_shared, n] with n = %d, got %s" % (n, shared.shape))
    if single and own.ndim in (1, 2):
        own = own.reshape((1, -1, own.shape[-1]))
    if own.ndim != 3 or own.shape[0] != n_curves or own.shape[2] != n:
        raise refusal(what, "own must be [n_curves, n_own, n] = [%d, n_own, %d]%s, got %s"
                      % (n_curves, n, " or [n_own, n] for one row" if single else "", own.shape))
    m = shared.shape[0] + own.shape[1]
    if not 1 <= m <= max_terms:
        raise refusal(what, "n_shared + n_own must lie in [1, %d], got %d + %d" % (max_terms, shared.shape[0], own.shape[1]))
    if not (numpy.all(numpy.isfinite(shared)) and numpy.all(numpy.isfinite(own))):
        raise refusal(what, "own and shared must be finite")
    return numpy.ascontiguousarray(shared), numpy.ascontiguousarray(own)


def segments(what, values, n):
    """values as contiguous int64 [n_seg + 1]: integers ascending strictly from 0 to n; None: the one segment [0, n]."""
    if values is None:
        return numpy.array([0, n], dtype=numpy.int64)
    v = numpy.asarray(values)
    if v.ndim != 1 or len(v) < 2 or v.dtype.kind not in "iu" or v[0] != 0 or v[-1] != n or not numpy.all(v[1:] > v[:-1]):
        raise refusal(what, "segments must hold integers ascending strictly from 0 to n = %d, got %r" % (n, values))
    return numpy.ascontiguousarray(v, dtype=numpy.int64)


# ---- spline detrending -----------------------------------------------------------------------------------------------------
def spacings(what, values, most):
    """(values as contiguous float64 [k], single): one number or a sequence of 1 .. `most` numbers, each finite and > 0;
    `single` says it was one number."""
    single = numpy.ndim(values) == 0
    try:
        v = numpy.atleast_1d(numpy.asarray(values, dtype=numpy.float64))
    except (TypeError, ValueError):
        raise refusal(what, "knot_spacing must be a number or a sequence of numbers, got %r" % (values,))
    if isinstance(values, (bool, numpy.bool_)) or v.ndim != 1 or not 1 <= len(v) <= most:
        raise refusal(what, "knot_spacing must be a number or a sequence of 1 to %d numbers, got %r" % (most, values))
    if not numpy.all(numpy.isfinite(v) & (v > 0.0)):
        raise refusal(what, "every knot spacing must be finite and > 0, got %r" % (values,))
    return numpy.ascontiguousarray(v), single


def knot_segments(what, t, break_tolerance, spacing, max_coef):
    """The index boundaries [n_seg + 1] (int64) of the segments of t, a new one behind every gap t[j] - t[j-1] >
    break_tolerance; refuses a segment that takes more than max_coef coefficients at one of the spacings, q + 3 with
    q = max(1, ceil(span / spacing))."""
    starts = numpy.concatenate([[0], 1 + numpy.flatnonzero(t[1:] - t[:-1] > break_tolerance), [len(t)]]).astype(numpy.int64)
    span = t[starts[1:] - 1] - t[starts[:-1]]
    with numpy.errstate(all="ignore"):
        most = numpy.maximum(1.0, numpy.ceil(span.max() / spacing.min())) + 3.0
    if not most <= max_coef:
        raise refusal(what, "a segment of %g d takes %g coefficients at a knot spacing of %g d, more than SPLINE_MAX_COEF = %d"
                      % (span.max(), most, spacing.min(), max_coef))
    return numpy.ascontiguousarray(starts)
