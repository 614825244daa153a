"""SysRem as tls_sysrem states it (include/tls_amd.h), restated line by line in numpy for test_sysrem_host.py and
test_sysrem.py.  Every operation is one IEEE double operation, and the two reduction orders are the statement's: rowsum over
256 lanes and a fixed tree, colsum over chunks of 32 rows.  Both are explicit loops over the order (vectorised over the
lanes, the rows and the columns they do not order), so the device's result must equal this one bit for bit, the iteration
counts included."""
import numpy

LANES = 256
ROW_CHUNK = 32
MAX_COMPONENTS = 8
MAX_ITER = 1000


def rowsum(v):
    """The row sum of v [..., n] along its last axis: lane l adds v[l], v[l + 256], ... in ascending order from 0.0, then
    the tree p[l] = p[l] + p[l + s] for s = 128, 64, ..., 1."""
    v = numpy.asarray(v, dtype=numpy.float64)
    n = v.shape[-1]
    steps = -(-n // LANES)
    # (a lane's missing last element is +0.0: p + 0.0 == p, and p is never -0.0 -- the sum starts from +0.0)
    padded = numpy.zeros(v.shape[:-1] + (steps * LANES,))
    padded[..., :n] = v
    padded = padded.reshape(v.shape[:-1] + (steps, LANES))
    p = numpy.zeros(v.shape[:-1] + (LANES,))
    for s in range(steps):
        p = p + padded[..., s, :]
    s = LANES // 2
    while s >= 1:
        p = p[..., :s] + p[..., s:2 * s]
        s //= 2
    return p[..., 0]


def colsum(v):
    """The column sum of v [n_rows, ...] along its first axis: chunks of 32 consecutive rows, each summed in ascending row
    order from 0.0; the chunk sums added in ascending chunk order from 0.0."""
    v = numpy.asarray(v, dtype=numpy.float64)
    total = numpy.zeros(v.shape[1:])
    for first in range(0, v.shape[0], ROW_CHUNK):
        part = numpy.zeros(v.shape[1:])
        for i in range(first, min(first + ROW_CHUNK, v.shape[0])):
            part = part + v[i]
        total = total + part
    return total


def _ratio(num, den):
    """num / den, or 0.0 where den is not > 0."""
    ok = den > 0.0
    with numpy.errstate(all="ignore"):
        return numpy.where(ok, num / numpy.where(ok, den, 1.0), 0.0)


def fit(y, n_components=1, dy=None, max_iter=50, tol=1e-6):
    """(flat, trend, c [n_rows, K], a [K, n], iters [K]) of y [n_rows, n] (and dy of the same shape, or None)."""
    y = numpy.asarray(y, dtype=numpy.float64)
    n_rows, n = y.shape
    K = int(n_components)
    with numpy.errstate(all="ignore"):
        m = rowsum(y) / float(n)
        x = y / m[:, None] - 1.0
        if dy is not None:
            r = numpy.asarray(dy, dtype=numpy.float64) / m[:, None]
            w = 1.0 / (r * r)
        else:
            v = rowsum(x * x) / float(n)
            w = numpy.broadcast_to(_ratio(numpy.ones(n_rows), v)[:, None], x.shape)
        C = numpy.zeros((n_rows, K))
        A = numpy.zeros((K, n))
        iters = numpy.zeros(K, dtype=numpy.int64)
        for k in range(K):
            c = numpy.ones(n_rows)
            a_prev = numpy.zeros(n)
            for it in range(1, int(max_iter) + 1):
                a = _ratio(colsum((x * c[:, None]) * w), colsum((c * c)[:, None] * w))
                c = _ratio(rowsum((x * a[None, :]) * w), rowsum((a * a)[None, :] * w))
                iters[k] = it
                if numpy.max(numpy.abs(a - a_prev)) <= tol * numpy.max(numpy.abs(a)):
                    break
                a_prev = a
            x = x - c[:, None] * a[None, :]
            C[:, k] = c
            A[k] = a
        s = numpy.zeros((n_rows, n))
        for k in range(K):
            s = s + C[:, k][:, None] * A[k][None, :]
        trend = m[:, None] * (1.0 + s)
        flat = y / trend
    return flat, trend, C, A, iters


def trend_ok(trend):
    """Every trend value finite and > 0 (what tls_sysrem checks behind the device work)."""
    return bool(numpy.all(numpy.isfinite(trend) & (trend > 0.0)))
