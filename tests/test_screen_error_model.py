"""CPU: the binary32 screens' error models against exact arithmetic.

Each screen is restated operation by operation as its kernel does it, every binary32 operation rounded correctly from its
exact rational value (subnormals included), and the bound written next to the kernel is checked against the exact distance:

* the stream screen (screen_scan / screen_margins / screen_threshold, rrt_device.hpp; stream kernel, RRT*, RRTConnect, and
  the PRM host twin host_screen_threshold in prm_kernels.hip):
      e_k = fl32(fl32(c_k) - fl32(q_k)),  v = fma(e_D-1, e_D-1, ... fma(e_1, e_1, e_0 * e_0))
      sqrt(v)(1 - R) - A <= d <= sqrt(v)(1 + R) + A,  A = sqrt(D) 4.1 u M + 1e-18,  R = 2^-19 + (D + 2) u
* the dot-product screen (rrt_lanes.hip, and the same margins in rrt_cells.hip):
      a = fl32(x - c0), cc = fl32(sum_k (double) a_k^2), Q = -2 fl32(q - c0), s' = fma chain cc + a . Q,
      |b|^2 = sum_k (double) b_k^2 (binary64),  |d^2 - (s' + |b|^2)| <= E = u H^2 D (3D + 9) (+ the binary32 underflow term)

over D = 1..8 and magnitudes 1e-158 .. 1e100: random pairs, heavy cancellation, per-coordinate extremes, clusters far from
the origin, coordinates that are binary32 subnormals and squares that underflow.  No GPU is involved."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np
import pytest

U = 2.0 ** -24
F32_MAX = Fraction(float(np.finfo(np.float32).max))

MAGS = [1e-158, 1e-120, 1e-80, 1e-60, 1e-46, 1e-44, 1e-42, 1e-40, 1e-39, 1e-38, 1e-36, 1e-30, 1e-26, 1e-25, 1e-24, 1e-23,
        1e-22, 1e-21, 1e-20, 1e-19, 1e-18, 1e-15, 1e-12, 1e-6, 1.0, 7.0, 1e3, 1e6, 1e10, 1e14, 5e14, 9.9e14]
HUGE = [1e15, 1e18, 1e30, 1e60, 1e100]


# ------------------------------------------------------------------------------------------ correctly rounded binary32
def _f32_neighbours(f):
    return (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf)))


def rn32(x):
    """x (a Fraction or a float) rounded to nearest-even binary32, subnormals included; +-inf beyond the range."""
    x = Fraction(x)
    if abs(x) > F32_MAX:   # (all values here stay far from the half-ulp above FLT_MAX)
        return np.float32(math.copysign(np.inf, x))
    f = np.float32(float(x))   # at most one binary32 ulp off: float(x) rounds once, the binary32 conversion once more
    best, best_err = None, None
    for c in _f32_neighbours(f):
        if not np.isfinite(c):
            continue
        err = abs(Fraction(float(c)) - x)
        if best is None or err < best_err or (err == best_err and (int(c.view(np.uint32)) & 1) == 0):
            best, best_err = c, err
    return best


def fma32(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return np.float32(np.inf)   # (only squares reach this: +inf stays +inf)
    return rn32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_rn32_rounds_like_the_hardware():
    rng = np.random.default_rng(4)
    # exact binary32 products / sums against numpy's own binary32 arithmetic (single rounding), normal and subnormal
    for scale in (1.0, 1e-20, 1e-22, 1e-40, 1e20):
        a = (rng.standard_normal(300) * scale).astype(np.float32)
        b = (rng.standard_normal(300)).astype(np.float32)
        for x, y in zip(a, b):
            assert rn32(Fraction(float(x)) * Fraction(float(y))).view(np.uint32) == (x * y).view(np.uint32)
            assert rn32(Fraction(float(x)) - Fraction(float(y * np.float32(scale)))).view(np.uint32) == \
                (x - y * np.float32(scale)).view(np.uint32)
    # ties to even, and the subnormal grid
    tiny = Fraction(1, 2 ** 149)
    assert rn32(tiny / 2) == 0.0 and rn32(3 * tiny / 2) == np.float32(2 * 2.0 ** -149)
    assert rn32(Fraction(1) + Fraction(1, 2 ** 24)) == np.float32(1.0)
    assert rn32(Fraction(1) + Fraction(3, 2 ** 24)) == np.float32(1.0 + 2.0 ** -22)
    # a value that double rounding (binary64, then binary32) gets wrong
    x = Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)
    assert float(np.float32(float(x))) == 1.0 and rn32(x) == np.float32(1.0 + 2.0 ** -23)


# ----------------------------------------------------------------------------------- stream screen (rrt_device.hpp)
def screen_margins(m_all, dim):
    """rrt_device.hpp screen_margins: (usable, a2, r_lo, r_hi), binary64 as the kernel computes them"""
    m = m_all * 1.001
    usable = m < 1e15
    a2 = 2.0 * (math.sqrt(float(dim)) * 4.1 * U * m + 1e-18)
    r2 = 2.0 * (2.0 ** -19 + float(dim + 2) * U)
    return usable, a2, 1.0 - r2, 1.0 + r2


def screen_threshold(mg, r):
    usable, a2, _, r_hi = mg
    if not usable or not (r < 1e18):
        return np.float32(np.inf)
    d = (r * (1.0 + 1e-12) + a2) * r_hi * r_hi
    return np.float32(d * d * (1.0 + 2.0 ** -20))


def host_screen_threshold(m_all, dim, thr):
    """prm_kernels.hip host_screen_threshold (the PRM's host twin of the two above)"""
    m = m_all * 1.001
    if not (m < 1e15) or not (thr >= 0.0):
        return np.float32(np.inf)
    r = math.sqrt(thr)
    if not (r < 1e18):
        return np.float32(np.inf)
    a2 = 2.0 * (math.sqrt(float(dim)) * 4.1 * U * m + 1e-18)
    r_hi = 1.0 + 2.0 * (2.0 ** -19 + float(dim + 2) * U)
    d = (r * (1.0 + 1e-12) + a2) * r_hi * r_hi
    return np.float32(d * d * (1.0 + 2.0 ** -20))


def stream_screen(node, query):
    """screen_scan: e = fl32(node) - fl32(query) in binary32, s = e0 * e0, then one binary32 FMA per further coordinate"""
    e = [rn32(Fraction(float(rn32(c))) - Fraction(float(rn32(q)))) for c, q in zip(node, query)]
    s = rn32(Fraction(float(e[0])) ** 2)
    for k in range(1, len(e)):
        s = fma32(e[k], e[k], s)
    return s


def exact_d2(a, b):
    return sum((Fraction(x) - Fraction(y)) ** 2 for x, y in zip(a, b))


def _dec(fr):
    return Decimal(fr.numerator) / Decimal(fr.denominator)


# ----------------------------------------------------------------------------- pairs where screens go wrong
def _pairs(dim, mag, rng):
    """(node, query) pairs of binary64 coordinates of magnitude <= ~mag"""
    out = []
    for _ in range(4):   # random pairs over [-mag, mag]^D
        out.append((rng.uniform(-mag, mag, dim), rng.uniform(-mag, mag, dim)))
    for _ in range(3):   # heavy cancellation: the pair is a relative 2^-10 .. 2^-40 apart
        a = rng.uniform(-mag, mag, dim)
        out.append((a, a * (1.0 + rng.standard_normal(dim) * 2.0 ** -rng.integers(10, 41))))
    for _ in range(2):   # a cluster far from the origin (an offset frame): extent 1e-3 .. 1e-7 of the offset
        o = rng.uniform(0.5, 1.0, dim) * mag * rng.choice([-1.0, 1.0])
        w = mag * 10.0 ** -rng.integers(3, 8)
        out.append((o + rng.uniform(-w, w, dim), o + rng.uniform(-w, w, dim)))
    for k in range(dim):   # per-coordinate extremes: one coordinate spans [-mag, mag], the others tiny or zero
        a, b = rng.uniform(-1, 1, dim) * mag * 1e-9, np.zeros(dim)
        a[k], b[k] = mag, -mag
        out.append((a, b))
    a = rng.uniform(-mag, mag, dim)   # identical but for the last coordinate's last bit
    b = a.copy()
    b[-1] = np.nextafter(b[-1], np.inf)
    out.append((a, b))
    out.append((a, a.copy()))          # identical
    return out


MODEL_DIMS = list(range(1, 9))


@pytest.mark.parametrize("dim", MODEL_DIMS)
def test_stream_screen_bounds_hold_exactly(dim):
    rng = np.random.default_rng(1000 + dim)
    checked = 0
    with localcontext() as ctx:
        ctx.prec = 80
        for mag in MAGS:
            for node, query in _pairs(dim, mag, rng):
                m_all = max(float(np.max(np.abs(node))), float(np.max(np.abs(query))))
                mg = screen_margins(m_all, dim)
                assert mg[0], (dim, mag)
                v = stream_screen(node, query)
                assert np.isfinite(v)
                A, R = mg[1] / 2.0, (mg[3] - 1.0) / 2.0
                d2 = exact_d2(node, query)
                d = _dec(d2).sqrt()
                sv = _dec(Fraction(float(v))).sqrt()
                lo = sv * (1 - _dec(Fraction(R))) - _dec(Fraction(A))
                hi = sv * (1 + _dec(Fraction(R))) + _dec(Fraction(A))
                assert lo <= d <= hi, (dim, mag, list(node), list(query), float(v))
                # the threshold screens (RRT* neighbours, PRM pairs): a node within r never shows more than the threshold
                r = float(np.nextafter(math.sqrt(float(d2)), np.inf))
                if float(d2) > 0.0 and Fraction(r) ** 2 >= d2:
                    for rr in (r, r * (1.0 + 2.0 ** -30), 2.0 * r):
                        assert v <= screen_threshold(mg, rr), (dim, mag, rr)
                        assert v <= host_screen_threshold(m_all, dim, rr * rr), (dim, mag, rr)
                checked += 1
    assert checked >= len(MAGS) * (10 + dim)


@pytest.mark.parametrize("dim", MODEL_DIMS)
def test_stream_screen_is_unusable_wherever_squares_can_overflow(dim):
    # just inside the usable range the worst pair (every coordinate at +M against -M) keeps a finite binary32 square sum
    m = 1e15 / 1.001
    m = float(np.nextafter(m, 0.0))
    assert screen_margins(m, dim)[0]
    v = stream_screen(np.full(dim, m), np.full(dim, -m))
    assert np.isfinite(v) and Fraction(float(v)) <= F32_MAX
    # beyond it -- and for non-finite magnitudes -- the screen is off, and the thresholds are +inf
    for mag in HUGE + [float(np.nextafter(1e15 / 1.001, np.inf)), np.inf, np.nan]:
        mg = screen_margins(mag, dim)
        assert not mg[0], mag
        assert screen_threshold(mg, 1.0) == np.inf and host_screen_threshold(mag, dim, 1.0) == np.inf
    # wherever the worst pair's binary32 square sum overflows, the margins say unusable
    overflowed = 0
    for mag in np.geomspace(1e14, 1e37, 47):
        if not np.isfinite(stream_screen(np.full(dim, mag), np.full(dim, -mag))):
            assert not screen_margins(float(mag), dim)[0], mag
            overflowed += 1
    assert overflowed > 0


# ---------------------------------------------------------------------------- dot-product screen (rrt_lanes.hip / cells)
def lanes_e(h, dim):
    """lanes_screen_e (lane_query_common.hpp), E of rrt_lanes.hip / rrt_cells.hip: LMargins::e2 is 2E, the scanners' ballot
    threshold 2.5E.  The last term bounds the binary32 roundings in the subnormal range (2^-150 each, whatever the value)."""
    return U * h * h * float(dim * (3 * dim + 9)) * 1.0001 + 1e-290 + float(dim + 1) * 2.0 ** -149


def lanes_screen(x, q, c0):
    """(s', |b|^2): a = fl32(x - c0) (binary64 difference first), cc = fl32(sum (double) a_k^2), Q = -2 fl32(q - c0),
    s' = fma(a_{D-1}, Q_{D-1}, ... fma(a_0, Q_0, cc)), |b|^2 = sum (double) b_k^2 in binary64"""
    a = [rn32(float(xk - ck)) for xk, ck in zip(x, c0)]   # (x - c0: one binary64 rounding)
    sq = 0.0
    for f in a:
        sq = sq + float(f) * float(f)
    s = rn32(sq)
    b = [rn32(float(qk - ck)) for qk, ck in zip(q, c0)]
    bb = 0.0
    for f in b:
        bb = bb + float(f) * float(f)
    for ak, bk in zip(a, b):
        s = fma32(ak, np.float32(-2.0) * bk, s)
    return s, bb


def _lanes_pairs(dim, mag, rng):
    """(node, query, c0): c0 the centre of the bounds, node and query within mag of it"""
    out = []
    for off in (0.0, 1e3 * mag, -5e4 * mag, 1e6 * mag):
        c0 = np.full(dim, off) + rng.uniform(-mag, mag, dim) * 0.1
        for x, q in _pairs(dim, mag, rng)[:9]:
            out.append((c0 + x, c0 + q, c0))
    return out


LANES_DIMS = [2, 3, 4, 5, 6]


@pytest.mark.parametrize("dim", LANES_DIMS)
def test_lanes_screen_bound_holds_exactly(dim):
    rng = np.random.default_rng(2000 + dim)
    checked = 0
    for mag in MAGS:
        for x, q, c0 in _lanes_pairs(dim, mag, rng):
            xs = np.array([float(v - c) for v, c in zip(x, c0)])
            qs = np.array([float(v - c) for v, c in zip(q, c0)])
            h = max(float(np.max(np.abs(xs))), float(np.max(np.abs(qs)))) * (1.0 + 2.0 ** -23) * 1.001
            if not (h < 1e15):
                continue
            E = lanes_e(h, dim)
            s, bb = lanes_screen(x, q, c0)
            assert np.isfinite(s)
            d2 = exact_d2(x, q)
            err = abs(d2 - (Fraction(float(s)) + Fraction(bb)))
            assert err <= Fraction(E), (dim, mag, float(err), E, list(x), list(q))
            checked += 1
    assert checked >= len(MAGS) * 30


@pytest.mark.parametrize("dim", LANES_DIMS)
def test_lanes_screen_separation_at_two_and_a_half_e(dim):
    """what the scanners' ballot relies on: a node whose s' exceeds another's by more than 2.5E is truly farther (here
    with both nodes drawn close to one query -- near-ties, clusters, subnormal coordinates and underflowing squares)"""
    rng = np.random.default_rng(3000 + dim)
    decided = 0
    for mag in MAGS:
        for off in (0.0, 1e6 * mag):
            c0 = np.full(dim, off)
            q = c0 + rng.uniform(-mag, mag, dim) * 0.5
            for _ in range(6):
                u = rng.standard_normal((2, dim))
                u /= np.linalg.norm(u, axis=1, keepdims=True)
                d = mag * (0.05 + 0.3 * rng.random())
                eps = 2.0 ** -rng.integers(2, 30)
                xa, xb = q + u[0] * d, q + u[1] * d * (1.0 + eps)
                xs = np.concatenate([xa - c0, xb - c0, q - c0])
                h = float(np.max(np.abs(xs))) * (1.0 + 2.0 ** -23) * 1.001
                E = lanes_e(h, dim)
                sa, _ = lanes_screen(xa, q, c0)
                sb, _ = lanes_screen(xb, q, c0)
                for (s1, x1), (s2, x2) in (((sa, xa), (sb, xb)), ((sb, xb), (sa, xa))):
                    if Fraction(float(s2)) > Fraction(float(s1)) + Fraction(2.5 * E):
                        assert exact_d2(x2, q) > exact_d2(x1, q), (dim, mag, off, eps)
                        decided += 1
    assert decided > 0


@pytest.mark.parametrize("dim", LANES_DIMS)
def test_lanes_screen_usable_range_keeps_binary32_finite(dim):
    h = float(np.nextafter(1e15, 0.0))
    c0 = np.zeros(dim)
    s, bb = lanes_screen(np.full(dim, h), np.full(dim, -h), c0)
    assert np.isfinite(s) and np.isfinite(bb)
    assert np.isfinite(np.float32(2.5 * lanes_e(h, dim)))
