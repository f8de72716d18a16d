"""CPU: the RRT batch's filter thresholds (oxhip_host.hpp: connect_grid_threshold, midpoint_threshold, star_edge_threshold,
filter_maxabs), the arithmetic refresh_filter and pair_params (oxhip_api.hip) build their filters from.  A stand-alone program with
its own main (tests/cpp/test_rrt_filter_host.cpp), built with AddressSanitizer and UBSan, prints inputs and results as bit patterns.
Here the three formulas are restated in plain float arithmetic -- the same IEEE operations in the same order as refresh_filter wrote
them out before they had names -- and compared bit for bit; and the thresholds are shown conservative with exact rationals: a sphere
is kept whenever d2 <= (r + h)^2, so the threshold must not lie below (r + h)^2 for any finite r >= 0."""
import math
import os
import struct
import subprocess
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


def f64(word):
    return struct.unpack("<d", struct.pack("<Q", int(word, 16)))[0]


def word(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def sqrt_le_threshold(r):
    """oxhip_host.hpp: the largest x with sqrt(x) <= r"""
    if math.isnan(r):
        return r
    if r < 0.0:
        return -1.0
    if math.isinf(r):
        return r
    x = r * r
    if math.isinf(x):
        x = 1.7976931348623157e308
    while math.sqrt(x) > r:
        x = math.nextafter(x, -1.0)
    while True:
        y = math.nextafter(x, INF)
        if math.isinf(y) or math.sqrt(y) > r:
            break
        x = y
    return x


def connect(r):
    t = sqrt_le_threshold(r)
    if not math.isfinite(t):
        return t
    return t * (1.0 + 1e-9) if t > 0.0 else t


def midpoint(r, h):
    if math.isnan(r) or math.isinf(r):
        return -1.0 if r < 0.0 else INF
    if r < 0.0:
        return -1.0
    return (r + h) * (r + h) * (1.0 + 1e-9)


def star(r, h_lo, h_hi):
    if math.isnan(r) or math.isinf(r):
        return INF
    a = (r + h_lo) * (r + h_lo)
    c = (r + h_hi) * (r + h_hi)
    return max(a, c) * (1.0 + 1e-9) * (1.0 + 1e-12)


def test_filter_thresholds_bit_for_bit_and_conservative(tmp_path):
    exe = str(tmp_path / "test_rrt_filter_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_rrt_filter_host.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "rrt filter thresholds: done"
    seen = {"connect": [], "midpoint": [], "star": []}
    maxabs = {}
    for line in lines[:-1]:
        kind, *words = line.split()
        if kind == "maxabs":
            maxabs[words[0]] = f64(words[1])
            continue
        *args, got = [f64(w) for w in words]
        want = dict(connect=connect, midpoint=midpoint, star=star)[kind](*args)
        assert word(want) == word(got) or (math.isnan(want) and math.isnan(got)), (line, want, got)
        seen[kind].append(args)
        rad, hs = args[0], args[1:]
        if kind == "connect" and rad >= 0.0:
            # the state test is "valid iff d2 > sqrt_le_threshold(r)", in floating point: every d2 that hits is at or below the grid's
            assert got >= sqrt_le_threshold(rad), (line, got)
        elif math.isfinite(rad) and rad >= 0.0:   # conservative, exactly: no rounding of the threshold's own arithmetic cuts into the ball
            for h in hs:
                assert Fraction(got) >= (Fraction(rad) + Fraction(h)) ** 2, (line, got)
        elif rad < 0.0 and kind != "star":
            assert got == -1.0                  # never hit: no squared distance lies below it
    # the cases the program has to cover
    radii = [a[0] for a in seen["connect"]]
    assert any(v < 0.0 and math.isfinite(v) for v in radii) and 0.0 in radii and any(math.isnan(v) for v in radii)
    assert INF in radii and -INF in radii and 1e150 in radii and any(0.0 < v < 10.0 for v in radii)
    assert sorted(map(word, radii)) == sorted(set(word(a[0]) for a in seen["midpoint"])) == sorted(set(word(a[0]) for a in seen["star"]))
    assert len({a[1] for a in seen["midpoint"]}) >= 3 and any(a[1] < a[2] for a in seen["star"])
    # the margin: the largest magnitude among what the caller names, never below 1; bounds beyond 2 * dim are not read
    assert maxabs == {"bounds": 20.5, "bounds+centres": 30.25, "bounds+centres+starts": 55.5, "bounds+starts": 55.5, "small": 1.0}
