"""CPU: the shortcut's dynamic programme (include/oxmpl_hip.h) as tests/simplify_helpers.py restates it,
against brute force over ALL subsequences of the raw path that keep both ends (L <= 10).  No kernel is involved: this pins the
model the GPU tests and the golden file compare with."""
import itertools
import random

import pytest

from simplify_helpers import expected_checks, shortcut_dp, span_of


def _brute(L, valid, dist, max_span):
    """every chain 0 = c_0 < c_1 < .. < c_m = L - 1 whose gaps are within the span and valid; cost = the left-to-right sum"""
    S = span_of(L, max_span)
    out = []
    for r in range(0, max(L - 2, 0) + 1):
        for mid in itertools.combinations(range(1, L - 1), r):
            chain = [0] + list(mid) + [L - 1] if L > 1 else [0]
            ok = True
            cost = 0.0
            for a, b in zip(chain, chain[1:]):
                if b - a > S or (b - a >= 2 and not valid(a, b)):
                    ok = False
                    break
                cost = cost + dist(a, b)
            if ok:
                out.append((cost, chain))
    return out


def _case(rng, L, integer_lengths, density):
    v = {(i, j): (j - i == 1) or rng.random() < density for i in range(L) for j in range(i + 1, L)}
    if integer_lengths:   # small integers: sums are exact and ties are common, so the tie rule decides the chain
        d = {k: float(rng.randint(1, 3)) for k in v}
    else:
        d = {k: rng.uniform(0.01, 2.0) for k in v}
    return (lambda i, j: v[(i, j)]), (lambda i, j: d[(i, j)])


@pytest.mark.parametrize("integer_lengths", [False, True])
def test_dp_equals_brute_force_over_all_subsequences(integer_lengths):
    rng = random.Random(1234 + integer_lengths)
    n_ties = 0
    for L in range(1, 11):
        for max_span in sorted({1, 2, 3, max(L - 1, 1), 0}):
            for density in (0.0, 0.3, 0.7, 1.0):
                for _ in range(3):
                    valid, dist = _case(rng, L, integer_lengths, density)
                    asked = []

                    def asking(i, j):
                        asked.append((i, j))
                        return valid(i, j)

                    idx, raw, cost, checks = shortcut_dp(L, asking, dist, max_span)
                    S = span_of(L, max_span)
                    # every pair within the span is asked exactly once, adjacent ones never
                    assert sorted(asked) == [(i, j) for i in range(L) for j in range(i + 2, min(i + S, L - 1) + 1)]
                    assert checks == len(asked) == expected_checks(L, max_span)
                    chains = _brute(L, valid, dist, max_span)
                    best = min(c for c, _ in chains)
                    assert cost == best                                   # binary64 addition is monotone: the DP is optimal
                    assert (cost, idx) in chains
                    assert idx[0] == 0 and idx[-1] == L - 1 and all(a < b for a, b in zip(idx, idx[1:]))
                    r = 0.0
                    for j in range(1, L):
                        r = r + dist(j - 1, j)
                    assert raw == r and cost <= raw
                    winners = [ch for c, ch in chains if c == best]
                    if integer_lengths:
                        # exact sums: among the cheapest chains the DP's is the one whose predecessors, read from the end,
                        # are lowest (ties keep the lowest i at every step)
                        assert idx == min(winners, key=lambda ch: ch[::-1])
                        n_ties += len(winners) > 1
                    elif len(winners) == 1:
                        assert idx == winners[0]
                    if max_span == 1:
                        assert idx == list(range(L)) and cost == raw
                    if density == 1.0 and max_span == 0 and L >= 2 and not integer_lengths:
                        assert len(idx) >= 2
    if integer_lengths:
        assert n_ties > 50   # the tie rule was exercised


def test_no_obstacles_gives_the_straight_line_when_the_triangle_inequality_holds():
    pts = [(0.0, 0.0), (1.0, 2.0), (2.0, -1.0), (3.0, 3.0), (5.0, 0.5)]
    dist = lambda i, j: ((pts[i][0] - pts[j][0]) ** 2 + (pts[i][1] - pts[j][1]) ** 2) ** 0.5  # noqa: E731
    idx, raw, cost, checks = shortcut_dp(len(pts), lambda i, j: True, dist)
    assert idx == [0, 4] and cost == dist(0, 4) and cost < raw and checks == 6
    assert shortcut_dp(1, None, None) == ([0], 0.0, 0.0, 0)
    assert shortcut_dp(0, None, None) == ([], 0.0, 0.0, 0)
    assert shortcut_dp(2, None, lambda i, j: 1.5) == ([0, 1], 1.5, 1.5, 0)
