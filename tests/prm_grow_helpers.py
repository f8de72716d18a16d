"""The host-side expectation of oxhip_prm_grow_roadmap, shared by its CPU and GPU tests.

expected_growth restates the edge rule and nothing else: a new milestone j gets the edge {i < j} iff i is live (an old milestone
that is valid now, or any milestone of this call), near(j, i) and motion(j -> i).  What "near" and "motion" are is the caller's: the
GPU tests pass the golden generators' distance and the RRT batch's check_motion, the CPU test passes hand-made tables."""
import numpy as np


def expected_growth(old_lists, n_total, live, near, motion):
    """old_lists: the rows of the roadmap before the call (n_old of them, entries < n_old); live: [n_old] bools;
    near(j, i) -> bool; motion(pairs) -> one bool per (j, i) of `pairs`.  -> the n_total rows after the call."""
    n_old = len(old_lists)
    assert len(live) == n_old and n_total >= n_old
    pairs = [(j, i) for j in range(n_old, n_total) for i in range(j) if (i >= n_old or live[i]) and near(j, i)]
    ok = list(motion(pairs)) if pairs else []
    assert len(ok) == len(pairs)
    rows = [list(r) for r in old_lists] + [[] for _ in range(n_total - n_old)]
    for (j, i), keep in zip(pairs, ok):   # j ascending, i ascending within j: every append is the row's largest entry so far
        if keep:
            rows[j].append(i)
            rows[i].append(j)
    return rows


def check_rows(rows):
    """the structure rules of a roadmap: no self-loop, every row strictly ascending, symmetric"""
    for u, row in enumerate(rows):
        assert u not in row and all(a < b for a, b in zip(row, row[1:])), u
        for v in row:
            assert u in rows[v], (u, v)


def make_near(states, n_old, radius, dist, so3=False):
    """near(j, i) = dist(states[j], states[i]) < radius, the new milestone first, by the golden generators' own distance; a numpy
    estimate with a 1 % margin spares the exact call for pairs far outside the radius"""
    s = np.asarray(states, dtype=np.float64)
    new = s[n_old:]
    if so3:
        approx = np.arccos(np.minimum(1.0, np.abs(new @ s.T)))
    else:
        approx = np.sqrt(((new[:, None, :] - s[None, :, :]) ** 2).sum(axis=2))
    maybe = approx < radius * 1.01 + 1e-6
    rows = s.tolist()

    def near(j, i):
        return bool(maybe[j - n_old, i]) and dist(rows[j], rows[i]) < radius
    return near


def rrt_motion(rrt, states):
    """motion(pairs) from an RRT batch's own check_motion, from = the new milestone j, to = the earlier one i"""
    s = np.asarray(states, dtype=np.float64)

    def motion(pairs):
        idx = np.array(pairs)
        return [bool(v) for v in rrt.check_motion(s[idx[:, 0]], s[idx[:, 1]])]
    return motion
