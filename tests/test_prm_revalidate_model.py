"""CPU: a Python model of oxhip_prm_revalidate's bookkeeping (prm_revalidate.hip) -- pair emission per CSR
entry, the mirror entry found by binary search, the exclusive scan over the keep bytes and the compaction -- against the plain
filter "keep {i < j} iff valid[i], valid[j] and ok(j, i)", on random symmetric CSRs with empty rows, rows longer than 256 and
cases in which everything goes.  The model works entry by entry, in a shuffled order where the device's order is free."""
import bisect
import random
import zlib

import pytest


def random_csr(rnd, n, p, hub=None):
    adj = [set() for _ in range(n)]
    for j in range(n):
        for i in range(j):
            if rnd.random() < p:
                adj[j].add(i)
                adj[i].add(j)
    if hub is not None:
        for v in range(n):
            if v != hub:
                adj[hub].add(v)
                adj[v].add(hub)
    offsets, nbrs = [0], []
    for u in range(n):
        nbrs.extend(sorted(adj[u]))
        offsets.append(len(nbrs))
    return offsets, nbrs


def row_of(offsets, n, e):
    """row_of (prm_csr.hpp): the last u with offsets[u] <= e"""
    lo, hi = 0, n
    while hi - lo > 1:
        mid = lo + ((hi - lo) >> 1)
        if offsets[mid] <= e:
            lo = mid
        else:
            hi = mid
    return lo


def find(offsets, nbrs, row, want):
    """row_find (prm_csr.hpp): the entry of `row` that holds `want`"""
    lo, hi = offsets[row], offsets[row + 1]
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if nbrs[mid] < want:
            lo = mid + 1
        else:
            hi = mid
    return lo if lo < offsets[row + 1] and nbrs[lo] == want else None


def model(offsets, nbrs, valid, ok, rnd):
    n, E = len(offsets) - 1, len(nbrs)
    pairs = []
    for e in range(E):                                     # emit: one "thread" per entry
        u, v = row_of(offsets, n, e), nbrs[e]
        if v < u and valid[u] and valid[v]:
            pairs.append((e, u, v))
    assert len(pairs) <= E // 2
    rnd.shuffle(pairs)                                     # the order of the list is free
    keep = [0] * E
    for e, u, v in pairs:                                  # check: own entry and the mirror
        if ok(u, v):
            keep[e] = 1
            m = find(offsets, nbrs, v, u)
            assert m is not None
            keep[m] = 1
    pos, run = [], 0
    for k in keep:                                         # exclusive scan
        pos.append(run)
        run += k
    out = [None] * run
    for e in range(E):
        if keep[e]:
            out[pos[e]] = nbrs[e]
    new_off = [pos[o] if o < E else (pos[E - 1] + keep[E - 1] if E else 0) for o in offsets]
    return new_off, out


def plain(offsets, nbrs, valid, ok):
    n = len(offsets) - 1
    rows = [[] for _ in range(n)]
    for j in range(n):
        for i in nbrs[offsets[j]:offsets[j + 1]]:
            if i < j and valid[i] and valid[j] and ok(j, i):
                rows[j].append(i)
                rows[i].append(j)
    off, out = [0], []
    for r in rows:
        out.extend(sorted(r))
        off.append(len(out))
    return off, out


CASES = [("sparse", 300, 0.01, None), ("dense", 120, 0.4, None), ("hub_300", 301, 0.005, 7), ("hub_last", 290, 0.0, 289),
         ("no_edges", 70, 0.0, None), ("one", 1, 0.0, None), ("two", 2, 1.0, None)]


@pytest.mark.parametrize("name,n,p,hub", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("mode", ["random", "all_kept", "all_motions_fail", "all_milestones_invalid"])
def test_model_equals_plain_filter(name, n, p, hub, mode):
    rnd = random.Random(zlib.crc32((name + "/" + mode).encode()))
    offsets, nbrs = random_csr(rnd, n, p, hub)
    if hub is not None:
        assert offsets[hub + 1] - offsets[hub] > 256
    if name in ("sparse", "no_edges"):
        assert any(offsets[u] == offsets[u + 1] for u in range(n))   # empty rows
    valid = [mode != "all_milestones_invalid" and (mode != "random" or rnd.random() < 0.85) for _ in range(n)]
    verdict = {}

    def ok(u, v):   # asked from the higher index to the lower, once per undirected edge
        assert v < u
        if (u, v) not in verdict:
            verdict[(u, v)] = mode == "all_kept" or (mode == "random" and rnd.random() < 0.7)
        return verdict[(u, v)]

    got = model(offsets, nbrs, valid, ok, rnd)
    want = plain(offsets, nbrs, valid, ok)
    assert got == want
    new_off, out = got
    for u in range(n):
        row = out[new_off[u]:new_off[u + 1]]
        assert row == sorted(set(row)) and (valid[u] or not row)
        for v in row:   # still symmetric
            at = bisect.bisect_left(out, u, new_off[v], new_off[v + 1])
            assert at < new_off[v + 1] and out[at] == u
    if mode == "all_kept":
        assert got == (offsets, nbrs)
    if mode in ("all_motions_fail", "all_milestones_invalid"):
        assert out == [] and set(new_off) == {0}
