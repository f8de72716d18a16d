"""CPU: the planted graphs of tests/prm_components_shapes.py are what the GPU tests take them for, and the host model they are
compared with (components, host_prune) keeps its own rules.  Prints, per shape, n, entries, components and the largest size.

The issue asks for the 65,537-chain "with bit-reversed indices, so that finds are deep" and for a check that the permuted chain's
initial forest is deeper than 1,000.  Measured here: bit reversal leaves an initial forest of depth 2 (32,768 trees, so nearly
every entry has to hook -- that is what the shape is good for).  The deep forest comes from the chain in index order (depth
65,536, no hook left to do) and from the strided chain added for it (64 trees 1,023 deep that 63 hooks must join).  All three
run on the GPU."""
import numpy as np
import pytest

import prm_components_shapes as S


@pytest.mark.parametrize("name", sorted(S.SHAPES))
def test_shape_is_a_roadmap_and_the_model_keeps_its_rules(name):
    n, off, nb = S.shape(name)
    rows, nbi = S.rows_of(off), nb.astype(np.int64)
    # the structure rules of oxhip_prm_set_roadmap
    assert off[0] == 0 and len(off) == n + 1 and off[n] == len(nb) and (np.diff(off.astype(np.int64)) >= 0).all()
    if len(nb):
        assert (nbi < n).all() and (nbi != rows).all()
        same_row = rows[1:] == rows[:-1]
        assert (nbi[1:][same_row] > nbi[:-1][same_row]).all()
        keys = set((rows * n + nbi).tolist())
        assert len(keys) == len(nb) and all(int(b) * n + int(a) in keys for a, b in zip(rows[::97], nbi[::97]))
    label, size, n_comp, largest_label, largest_size = S.components(n, off, nb)
    print("%-22s n %6d entries %7d components %6d largest %6d (label %d)" % (name, n, len(nb), n_comp, largest_size, largest_label))
    idx = np.arange(n)
    assert (label <= idx).all() and (label[label] == label).all()
    roots = label == idx
    assert int(size[roots].sum()) == n and n_comp == int(roots.sum())
    assert (size == np.bincount(label, minlength=n)[label]).all()
    if len(nb):
        assert (label[rows] == label[nbi]).all()                       # an edge never leaves its component
    assert largest_size == size.max() and largest_label == int(np.nonzero(roots & (size == largest_size))[0][0])


def test_model_against_a_flood_fill():
    """the union-find against a second method (breadth-first flood fill) on the graphs below, at and above the giant component"""
    for name in ("random_0.5", "random_1", "random_2", "grid_64x64", "two_cliques", "tie_interleaved"):
        n, off, nb = S.shape(name)
        label = S.components(n, off, nb)[0]
        seen = np.full(n, -1, dtype=np.int64)
        for v in range(n):
            if seen[v] >= 0:
                continue
            seen[v] = v
            todo = [v]
            while todo:
                u = todo.pop()
                for w in nb[int(off[u]):int(off[u + 1])].tolist():
                    if seen[w] < 0:
                        seen[w] = v
                        todo.append(w)
        assert np.array_equal(seen, label.astype(np.int64)), name


def test_shapes_serve_their_purpose():
    comp = {name: S.components(*S.shape(name)) for name in S.SHAPES}
    assert comp["pair_apart"][2:] == (2, 0, 1) and comp["pair_joined"][2:] == (1, 0, 2) and comp["one"][2:] == (1, 0, 1)
    assert comp["isolated_1000"][2:] == (1000, 0, 1) and S.shape("isolated_1000")[2].size == 0
    for name in ("chain_65537", "bitrev_chain_65537", "strided_chain_65537", "star_hub_first", "star_hub_last"):
        assert comp[name][2:] == (1, 0, 65537)
    # one row of 65,536 entries, and every other row hooks onto it
    for name, hub in (("star_hub_first", 0), ("star_hub_last", 65536)):
        _, off, _ = S.shape(name)
        assert int(off[hub + 1] - off[hub]) == 65536
    # finds are deep: the initial forest of the in-order chain is one path, the strided chain's 64 paths need 63 hooks
    depth, trees = S.init_forest(*S.shape("chain_65537"))
    assert depth == 65536 and trees == 1
    depth, trees = S.init_forest(*S.shape("strided_chain_65537"))
    print("strided chain: initial forest depth %d, %d trees" % (depth, trees))
    assert depth > 1000 and trees == 64
    # hooks do the work: bit reversal leaves 32,768 trees to join (and, measured, a forest only 2 deep -- see the module's text)
    depth, trees = S.init_forest(*S.shape("bitrev_chain_65537"))
    print("bit-reversed chain: initial forest depth %d, %d trees" % (depth, trees))
    assert trees > 30000
    assert S.init_forest(*S.shape("star_hub_last"))[1] == 65536          # every leaf is a root until its hook lands on root 0
    # the cliques are joined by their two highest indices only
    n, off, nb = S.shape("two_cliques")
    assert 127 in nb[int(off[63]):int(off[64])] and sum(1 for r, v in zip(S.rows_of(off), nb) if (r < 64) != (v < 64)) == 2
    # below, at and above the giant component
    assert comp["random_0.5"][4] < 100 and 1000 < comp["random_1"][4] < 10000 and comp["random_2"][4] > 30000
    assert comp["random_12"][2] == 1


def test_the_tie_scenes_tie():
    label, size, n_comp, largest_label, largest_size = S.components(*S.shape("tie_low_first"))
    assert n_comp == 3 and sorted(size[label == np.arange(10)].tolist()) == [2, 4, 4] and (largest_label, largest_size) == (0, 4)
    label, size, n_comp, largest_label, largest_size = S.components(*S.shape("tie_interleaved"))
    assert label.tolist() == [0, 1, 1, 1, 0, 0, 6] and (largest_label, largest_size) == (0, 3)
    n, off, nb = S.shape("tie_interleaved")
    out = S.host_prune(S.states_for(n, 2), off, nb, np.ones(n, dtype=bool), largest=True)
    assert out["new_index"].tolist() == [0, -1, -1, -1, 1, 2, -1] and out["n_kept"] == 3 and out["n_removed_entries"] == 4


def test_the_cut_vertex_scene_splits():
    n, off, nb = S.shape("cut_vertex")
    assert S.components(n, off, nb)[2] == 1
    alive = np.ones(n, dtype=bool)
    alive[S.CUT] = False
    label, size, n_comp, largest_label, largest_size = S.components(n, off, nb, alive=alive)
    assert n_comp == 2 and (largest_label, largest_size) == (0, 6) and size[S.CUT] == 0 and label[S.CUT] == S.CUT
    assert label.tolist() == [0] * 6 + [6, 7, 7, 7]
    states = S.states_for(n, 3)
    stage1_only = S.host_prune(states, off, nb, alive)
    assert stage1_only["n_kept"] == 9 and stage1_only["n_removed_entries"] == 4
    both = S.host_prune(states, off, nb, alive, largest=True)            # the smaller piece goes in the same call
    assert both["new_index"].tolist() == [0, 1, 2, 3, 4, 5, -1, -1, -1, -1] and both["n_removed_entries"] == 38 - 30
    assert np.array_equal(both["states"].view(np.uint64), states[:6].view(np.uint64))


def test_host_prune_keeps_order_symmetry_and_bits():
    n, off, nb = S.shape("grid_64x64")
    states = S.states_for(n, 3)
    keep = np.arange(n) % 2 == 0
    out = S.host_prune(states, off, nb, keep)
    # index parity is column parity (the width is even): the 32 kept columns keep their 63 vertical edges each, nothing else
    assert out["n_kept"] == 2048 and out["n_removed_entries"] == len(nb) - 2 * 32 * 63
    keep = np.ones(n, dtype=bool)
    keep[[0, 65, n - 1]] = False
    out = S.host_prune(states, off, nb, keep)
    ni = out["new_index"]
    kept = ni[ni >= 0]
    assert (np.diff(kept) == 1).all() and kept[0] == 0 and out["n_kept"] == n - 3
    assert np.array_equal(out["states"].view(np.uint64), states[keep].view(np.uint64))
    rows, nbi = S.rows_of(out["offsets"]), out["nbrs"].astype(np.int64)
    same_row = rows[1:] == rows[:-1]
    assert (nbi[1:][same_row] > nbi[:-1][same_row]).all()
    keys = set((rows * n + nbi).tolist())
    assert all(int(b) * n + int(a) in keys for a, b in zip(rows, nbi))
    assert out["n_removed_entries"] == 2 * (2 + 4 + 2)
    # min_size = 1 is the identity, min_size = 2 drops exactly the rows without entries
    n, off, nb = S.shape("random_1")
    everything = S.host_prune(S.states_for(n, 2), off, nb, np.ones(n, dtype=bool), min_size=1)
    assert np.array_equal(everything["new_index"], np.arange(n)) and everything["n_removed_entries"] == 0
    two = S.host_prune(S.states_for(n, 2), off, nb, np.ones(n, dtype=bool), min_size=2)
    empty_rows = np.diff(off.astype(np.int64)) == 0
    assert empty_rows.any() and np.array_equal(two["new_index"] < 0, empty_rows) and two["n_removed_entries"] == 0
    with pytest.raises(ValueError):
        S.host_prune(S.states_for(n, 2), off, nb, np.zeros(n, dtype=bool))
    with pytest.raises(ValueError):
        S.host_prune(S.states_for(n, 2), off, nb, np.ones(n, dtype=bool), min_size=10 ** 6)
