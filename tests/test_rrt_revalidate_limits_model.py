"""CPU: every shape of tests/rrt_revalidate_limits_shapes.py held to the property it exists for, by the references alone (the C
oracle over R^n, make_golden_so3.py, make_golden_so2.py, the plain loops of rrt_revalidate_helpers.py): a shape that lost its
property would leave tests/test_gpu_rrt_revalidate_limits.py green and empty.  Every edge of every shape takes at most MAX_STEPS
check steps.  `pytest -s` prints what the reference removes from every shape."""
import numpy as np
import pytest

import rrt_revalidate_helpers as rh
import rrt_revalidate_limits_shapes as sh


def held(S, partial=()):
    """the reference of S, after the checks every shape owes: the step cap, 0 < removed < n - 1 for the problems called partial"""
    ref = sh.reference(S)
    print(sh.counts(S), "steps <=", max(e["max_steps"] for e in ref))
    for p, e in enumerate(ref):
        assert e["max_steps"] <= sh.MAX_STEPS, (S["name"], p)
    for p in partial:
        assert 0 < ref[p]["n_removed"] < sh.sizes(S)[p] - 1, (S["name"], p)
    return ref


# ------------------------------------------------------------------------------------------------ A
def test_a_mixed_r3():
    S = sh.mixed_rn()
    ref = held(S, partial=[3, 4])
    assert sh.sizes(S) == [1, 2, 64, 257, 1024, 65, 512, 1] and S["max_nodes"] == 1024
    removed = [e["n_removed"] for e in ref]
    assert removed[2] == 0 and removed[6] == 511 and removed[1] == 1 and removed[5] > 0
    assert ref[4]["n"] % 256 != 0
    for p in (0, 7):
        assert removed[p] == 0 and list(ref[p]["new_index"]) == [0]
    assert held(sh.mixed_257(), partial=[0])[0]["removed"] == ref[3]["removed"]


def test_a_mixed_so3_and_its_staging_chunks():
    S = sh.mixed_so3()
    held(S, partial=[1, 2])
    n = sh.sizes(S)
    assert n == [1, 600, 130] and S["max_nodes"] == 1024 and sh.so3_stage_cap(3, 1024, 3) == 283
    ends = sh.so3_chunk_ends(S)
    assert any(1 <= i < n[p] for p, i in ends)                              # a chunk ends inside a tree ...
    assert any(i >= n[p] and p + 1 < len(n) for p, i in ends)               # ... and one behind a tree, before the next problem
    assert (1, 81) in ends       # slot (1, 80) is the last of its chunk, (1, 81) the first of the next: both edges fail
    ref = sh.reference(S)
    assert not ref[1]["edge_ok"][80] and not ref[1]["edge_ok"][81]


def test_a_mixed_so2():
    S = sh.mixed_so2()
    held(S, partial=[1, 2])
    assert sh.sizes(S) == [1, 300, 1024] and S["max_nodes"] == 1024


# ------------------------------------------------------------------------------------------------ B
def test_b_the_removed_set_is_the_chosen_range():
    S = sh.moves()
    ref = held(S)
    for p, name in enumerate(S["problems"]):
        n, gone = sh.B_RANGES[name]
        assert sh.sizes(S)[p] == n and ref[p]["removed"] == list(gone), name
    shift = {k: ref[S["problems"].index(k)]["new_index"] for k in S["problems"]}
    assert all(shift["tile_256"][i] == i - 256 for i in range(257, 1024))
    assert all(shift["tile_255"][i] == i - 255 for i in range(256, 1024)) and all(shift["tile_257"][i] == i - 257 for i in range(258, 1024))
    assert shift["lone_survivor"][1024] == 1 and all(shift["only_node_1"][i] == i - 1 for i in range(2, 1024))
    assert all(shift["every_second"][i] == i // 2 for i in range(0, 1024, 2))
    assert held(sh.move_256())[0]["removed"] == list(range(1, 257))


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("leg", sh.c_legs(), ids=lambda leg: "r%d_%d_at%d%s" % (leg[0], leg[1], leg[2], "_boxes" if leg[3] else ""))
def test_c_the_decisive_sphere_alone_cuts_the_edge(leg):
    dim, m, place, with_boxes = leg
    S = sh.window_scene(*leg)
    ref = held(S, partial=[0])
    assert len(S["sph_r"]) == m and len(S["box_lo"]) == (2 if with_boxes else 0) and S["sph_r"][place] == sh.THIN
    assert not ref[0]["edge_ok"][sh.C_EDGE]
    st, par = S["trees"][0]
    assert sh.Ref(S, without_sphere=place).check_motion(st[par[sh.C_EDGE]], st[sh.C_EDGE])


# ------------------------------------------------------------------------------------------------ D
def test_d_steps_and_direction():
    S = sh.steps_scene()
    ref = held(S, partial=[0, 1])
    r, (st, par) = sh.Ref(S), S["trees"][0]
    for name, (i, n_steps, kept) in S["cases"].items():
        assert r.steps(st[par[i]], st[i]) == n_steps and bool(ref[0]["edge_ok"][i]) == kept, name
    assert ref[0]["max_steps"] >= 2000
    i = S["cases"]["duplicate"][0]
    assert np.array_equal(st[i], st[par[i]]) and ref[0]["new_index"][i] >= 0
    assert np.array_equal(st[1], st[0]) and ref[0]["new_index"][1] < 0
    # the root inside an obstacle: it is never tested, a child survives, and the same motion backwards is invalid
    (st, par), e = S["trees"][1], ref[1]
    kept = [i for i in range(1, 4) if e["new_index"][i] >= 0]
    assert kept and len(kept) < 3
    assert all(not r.check_motion(st[i], st[0]) for i in kept)


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("dim", sh.E_DIMS)
def test_e_outside_the_bounds(dim):
    S = sh.outside_scene(dim)
    ref = held(S, partial=[0, 1])
    assert S["bounds"] == [(0.0, 10.0)] * dim
    flat = np.concatenate([s.reshape(-1) for s, _ in S["trees"]])
    assert flat.min() <= -50.0 and (flat == 1e3).any() and (flat == 1e5).any()
    for name, (p, i, kind) in S["roles"].items():
        assert bool(ref[p]["edge_ok"][i]) == (kind in ("far", "miss")), name
        if kind == "graze":   # cut by one comparison: the same sphere one ulp smaller lets the motion pass
            k = S["sphere_of"][name]
            r = S["sph_r"].copy()
            r[k] = np.nextafter(r[k], 0.0)
            T = sh.shape(S["name"] + "_" + name, "rn", dim, S["trees"], S["goals"], (S["sph_c"], r), fraction=S["fraction"])
            st, par = S["trees"][p]
            assert sh.Ref(T).check_motion(st[par[i]], st[i]), name


@pytest.mark.parametrize("which", ["a257", "b256"])
def test_e_the_same_removed_set_in_every_frame(which):
    home = held(dict(a257=sh.mixed_257, b256=sh.move_256)[which](), partial=[0])[0]
    for k in range(len(sh.FRAMES)):
        S = sh.framed(which, k)
        e = held(S, partial=[0])[0]
        assert e["removed"] == home["removed"] and e["max_steps"] <= home["max_steps"] + 1, S["name"]


# ------------------------------------------------------------------------------------------------ F
def test_f_the_threshold_itself():
    S = sh.threshold_scene()
    ref = held(S)
    r = sh.Ref(S)
    d = {k: r.distance(st[1], sh.F_CENTRE) for k, (st, _) in zip(S["probes"], S["trees"])}
    for line in ("axis", "diag"):
        assert d[line + "+0"] == sh.F_RADIUS and d[line + "-1"] < sh.F_RADIUS < d[line + "+1"], (line, d)
    for k, e in zip(S["probes"], ref):
        assert e["goal_before"] == e["goal_node"] == (1 if d[k] <= sh.F_RADIUS else -1) and e["n_removed"] == 0, k
    assert sorted({e["goal_node"] for e in ref}) == [-1, 1]


@pytest.mark.parametrize("space", ["rn", "so3", "so2"])
def test_f_the_goal_ladder(space):
    S = sh.ladder_scene(space)
    ref = held(S)
    for p, leg in enumerate(S["legs"]):
        e, what = ref[p], sh.F_LEGS[leg]
        if what is None:
            assert list(np.flatnonzero(e["sat"])) == [0] and e["goal_before"] == e["goal_node"] == -1 and not e["goal_lost"], leg
            continue
        nodes, killed = what
        assert list(np.flatnonzero(e["sat"])) == nodes and e["goal_before"] == 3, leg
        assert [i for i in nodes if e["new_index"][i] < 0] == killed, leg
        left = [i for i in nodes if i not in killed]
        assert e["goal_node"] == (e["new_index"][left[0]] if left else -1) and e["goal_lost"] == (not left), leg
    assert sh.F_LANE[0] % 256 == sh.F_LANE[2] % 256 and sh.F_LANE[0] // 256 != sh.F_LANE[2] // 256


# ------------------------------------------------------------------------------------------------ G
def test_g_twins():
    S = sh.twin_scene()
    ref = held(S, partial=range(len(S["legs"])))
    for p, leg in enumerate(S["legs"]):
        n, groups, at_goal = sh.G_LEGS[leg]
        (st, _), e, (centre, _) = S["trees"][p], ref[p], S["goals"][p]
        new = e["new_index"]
        for members in groups:
            assert new[members[0]] < 0 and all(new[i] >= 0 for i in members[1:]), leg      # the lower twin goes, the others stay
            assert all(np.array_equal(st[i], st[members[0]]) for i in members), leg        # (as values: -0.0 == 0.0)
            upper = members[1]
            assert not any(new[j] >= 0 and np.array_equal(st[j], st[upper]) for j in range(upper)), leg
            assert rh.skip_flags(st)[upper] == 1 and e["skip"][new[upper]] == 0, leg       # the flag set_tree gave it must go
        d = np.sqrt(((e["states"] - centre) ** 2).sum(axis=1))
        twins = {int(new[i]) for i in groups[at_goal][1:]}
        others = [d[j] for j in range(e["n"]) if j not in twins]
        assert all(abs(d[j] - 0.2) < 1e-12 for j in twins) and min(others) > sh.G_CLEAR, leg   # strictly nearest, by a clear margin
    e = ref[S["legs"].index("pair_far_tiles")]
    assert e["new_index"][1800] == 900 and sum(1 for i in range(401) if e["new_index"][i] >= 0) == 201
    e = ref[S["legs"].index("four_in_a_wave")]
    assert {int(e["new_index"][i]) // 64 for i in (130, 140, 150, 160)} == {1}
    assert np.signbit(S["trees"][S["legs"].index("signed_zero")][0][5, 2])
