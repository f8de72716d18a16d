"""CPU: the host model of a PRM handle's life (tests/prm_lifecycle_model.py) and the shapes and scripts built on it
(tests/prm_lifecycle_shapes.py), without a GPU.  The model is pinned to the golden files that already pin the device and to the
generators' own construction loops; its grow, re-check and prune are held to the identities DESIGN.md sections 20, 23 and 24
state; every filter shape has the counts its row claims and every script meets the conditions that keep it from being vacuous.
tests/test_gpu_prm_lifecycle.py then holds the device to this model bit for bit."""
import json
import os
import sys
import time

import numpy as np
import pytest

import prm_lifecycle_shapes as ls
from helpers import bits
from prm_components_shapes import components
from prm_grow_helpers import check_rows
from prm_lifecycle_model import HostRoadmap, Refusal, capacity_of, grown_capacity
from prm_revalidate_helpers import edge_lists

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402
import make_golden_prm as mp  # noqa: E402
import make_golden_prm_knn as mk  # noqa: E402
import make_golden_prm_revalidate as mr  # noqa: E402
import make_golden_prm_so3 as mp3  # noqa: E402
import make_golden_so3 as g3  # noqa: E402


def golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def same_roadmap(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------------------- the model and the goldens
def rn_model(P, max_milestones=None):
    spheres = [(mr.unhex_row(c), mr.unhex(r)) for c, r in P["spheres"]]
    k = P.get("knn_k", 0)
    return HostRoadmap("knn" if k else "rn", P["dim"], [tuple(b) for b in P["bounds"]], P["radius"], max_milestones or P["max_milestones"], knn_k=k,
                       lvs_fraction=P["fraction"], seed=P["seed"], stream=P["stream"], max_samples=0 if P["max_samples"] >= 10 ** 9 else P["max_samples"],
                       spheres=spheres, boxes=P["boxes"])


RN_GOLDEN = [("prm_golden.json", n) for n in ("wall", "r3", "r6", "sample_cap")] + [("prm_knn_golden.json", n) for n in ("wall_k6", "r3_k10", "r6_k8", "wall_k1")]


@pytest.mark.parametrize("path,name", RN_GOLDEN, ids=[n for _, n in RN_GOLDEN])
def test_construct_reproduces_the_rn_goldens(path, name):
    rec = golden(path)[name]
    m = rn_model(rec["params"])
    m.construct()
    run = rec["run"]
    assert m.sizes() == (run["n"], run["edge_entries"], run["n_samples"])
    assert "%016x" % mp.states_checksum(m.states_array()) == run["states_checksum"]
    assert "%016x" % mp.csr_checksum(m.rows) == run["csr_checksum"]
    assert [[mg.hexf(v) for v in row] for row in m.states[:48]] == run["states_head"] and m.rows[:48] == run["edges_head"]
    assert m.capacity == capacity_of(rec["params"]["max_milestones"]) and m.rng is not None


@pytest.mark.parametrize("name", ["bounded", "wide_radius", "tiny_radius", "degenerate", "sample_cap"])
def test_construct_reproduces_the_so3_golden(name):
    rec = golden("prm_so3_golden.json")[name]
    P, run = rec["params"], rec["run"]
    bounds = None if P["bounds"] is None else (mr.unhex_row(P["bounds"][0]), mr.unhex(P["bounds"][1]))
    m = HostRoadmap("so3", 4, bounds, mr.unhex(P["radius"]), P["max_milestones"], lvs_fraction=mr.unhex(P["fraction"]), seed=P["seed"], stream=P["stream"],
                    max_samples=0 if P["max_samples"] >= 10 ** 9 else P["max_samples"], spheres=[(mr.unhex_row(c), mr.unhex(r)) for c, r in P["cones"]])
    m.construct()
    assert (m.n, m.n_samples, m.rng.draws) == (run["n"], run["n_samples"], run["draws"])
    assert [[mg.hexf(v) for v in row] for row in m.states] == run["states"] and m.rows == run["edges"]


def test_construct_is_the_generators_own_loops():
    """the model's one loop against make_golden_prm.prm_construct, make_golden_prm_knn.prm_construct_knn and
    make_golden_prm_so3.prm_construct called as they stand, in the scenes the scripts use"""
    for name in ("refill", "knn_life", "so3_life"):
        sc = ls.SCRIPTS[name]
        sp, ob = sc["spec"], ls.scene(sc["scene"], "B")
        m = ls.model_of(sp, ob, max_milestones=150)
        m.construct()
        if sp["kind"] == "so3":
            rm = mp3.prm_construct(None, sp["radius"], ls.FRACTION, g3.Cones(ob["spheres"]), ls.SEED, sp["stream"], 150, 10 ** 9)
        elif sp["kind"] == "knn":
            rm = mk.prm_construct_knn(sp["dim"], m.bounds, sp["knn_k"], ls.FRACTION, mg.Field(sp["dim"], ob["spheres"], ob["boxes"]), ls.SEED, sp["stream"], 150, 10 ** 9)
        else:
            rm = mp.prm_construct(sp["dim"], m.bounds, sp["radius"], ls.FRACTION, mg.Field(sp["dim"], ob["spheres"], ob["boxes"]), ls.SEED, sp["stream"], 150, 10 ** 9)
        assert np.array_equal(bits(m.states_array()), bits(np.array(rm["states"]))) and m.rows == rm["edges"] and m.n_samples == rm["n_samples"]
        assert sum(len(r) for r in m.rows) > 0
        check_rows(m.rows)


def test_capacity_rule():
    assert [capacity_of(v) for v in (1, 1024, 1025, 2049)] == [1024, 1024, 2048, 3072]
    assert grown_capacity(1024, 1024) == 1024 and grown_capacity(1024, 1025) == 2048 and grown_capacity(3072, 3072) == 3072
    assert grown_capacity(3072, 3073) == 4096 and grown_capacity(2048, 2049) == 4096 and grown_capacity(1024, 5000) == 8192


# ---------------------------------------------------------------------------------------------------------------- identities of the model
def handle(kind, n, scene_b=False, stream=3):
    sp = ls.spec(kind, 3 if kind == "knn" else 2, 1.5 if kind == "knn" else 0.9, n, stream, knn_k=5 if kind == "knn" else 0)
    return ls.model_of(sp, ls.scene("r3" if kind == "knn" else "r2", "B" if scene_b else "A"))


@pytest.mark.parametrize("n1,n2", [(1, 1), (63, 1), (64, 64)])
@pytest.mark.parametrize("kind", ["rn", "knn"])
def test_growth_equals_construction(kind, n1, n2):
    whole = handle(kind, n1 + n2)
    whole.construct()
    m = handle(kind, n1)
    m.construct()
    before = m.n_samples
    assert m.grow(n2) == (n2, whole.n_samples - before)
    assert same_roadmap(m.roadmap(), whole.roadmap()) and m.sizes() == whole.sizes() and m.rng.draws == whole.rng.draws


def test_growth_after_planting_in_two_steps_equals_one():
    src = handle("rn", 120)
    src.construct()

    def planted():
        m = handle("rn", 120, scene_b=True)     # some planted milestones are dead, their rows stale
        m.plant(*src.roadmap())
        return m
    one, two = planted(), planted()
    assert not all(one.is_valid(s) for s in one.states)
    with pytest.raises(Refusal) as e:
        one.grow(10)
    assert (e.value.status, e.value.fragment) == ("BAD_ARG", "OXHIP_PRM_GROW_NEW_STREAM") and same_roadmap(one.roadmap(), src.roadmap())
    a1, d1 = two.grow(40, new_stream=7)
    a2, d2 = two.grow(25)                       # the default continues stream 7
    assert one.grow(65, new_stream=7) == (a1 + a2, d1 + d2) == (65, one.n_samples)
    assert same_roadmap(one.roadmap(), two.roadmap()) and one.sizes() == two.sizes()
    assert np.array_equal(bits(one.states_array()[:120]), bits(src.states_array()))
    check_rows(one.rows)
    with pytest.raises(Refusal):
        one.grow(0)


def test_a_grow_that_finds_nothing_valid_changes_nothing_but_the_sample_count():
    m = handle("rn", 80)
    m.construct()
    before, sizes, cap = m.roadmap(), m.sizes(), m.capacity
    m.set_obstacles(spheres=[([5.0, 5.0], 20.0)])
    assert m.grow(1, max_samples=1) == (0, 1)
    assert same_roadmap(m.roadmap(), before) and m.sizes() == (sizes[0], sizes[1], sizes[2] + 1) and m.capacity == cap


def test_recheck_after_growth_removes_nothing_and_prune_leaves_only_valid_milestones():
    m = handle("rn", 200)
    m.construct()
    m.set_obstacles(**ls.scene("r2", "B"))
    valid, removed = m.revalidate()
    assert not valid.all() and removed > 0
    m.grow(100)
    rm = m.roadmap()
    valid2, removed2 = m.revalidate()
    assert removed2 == 0 and same_roadmap(m.roadmap(), rm) and np.array_equal(valid2[:200], valid) and valid2[200:].all()
    new_index, kept, _ = m.prune(invalid=True)
    assert kept == int(valid2.sum()) and np.array_equal(new_index >= 0, valid2)
    valid3, removed3 = m.revalidate()
    assert valid3.all() and removed3 == 0 and m.n == kept
    k = handle("knn", 200)                       # k-nearest over a dead milestone
    k.construct()
    k.set_obstacles(**ls.scene("r3", "B"))
    before = k.roadmap()
    assert not all(k.is_valid(s) for s in k.states)
    with pytest.raises(Refusal) as e:
        k.grow(5, new_stream=9)
    assert e.value.fragment == "not built" and same_roadmap(k.roadmap(), before) and k.rng_stream == 3


# ---------------------------------------------------------------------------------------------------------------- the filter shapes
@pytest.mark.parametrize("name", sorted(ls.SHAPES))
def test_filter_shape_has_the_counts_it_claims(name):
    sh, g = ls.shape(name), ls.grown(name)
    m, c, n_old = g["model"], sh["ring"], len(sh["states"])
    live, rows = g["live"], m.rows
    ring_dead, far_dead = int(np.count_nonzero(~live[:c])), int(np.count_nonzero(~live[c:]))
    cand = ls.candidate_count(sh, m.states)
    survivors = sum(1 for j in range(n_old, m.n) for i in range(j) if (i >= n_old or live[i]) and m.distance(m.states[j], m.states[i]) < sh["spec"]["radius"])
    print("%s: ring %d, dead on it %d, dead elsewhere %d, candidates %d, of which live %d, new entries %d"
          % (name, c, ring_dead, far_dead, cand, survivors, sum(len(r) for r in rows[n_old:])))
    assert (ring_dead, far_dead, cand) == (sh["ring_dead"], sh["far_dead"], sh["candidates"])
    assert ring_dead + far_dead > 0                                                # the filter runs
    assert (g["added"], m.n) == (sh["n_more"], n_old + sh["n_more"]) and g["removed_after"] == 0
    assert np.array_equal(g["valid_after"][:n_old], live) and g["valid_after"][n_old:].all()
    check_rows(rows)
    old = edge_lists(sh["offsets"], sh["nbrs"])
    assert [[v for v in row if v < n_old] for row in rows[:n_old]] == old and all(rows[i] == [] for i in np.nonzero(~live)[0])
    if sh["q0"] is not None:                                                       # the new milestone is q0, the first sample of the stream
        assert m.states[n_old] == sh["q0"] and g["drawn"] == 1
        assert all(m.distance(sh["q0"], s) < sh["spec"]["radius"] for s in m.states[:c])
        assert all(m.distance(sh["q0"], s) > 2.0 * sh["spec"]["radius"] for s in m.states[c:n_old])
        assert survivors == c - ring_dead
    if sh["spec"]["kind"] == "rn":
        assert (sh["states"] >= 0.0).all() and (sh["states"] <= 10.0).all()
    if name.startswith("edge_") or name.startswith("so3_edge"):
        assert abs(ring_dead - c / 2.0) <= 1.0 and (len(rows[n_old]) > 0 or c == 1)
    if "all_dropped" in name:
        assert survivors == 0 and rows[n_old] == [] and rows[:n_old] == old and sum(len(r) for r in old) > 0
    if name == "identity_257":
        twin = ls.planted_model(sh, ls.NOTHING)
        assert twin.grow(1, new_stream=sh["stream"]) == (g["added"], g["drawn"]) and twin.rows == rows and len(rows[n_old]) == 257
    if name.startswith("one_kept"):
        assert survivors == 1 and len(rows[n_old]) == 1
    if name == "new_new_only":
        assert survivors == 65 * 64 // 2 and not live.any() and all(i >= n_old for row in rows[n_old:] for i in row)
        assert sum(len(r) for r in rows[n_old:]) > 65


def test_the_one_kept_shapes_keep_three_different_milestones():
    kept = [ls.grown("one_kept_%s" % k)["model"].rows[-1] for k in ("first", "63", "last")]
    assert kept == [[0], [63], [256]]


# ---------------------------------------------------------------------------------------------------------------- the scripts
def stage1_mask(sp, t, before):
    """the stage-1 survivors of the prune step t on the roadmap `before`"""
    m = ls.model_of(sp, t["obstacles"])
    keep = np.ones(len(before[0]), dtype=bool)
    if t["args"].get("invalid"):
        keep &= np.array([m.is_valid([float(v) for v in s]) for s in before[0]])
    if "keep" in t["args"]:
        keep &= t["args"]["keep"]
    return keep


@pytest.mark.parametrize("name", sorted(ls.SCRIPTS))
def test_script_meets_its_conditions(name):
    t0 = time.process_time()
    trace = ls.run_script(name)
    seconds = time.process_time() - t0
    sc = ls.SCRIPTS[name]
    sp = sc["spec"]
    killed = cut = 0
    for k, t in enumerate(trace):
        before = trace[k - 1]["roadmap"] if k else None
        op, res = t["op"], t["result"]
        assert t["sizes"][0] > 0 or op == "setup"
        check_rows(edge_lists(*t["roadmap"][1:]))
        if op in ("scene", "plant"):
            m = ls.model_of(sp, t["obstacles"])
            killed += sum(1 for s in t["roadmap"][0] if not m.is_valid([float(v) for v in s]))
        if op == "revalidate":
            valid, removed = res
            was, now = edge_lists(*before[1:]), edge_lists(*t["roadmap"][1:])
            cut += sum(1 for j, row in enumerate(was) for i in row if i < j and valid[i] and valid[j] and i not in now[j])
        if op == "grow":
            want = t["args"].get("refused")
            if want:
                assert isinstance(res, Refusal) and (res.status, res.fragment) == want and same_roadmap(t["roadmap"], before)
                continue
            assert res[0] == t["args"]["n_more"] and t["sizes"][0] == t["n_before"] + res[0]          # no budget ran out
            if t["args"].get("cap") == "moves":
                assert t["n_before"] + res[0] > t["cap_before"] and t["capacity"] == grown_capacity(t["cap_before"], t["sizes"][0]) > t["cap_before"]
            else:
                assert t["capacity"] == t["cap_before"]
                if t["args"].get("cap") == "stays":
                    assert t["sizes"][0] == t["capacity"]
        if op == "prune":
            keep = stage1_mask(sp, t, before)
            label, size, n_comp, _, _ = components(len(before[0]), before[1], before[2], alive=keep)
            if t["args"].get("largest"):
                assert n_comp > 1 and res[1] < int(keep.sum())
        if op == "fresh":
            assert same_roadmap(res[0], t["roadmap"]) and res[1] == t["sizes"]
        if t["marked"]:                                                                          # the twin check will not be vacuous
            s, g, r = ls.queries(sp, 32, 100 + k)
            solved = sum(ls.model_solve(sp, t["obstacles"], t["roadmap"], s[q], g[q], r[q])[0] == "solved" for q in range(32))
            assert solved >= 4, (k, solved)
    moves = [t for t in trace if t["capacity"] != t["cap_before"]]
    print("%s: %.1f s of model time, %d steps, %d milestones at the end, capacity moves %s, killed %d, cut between valid ends %d"
          % (name, seconds, len(trace), trace[-1]["sizes"][0], [(t["cap_before"], t["capacity"]) for t in moves], killed, cut))
    if any(t["op"] == "scene" for t in trace) or name == "planted_veteran":
        assert killed > 0 and cut > 0
    assert len(moves) == sum(1 for _, kw in sc["steps"] if kw.get("cap") == "moves") > 0
    assert all(t["marked"] for t in moves) and all(t["marked"] for t in trace if t["op"] == "prune") and [t for t in trace if t["changed"]][-1]["marked"]


def test_the_scripts_cover_what_no_single_one_has_to():
    traces = {name: ls.run_script(name) for name in ls.SCRIPTS}
    dropped = 0
    for name, trace in traces.items():
        for k, t in enumerate(trace):
            if t["op"] == "prune" and t["args"].get("min_size"):
                before = trace[k - 1]["roadmap"]
                label, size, _, _, _ = components(len(before[0]), before[1], before[2], alive=stage1_mask(ls.SCRIPTS[name]["spec"], t, before))
                dropped += int(np.count_nonzero((label == np.arange(len(label))) & (size > 1) & (size < t["args"]["min_size"])))
    assert dropped > 0                                                # a prune(min_size) drops a component of more than one milestone
    assert len([t for t in traces["refill"] if t["capacity"] != t["cap_before"]]) == 2          # one handle moves twice
    assert traces["odd_capacity"][0]["capacity"] == 3072 and traces["odd_capacity"][-1]["capacity"] == 4096
    first = traces["setup_again"][0]
    again = [t for t in traces["setup_again"] if t["op"] == "construct"][1]
    assert same_roadmap(first["roadmap"], again["roadmap"]) and first["sizes"] == again["sizes"] and again["capacity"] == 2048
