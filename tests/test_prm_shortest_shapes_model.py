"""CPU: the scenes of tests/prm_shortest_shapes.py hold what tests/test_gpu_prm_shortest_shapes.py needs them to hold, by the
pure-Python generators alone (make_golden_prm.py's prm_construct / prm_solve, make_golden_prm_shortest.py's checker).  The
device's roadmap is the generators' bit for bit (the golden tests), so these conditions carry over to the device's run:
every lane group is selected by some scene, distance weights meet the tie rule on the line, the levels are deep, some roadmaps
have isolated milestones, and no start is invalid."""
import pytest

import prm_shortest_shapes as shapes

NAMES = sorted(shapes.SCENES)


@pytest.mark.parametrize("name", NAMES)
def test_scene_conditions(name):
    m = shapes.model(name)
    q = shapes.n_queries(name)
    print("%-10s n %3d group %2d mean degree %6.2f isolated %3d solved %2d/%2d multi-tight %5d chain ties %2d max hops %2d demoted sources %d"
          % (name, m["n"], m["group"], m["mean_degree"], m["isolated"], m["solved"], q, m["multi_tight"], m["chain_ties"], m["max_hops"],
             m["demoted"]))
    assert m["n"] == shapes.SCENES[name]["max_milestones"] and len(m["results"]) == q
    assert m["group"] == shapes.GROUP[name]
    assert m["invalid_starts"] == 0                       # the GPU test may require that no query is skipped
    if name in ("line", "line_dense"):
        assert m["multi_tight"] >= 1000                   # distance weights meet the tie rule
    if name == "strip":
        assert m["multi_tight"] == 0                      # the control: as deep, no ties
    if name == "line":
        assert m["chain_ties"] >= 1                       # the node list returned depends on the rule
    if name in ("line", "strip"):
        assert m["max_hops"] >= 40
    if name == "sparse":
        assert m["isolated"] >= 10 and m["solved"] >= 2
    elif name == "dust":
        assert m["isolated"] >= 100 and m["solved"] == 0
    else:
        assert 2 * m["solved"] >= q


def test_the_scenes_select_every_group():
    assert {shapes.model(name)["group"] for name in NAMES} == {4, 8, 16, 32, 64}
    assert set(shapes.GROUP.values()) == {4, 8, 16, 32, 64} and set(shapes.GROUP) == set(shapes.SCENES)
    for n, entries, want in ((1, 0, 4), (0, 0, 4), (10, 40, 4), (10, 41, 8), (10, 80, 8), (10, 81, 16), (10, 320, 32), (10, 321, 64),
                             (10, 6400, 64)):
        assert shapes.batch_group(n, entries) == want
