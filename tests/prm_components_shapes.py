"""Planted graphs and the host model of oxhip_prm_components / oxhip_prm_prune, shared by the CPU and
GPU tests.  Pure Python + numpy: a graph is (n, offsets [n + 1] u64, neighbours [E] u32) in the layout get_roadmap writes (rows
ascending, symmetric, no self-loop); the states that go with it are arbitrary finite numbers, because neither call reads them.

components(n, offsets, nbrs)          -> label, size, n_components, largest_label, largest_size (a union-find on the host)
host_prune(states, offsets, nbrs, stage1_keep, min_size, largest) -> the roadmap oxhip_prm_prune must leave, and new_index."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------- graphs
def csr_from_edges(n, edges):
    """undirected edges [(a, b)] (a != b; duplicates are merged) -> (n, offsets u64, nbrs u32), rows ascending and symmetric"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    assert (e[:, 0] != e[:, 1]).all() and (e >= 0).all() and (e < n).all()
    both = np.concatenate([e, e[:, ::-1]])
    keys = np.unique(both[:, 0] * n + both[:, 1])
    rows, nbrs = keys // n, keys % n
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return n, offsets, nbrs.astype(np.uint32)


def isolated(n):
    return n, np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32)


def ring(n):
    a = np.arange(n)
    return csr_from_edges(n, np.stack([a, (a + 1) % n], axis=1))


def chain(n):
    a = np.arange(n - 1)
    return csr_from_edges(n, np.stack([a, a + 1], axis=1))


def bit_reverse16(p):
    p = np.asarray(p, dtype=np.int64)
    out = np.zeros_like(p)
    for b in range(16):
        out |= ((p >> b) & 1) << (15 - b)
    return out


def bitrev_chain(n=65537):
    """the chain 0 - 1 - ... - n-1 with position p renamed to bit_reverse16(p) (the last position keeps the index 65536):
    neighbours in the chain lie far apart in index, the initial forest is almost flat (its depth is 2) and nearly every entry
    has to hook: the trees grow while they are searched, and hooks that lose their swap start again"""
    assert n == 65537
    name = np.concatenate([bit_reverse16(np.arange(65536)), [65536]])
    return csr_from_edges(n, np.stack([name[:-1], name[1:]], axis=1))


def strided_chain(n=65537):
    """the same chain with position 1024 s + o renamed to 64 o + s (the last position keeps the index 65536): 64 initial trees,
    each a path 1,023 deep with the root s, which 63 hooks -- every one a find from the bottom of a tree -- join root to root"""
    assert n == 65537
    p = np.arange(65536)
    name = np.concatenate([64 * (p % 1024) + p // 1024, [65536]])
    return csr_from_edges(n, np.stack([name[:-1], name[1:]], axis=1))


def star(n, hub):
    leaves = np.array([i for i in range(n) if i != hub])
    return csr_from_edges(n, np.stack([np.full(n - 1, hub), leaves], axis=1))


def two_cliques(k=64):
    """cliques {0 .. k-1} and {k .. 2k-1}, joined by one edge between their two highest indices"""
    edges = [(a, b) for base in (0, k) for a in range(base, base + k) for b in range(a + 1, base + k)]
    return csr_from_edges(2 * k, edges + [(k - 1, 2 * k - 1)])


def grid(w, h):
    idx = np.arange(w * h).reshape(h, w)
    edges = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], axis=1),
                            np.stack([idx[:-1, :].ravel(), idx[1:, :].ravel()], axis=1)])
    return csr_from_edges(w * h, edges)


def random_graph(n, mean_degree, seed):
    rng = np.random.default_rng(seed)
    m = int(n * mean_degree / 2)
    e = rng.integers(0, n, size=(m, 2))
    return csr_from_edges(n, e[e[:, 0] != e[:, 1]])


def tie_low_first():
    """two components of four milestones, {0, 1, 2, 3} and {4, 5, 6, 7}, and a pair {8, 9}: the largest is a tie, label 0 wins"""
    return csr_from_edges(10, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7), (8, 9)])


def tie_interleaved():
    """{1, 2, 3} (label 1) and {0, 4, 5} (label 0) tie at three milestones; the component found first by index order of its
    edges is not the winner: label 0 wins.  {6} is alone."""
    return csr_from_edges(7, [(1, 2), (2, 3), (0, 4), (4, 5)])


def cut_vertex():
    """a 6-clique {0 .. 5}, the cut milestone 6 (joined to 5 and to 7), a path 7 - 8 - 9: without 6 the graph splits in two"""
    edges = [(a, b) for a in range(6) for b in range(a + 1, 6)] + [(5, 6), (6, 7), (7, 8), (8, 9)]
    return csr_from_edges(10, edges)


CUT = 6   # the cut milestone of cut_vertex()

# name -> constructor; what each is for is said where it is made
SHAPES = {
    "one": lambda: isolated(1),
    "pair_apart": lambda: isolated(2),
    "pair_joined": lambda: csr_from_edges(2, [(0, 1)]),
    "isolated_1000": lambda: isolated(1000),
    "ring_255": lambda: ring(255), "ring_256": lambda: ring(256), "ring_257": lambda: ring(257),
    "ring_1023": lambda: ring(1023), "ring_1024": lambda: ring(1024), "ring_1025": lambda: ring(1025),
    "chain_65537": lambda: chain(65537),
    "bitrev_chain_65537": bitrev_chain,
    "strided_chain_65537": strided_chain,
    "star_hub_first": lambda: star(65537, 0),
    "star_hub_last": lambda: star(65537, 65536),
    "two_cliques": two_cliques,
    "grid_64x64": lambda: grid(64, 64),
    "random_0.5": lambda: random_graph(50000, 0.5, 11),
    "random_1": lambda: random_graph(50000, 1.0, 12),
    "random_2": lambda: random_graph(50000, 2.0, 13),
    "random_12": lambda: random_graph(50000, 12.0, 14),
    "tie_low_first": tie_low_first,
    "tie_interleaved": tie_interleaved,
    "cut_vertex": cut_vertex,
}
_MADE = {}


def shape(name):
    """the graph, made once per process and never changed"""
    if name not in _MADE:
        n, off, nb = SHAPES[name]()
        off.setflags(write=False)
        nb.setflags(write=False)
        _MADE[name] = (n, off, nb)
    return _MADE[name]


def states_for(n, dim, seed=0, unit=False):
    """arbitrary finite states [n][dim] -- the sign of zero, a subnormal and a huge value among them -- or, unit=True, unit
    quaternions (what an SO(3) handle's services expect; dim is then 4)"""
    rng = np.random.default_rng(1000 + seed)
    s = rng.normal(size=(n, dim)) * 3.0
    if unit:
        return s / np.linalg.norm(s, axis=1, keepdims=True)
    special = [-0.0, 5e-324, 1e150, -1e150, 2.2250738585072014e-308]
    for k, v in enumerate(special):
        s[(k * 7) % n, k % dim] = v
    return s


def rows_of(offsets):
    off = np.asarray(offsets, dtype=np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


# ---------------------------------------------------------------------------------------------------------------- the host model
def _roots(n, rows, nbrs):
    """union-find over the entries (row, nbr) with nbr < row; the smaller root always becomes the parent, so a component's
    root is its lowest index"""
    parent = list(range(n))
    for a, b in zip(rows.tolist(), nbrs.tolist()):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:
            if a < b:
                parent[b] = a
            else:
                parent[a] = b
    label = np.arange(n, dtype=np.int64)
    for v in range(n):       # parent[v] <= v: every earlier label is final
        label[v] = label[parent[v]] if parent[v] != v else v
    return label


def components(n, offsets, nbrs, alive=None):
    """label [n] u32, size [n] u32, n_components, largest_label, largest_size.  alive (optional [n] bools): a dead milestone is
    left out altogether -- its entries connect nothing, it is no component, its label is itself and its size 0."""
    rows, nb = rows_of(offsets), np.asarray(nbrs, dtype=np.int64)
    live = np.ones(n, dtype=bool) if alive is None else np.asarray(alive, dtype=bool)
    use = (nb < rows) & live[rows] & live[nb] if len(nb) else np.zeros(0, dtype=bool)
    label = _roots(n, rows[use], nb[use])
    count = np.bincount(label[live], minlength=n)
    size = np.where(live, count[label], 0)
    roots = np.nonzero(live & (label == np.arange(n)))[0]
    if len(roots) == 0:
        return label.astype(np.uint32), size.astype(np.uint32), 0, None, 0
    largest_size = int(count[roots].max())
    largest_label = int(roots[count[roots] == largest_size].min())
    return label.astype(np.uint32), size.astype(np.uint32), len(roots), largest_label, largest_size


def host_prune(states, offsets, nbrs, stage1_keep, min_size=0, largest=False):
    """The roadmap oxhip_prm_prune leaves: stage 1 = stage1_keep ([n] bools: INVALID and MASK already combined); stage 2 on the
    components of the stage-1 survivors: min_size (0: not asked), largest.  -> dict(states, offsets u64, nbrs u32, new_index i32,
    n_kept, n_removed_entries); ValueError when no milestone would stay."""
    s = np.asarray(states)
    n = len(s)
    keep = np.asarray(stage1_keep, dtype=bool).copy()
    assert keep.shape == (n,)
    if min_size or largest:
        label, size, _, largest_label, _ = components(n, offsets, nbrs, alive=keep)
        if min_size:
            keep &= size >= min_size
        if largest:
            keep &= (label == largest_label) if largest_label is not None else False
    if not keep.any():
        raise ValueError("would keep no milestone")
    new_index = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    rows, nb = rows_of(offsets), np.asarray(nbrs, dtype=np.int64)
    ekeep = keep[rows] & keep[nb] if len(nb) else np.zeros(0, dtype=bool)
    n_kept = int(keep.sum())
    new_off = np.zeros(n_kept + 1, dtype=np.uint64)
    new_off[1:] = np.cumsum(np.bincount(new_index[rows[ekeep]], minlength=n_kept))
    return dict(states=s[keep].copy(), offsets=new_off, nbrs=new_index[nb[ekeep]].astype(np.uint32), new_index=new_index,
                n_kept=n_kept, n_removed_entries=int(len(nb) - ekeep.sum()))


def init_forest(n, offsets, nbrs):
    """(deepest chain, number of trees) of the union-find's initial forest: parent[v] = v's first neighbour when that lies below v"""
    off = np.asarray(offsets, dtype=np.int64)
    depth = np.zeros(n, dtype=np.int64)
    trees = 0
    for v in range(n):
        if off[v] < off[v + 1] and nbrs[off[v]] < v:
            depth[v] = depth[nbrs[off[v]]] + 1
        else:
            trees += 1
    return int(depth.max()), trees
