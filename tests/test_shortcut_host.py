"""CPU: the shortcut's host rules (oxhip_host.hpp: shortcut_shape, shortcut_rounds, shortcut_matrix_bytes), which both entries --
oxhip_rrt_batch_simplify_paths with m = 1 and oxhip_prm_batch_simplify_paths -- size their workspaces, cut their rounds and expand
their test hooks' matrices with.  A stand-alone program with its own main (tests/cpp/test_shortcut_host.cpp), built with
AddressSanitizer and UBSan, reads the cases written here and prints what the helpers give; the expectations are the Python models
the GPU tests already trust (prm_simplify_helpers, simplify_limits_shapes) and restatements below."""
import os
import subprocess

import numpy as np
import pytest

import prm_simplify_helpers as ph
import simplify_limits_shapes as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 1 << 30


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shortcut_host") / "test_shortcut_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_shortcut_host.cpp"),
                           "-o", exe])

    def go(cases):
        r = subprocess.run([exe], input="".join(c + "\n" for c in cases), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        lines = r.stdout.splitlines()
        assert lines[-1] == "shortcut host rules: done" and len(lines) == len(cases) + 1, r.stdout
        return lines[:-1]

    return go


def words_of(L, m, max_span):
    return -(-ph.matrix_bits(L, m, max_span) // 64)


def test_shape_against_the_models(run):
    cases = [(L, m, s) for L in range(10) for m in (1, 2, 5, 256) for s in sorted({0, 1, 2, max(L - 1, 0), L + 3})]
    got = run(["shape %d %d %d" % c for c in cases])
    for (L, m, s), line in zip(cases, got):
        rows, window, words, checks = (int(x) for x in line.split()[1:])
        assert rows == ((L - 1) * m + 1 if L else 0), (L, m, s, line)
        assert window == (ph.span_of(L, s) * m if L else 0), (L, m, s, line)
        assert words == words_of(L, m, s) and checks == ph.expected_checks(L, m, s), (L, m, s, line)
        if m == 1:   # the waypoint case is the RRT shortcutter's own slot count, and its checks are the pairs with 2 <= d <= S
            S = ph.span_of(L, s)
            assert words == -(-sl.slot_count(L, s) // 64), (L, s, line)
            assert checks == (sum(L - d for d in range(2, S + 1)) if L else 0), (L, s, line)


def plan(lengths, m, max_span, budget, max_paths):
    """the round rule restated: paths in order while their words stay within the budget together (at least one per round) and the round
    holds fewer than max_paths; -> list of (first path, prefix sums of the words), or the first path that fits no round"""
    rounds = []
    for q, L in enumerate(lengths):
        w = words_of(L, m, max_span)
        if w * 8 > budget or (L and (L - 1) * m + 1 > 0x7FFFFFFF):
            return q
        if not rounds or (rounds[-1][1][-1] + w) * 8 > budget or (max_paths and len(rounds[-1][1]) - 1 >= max_paths):
            rounds.append((q, [0]))
        rounds[-1][1].append(rounds[-1][1][-1] + w)
    return rounds


def parse_rounds(line, n):
    head, *parts = [p.split() for p in line.split("|")]
    if head[1] == "refused":
        return int(head[2])
    assert head[1] == "ok" and parts[-1] == ["end", str(n)], line
    return [(int(p[0]), [int(x) for x in p[1:]]) for p in parts[:-1]]


def test_rounds_against_the_models(run):
    mixed = list(sl.MIXED_LENGTHS)
    w130, w66 = words_of(130, 1, 0), words_of(66, 1, 0)
    assert (w130, w66) == (260, 66)
    cases = [(1, s, GIB, c, mixed) for s in (0, 2) for c in sl.MIXED_CHUNKS]
    cases += [(4, s, GIB, c, mixed) for s in (0, 1) for c in (0, 2, 65535)]
    two = (w130 + w66) * 8
    cases += [(1, 0, b, 0, [130, 66, 130]) for b in (two, two + 7, two - 1, two - 8)]   # splits at a word count and one word below
    cases += [(1, 0, GIB, 1, mixed), (3, 2, GIB, 1, [4, 0, 9])]                         # a cap of 1
    cases += [(1, 0, 100 * 8, 0, l) for l in ([130, 3, 3], [3, 130, 3], [3, 3, 130], [130, 130])]   # alone too large: first, middle, last
    cases += [(256, 0, GIB, 0, [3, 2000, 3])]                                           # ... by its subdivision
    cases += [(1, 2, GIB, 0, [3, 0x7FFFFFFF]), (1, 2, GIB, 0, [3, 0x7FFFFFFF + 6])]     # ... by its rows alone: 2^25 words fit
    cases += [(1, 0, GIB, 0, []), (5, 3, GIB, 7, []), (1, 0, GIB, 0, [0, 0, 0])]        # an empty batch; paths without states
    got = run(["rounds %d %d %d %d %d %s" % (m, s, b, c, len(l), " ".join(map(str, l))) for m, s, b, c, l in cases])
    seen_refused, seen_split = set(), set()
    for (m, s, b, c, l), line in zip(cases, got):
        res = parse_rounds(line, len(l)) if l else line
        if not l:
            assert line == "rounds ok | end 0", line
            continue
        assert res == plan(l, m, s, b, c), (m, s, b, c, l, line)
        if isinstance(res, int):
            seen_refused.add((res, len(l)))
            continue
        assert res[0][0] == 0 and all(len(w) >= 2 for _, w in res)                       # in order, at least one path per round
        assert all(q1 == q0 + len(w) - 1 for (q0, w), (q1, _) in zip(res, res[1:]))
        if l is mixed and m == 1 and b == GIB:
            assert [w for _, w in res] == sl.round_word_offsets(mixed, s, c), (s, c, line)
        if l == [130, 66, 130]:
            seen_split.add(tuple(q for q, _ in res))
            assert [q for q, _ in res] == ([0, 2] if b >= two else [0, 1, 2]), (b, line)
        if c == 1:
            assert [q for q, _ in res] == list(range(len(l)))
    assert {(0, 3), (1, 3), (2, 3), (0, 2), (1, 2)} <= seen_refused and seen_split == {(0, 2), (0, 1, 2)}
    assert plan([3, 0x7FFFFFFF], 1, 2, GIB, 0) != 1 and words_of(0x7FFFFFFF + 6, 1, 2) * 8 <= GIB   # (the longer one is refused for its rows)


def matrix_bytes(words, L, m, max_span):
    """the expansion restated: 1 on one original edge, the pair's bit inside the window, 0 elsewhere"""
    M, W = (L - 1) * m + 1, ph.span_of(L, max_span) * m
    out = np.zeros((M, M), dtype=np.uint8)
    for u in range(M):
        for v in range(u + 1, min(M, u + W + 1)):
            slot = (v - u - 2) * M + u
            out[u, v] = 1 if ph.same_edge(u, v, m) else (words[slot >> 6] >> (slot & 63)) & 1
    return out


def test_matrix_expansion_bit_for_bit(run):
    shapes = ph.limit_shapes()
    rng = np.random.RandomState(5)
    cases = []
    for name in ("matrix_63", "matrix_64", "matrix_65", "matrix_128"):
        pts, _, _, m, span, _ = shapes[name]
        L = len(pts)
        assert ph.matrix_bits(L, m, span) == int(name.split("_")[1])
        n = words_of(L, m, span)
        for fill in ("random", "ones", "zeros"):   # (ones: the padding and the same-edge slots hold bits that must not show)
            words = [int(rng.randint(0, 1 << 32)) << 32 | int(rng.randint(0, 1 << 32)) if fill == "random" else ((1 << 64) - 1 if fill == "ones" else 0)
                     for _ in range(n)]
            cases.append((L, m, span, words))
    cases += [(2, 1, 0, []), (2, 2, 0, []), (1, 3, 0, []), (0, 1, 0, [])]   # no words: edges alone, one row, none
    got = run(["matrix %d %d %d %d %s" % (L, m, s, len(w), " ".join("%x" % x for x in w)) for L, m, s, w in cases])
    for (L, m, s, words), line in zip(cases, got):
        _, M, *rows = line.split()
        want = matrix_bytes(words, L, m, s) if L else np.zeros((0, 0), dtype=np.uint8)
        assert int(M) == want.shape[0] == len(rows), line
        assert rows == ["".join(map(str, r)) for r in want.tolist()], (L, m, s, line)
    full = matrix_bytes([(1 << 64) - 1], 9, 1, 0)
    assert full.sum() == 9 * 8 // 2 and not np.tril(full).any()
