"""The row passes around the walks of the 4-byte-entry packed level solve
(srt_level.hip level_solve_body<..., CE4>; the LVL_LEAN_SCAN / DEFER / PULL
bits of srt_internal.h, knob SRT_LVL_LEAN):
  SCAN   the unsettled scan before a pull level reads the 4-bit levels 32
         vertices a 16-byte word and works a vertex only where a word hits;
  DEFER  a collect counts its level's members and writes their list only where
         a later level can still push from it (nl <= V - settled - nl);
  PULL   a level behind an unsettled list of at most V / 4 vertices collects
         over that list, packing the members to its front in place.
The `idn` output pass and the levels' plan are the parent's (a leaner pass and a
plan a class a lane did not pay, profiles/r14_level_rows); their cases stay as
those passes' own edge tests behind the new stages.

Every case runs through test_gpu_level_ce4_wide._agree -- packed on 4-byte
entries at 768, 640 and 512 threads, packed on 8-byte entries and unpacked: one
table bit for bit on the device, one edge-visit count, one minimum latency,
the oracle's table -- with every stage on (the knob unset) and with each one
off alone.  The graphs are test_gpu_level_ce4.sym_case's (complete, undirected,
identity rows; the short pairs of 1 or 2 units, every other pair of 40 to 300),
built here from arrays so that the self-loops' latency is the case's to choose.
Every vertex is a source, so the diagonal falls on each place of a quad and in
the last quad in every case.

  wide scan   V = 33, 61, 130 (no multiple of 32; 33, 61 and 130 none of 4: the
              last word lies partly past V) with exactly one vertex unsettled
              before the pull level, at vertex 0, 31, 32 and V - 1; one 16-byte
              word (vertices 32 .. 63) all unsettled beside words with none;
  deferred    a row whose level 2 has exactly as many members as vertices are
              left behind it (level 3 pushes from its list: it is written), the
              twin with one member more (level 3 pulls: never written), and a
              level listed by the scan right behind a level whose members were
              listed as they were hit (mem's ranges stay contiguous);
  pull list   U = 1 (the wide-scan cases), U = 769 (one past a 768-thread step),
              U = V / 4 exactly and one over (V = 132: 33 and 34); U = 769 needs
              V >= 3,076, whose whole oracle table takes 18 s: there the five
              builds agree in every row and the oracle checks five rows;
  plan        a row of fourteen levels: the last plans sum classes 1 .. 14;
  output      a self-loop longer than g x the first level (3 and 300 units over
              a level 1 at 1 unit); every edge of 2 units or more -- level 1
              empty, the first members at level 2 -- with a self-loop of 1 unit
              (the row's minimum) and of 3 (the minimum is level 2's);
              1,100 rows over the resident workgroups, dealt by the counter and
              statically: the init fused behind the pass serves the next row.
A row without a self-loop cannot reach this code: 4-byte entries are a
symmetric plan's, whose identity rows hold an entry for every pair (u, u)."""
import functools

import numpy as np
import pytest

import level_cases as LC
import test_gpu_level_ce4 as G
import test_gpu_level_ce4_wide as WD
import test_gpu_level_wave as WV
from shadow_amd import synth

pytestmark = pytest.mark.gpu

LIST_T = WV.LIST_T
OLD = WV.LEAN_LIST | WV.LEAN_INIT | WV.LEAN_WAVE
BITS = {name: WV._const("srt_internal.h", rf"LVL_LEAN_{name} = (\d+)") for name in ("SCAN", "DEFER", "PULL")}
PULL_DIV = WV._const("srt_level.hip", r"constexpr uint32_t PULL_LIST_DIV = (\d+);")
# every stage on (the knob unset), and each one off alone
LEANS = {"all": None}
LEANS.update({"no" + k.lower(): {"SRT_LVL_LEAN": str((OLD | sum(BITS.values())) & ~b)} for k, b in BITS.items()})
lean = pytest.mark.parametrize("lean", sorted(LEANS))


def test_constants():
    assert BITS == {"SCAN": 16, "DEFER": 32, "PULL": 64} and OLD == 14 and PULL_DIV == 4
    assert sorted(v["SRT_LVL_LEAN"] for v in LEANS.values() if v) == ["110", "62", "94"]
    with open(WV.CSRC + "/srt_internal.h") as f:
        src = f.read()
    assert "LVL_LEAN_ROWS = LVL_LEAN_SCAN | LVL_LEAN_DEFER | LVL_LEAN_PULL;" in src
    assert "LVL_LEAN_ROWS_KEPT = LVL_LEAN_ROWS;" in src  # unset: every stage runs


# ------------------------------------------------------------ graphs
def rows_case(n, pairs, seed, loops=3):
    """test_gpu_level_ce4.sym_case from an array of short pairs (a, b, units), the
    self-loops of `loops` units (a number, or one a vertex)."""
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 0)
    units = rng.integers(40, 301, size=len(iu)).astype(np.int64)
    units[iu == ju] = loops
    ls = LC._losses(rng, len(iu))
    p = np.asarray(pairs, np.int64).reshape(-1, 3)
    a, b = np.minimum(p[:, 0], p[:, 1]), np.maximum(p[:, 0], p[:, 1])
    assert (a < b).all() and b.max() < n
    k = a * n - a * (a - 1) // 2 + (b - a)  # the pair's place in the upper triangle, row-major with the diagonal
    assert np.array_equal(iu[k], a) and np.array_equal(ju[k], b)
    units[k] = p[:, 2]
    edges = (iu.astype(np.uint32), ju.astype(np.uint32), units.astype(np.uint64) * np.uint64(LC.MS), ls)
    U = np.full((n, n), 1 << 20, np.int64)
    U[a, b] = U[b, a] = p[:, 2]
    return LC._case(n, *edges, False, np.arange(n), csr=synth.complete_csr(n, seed, edges=edges), units=U,
                    vb=LC.level_vbits(n))


@functools.lru_cache(maxsize=None)
def pull_case(n, src, rest):
    """src - every vertex A outside `rest` at 1 unit, every r of `rest` - two of A
    at 1 unit.  Row src: level 1 is A (listed as it is hit: one item), level 2
    pulls class 1 into the unsettled `rest` (|A| > |rest|) and pushes the source's
    empty class 2."""
    A = [v for v in range(n) if v != src and v not in rest]
    pairs = [(src, a, 1) for a in A]
    for i, r in enumerate(rest):
        pairs += [(r, A[(3 * i + 7 * t) % len(A)], 1) for t in range(2)]
    case = rows_case(n, pairs, 1000 + n + 7 * len(rest) + rest[0])
    assert G.level_sizes(case, src) == [1, len(A), len(rest)] and len(A) > len(rest)
    return case


@functools.lru_cache(maxsize=None)
def chain_case(sizes, unit=1, loops=3):
    """Row 0's levels have `sizes` vertices (sizes[0] = 1), in vertex order; a
    vertex of level k - three of level k - 1 at `unit` units and no other short pair."""
    start = np.concatenate([[0], np.cumsum(sizes)])
    pairs = []
    for k in range(1, len(sizes)):
        prev = np.arange(start[k - 1], start[k])
        for i, v in enumerate(range(start[k], start[k + 1])):
            pairs += [(int(v), int(prev[(5 * i + 11 * t) % len(prev)]), unit) for t in range(min(3, len(prev)))]
    case = rows_case(int(start[-1]), sorted(set(pairs)), 2000 + int(start[-1]) + unit + loops, loops)
    got = G.level_sizes(case, 0)
    assert [c for c in got if c] == list(sizes) and all(got[unit * k] == c for k, c in enumerate(sizes))
    return case


def _run(monkeypatch, case, lean, extra=None):
    WD._agree(monkeypatch, case, dict(LEANS[lean] or {}, **(extra or {})) or None)


# ------------------------------------------------------------ wide scan
ONE_LEFT = [(n, v) for n in (33, 61, 130) for v in sorted({0, 31, 32, n - 1})]


@lean
@pytest.mark.parametrize("n,v", ONE_LEFT)
def test_one_vertex_unsettled_before_the_pull_level(monkeypatch, n, v, lean):
    assert n % 32 and n % 4 and (n + 31) // 32 * 32 > n  # the last 16-byte word lies partly past V
    _run(monkeypatch, pull_case(n, 1, (v,)), lean)


@lean
def test_one_word_all_unsettled_beside_words_with_none(monkeypatch, lean):
    rest = tuple(range(32, 64))
    assert len(rest) <= 130 // PULL_DIV  # (and collected over the list)
    _run(monkeypatch, pull_case(130, 0, rest), lean)


# ------------------------------------------------------------ deferred lists
@lean
@pytest.mark.parametrize("n2", [60, 61])
def test_level_of_exactly_and_one_over_what_is_left(monkeypatch, n2, lean):
    """Level 2 (21 items: no listed level, its collect scans the row) has n2 members
    and 60 vertices stay behind it: 60 is pushed from at level 3, 61 never."""
    sizes = (1, 20, n2, 40, 20)
    case = chain_case(sizes)
    left = case.n_nodes - 1 - 20 - n2
    assert left == 60 and 20 + 1 > LIST_T
    assert (n2 <= left) == (n2 == 60)  # the plan's own test at level 3, and the collect's behind level 2
    assert 40 > 20                     # level 3's list is never written either: level 4 pulls
    _run(monkeypatch, case, lean)


@lean
def test_level_listed_by_the_scan_behind_a_level_listed_as_hit(monkeypatch, lean):
    sizes = (1, 10, 30, 25, 30)
    case = chain_case(sizes)
    assert 10 + 1 <= LIST_T      # level 2: 11 items, its 30 members listed as they are hit
    assert 30 + 10 + 1 > LIST_T  # level 3: the wave walk, collected by the row scan ...
    assert 25 <= 30              # ... and listed: level 4 pushes from its 25 members
    _run(monkeypatch, case, lean)


# ------------------------------------------------------------ the plan
@lean
def test_plan_of_many_classes(monkeypatch, lean):
    """Seven levels below row 0 and fourteen below a chain end's row (PACK_LMAX): the
    plans of its last levels run over classes 1 .. 14, pushes and pulls mixed."""
    case = two_chains()
    assert G.level_sizes(case, 14) == [1] * 8 + [21] + [1] * 6  # levels 0 .. 14 of vertex 14's row
    _run(monkeypatch, case, lean)


@functools.lru_cache(maxsize=None)
def two_chains():
    """0 - 1 - 2 - ... - 7 and 0 - 8 - 9 - ... - 14 at 1 unit, 0 - twenty leaves at 1 unit."""
    pairs = [(0, 1, 1), (0, 8, 1)] + [(v, v + 1, 1) for v in list(range(1, 7)) + list(range(8, 14))]
    pairs += [(0, v, 1) for v in range(15, 35)]
    return rows_case(35, pairs, 3535)


# ------------------------------------------------------------ pull collect over the list
@lean
@pytest.mark.parametrize("n,u", [(3080, 769), (132, 132 // 4), (132, 132 // 4 + 1)])
def test_unsettled_list_of_u_vertices(monkeypatch, n, u, lean):
    assert (u <= n // PULL_DIV) == ((n, u) != (132, 34)) and 769 == 768 + 1
    rest = tuple(range(5, 5 + u)) if n == 132 else tuple(range(n - 1 - 2 * u, n - 1, 2))
    assert len(rest) == u
    if n == 132:
        _run(monkeypatch, pull_case(n, 0, rest), lean)
    else:
        _agree_some_rows(monkeypatch, pull_case(n, 0, rest), lean, [0, 1, rest[0], rest[-1], n - 1])


def _agree_some_rows(monkeypatch, case, lean, rows):
    """test_gpu_level_ce4_wide._agree for a graph whose whole oracle table would take a
    quarter of a minute: the five builds' tables equal bit for bit in every row (the
    unpacked build's is the reference), one visit count, one minimum, and the oracle's
    rows `rows` (row 0, the one the case is built for, among them; the oracle leaves the
    diagonal of a partial table unset: the diagonal is compared between the builds)."""
    import torch

    import test_gpu_level_edges as E

    runs = []
    try:
        for env in [WD.ce4_env(t) for t in WD.THREADS] + [G.CE8, G.NOPACK]:
            p = E._plan(monkeypatch, case, dict(env, **(LEANS[lean] or {})))
            runs.append(p)
            p.run()
        d = [p.describe() for p in runs]
        assert all(G.CE_TOKEN in x for x in d[:3]) and G.CE_TOKEN not in d[3] + d[4], d
        L0, P0, _, _ = E._tables(runs[4])
        vis, mins = [], []
        for p in runs:
            L, P, _, _ = E._tables(p)
            assert torch.equal(L0, L) and torch.equal(P0, P), p.describe()
            vis.append(p.timing()["edge_visits"])
            p.fetch(table=False)
            mins.append(p.min_latency_ns)
        assert vis[0] > 0 and vis == [vis[0]] * 5, vis
        assert mins == [mins[0]] * 5 and mins[0] == int(case.lat.min()), mins  # a complete graph: the shortest edge
        if not hasattr(case, "_some_rows"):
            case._some_rows = E._expected_rows(case, np.asarray(rows))
        E._check_device_rows(runs[0], case, rows, *case._some_rows, diagonal=False)
    finally:
        for p in runs:
            p.close()


# ------------------------------------------------------------ output pass
@lean
@pytest.mark.parametrize("loops", [3, 300])
def test_self_loop_longer_than_the_first_level(monkeypatch, loops, lean):
    case = chain_case((1, 20, 60, 40, 20), 1, loops)
    _run(monkeypatch, case, lean)


@lean
@pytest.mark.parametrize("loops", [1, 3])
def test_level_one_empty(monkeypatch, loops, lean):
    """Every edge of 2 units or more: the first members at level 2.  A self-loop of 1
    unit is shorter than every edge and the row's minimum; one of 3 is not."""
    case = chain_case((1, 20, 60), 2, loops)
    assert int(case.units.min()) == 2 and int(case.lat.min()) == min(loops, 2) * LC.MS
    _run(monkeypatch, case, lean)


@lean
@pytest.mark.parametrize("dyn", ["1", "0"])
def test_workgroups_walk_rows_one_after_another(monkeypatch, dyn, lean):
    _run(monkeypatch, LC.complete_over(False), lean, {"SRT_LVL_DYN": dyn})
