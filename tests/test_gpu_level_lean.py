"""The packed level solve's lean stages (srt_level.hip level_solve_kernel,
`lean`; knob SRT_LVL_LEAN): push levels of at most LIST_T items that list
their members as they are hit instead of scanning the row for them, and the
next row's init riding on the `idn` output pass.  Every case runs packed with the stages (SRT_LVL_LEAN unset), packed without
(SRT_LVL_LEAN=0) and unpacked: one table bit for bit on the device (latency,
and the loss bits as i32), one edge-visit count, one minimum latency, and the
oracle's table.

The graphs are the smallest at which a stage can go wrong:
  threshold   level 2 of row 0 has LIST_T - 1, LIST_T and LIST_T + 1 items
              (threshold_case), with and without the K spread;
  one owner   one head hit in a listed level by 75 entries at once (15 tails
              of 5 parallel edges: more lanes than a wave, in several waves): a
              head listed twice overshoots the settled count and shifts every
              later level; on the pull side (never listed) walk_case's ZA / ZB
              with 1, 33 and 97 tails behind a listed level;
  shared quad every vertex of a quad (and of a quad pair, whose levels share a
              32-bit word) enters in one listed level, V mod 4 = 0 .. 3 with the
              last vertex a member, every vertex a source in turn: the source in
              each quad position and in the last, partial quad;
  pull levels right behind a full-scan level and right behind a listed level,
              and with 20 vertices that no edge reaches, pulled with empty
              lists to the end;
  fused init  1,100 rows over at most 512 resident workgroups, so a workgroup
              solves several rows one after another, rows dealt by the counter
              and statically; and the same graph with a shuffled subset in use
              (the output loop that does not cover the row: the full init)."""
import copy
import os
import re

import numpy as np
import pytest

import level_cases as LC
import test_gpu_level_edges as E
import test_gpu_level_walk as W
import test_level_packed_cpu as PC

pytestmark = pytest.mark.gpu

PACK, LEAN0, NOPACK = {"SRT_LVL_PACK": "1"}, {"SRT_LVL_PACK": "1", "SRT_LVL_LEAN": "0"}, {"SRT_LVL_PACK": "0"}


def _const(pattern):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "shadow_amd", "csrc", "srt_level.hip")) as f:
        (v,) = re.findall(pattern, f.read())
    return int(v)


LIST_T = _const(r"#define SRT_LIST_T (\d+)")


def test_constants():
    assert 2 <= LIST_T and 512 % LIST_T == 0  # a listed level's items share PACK_NT threads evenly


def _agree(monkeypatch, case, extra=None):
    """Lean, not lean and unpacked: one table, one visit count, one minimum, the oracle's table."""
    import torch

    runs = []
    try:
        for env in (PACK, LEAN0, NOPACK):
            p = E._plan(monkeypatch, case, dict(env, **(extra or {})))
            runs.append(p)
            p.run()
        d = [p.describe() for p in runs]
        assert W.TOKEN in d[0] and W.TOKEN in d[1] and W.TOKEN not in d[2], d
        assert LC.lmax_of(d[0]) <= PC.PACK_LMAX and len({LC.lmax_of(x) for x in d}) == 1, d
        L0, P0, _, _ = E._tables(runs[0])
        vis, mins = [], []
        for p in runs:
            L, P, _, _ = E._tables(p)
            assert torch.equal(L0, L) and torch.equal(P0, P), p.describe()
            vis.append(p.timing()["edge_visits"])
            p.fetch(table=False)
            mins.append(p.min_latency_ns)
        assert vis[0] > 0 and vis == [vis[0]] * 3, vis
        assert mins == [mins[0]] * 3, mins
        E._check(runs[0].fetch(), case)
    finally:
        for p in runs:
            p.close()


# ------------------------------------------------------------ listed levels
def threshold_case(n1):
    """test_gpu_level_walk.spread_case with 40 vertices B, so that a few
    vertices A reach them all: 0 -> n1 vertices A at 1 unit, each a -> 33 to 39
    of B at 1 unit, every b -> 0: row 0's level 2 has n1 + 1 items (A on class 1,
    the source on class 2)."""
    A, B = np.arange(1, 1 + n1), np.arange(1 + n1, 41 + n1)
    e = [(0, int(a), 1) for a in A]
    e += [(int(a), int(B[(7 * i + r) % 40]), 1) for i, a in enumerate(A) for r in range(33 + i % 7)]
    e += [(int(b), 0, 1) for b in B]
    return W._finish(41 + n1, e, n1, np.arange(41 + n1, dtype=np.uint32))


@pytest.mark.parametrize("spread", ["1", "0"])
@pytest.mark.parametrize("T", [LIST_T - 1, LIST_T, LIST_T + 1])
def test_level_at_the_list_threshold(monkeypatch, T, spread):
    _agree(monkeypatch, threshold_case(T - 1), {"SRT_LVL_SPREAD": spread})


def owner_case(tails, par):
    """0 -> `tails` vertices A at 1 unit, every a -> H by `par` parallel edges
    of 1 unit (their losses differ) and -> three of 40 vertices B; every vertex
    -> 0 at 1 unit.  Row 0's level 2 (tails + 1 items) hits H from tails * par
    entries at once."""
    A = np.arange(1, 1 + tails)
    H = 1 + tails
    B = np.arange(2 + tails, 42 + tails)
    V = 42 + tails
    e = [(0, int(a), 1) for a in A]
    e += [(int(a), H, 1) for a in A for _ in range(par)]
    e += [(int(a), int(B[(3 * i + r) % 40]), 1) for i, a in enumerate(A) for r in range(3)]
    e += [(int(v), 0, 1) for v in range(1, V)]
    return W._finish(V, e, 500 + tails, np.arange(V, dtype=np.uint32))


@pytest.mark.parametrize("tails,par", [(LIST_T - 1, 5), (LIST_T - 1, 1), (LIST_T, 5)], ids=["listed-75", "listed", "scanned"])
def test_one_head_hit_by_many_entries_is_listed_once(monkeypatch, tails, par):
    _agree(monkeypatch, owner_case(tails, par))


@pytest.mark.parametrize("m", [1, 33, 97])
def test_pulled_vertex_hit_by_many_tails(monkeypatch, m):
    _agree(monkeypatch, W.walk_case(m, 1))


def quad_case(V):
    """Every ordered pair an edge of 1 or 2 units (seeded), every vertex in use:
    a row's level 1 is one item's list of about V / 2 heads, whole quads among
    them; level 2 takes the rest."""
    rng = np.random.default_rng(900 + V)
    u, v = np.nonzero(~np.eye(V, dtype=bool))
    units = rng.integers(1, 3, size=len(u))
    units[(u + 1) % V == v] = 1  # a ring of unit edges: the probe's bound stays small
    e = list(zip(u.tolist(), v.tolist(), units.tolist()))
    return W._finish(V, e, V, np.arange(V, dtype=np.uint32))


@pytest.mark.parametrize("V", [40, 41, 42, 43])
def test_members_sharing_a_level_word(monkeypatch, V):
    _agree(monkeypatch, quad_case(V))


def star_case(V):
    """Every vertex -> every other at 1 unit: level 1 of every row is all of
    the row but its source, the last vertex and every quad whole."""
    u, v = np.nonzero(~np.eye(V, dtype=bool))
    return W._finish(V, list(zip(u.tolist(), v.tolist(), [1] * len(u))), 70 + V, np.arange(V, dtype=np.uint32))


@pytest.mark.parametrize("V", [9, 10, 11, 12])
def test_whole_quads_enter_in_one_listed_level(monkeypatch, V):
    _agree(monkeypatch, star_case(V))


# ------------------------------------------------------------ pull levels
def pull_case(nq, nz, iso=0):
    """0 -> 200 vertices P at 1 unit; P -> nq vertices Q at 1 unit (each q from
    two p); Q -> nz vertices Z at 1 unit (each z from three q); every vertex -> 0
    at 1 unit; `iso` vertices more, not in use, that no edge touches.  Row 0:
    level 1 is listed (one item), level 2 has 201 items (a full scan) and leaves
    nz + iso unsettled, level 3 pulls them: nq > nz + iso."""
    assert nq > nz + iso and 201 > LIST_T
    P = np.arange(1, 201)
    Q = np.arange(201, 201 + nq)
    Z = np.arange(201 + nq, 201 + nq + nz)
    n = 201 + nq + nz
    e = [(0, int(p), 1) for p in P]
    e += [(int(P[(i + 77 * r) % 200]), int(q), 1) for i, q in enumerate(Q) for r in range(2)]
    e += [(int(Q[(5 * i + 131 * r) % nq]), int(z), 1) for i, z in enumerate(Z) for r in range(3)]
    e += [(int(v), 0, 1) for v in range(1, n)]
    return W._finish(n + iso, e, nq + nz + iso, np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("nq,nz,iso", [(300, 3, 0), (300, 3, 20), (300, 3, 1)], ids=["few", "isolated20", "ragged"])
def test_pull_level_behind_a_full_scan_level(monkeypatch, nq, nz, iso):
    _agree(monkeypatch, pull_case(nq, nz, iso))


@pytest.mark.parametrize("iso", [0, 3, 20])
def test_pull_level_behind_a_listed_level(monkeypatch, iso):
    """walk_case: a pool row's level 2 has two items (listed) and level 3 pulls
    ZA, ZB and the isolated vertices."""
    _agree(monkeypatch, W.walk_case(33, 0, iso))


# ------------------------------------------------------------ fused init
@pytest.mark.parametrize("dyn", ["1", "0"])
def test_workgroups_solve_rows_one_after_another(monkeypatch, dyn):
    _agree(monkeypatch, LC.complete_over(False), {"SRT_LVL_DYN": dyn})


def test_in_use_subset_keeps_the_full_init(monkeypatch):
    case = copy.copy(LC.complete_over(False))
    if hasattr(case, "_expected"):
        del case._expected
    case.nodes = np.random.default_rng(5).permutation(1100)[:700].astype(np.uint32)
    _agree(monkeypatch, case)
