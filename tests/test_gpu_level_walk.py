"""The packed level solve's walk (srt_level.hip level_solve_kernel PK: the
branch-free push, the register-folded pull, the per-item visit count) on small
graphs built so that one class list has exactly m entries, m around the chunk
size CH = 32 and its multiples, starting at an even and at an odd place of the
entry array, on the push and on the pull side, with and without the small
levels' K spread.  Every table is compared bit for bit (latency and loss bits)
with the unpacked row's on the device and with the oracle's; the edge visits a
plan reports are the same packed, unpacked and by the per-item walk, which
counts entry by entry.

walk_case(m, k) -- directed, every edge 1 or 2 units, so the probe's bound
(>= 2) prunes none and a vertex's class row is its out-edges (the in-use
nodes' self-loops of 3 units are never class entries):
  hub 0 -> every pool vertex, T and D at 1 unit, -> ZA and ZB at 2;
  every vertex but T -> hub at 1 unit, T -> hub only if k = 1;
  T -> pool[0 .. m) at 2 units: T's class-2 out-list, m entries, behind k
  class-1 entries in its row;
  pool[0 .. m) -> ZA and -> ZB at 1 unit: their class-1 in-lists, m entries;
  pool[i] -> pool[i + 1] and ZA, ZB, D -> a pool vertex at 2 units.
Every out-row but T's has an even number of entries, so T's row starts at an
even place wherever the out-rows' cursor puts it and its class-2 list at a
place of k's parity.  The in-rows lie in vertex order (a scan), the hub's
first with 107 + k entries, so ZA's class-1 in-list starts at a place of parity
1 - k.  Row T pushes its own list at level 2 (one item beside T's neighbours:
spread over the lane groups, or one group chunk by chunk with
SRT_LVL_SPREAD=0).  A row from a pool vertex that is no tail settles the hub at
level 1, 105 vertices at level 2 and then pulls ZA and ZB (and any isolated
vertex, whose lists are empty) along their class-1 in-edges, every tail a hit.
Losses are drawn from {0, 1, 1/2, 1/4, 1/8}: zero and 1.0f bits and equal
candidates from several tails abound."""
import numpy as np
import pytest

import level_cases as LC
import test_gpu_level_edges as E
import test_level_packed_cpu as PC

pytestmark = pytest.mark.gpu

TOKEN = " row=packed"
PACK, NOPACK = {"SRT_LVL_PACK": "1"}, {"SRT_LVL_PACK": "0"}
LENGTHS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 96, 97]  # CH = 32 and its multiples, +- 1
POOL = 104
HUB, ZA, D, ZB, T = 0, 1, 2, 3, 4
NGRP = 512 // 4  # lane groups of a packed workgroup (PACK_NT threads, 4 lanes an item)
LOSSES = np.array([0.0, 1.0, 0.5, 0.25, 0.125], np.float32)


def _finish(V, edges, seed, nodes, **kw):
    edges = edges + [(int(v), int(v), 3) for v in nodes]  # an in-use node has a self-loop (never a class entry)
    src, dst, units = (np.array(x, np.int64) for x in zip(*edges))
    rng = np.random.default_rng(seed)
    loss = LOSSES[rng.integers(0, len(LOSSES), size=len(src))]
    return LC._case(V, src, dst, units.astype(np.uint64) * np.uint64(LC.MS), loss, True, nodes, **kw)


def walk_case(m, k, iso=0):
    pool = np.arange(5, 5 + POOL)
    V = 5 + POOL + iso
    e = [(HUB, int(v), 1) for v in pool] + [(HUB, T, 1), (HUB, D, 1), (HUB, ZA, 2), (HUB, ZB, 2)]
    e += [(int(v), HUB, 1) for v in pool] + [(ZA, HUB, 1), (ZB, HUB, 1), (D, HUB, 1)]
    e += [(T, HUB, 1)] * k
    e += [(int(pool[i]), int(pool[(i + 1) % POOL]), 2) for i in range(POOL)]
    e += [(T, int(pool[i]), 2) for i in range(m)]
    e += [(int(pool[i]), z, 1) for i in range(m) for z in (ZA, ZB)]
    e += [(ZA, int(pool[0]), 2), (ZB, int(pool[1]), 2), (D, int(pool[2]), 2)]
    nodes = np.arange(5 + POOL, dtype=np.uint32)  # the isolated vertices are not in use
    return _finish(V, e, 1000 * m + 10 * k + iso, nodes, m=m, k=k)


def spread_case(n1):
    """Source 0 -> n1 vertices A at 1 unit, each a -> 33 to 62 of 200 vertices B
    at 1 unit, every b -> 0: row 0's level 2 has T = n1 + 1 items (A on class
    1, the source on class 2)."""
    A, B = np.arange(1, 1 + n1), np.arange(1 + n1, 201 + n1)
    e = [(0, int(a), 1) for a in A]
    e += [(int(a), int(B[(7 * i + r) % 200]), 1) for i, a in enumerate(A) for r in range(33 + i % 30)]
    e += [(int(b), 0, 1) for b in B]
    return _finish(201 + n1, e, n1, np.arange(201 + n1, dtype=np.uint32))


def _places(case):
    """(first place of T's class-2 out-list relative to its row's start, the
    counts of the other out-rows, first place of ZA's class-1 in-list in the in
    entry array): from the edge list, as lvl_out_kernel and the in-row scan lay
    them out."""
    real = case.src != case.dst  # (self-loops are no class entries)
    src, dst = case.src[real].astype(np.int64), case.dst[real].astype(np.int64)
    cls = (case.lat[real] // np.uint64(LC.MS)).astype(np.int64)
    out_counts = np.bincount(src, minlength=case.n_nodes)
    in_before_za = int(np.sum(dst < ZA))  # in-rows in vertex order, a row's classes in class order
    return int(np.sum((src == T) & (cls < 2))), np.delete(out_counts, T), in_before_za


def _run(monkeypatch, case, env):
    """(plan, latency table, loss-bit table on the device, edge visits) of one run."""
    p = E._plan(monkeypatch, case, env)
    p.run()
    L, P, _, _ = E._tables(p)
    return p, L, P, p.timing()["edge_visits"]


def _all_ways_agree(monkeypatch, case):
    """Packed with and without the K spread, unpacked, and the unpacked per-item
    walk: one table, one visit count, the oracle's table."""
    import torch

    runs = []
    try:
        for env in (PACK, dict(PACK, SRT_LVL_SPREAD="0"), NOPACK, dict(NOPACK, SRT_LVL_SP="0")):
            runs.append(_run(monkeypatch, case, env))
        d = [r[0].describe() for r in runs]
        assert TOKEN in d[0] and TOKEN in d[1] and TOKEN not in d[2] and TOKEN not in d[3], d
        assert 2 <= LC.lmax_of(d[0]) <= PC.PACK_LMAX and len({LC.lmax_of(x) for x in d}) == 1, d
        for p, L, P, vis in runs[1:]:
            assert torch.equal(runs[0][1], L) and torch.equal(runs[0][2], P), p.describe()
        assert runs[0][3] > 0 and [r[3] for r in runs] == [runs[0][3]] * 4, [r[3] for r in runs]
        E._check(runs[0][0].fetch(), case)
    finally:
        for r in runs:
            r[0].close()


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("m", LENGTHS)
def test_list_of_m_entries_pushed_and_pulled(monkeypatch, m, k):
    case = walk_case(m, k)
    front, others, za_first = _places(case)
    assert front == k and not (others % 2).any()  # T's list starts at a place of k's parity
    assert za_first % 2 == 1 - k                   # ZA's in-list at the other parity
    assert int(np.sum((case.src == T) & (case.lat == 2 * LC.MS))) == m
    assert int(np.sum((case.dst == ZA) & (case.lat == LC.MS))) == m  # (the hub's edge to ZA is class 2)
    _all_ways_agree(monkeypatch, case)


@pytest.mark.parametrize("iso", [1, 2, 3, 20])
def test_ragged_sizes_and_vertices_never_reached(monkeypatch, iso):
    """V mod 4 = 2, 3, 0 and 1 with the last in-use vertex (a source) in the last
    quad or the one before; the isolated vertices, not in use, keep the all-ones
    key and the 0xF level to the end, and are pulled with empty lists."""
    case = walk_case(33, 1, iso)
    assert case.n_nodes % 4 == (1 + iso) % 4
    _all_ways_agree(monkeypatch, case)


def test_in_use_subset(monkeypatch):
    """Every third vertex in use, in a shuffled order that starts at the hub."""
    case = walk_case(65, 0, 2)
    pick = np.arange(0, 5 + POOL, 3)
    case.nodes = np.concatenate([[0], np.random.default_rng(7).permutation(pick[1:])]).astype(np.uint32)
    _all_ways_agree(monkeypatch, case)


@pytest.mark.parametrize("n1", [NGRP // 2 - 1, NGRP // 2], ids=["T-64-spread", "T-65-no-spread"])
def test_level_at_the_spread_threshold(monkeypatch, n1):
    """Row 0's level 2 has n1 + 1 items: 64 = half the lane groups (K = 2 groups
    an item), 65 (one group an item)."""
    _all_ways_agree(monkeypatch, spread_case(n1))
