"""The packed level solve's wave walk (srt_level.hip level_solve_kernel, the
LVL_LEAN_WAVE stage of `lean`): a push-only level of more than LIST_T items is
walked one wave an item, batches of at most WAVE_B items dealt to the waves by
a counter, a batch's lists as one stream of 64-entry passes.  Every case runs
packed with the stage (SRT_LVL_LEAN unset), packed without it (SRT_LVL_LEAN=6:
the pipelined chunk walk) and unpacked: one table bit for bit on the device
(latency, and the loss bits as i32), one edge-visit count, one minimum
latency, and the oracle's table.

The graphs are directed with edges of 1 to 3 units and are the smallest at
which the walk can go wrong:
  list length  one item's list has m = 1, 63, 64, 65, 127, 128, 129 entries
               (one pass, two, three; full and one over), starting at an even
               and at an odd place of the entry array, in a level of two classes
               whose boundary lies inside a batch, with empty lists first and
               last in a batch (wave_case);
  level size   T = LIST_T + 1 (the first level not listed), 63, 64, 65, around
               8 (WAVE_B - 1) + 1 where a batch reaches WAVE_B items, and 511,
               512, 513 (the last batch full, and one item over);
  one owner    one head hit by 85 and by 350 entries at once, from several
               waves and from several passes of one wave, losses from
               {0, 1, 1/2, 1/4, 1/8}: equal candidates and the 1.0f bits;
  mixed level  a level with a push class and a pull class right behind a
               wave-walked level keeps the chunk walk, a pull level follows;
  rows         1,100 rows over at most 512 resident workgroups, dealt by the
               counter and statically: the level's batch counter and the fused
               init are used again by a workgroup's next row."""
import os
import re

import numpy as np
import pytest

import level_cases as LC
import test_gpu_level_edges as E
import test_gpu_level_lean as LN
import test_gpu_level_walk as W
import test_level_packed_cpu as PC

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "shadow_amd", "csrc")


def _const(name, pattern):
    with open(os.path.join(CSRC, name)) as f:
        (v,) = re.findall(pattern, f.read())
    return int(v)


LIST_T = LN.LIST_T
WAVE_B = _const("srt_level.hip", r"#define SRT_WAVE_B (\d+)")
LEAN_LIST = _const("srt_internal.h", r"LVL_LEAN_LIST = (\d+)")
LEAN_INIT = _const("srt_internal.h", r"LVL_LEAN_INIT = (\d+)")
LEAN_WAVE = _const("srt_internal.h", r"LVL_LEAN_WAVE = (\d+)")
NW = 512 // 64  # waves of a packed workgroup (PACK_NT threads)

PACK = {"SRT_LVL_PACK": "1"}
NOWAVE = {"SRT_LVL_PACK": "1", "SRT_LVL_LEAN": str(LEAN_LIST | LEAN_INIT)}
NOPACK = {"SRT_LVL_PACK": "0"}


def test_constants():
    assert (LEAN_LIST, LEAN_INIT, LEAN_WAVE) == (2, 4, 8) and NOWAVE["SRT_LVL_LEAN"] == "6"
    assert 1 <= WAVE_B <= 64  # a batch's items: a lane each
    with open(os.path.join(CSRC, "srt_internal.h")) as f:
        src = f.read()
    assert "LVL_LEAN_ALL = LVL_LEAN_LIST | LVL_LEAN_INIT | LVL_LEAN_WAVE;" in src
    assert "LVL_LEAN_KEPT = LVL_LEAN_ALL;" in src  # unset: the stage runs


def _agree(monkeypatch, case, extra=None):
    """With the wave walk, without it and unpacked: one table, one visit count, one minimum, the oracle's table."""
    import torch

    runs = []
    try:
        for env in (PACK, NOWAVE, NOPACK):
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


def _level_sizes(case, s):
    """Vertices at each distance (units) from s, the self-loops aside: [1, |N_1|, |N_2|, ...]."""
    real = case.src != case.dst
    src, dst = case.src[real].astype(np.int64), case.dst[real].astype(np.int64)
    w = (case.lat[real] // np.uint64(LC.MS)).astype(np.int64)
    INF = np.iinfo(np.int64).max // 2
    d = np.full(case.n_nodes, INF)
    d[s] = 0
    while True:
        nd = d.copy()
        np.minimum.at(nd, dst, d[src] + w)
        if np.array_equal(nd, d):
            break
        d = nd
    return np.bincount(d[d < INF]).tolist()


# ------------------------------------------------------------ list length
NP = 132  # pool vertices of wave_case


def wave_case(m, k):
    """Source S = 0 -> F fillers at 1 unit (F > LIST_T, of k's parity) and ->
    pool[0 .. m) at 2 units: S's class-2 list has m entries behind F class-1
    entries.  A filler -> 10 pool vertices at 1 unit (the fillers together reach
    the whole pool) and -> S by two parallel edges of 2 units; four fillers (the
    first and third of the first batch, the first of the second, the last of
    all, if the members lie in vertex order) have no class-1 entry.  A pool
    vertex -> S by two parallel edges of 1 unit.  Every out-row but S's has an even number of entries, so S's
    row starts at an even place and its class-2 list at a place of k's parity.
    Row S: level 1 is the fillers (listed: one item), level 2 has F + 1 items,
    the fillers on class 1 and S on class 2 -- the class boundary inside the
    last batch -- and settles the pool; nothing is left for a pull."""
    F = LIST_T + 2
    F += (F + k) % 2
    fill = np.arange(1, 1 + F)
    pool = np.arange(1 + F, 1 + F + NP)
    empty = {0, 2, 3, F - 1}
    e = [(0, int(f), 1) for f in fill]
    e += [(0, int(pool[i]), 2) for i in range(m)]
    full = [i for i in range(F) if i not in empty]
    assert 10 * len(full) >= NP
    e += [(int(fill[i]), int(pool[(10 * q + r) % NP]), 1) for q, i in enumerate(full) for r in range(10)]
    e += [(int(f), 0, 2) for f in fill for _ in range(2)]
    e += [(int(p), 0, 1) for p in pool for _ in range(2)]
    return W._finish(1 + F + NP, e, 7000 + 10 * m + k, np.arange(1 + F + NP, dtype=np.uint32), m=m, k=k, F=F)


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 127, 128, 129])
def test_list_of_m_entries_walked_by_a_wave(monkeypatch, m, k):
    case = wave_case(m, k)
    real = case.src != case.dst
    src = case.src[real].astype(np.int64)
    units = (case.lat[real] // np.uint64(LC.MS)).astype(np.int64)
    counts = np.bincount(src, minlength=case.n_nodes)
    assert int(np.sum((src == 0) & (units == 1))) % 2 == k and not (counts[1:] % 2).any()
    assert int(np.sum((src == 0) & (units == 2))) == m
    assert _level_sizes(case, 0) == [1, case.F, NP] and case.F + 1 > LIST_T
    # the fillers alone can push: more vertices unsettled than tails
    assert case.F <= NP
    _agree(monkeypatch, case)


# ------------------------------------------------------------ level size
def level_case(T):
    """test_gpu_level_walk.spread_case with max(200, T) vertices B, so that the
    level stays a push: source 0 -> T - 1 vertices A at 1 unit and -> every b at
    2 units, each a -> 33 to 62 of B at 1 unit, every b -> 0: row 0's level 2
    has T items, A on class 1 and the source on class 2, its list of four or
    more passes the last item of the last batch."""
    n1, nb = T - 1, max(200, T)
    A, B = np.arange(1, 1 + n1), np.arange(1 + n1, 1 + n1 + nb)
    e = [(0, int(a), 1) for a in A] + [(0, int(b), 2) for b in B]
    e += [(int(a), int(B[(7 * i + r) % nb]), 1) for i, a in enumerate(A) for r in range(33 + i % 30)]
    e += [(int(b), 0, 1) for b in B]
    return W._finish(1 + n1 + nb, e, 300 + T, np.arange(1 + n1 + nb, dtype=np.uint32))


SIZES = sorted({LIST_T + 1, 63, 64, 65, NW * (WAVE_B - 1), NW * (WAVE_B - 1) + 1, 511, 512, 513})


@pytest.mark.parametrize("T", SIZES)
def test_level_of_t_items(monkeypatch, T):
    case = level_case(T)
    sizes = _level_sizes(case, 0)
    assert sizes == [1, T - 1, case.n_nodes - T] and T - 1 <= case.n_nodes - T and T > LIST_T  # level 2: a push of T items
    _agree(monkeypatch, case)


# ------------------------------------------------------------ one owner
@pytest.mark.parametrize("tails", [LIST_T + 1, 70])
def test_one_head_hit_from_many_waves_and_passes(monkeypatch, tails):
    """test_gpu_level_lean.owner_case: H takes 5 * tails candidates in one
    wave-walked level (tails + 1 items over 8 waves: several items, so several
    passes, a wave)."""
    assert tails + 1 > LIST_T and 5 * tails > 64
    _agree(monkeypatch, LN.owner_case(tails, 5))


# ------------------------------------------------------------ mixed and pull levels
def mixed_case():
    """0 -> 100 P at 1 unit; P -> 45 Q at 1 unit; Q -> 50 Z3 at 1 unit and P ->
    Z3 at 2 units; Z3 -> 10 Z4 at 1 unit, Q -> Z4 at 2, P -> Z4 at 3; every
    vertex -> 0 at 1 unit.  Row 0: level 2 pushes from P (101 items, 105
    unsettled: the wave walk), level 3 pushes class 1 from Q (45 tails, 60
    unsettled) and pulls class 2 from P (100 tails): the chunk walk; level 4
    pulls the 10 vertices left along three classes (the source's own class, one
    tail with an empty list, is a push in both)."""
    P, Q = np.arange(1, 101), np.arange(101, 146)
    Z3, Z4 = np.arange(146, 196), np.arange(196, 206)
    e = [(0, int(p), 1) for p in P]
    e += [(int(p), int(Q[i % 45]), 1) for i, p in enumerate(P)]
    e += [(int(q), int(Z3[(j + 7 * r) % 50]), 1) for j, q in enumerate(Q) for r in range(2)]
    e += [(int(p), int(Z3[i % 50]), 2) for i, p in enumerate(P)]
    e += [(int(z), int(Z4[i % 10]), 1) for i, z in enumerate(Z3)]
    e += [(int(q), int(Z4[j % 10]), 2) for j, q in enumerate(Q)]
    e += [(int(p), int(Z4[i % 10]), 3) for i, p in enumerate(P)]
    e += [(int(v), 0, 1) for v in range(1, 206)]
    return W._finish(206, e, 4242, np.arange(206, dtype=np.uint32))


def test_mixed_level_behind_a_wave_walked_level(monkeypatch):
    case = mixed_case()
    n = _level_sizes(case, 0)
    assert n == [1, 100, 45, 50, 10]
    u2, u3, u4 = 206 - 1 - n[1], 206 - 1 - n[1] - n[2], n[4]
    assert n[1] <= u2 and n[1] + 1 > LIST_T   # level 2: push only
    assert n[2] <= u3 < n[1]                  # level 3: class 1 pushes, class 2 pulls
    assert min(n[1], n[2], n[3]) > u4         # level 4: every class but the source's pulls
    _agree(monkeypatch, case)


def test_pull_level_behind_a_wave_walked_level(monkeypatch):
    """test_gpu_level_lean.pull_case: level 2 of row 0 has 201 items (the wave
    walk) and leaves 3 vertices, which level 3 pulls."""
    _agree(monkeypatch, LN.pull_case(300, 3, 0))


# ------------------------------------------------------------ rows back to back
@pytest.mark.parametrize("dyn", ["1", "0"])
def test_workgroups_walk_rows_one_after_another(monkeypatch, dyn):
    _agree(monkeypatch, LC.complete_over(False), {"SRT_LVL_DYN": dyn})
