"""The 4-byte-entry packed level solve in workgroups of 640 and 768 threads
(srt_level.hip level_ce4_wide_kernel<NT, 640 | 768, 2>: the body of
level_ce4_kernel with the workgroup's own thread and wave counts -- 10 or 12
waves share a level's batches, its reductions and its row passes -- and the
chunk walk at two entry pairs a lane, 16-entry chunks).

The 4-byte entries are a symmetric plan's, so the graphs are complete and
undirected (test_gpu_level_ce4.sym_case: the short pairs of 1 to 3 units, every
other pair of 40 to 300).  Every case runs packed on 4-byte entries with
SRT_LVL_CE4_NT = 768, 640 and 512, packed on 8-byte entries (SRT_LVL_CE4=0) and
unpacked: one table bit for bit on the device (latency, and the loss bits as
i32), one edge-visit count, one minimum latency, and the oracle's table.

  level size   T = LIST_T + 1 (the first level not listed); T = 2 nw - 1, 2 nw +
               1 for nw = 10 and 12 waves (a wave with one item, with two);
               T = nw (WAVE_B - 1) + 1, the first T whose waves' share ceil(T /
               nw) reaches WAVE_B, and one over; 511, 512, 513;
  list length  vertex 0's class-1 list, the first entries of the array, has 1,
               63, 64, 65, 128, 129 entries, and the last vertex's one-entry
               list is the array's last entry (a pass's lanes past the list read
               its last entry: here the end of the array); a level whose class-2 and class-3
               items have empty lists, the last item of the last batch among
               them (all but two of the 20 class-2 lists are empty, so batches
               begin with one too, wherever the members were listed);
  one owner    one head hit by 85 and by 350 entries at once, from several
               waves; the candidates arrive in increasing order (only the first
               lowers the key), in decreasing order (every one does) and all
               equal (ties).  A loss of 1 (the bits of 1.0f) does not fit a
               4-byte entry (its difference is 0x3f800000), nor does 1/2 past
               512 vertices: the losses are those of {0, 1/2, 1/4, 1/8} that
               fit (85: all four; 350, vb = 10: 0 and 1/8, 1/16, 1/32), and the
               all-ones case runs too -- through the overflow repeat;
  mixed level  a level that pushes class 2 (lists of 15, 16, 17 and 33 entries:
               the chunk walk's 16-entry chunks at two pairs a lane, starting
               at odd and at even places) and pulls class 1, right behind a
               wave-walked level, then a pull level;
  rows         1,100 rows over at most 512 resident workgroups, dealt by the
               counter and statically: the batch counter and the fused init are
               used again by a 12-wave workgroup's next row;
  knob         SRT_LVL_CE4_NT = 700 is refused; unset, the plan takes the widest
               count of which the occupancy query keeps two workgroups a CU
               (SRT_TRACE prints the choice and the three answers);
  overflow     one loss past the 4-byte field at 768 threads: the run repeats on
               8-byte entries (512 threads) and matches the unpacked table."""
import os
import re

import numpy as np
import pytest

import level_cases as LC
import test_gpu_level_ce4 as G
import test_gpu_level_edges as E
import test_gpu_level_walk as W
import test_gpu_level_wave as WV
import test_level_packed_cpu as PC
import test_level_walk_resources as WR
from shadow_amd import _lib

pytestmark = pytest.mark.gpu

LIST_T, WAVE_B = WV.LIST_T, WV.WAVE_B
THREADS = (768, 640, 512)
CE8, NOPACK = G.CE8, G.NOPACK


def ce4_env(threads):
    return dict(G.CE4, SRT_LVL_CE4_NT=str(threads))


def test_constants():
    """The thread counts in the source: PACK_NT and the wide instantiations'."""
    src = open(os.path.join(WV.CSRC, "srt_level.hip")).read()
    (wide,) = re.findall(r"constexpr uint32_t CE4_WIDE_NT\[\] = \{(\d+), (\d+)\};", src)
    assert tuple(sorted(map(int, wide), reverse=True)) + (WR._pack_nt(),) == THREADS
    assert re.search(r"__launch_bounds__\(NTH, 2 \* NTH / 256\) void level_ce4_wide_kernel", src)
    for t in THREADS[:2]:
        assert f"level_ce4_wide_kernel<true, {t}, 2>" in src and f"level_ce4_wide_kernel<false, {t}, 2>" in src


# ------------------------------------------------------------ the comparison
def _agree(monkeypatch, case, extra=None, overflow=False):
    """768, 640 and 512 threads on 4-byte entries, 8-byte entries and unpacked: one
    table, one visit count, one minimum, the oracle's table.  overflow: every
    first run on 4-byte entries must have left them."""
    import torch

    runs = []
    try:
        for env in [ce4_env(t) for t in THREADS] + [CE8, NOPACK]:
            p = E._plan(monkeypatch, case, dict(env, **(extra or {})))
            runs.append(p)
            if "SRT_LVL_CE4_NT" in env:
                assert G.CE_TOKEN in p.describe(), p.describe()  # chosen at the create
            p.run()
        d = [p.describe() for p in runs]
        assert all("rows=sym" in x for x in d), d
        assert all(W.TOKEN in x for x in d[:4]) and W.TOKEN not in d[4], d
        assert all((G.CE_TOKEN in x) == (not overflow) for x in d[:3]) and G.CE_TOKEN not in d[3] + d[4], d
        assert len({x.replace(G.CE_TOKEN, "") for x in d[:4]}) == 1, d  # the thread count is not described
        assert LC.lmax_of(d[0]) <= PC.PACK_LMAX and len({LC.lmax_of(x) for x in d}) == 1, d
        L0, P0, _, _ = E._tables(runs[4])
        vis, mins = [], []
        for p in runs:
            L, P, _, _ = E._tables(p)
            assert torch.equal(L0, L) and torch.equal(P0, P), p.describe()
            vis.append(p.timing()["edge_visits"])
            p.fetch(table=False)
            mins.append(p.min_latency_ns)
        assert vis[0] > 0 and vis == [vis[0]] * 5, vis
        assert mins == [mins[0]] * 5, mins
        E._check(runs[0].fetch(), case)
    finally:
        for p in runs:
            p.close()


def _sym(n, short, loss, seed):
    """sym_case with the pairs in any order."""
    key = lambda a, b: (min(a, b), max(a, b))
    return G.sym_case(n, {key(a, b): u for (a, b), u in short.items()}, {key(a, b): e for (a, b), e in loss.items()}, seed)


# ------------------------------------------------------------ level size
def level_case(T):
    """0 - T - 1 vertices A at 1 unit and - every b of max(200, T) vertices B at
    2 units, each a - 33 to 62 of B at 1 unit: row 0's level 2 has T items, A on
    class 1 and the source on class 2 (its list of four or more passes the last
    item of the last batch), and is a push (T - 1 tails, |B| unsettled)."""
    n1, nb = T - 1, max(200, T)
    short = {(0, a): 1 for a in range(1, 1 + n1)}
    short.update({(0, 1 + n1 + b): 2 for b in range(nb)})
    for i in range(n1):
        for r in range(33 + i % 30):
            short[(1 + i, 1 + n1 + (7 * i + r) % nb)] = 1
    return _sym(1 + n1 + nb, short, {}, 300 + T)


def share_reaches_wave_b(nw):
    """The smallest T with ceil(T / nw) = WAVE_B."""
    return nw * (WAVE_B - 1) + 1


SIZES = sorted({LIST_T + 1, 19, 21, 23, 25, 511, 512, 513} |
               {share_reaches_wave_b(nw) + d for nw in (10, 12) for d in (0, 1)})


@pytest.mark.parametrize("T", SIZES)
def test_level_of_t_items(monkeypatch, T):
    assert {19, 21, 23, 25} == {2 * nw + d for nw in (10, 12) for d in (-1, 1)} and LIST_T + 1 < 19
    case = level_case(T)
    sizes = G.level_sizes(case, 0)
    assert sizes == [1, T - 1, case.n_nodes - T] and T - 1 <= case.n_nodes - T and T > LIST_T  # level 2: a push of T items
    _agree(monkeypatch, case)


# ------------------------------------------------------------ list length
NPOOL = 132


def lists_case(m):
    """Source 1 - A = {0, 2 .. F, n - 1} at 1 unit (F + 1 > LIST_T items) and -
    every pool vertex at 2 units; vertex 0 - pool[0 .. m - 1) at 1 unit: its
    class-1 list (the source and those: m entries) lies first in the entry
    array; the last vertex has the source alone: its list is the array's last
    entry; every other a - 10 pool vertices at 1 unit.  Row 1: level 2 has F + 2
    items (A and the source's class 2) and is a push."""
    F = LIST_T + 2
    n = 1 + F + NPOOL + 1  # 0 .. F, the pool, the last vertex
    pool = list(range(F + 1, F + 1 + NPOOL))
    A = [0] + list(range(2, F + 1)) + [n - 1]
    short = {(1, a): 1 for a in A}
    short.update({(1, b): 2 for b in pool})
    short.update({(0, pool[i]): 1 for i in range(m - 1)})
    for q, a in enumerate(range(2, F + 1)):
        short.update({(a, pool[(10 * q + r) % NPOOL]): 1 for r in range(10)})
    return _sym(n, short, {}, 7000 + m)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 128, 129])
def test_list_of_m_entries_at_the_ends_of_the_array(monkeypatch, m):
    case = lists_case(m)
    n, U = case.n_nodes, case.units
    short = U < 40
    assert int(short[0].sum()) == m and not short[0, 0]            # vertex 0: one list of m entries, from entry 0 on
    assert int(short[n - 1].sum()) == 1 and U[n - 1, 1] == 1       # the last vertex: one entry, the array's last
    sizes = G.level_sizes(case, 1)
    assert sizes == [1, LIST_T + 3, NPOOL] and sizes[1] + 1 > LIST_T and sizes[1] <= NPOOL  # level 2: a push of 20 items
    _agree(monkeypatch, case)


def empty_lists_case():
    """0 - A (20) at 1 unit; a - 3 of B (60) at 1 unit; b - 4 of C (200) at 1 unit;
    a_0 - c_0 and a_1 - c_1 at 2 units and no other pair at 2 or 3.  Row 0's
    level 3 pushes B on class 1 (60 items), A on class 2 (20 items, 18 lists
    empty) and the source on class 3 (the last item, its list empty)."""
    A, B, C = range(1, 21), range(21, 81), range(81, 281)
    short = {(0, a): 1 for a in A}
    for i, b in enumerate(B):
        for r in range(3):
            short[(A[(i + 7 * r) % 20], b)] = 1
    for i, c in enumerate(C):
        for r in range(4):
            short[(B[(3 * i + 17 * r) % 60], c)] = 1
    short[(A[0], C[0])] = 2
    short[(A[1], C[1])] = 2
    return _sym(281, short, {}, 8100)


def test_empty_lists_first_and_last_in_a_batch(monkeypatch):
    case = empty_lists_case()
    assert G.level_sizes(case, 0) == [1, 20, 60, 200]
    U = case.units
    assert sorted(int((U[a] == 2).sum()) for a in range(1, 21)) == [0] * 18 + [1, 1] and not (U[0] == 3).any()
    assert 60 <= 200 and 60 + 20 + 1 > LIST_T  # level 3: every class pushes, 81 items
    _agree(monkeypatch, case)


# ------------------------------------------------------------ one owner
def owner_case(tails, order):
    """0 - `tails` vertices A at 1 unit without loss, every a - H at 1 unit and -
    three of `tails` + 50 vertices B: row 0's level 2 (tails + 1 items, a push)
    hits H from `tails` entries at once.  The pairs (a, H) lose, by a's place:
    'inc' non-decreasing, 'dec' non-increasing, 'equal' all the same, 'ones' all
    1 (which no 4-byte entry holds: the overflow repeat)."""
    nb = tails + 50
    n = 2 + tails + nb
    H = 1 + tails
    vb = LC.level_vbits(n)
    steps = [e for e in (0.0, 0.125, 0.25, 0.5) if G.delta_of(e) < 1 << (32 - vb)]
    if len(steps) < 4:
        steps = [0.0, 0.03125, 0.0625, 0.125]
    assert all(G.delta_of(e) < 1 << (32 - vb) for e in steps)
    short = {(0, a): 1 for a in range(1, 1 + tails)}
    loss = {(0, a): 0.0 for a in range(1, 1 + tails)}
    for i in range(tails):
        a = 1 + i
        short[(a, H)] = 1
        k = (4 * i) // tails
        loss[(a, H)] = {"inc": steps[k], "dec": steps[3 - k], "equal": steps[2], "ones": 1.0}[order]
        for r in range(3):
            short[(a, H + 1 + (3 * i + r) % nb)] = 1
    return _sym(n, short, loss, 500 + tails)


@pytest.mark.parametrize("order", ["inc", "dec", "equal"])
@pytest.mark.parametrize("tails", [85, 350])
def test_one_head_hit_from_many_waves(monkeypatch, tails, order):
    case = owner_case(tails, order)
    assert G.level_sizes(case, 0)[:2] == [1, tails] and tails + 1 > LIST_T and tails <= case.n_nodes - 1 - tails
    assert int((case.units[1 + tails] == 1).sum()) == tails  # H: `tails` tight in-edges in row 0's level 2
    _agree(monkeypatch, case)


def test_one_head_hit_by_ties_of_one(monkeypatch):
    """Every candidate the bits of 1.0f: past the 4-byte field, so the run repeats on 8-byte entries."""
    _agree(monkeypatch, owner_case(85, "ones"), overflow=True)


# ------------------------------------------------------------ mixed and pull levels
MIXED_LISTS = (15, 16, 17, 33)


def mixed_case():
    """0 - A (20) at 1 unit; every b of B (140) - one or two of A at 1 unit; every
    c of C (40) - three of B at 1 unit; a_k - C at 2 units: a_0 .. a_3 have
    class-2 lists of 15, 16, 17 and 33 entries; every d of D (5) - two of C at 1
    unit.  Row 0: level 2 pushes (21 items: the wave walk); level 3 pulls class
    1 (140 tails, 45 unsettled) and pushes classes 2 and 3 (20 tails, 1): the
    chunk walk; level 4 (5 unsettled) pulls."""
    A, B, C, D = range(1, 21), range(21, 161), range(161, 201), range(201, 206)
    short = {(0, a): 1 for a in A}
    for i, b in enumerate(B):
        short[(A[i % 20], b)] = 1
        if i % 3 == 0:
            short[(A[(i + 9) % 20], b)] = 1
    for i, c in enumerate(C):
        for r in range(3):
            short[(B[(5 * i + 47 * r) % 140], c)] = 1
    for k, m in enumerate(MIXED_LISTS):
        for r in range(m):
            short[(A[k], C[(11 * k + r) % 40])] = 2
    for i, d in enumerate(D):
        for r in range(2):
            short[(C[(7 * i + 3 * r) % 40], d)] = 1
    return _sym(206, short, {}, 4242)


def test_mixed_level_behind_a_wave_walked_level(monkeypatch):
    case = mixed_case()
    U = case.units
    assert G.level_sizes(case, 0) == [1, 20, 140, 40, 5]
    assert 20 + 1 > LIST_T and 20 <= 185        # level 2: push only
    assert 140 > 45 and 20 <= 45                # level 3: class 1 pulls, class 2 pushes
    assert min(40, 140, 20) > 5                 # level 4: pulls
    assert tuple(int((U[a] == 2).sum()) for a in range(1, 5)) == MIXED_LISTS
    # the entry array: vertex-major, class-major; where each of the four lists starts
    deg = (U < 40).sum(axis=1)
    starts = [int(deg[:a].sum() + (U[a] == 1).sum()) for a in range(1, 5)]
    assert {s % 2 for s in starts} == {0, 1}, starts
    _agree(monkeypatch, case)


# ------------------------------------------------------------ rows back to back
@pytest.mark.parametrize("dyn", ["1", "0"])
def test_workgroups_walk_rows_one_after_another(monkeypatch, dyn):
    _agree(monkeypatch, LC.complete_over(False), {"SRT_LVL_DYN": dyn})


# ------------------------------------------------------------ the knob
def test_invalid_thread_count_is_refused(monkeypatch):
    case = G.random_sym(255, 9055)
    with pytest.raises(_lib.SrtError) as ei:
        E._plan(monkeypatch, case, ce4_env(700)).close()
    assert ei.value.code == _lib.SRT_ERR_INVALID and "SRT_LVL_CE4_NT" in str(ei.value)


def _traced_threads(capfd):
    err = capfd.readouterr().err
    (m,) = re.findall(r"\[srt\] level ce4: (\d+) threads a workgroup( \(forced\))? "
                      r"\(workgroups a CU: 768 x(\d+), 640 x(\d+), 512 x(\d+)\)", err)
    return int(m[0]), bool(m[1]), dict(zip(THREADS, map(int, m[2:])))


def test_unset_takes_the_widest_count_that_fits_twice(monkeypatch, capfd):
    case = G.random_sym(255, 9055)
    capfd.readouterr()
    p = E._plan(monkeypatch, case, dict(G.CE4, SRT_TRACE="1"))
    try:
        chosen, forced, fits = _traced_threads(capfd)
        assert not forced and fits[512] >= 2
        assert chosen == max(t for t in THREADS if fits[t] >= 2)
        E._check(p.run().fetch(), case)
    finally:
        p.close()
    p = E._plan(monkeypatch, case, dict(ce4_env(640), SRT_TRACE="1"))
    try:
        assert _traced_threads(capfd)[:2] == (640, True)
    finally:
        p.close()


# ------------------------------------------------------------ overflow
def test_overflow_at_768_threads_repeats_on_8_byte_entries(monkeypatch):
    e = G.over_min(9)
    case = G.random_sym(257, 9057, {(0, 1): e})
    assert case.vb == 9 and G.delta_of(e) == 1 << (32 - 9) and case.units[0, 1] == 1
    _agree(monkeypatch, case, overflow=True)
