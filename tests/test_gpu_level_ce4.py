"""The packed level solve on 4-byte class entries (srt_level.hip: lvl_out_kernel
<..., CE4> writes v | (0x3f800000 - bits(1f32 - e)) << vb, vb the bits of V - 1,
and every walker of level_ce4_kernel, the packed row's body, decodes it).  The form is
a symmetric plan's (identity rows, mirrored latencies and losses: the in-rows
are the out-rows), so the graphs here are complete and undirected, their short
pairs of 1 to 4 units and every other pair of 40 to 300.  Every case runs packed
with SRT_LVL_CE4=1, packed with SRT_LVL_CE4=0 and unpacked: one table bit for
bit on the device (latency, and the loss bits as i32), one edge-visit count,
one minimum latency, and the oracle's table.

  vertex bits  V = 255, 256, 257: vb = 8, 8, 9; the top vertex's index has every
               mask bit set at 256 and is the first of a new bit at 257;
  field edges  losses of exactly 0 (difference 0) and the largest loss that fits
               (difference 2^(32 - vb) - 1 where an f32 loss has it: vb >= 9; the
               largest one below at vb = 8) on edges that shortest paths use;
  overflow     the smallest loss whose difference is 2^(32 - vb), on one edge that
               is a shortest path: the run repeats on 8-byte entries, returns
               their table, describes itself without ' ce=4' from then on, and
               its next run is right too -- through srt_plan_run and through
               srt_plan_run_async + srt_plan_fetch;
  walkers      row 0 of walker_case: a listed level, a wave-walked level whose
               lists have 63 / 64 / 65 / 129 entries, a level that pushes one
               class and pulls another, and a pull level;
  rows         1,100 rows over at most 512 resident workgroups, dealt by the
               counter and statically."""
import numpy as np
import pytest

import level_cases as LC
import test_gpu_level_edges as E
import test_gpu_level_walk as W
import test_level_packed_cpu as PC
from shadow_amd import synth

pytestmark = pytest.mark.gpu

CE4 = {"SRT_LVL_PACK": "1", "SRT_LVL_CE4": "1"}
CE8 = {"SRT_LVL_PACK": "1", "SRT_LVL_CE4": "0"}
NOPACK = {"SRT_LVL_PACK": "0"}
CE_TOKEN = " ce=4"
ONE = 0x3F800000  # bits of 1.0f
LIST_T = 16       # srt_level.hip SRT_LIST_T (test_constants of test_gpu_level_lean.py pins it)


# ------------------------------------------------------------ the field's arithmetic
def delta_of(e):
    """0x3f800000 - bits(1f32 - e): what the 4-byte entry keeps of a loss."""
    x = np.float32(1.0) - np.float32(e)
    return ONE - int(np.float32(x).view(np.uint32))


def loss_with_delta(d):
    """An f32 loss in [0, 1] whose difference is exactly d, or None (below 0.5
    the spacing of 1 - e is finer than that of e: not every d has one)."""
    x = np.uint32(ONE - d).view(np.float32)
    e0 = np.float32(1.0 - float(x))
    for e in (e0, np.nextafter(e0, np.float32(0)), np.nextafter(e0, np.float32(1))):
        if 0.0 <= float(e) <= 1.0 and delta_of(e) == d:
            return np.float32(e)
    return None


def fit_max(vb):
    """(loss, difference): the largest difference below 2^(32 - vb) that a loss has."""
    d = (1 << (32 - vb)) - 1
    while loss_with_delta(d) is None:
        d -= 1
    return loss_with_delta(d), d


def over_min(vb):
    """The smallest loss whose difference does not fit: 2^(32 - vb) exactly."""
    e = loss_with_delta(1 << (32 - vb))
    assert e is not None
    return e


# ------------------------------------------------------------ graphs
def sym_case(n, short, loss, seed):
    """The complete undirected graph over n vertices in identity rows: the pairs
    of `short` {(i, j): units} (i < j), every other pair 40-300 units, self-loops
    of 3 units; losses U[0, 0.05] but for the pairs of `loss` {(i, j): f32}.
    Every vertex in use, in node order."""
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 0)
    units = rng.integers(40, 301, size=len(iu)).astype(np.int64)
    units[iu == ju] = 3
    ls = LC._losses(rng, len(iu))
    at = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(iu, ju))}
    for (a, b), u in short.items():
        assert a < b
        units[at[(a, b)]] = u
    for (a, b), e in loss.items():
        assert a < b and (a, b) in short
        ls[at[(a, b)]] = np.float32(e)
    edges = (iu.astype(np.uint32), ju.astype(np.uint32), units.astype(np.uint64) * np.uint64(LC.MS), ls)
    U = np.full((n, n), 1 << 20, np.int64)
    for (a, b), u in short.items():
        U[a, b] = U[b, a] = u
    return LC._case(n, *edges, False, np.arange(n), csr=synth.complete_csr(n, seed, edges=edges), units=U,
                    vb=LC.level_vbits(n))


def level_sizes(case, s):
    """Vertices at each distance (units) from s over the short pairs: [1, |N_1|, |N_2|, ...]."""
    n, U = case.n_nodes, case.units
    d = np.full(n, 1 << 20, np.int64)
    d[s] = 0
    while True:
        nd = np.minimum(d, (d[:, None] + U).min(axis=0))
        if np.array_equal(nd, d):
            return np.bincount(d).tolist()
        d = nd


def random_sym(n, seed, extra_loss=None):
    """A ring of unit pairs plus each pair with probability 0.08 at 1-3 units.
    The ring pairs (0, 1) and (n - 2, n - 1) lose exactly 0, (1, 2) and (0, n - 1)
    the largest loss that fits: each is the one shortest path between its ends."""
    rng = np.random.default_rng(seed)
    short = {}
    iu, ju = np.nonzero(np.triu(rng.random((n, n)) < 0.08, 1))
    for a, b, u in zip(iu, ju, rng.integers(1, 4, size=len(iu))):
        short[(int(a), int(b))] = int(u)
    for i in range(n):
        a, b = min(i, (i + 1) % n), max(i, (i + 1) % n)
        short[(a, b)] = 1
    vb = LC.level_vbits(n)
    big, _ = fit_max(vb)
    loss = {(0, 1): 0.0, (n - 2, n - 1): 0.0, (1, 2): big, (0, n - 1): big}
    loss.update(extra_loss or {})
    return sym_case(n, short, loss, seed)


NA, NB, NC, ND = 20, 140, 30, 5
LISTS = (63, 64, 65, 129)


def walker_case(extra_loss=None):
    """0 - A (20 vertices) at 1 unit; a_k - B (140) at 1 unit: a_0 .. a_3 have
    class-1 lists of 63 / 64 / 65 / 129 entries (the pair with 0 among them), the
    other a 11, and every b has a neighbour in A; B - C (30) at 1 unit, A - C at
    2 units; C - D (5) at 1 unit.  Row 0: level 1 is one item (listed); level 2
    has 21 items and pushes (the wave walk); level 3 pulls class 1 (140 tails,
    35 unsettled) and pushes classes 2 and 3 (20 tails, 1); level 4 (5 unsettled)
    pulls classes 1 to 3 and pushes the source's."""
    A = np.arange(1, 1 + NA)
    B = np.arange(1 + NA, 1 + NA + NB)
    C = np.arange(1 + NA + NB, 1 + NA + NB + NC)
    D = np.arange(1 + NA + NB + NC, 1 + NA + NB + NC + ND)
    short = {(0, int(a)): 1 for a in A}
    at = 0
    for k, a in enumerate(A):
        m = (LISTS[k] if k < len(LISTS) else 11) - 1
        for r in range(m):
            short[(int(a), int(B[(at + r) % NB]))] = 1
        at += m if k >= len(LISTS) else 0  # the long lists overlap, the short ones tile B
    for i, c in enumerate(C):
        for r in range(3):
            short[(int(B[(5 * i + 47 * r) % NB]), int(c))] = 1
        short[(int(A[i % NA]), int(c))] = 2
    for i, d in enumerate(D):
        for r in range(2):
            short[(int(C[(7 * i + 3 * r) % NC]), int(d))] = 1
    n = 1 + NA + NB + NC + ND
    big, _ = fit_max(LC.level_vbits(n))
    loss = {(0, 1): 0.0, (0, 2): big, (1, int(B[0])): big, (2, int(B[1])): 0.0}
    loss.update(extra_loss or {})
    return sym_case(n, short, loss, 9100)


# ------------------------------------------------------------ the comparison
def _agree(monkeypatch, case, extra=None, overflow=False):
    """4-byte entries, 8-byte entries and unpacked: one table, one visit count,
    one minimum, the oracle's table.  overflow: the first run on 4-byte entries
    must have left them."""
    import torch

    runs = []
    try:
        for env in (CE4, CE8, NOPACK):
            p = E._plan(monkeypatch, case, dict(env, **(extra or {})))
            runs.append(p)
            if env is CE4:
                assert CE_TOKEN in p.describe(), p.describe()  # chosen at the create, before any run
            p.run()
        d = [p.describe() for p in runs]
        assert all("rows=sym" in x for x in d), d
        assert W.TOKEN in d[0] and W.TOKEN in d[1] and W.TOKEN not in d[2], d
        assert (CE_TOKEN in d[0]) == (not overflow) and CE_TOKEN not in d[1] and CE_TOKEN not in d[2], d
        assert d[0].replace(CE_TOKEN, "") == d[1], d
        assert LC.lmax_of(d[0]) <= PC.PACK_LMAX and len({LC.lmax_of(x) for x in d}) == 1, d
        L0, P0, _, _ = E._tables(runs[1])
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
        if overflow:  # the next run: on 8-byte entries from its start
            L, P, lb, pb = E._tables(runs[0])
            lb.zero_()
            pb.zero_()
            runs[0].run()
            assert CE_TOKEN not in runs[0].describe()
            assert torch.equal(L0, L) and torch.equal(P0, P)
            assert runs[0].timing()["edge_visits"] == vis[1]
    finally:
        for p in runs:
            p.close()


def _deltas(case):
    """The differences of the short pairs' losses."""
    real = (case.src != case.dst) & (case.lat < np.uint64(40 * LC.MS))
    return np.array([delta_of(e) for e in case.loss[real]], np.int64)


# ------------------------------------------------------------ vertex bits, field edges
@pytest.mark.parametrize("n", [255, 256, 257])
def test_vertex_bits_and_field_edges(monkeypatch, n):
    case = random_sym(n, 8800 + n)
    vb = case.vb
    assert vb == (9 if n == 257 else 8) and (n - 1) >> (vb - 1) == 1  # the top vertex uses the top bit
    assert n != 256 or n - 1 == (1 << vb) - 1                        # ... every mask bit at 256
    _, dmax = fit_max(vb)
    assert dmax == (1 << (32 - vb)) - (1 if vb >= 9 else 2)
    d = _deltas(case)
    assert d.min() == 0 and d.max() == dmax and d.max() < 1 << (32 - vb)
    _agree(monkeypatch, case)


# ------------------------------------------------------------ every walker
def test_listed_wave_mixed_and_pull_levels(monkeypatch):
    case = walker_case()
    n = level_sizes(case, 0)
    assert n == [1, NA, NB, NC, ND]
    u2, u3, u4 = NB + NC + ND, NC + ND, ND
    assert 1 <= LIST_T < NA + 1 and NA <= u2             # level 1 listed; level 2: 21 items, push only
    assert NB > u3 and NA <= u3                          # level 3: class 1 pulls, class 2 pushes
    assert min(NC, NB, NA) > u4                          # level 4: classes 1 to 3 pull
    row = case.units
    got = sorted(int(np.sum(row[a] == 1)) for a in range(1, 5))
    assert got == sorted(LISTS)                          # the wave-walked lists: 63 / 64 / 65 / 129 entries
    d = _deltas(case)
    assert d.min() == 0 and d.max() == fit_max(case.vb)[1]
    _agree(monkeypatch, case)


# ------------------------------------------------------------ overflow
@pytest.mark.parametrize("which", ["v257", "walker"])
def test_a_loss_that_does_not_fit_falls_back(monkeypatch, which):
    """One pair's loss has the difference 2^(32 - vb) exactly: the pair (0, 1), a
    unit edge and so the one shortest path between its ends."""
    vb = 9 if which == "v257" else LC.level_vbits(1 + NA + NB + NC + ND)
    e = over_min(vb)
    assert delta_of(e) == 1 << (32 - vb) and float(e) == (0.5 if vb == 9 else 0.75)
    case = random_sym(257, 9057, {(0, 1): e}) if which == "v257" else walker_case({(0, 1): e})
    assert case.vb == vb and case.units[0, 1] == 1
    d = _deltas(case)
    assert int(np.sum(d >= 1 << (32 - vb))) == 1 and d.max() == 1 << (32 - vb)
    _agree(monkeypatch, case, overflow=True)


def test_fallback_through_run_async_and_fetch(monkeypatch):
    """No srt_plan_sync between the run and the fetch: the fetch reads the
    overflow word and repeats the run."""
    case = random_sym(257, 9057, {(0, 1): over_min(9)})
    p = E._plan(monkeypatch, case, CE4)
    try:
        assert CE_TOKEN in p.describe()
        p.run_async()
        t = p.fetch()
        assert CE_TOKEN not in p.describe() and W.TOKEN in p.describe()
        E._check(t, case)
        E._check(p.run().fetch(), case)
    finally:
        p.close()


# ------------------------------------------------------------ rows back to back
@pytest.mark.parametrize("dyn", ["1", "0"])
def test_workgroups_walk_rows_one_after_another(monkeypatch, dyn):
    """(the counter's case also reads the out-rows from the u16-unit adjacency copy, as the 16k build does)"""
    extra = {"SRT_LVL_DYN": dyn}
    if dyn == "1":
        extra["SRT_LAT16"] = "1"
    _agree(monkeypatch, LC.complete_over(False), extra)
