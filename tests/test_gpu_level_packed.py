"""The level solve's packed LDS row (level_solve_kernel PK: a u32 key of state
| loss bits and a 4-bit level a vertex, the members in a per-workgroup global
scratch): forced with SRT_LVL_PACK=1 on the small graphs of
tests/level_cases.py, at the level cap 14 | 15, on the pull side of the walk,
over reruns, in the in-process multi-GPU build, and unforced on either side of
the two plan sizes between which it is the default.  Every table is compared
bit for bit, latency and loss bits, with the oracle's or with the unpacked
row's on the device.  tests/test_level_packed_cpu.py derives the sizes and
proves, from the oracle's distances, which graphs pull and reach level 14."""
import numpy as np
import pytest

import level_cases as LC
import test_gpu_level_edges as E
import test_level_packed_cpu as PC
from shadow_amd import RoutingInfo, _lib

pytestmark = pytest.mark.gpu

LEVEL = _lib.SRT_ALGO_LEVEL
TOKEN = " row=packed"
PACK, NOPACK = {"SRT_LVL_PACK": "1"}, {"SRT_LVL_PACK": "0"}

_SMALL = {
    "hub-cap-undirected": lambda: LC.hub_cap(False),
    "hub-cap-directed": lambda: LC.hub_cap(True),
    "circulant": lambda: LC.circulant(False),
    "complete-400": lambda: _complete(),
}
_SMALL.update({f"ragged-{name}": (lambda name=name: LC.ragged(name)) for name in LC.RAGGED})
_SMALL.update({f"ragged-short-{name}": (lambda name=name: PC.ragged_short(name)) for name in LC.RAGGED})
_CASES = {}


def _complete():
    """Some level of every row takes the pull side (test_level_packed_cpu.py)."""
    return _CASES.setdefault("complete", LC.complete_identity(400, 49, lat_ms=(1, 40)))


def _token_in_place(d):
    """` row=packed` after the rows= part, before auto-price=."""
    assert d.count(TOKEN) == 1, d
    head, tail = d.split(TOKEN)
    assert "auto-price=" not in head and "rows=" not in tail, d
    assert tail == "" or tail.startswith(" auto-price="), d
    if "rows=sym" in d:
        assert head.endswith("rows=sym") or head.endswith("rows=sym lat16"), d


@pytest.mark.parametrize("name", list(_SMALL))
def test_forced_packed_row_equals_the_unpacked_row(monkeypatch, name):
    """SRT_LVL_PACK=1 against SRT_LVL_PACK=0 on the device, and the oracle.
    Six of the eight RAGGED graphs (edges of 1-9 units) have probe bounds of 16
    or 18, past the 4-bit levels, so forcing must leave them unpacked (n1 and
    n2, bounds 0 and 12, run packed); their ragged-short twins -- the same
    sizes and in-use lists over edges of 1-5 units, bounds <= 12
    (test_level_packed_cpu.py) -- put V mod 4 of 2 and 3, sources in the last
    quad, 1 to 9 in-use nodes and vertices that never settle on the packed row."""
    import torch

    case = _SMALL[name]()
    a = E._plan(monkeypatch, case, PACK)
    b = E._plan(monkeypatch, case, NOPACK)
    try:
        da, db = a.describe(), b.describe()
        if LC.lmax_of(da) <= PC.PACK_LMAX:
            _token_in_place(da)
        else:
            assert name in PC.RAGGED_PAST_THE_CAP and TOKEN not in da, da
        assert TOKEN not in db and da.replace(TOKEN, "") == db, (da, db)
        a.run()
        b.run()
        La, Pa, _, _ = E._tables(a)
        Lb, Pb, _, _ = E._tables(b)
        assert torch.equal(La, Lb) and torch.equal(Pa, Pb), da
        E._check(a.fetch(), case)
    finally:
        a.close()
        b.close()


def test_small_plans_are_unpacked_by_default(monkeypatch):
    p = E._plan(monkeypatch, LC.ragged("v303"))
    try:
        assert TOKEN not in p.describe(), p.describe()
    finally:
        p.close()


@pytest.mark.parametrize("make,packed", [(lambda: LC.path_graph(14, 14), True), (lambda: LC.two_cycle(13), True),
                                         (lambda: LC.path_graph(15, 15), False), (lambda: LC.two_cycle(14), False)],
                         ids=["path-14", "two-cycle-13", "path-15", "two-cycle-14"])
def test_the_level_cap(monkeypatch, make, packed):
    """Bound 14: the last level a 4-bit field holds; bound 15: never packed,
    even when forced."""
    case = make()
    p = E._plan(monkeypatch, case, PACK)
    try:
        d = p.describe()
        assert d.startswith("level:u16 ") and LC.lmax_of(d) == case.bound == (14 if packed else 15), d
        assert (TOKEN in d) == packed, d
        E._check(p.run().fetch(), case)
    finally:
        p.close()


@pytest.mark.parametrize("kind", ["integer", "sym", "shard", "static-rows"])
def test_rerun_rebuilds_a_clobbered_table(monkeypatch, kind):
    """As test_gpu_level_edges.py's, with the packed row: the table filled with
    0xA5 bytes and run again, three times."""
    import torch

    case = _complete() if kind == "sym" else PC.ragged_short("v303")
    elat, eloss = E._expected(case)
    n = len(case.nodes)
    env = dict(PACK, SRT_LVL_DYN="0") if kind == "static-rows" else PACK
    p = E._plan(monkeypatch, case, env)
    try:
        d = p.describe()
        _token_in_place(d)
        assert ("rows=sym" in d) == (kind == "sym"), d
        r0, r1 = (n // 3, 2 * n // 3) if kind == "shard" else (0, n)
        if kind == "shard":
            p.shard_rows(3, 1)
        p.run()
        for _ in range(3):
            L, P, lb, pb = E._tables(p)
            lb.fill_(0xA5)
            pb.fill_(0xA5)
            torch.cuda.synchronize()
            assert int(L[r0, 0].item()) == -0x5A5A5A5A5A5A5A5B
            p.run()
            L, P, _, _ = E._tables(p)
            got_l, got_p = L[r0:r1].cpu().numpy().view(np.uint64), P[r0:r1].cpu().numpy().view(np.uint32)
            assert np.array_equal(got_l, elat[r0:r1]) and np.array_equal(got_p, E._bits(eloss[r0:r1]))
            p.fetch(table=False)
            if kind != "shard":
                assert p.min_latency_ns == int(elat.min())
    finally:
        p.close()


def test_in_process_multi_gpu(monkeypatch):
    """Two contexts on one device, each with its own scratch, their rows staged
    as u16 units + f32 loss: the one-device table, and the oracle's off the
    diagonal."""
    case = _complete()
    g = LC.network_graph(case)
    monkeypatch.setenv("SRT_LVL_PACK", "1")
    one = RoutingInfo.build(g, case.nodes, algo=LEVEL, device=0)
    two = RoutingInfo.build(g, case.nodes, algo=LEVEL, device=0, n_gpus=2, same_device=True)
    try:
        l1, p1 = one.table()
        l2, p2 = two.table()
        assert np.array_equal(l1, l2) and np.array_equal(E._bits(p1), E._bits(p2))
        E._check_off_diagonal(l2, p2, case)
    finally:
        one.close()
        two.close()


_LO, _HI = PC.default_edges()


@pytest.mark.parametrize("V,packed", [(_LO, False), (_LO + 1, True), (_HI, True), (_HI + 1, False)],
                         ids=["below", "first", "last", "past"])
def test_default_choice_at_its_edges(monkeypatch, V, packed):
    """Unforced, on either side of the sizes the layout functions give (the
    unpacked row allows fewer than two workgroups a CU, the packed row two):
    sparse hub graphs of bound 2, 64 in-use nodes."""
    case = LC.hub_wide(V)
    p = E._plan(monkeypatch, case)
    try:
        d = p.describe()
        assert d.startswith("level:u16 ") and LC.lmax_of(d) == 2, d
        assert (TOKEN in d) == packed, d
        if packed:
            _token_in_place(d)
        E._check(p.run().fetch(), case)
    finally:
        p.close()
