"""The level solve (srt_level.hip) at its kernel constants: class-CSR rows
at and over the staging cap (OUT_SCAP), a row of more than 65,536 entries, an
entry estimate too small, the needed-loss index past its LDS chunks (TR_CH),
LEVEL_V_MAX, the bounds where the class table changes size, reruns over a
clobbered table, and small / ragged in-use lists.  The graphs are
tests/level_cases.py's; tests/test_level_cases_cpu.py proves on the CPU that
each reaches its branch.  Every table is compared bit for bit with the
oracle's; the bound a plan reports with the hand-derived one or the oracle's
restatement of the probe (level_cases.probe_bound)."""
import numpy as np
import pytest

import level_cases as LC
from oracle import oracle as O
from shadow_amd import RoutingInfo, _lib
from shadow_amd import dist as sdist
from shadow_amd.plan import RoutingPlan

pytestmark = pytest.mark.gpu

LEVEL = _lib.SRT_ALGO_LEVEL


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _expected(case):
    """The oracle's whole table over case.nodes, computed once a case."""
    if not hasattr(case, "_expected"):
        elat, eloss = O.compute_shortest_paths(LC.oracle_graph(case), case.nodes)
        elat.setflags(write=False)
        eloss.setflags(write=False)
        case._expected = (elat, eloss)
    return case._expected


def _expected_rows(case, rows):
    """The oracle's rows `rows` (places in case.nodes) in the table's column order."""
    n = len(case.nodes)
    rest = np.setdiff1d(np.arange(n), rows)
    order = np.concatenate([rows, rest]).astype(np.int64)
    elat, eloss = O.compute_shortest_paths(LC.oracle_graph(case), case.nodes[order], src_count=len(rows))
    inv = np.empty(n, np.int64)
    inv[order] = np.arange(n)
    return elat[: len(rows)][:, inv], eloss[: len(rows)][:, inv]


def _check(t, case):
    elat, eloss = _expected(case)
    assert np.array_equal(t.latency_ns, elat)
    assert np.array_equal(_bits(t.packet_loss), _bits(eloss))
    assert t.min_latency_ns == int(elat.min())


def _plan(monkeypatch, case, env=None, algo=LEVEL, graph=None):
    """A plan created with the knobs `env` (read at the create)."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        return RoutingPlan(graph or LC.network_graph(case), case.nodes, algo=algo, device=0)
    finally:
        for k in env or {}:
            monkeypatch.delenv(k)


def _tables(p):
    """(latency i64 [n, n], loss bits i32 [n, n], both as bytes): views of the plan's device table."""
    import torch

    la, pa, n = p.table_ptrs()
    dev = torch.device("cuda", 0)
    lb = torch.as_tensor(sdist._CudaBuf(la, n * n * 8), device=dev)
    pb = torch.as_tensor(sdist._CudaBuf(pa, n * n * 4), device=dev)
    return lb.view(torch.int64).view(n, n), pb.view(torch.int32).view(n, n), lb, pb


def _check_device_rows(p, case, rows, elat, eloss, diagonal=True):
    L, P, _, _ = _tables(p)
    for k, r in enumerate(rows):
        got_l = L[int(r)].cpu().numpy().view(np.uint64)
        got_p = P[int(r)].cpu().numpy().view(np.uint32)
        m = np.ones(len(got_l), bool)
        m[int(r)] = diagonal  # fewer oracle rows than nodes: the oracle leaves the diagonal unset
        assert np.array_equal(got_l[m], elat[k][m]) and np.array_equal(got_p[m], _bits(eloss[k])[m]), f"row {r}"


def _assert_counts_straddle_the_cap(case, lmax):
    row_ptr, col, lat, _ = LC.case_csr(case)
    g, _ = LC.units_of(lat)
    c = set(LC.short_counts(row_ptr, col, lat, lmax * g).tolist())
    assert {LC.OUT_SCAP - 1, LC.OUT_SCAP, LC.OUT_SCAP + 1} <= c and max(c) > LC.OUT_SCAP + 64


# ------------------------------------------------------------ the staging cap
@pytest.mark.parametrize("directed,env", [(False, None), (True, None), (False, {"SRT_LVL_SP": "0"})],
                         ids=["undirected", "directed", "undirected-per-item-walk"])
def test_general_rows_at_and_over_the_staging_cap(monkeypatch, directed, env):
    """Hub graph, V = 1,201: class-CSR rows of 1,023 / 1,024 / 1,025 / 1,150 /
    1,200 entries at the run's bound (2), read through their columns; directed:
    the long rows on the out side only."""
    case = LC.hub_cap(directed)
    p = _plan(monkeypatch, case, env)
    try:
        d = p.describe()
        assert d.startswith("level:u16 ") and "rows=sym" not in d and LC.lmax_of(d) == 2 == case.bound, d
        _assert_counts_straddle_the_cap(case, LC.lmax_of(d))
        _check(p.run().fetch(), case)
    finally:
        p.close()


def _three_builds_agree(monkeypatch, case, kind, lat16):
    """Default, SRT_LAT16=1 and SRT_LVL_SYM=0 builds of an identity-row graph:
    the three tables equal on the device, 6 rows of them the oracle's."""
    import torch

    a = _plan(monkeypatch, case).run()
    b = _plan(monkeypatch, case, {"SRT_LAT16": "1"}).run()
    c = _plan(monkeypatch, case, {"SRT_LVL_SYM": "0"}).run()
    try:
        da, db, dc = a.describe(), b.describe(), c.describe()
        assert all(d.startswith(kind) for d in (da, db, dc)), (da, db, dc)
        assert "rows=sym" in da and "rows=sym" in db and "rows=sym" not in dc, (da, db, dc)
        assert "lat16" not in da and ("lat16" in db) == lat16 and "lat16" not in dc, (da, db, dc)
        assert LC.lmax_of(da) == LC.lmax_of(db) == LC.lmax_of(dc)
        La, Pa, _, _ = _tables(a)
        for other in (b, c):
            Lo, Po, _, _ = _tables(other)
            assert torch.equal(La, Lo) and torch.equal(Pa, Po), other.describe()
        n = len(case.nodes)
        rows = np.sort(np.random.default_rng(n).choice(n, 6, replace=False))
        elat, eloss = _expected_rows(case, rows)
        _check_device_rows(a, case, rows, elat, eloss, diagonal=False)
        a.fetch(table=False)
        assert a.min_latency_ns == int(case.lat.min())  # a complete graph: the shortest edge or self-loop
        return da
    finally:
        for p in (a, b, c):
            p.close()


@pytest.mark.parametrize("antipode", [False, True], ids=["1024-hits", "1025-hits"])
def test_identity_rows_at_and_over_the_staging_cap(monkeypatch, antipode):
    """Circulant complete graphs, n = 1,100, every row exactly 1,024 (staged) or
    1,025 (tested again) hits at the bound 4: the u64 identity rows, the u16
    copy and (SRT_LVL_SYM=0) the rows with columns."""
    case = LC.circulant(antipode)
    d = _three_builds_agree(monkeypatch, case, "level:u16 ", lat16=True)
    assert LC.lmax_of(d) == 4
    row_ptr, col, lat, _ = LC.case_csr(case)
    assert set(LC.short_counts(row_ptr, col, lat, 4 * LC.MS).tolist()) == {LC.OUT_SCAP + int(antipode)}


@pytest.mark.parametrize("ns", [False, True], ids=["units", "ns"])
def test_identity_rows_all_over_the_staging_cap(monkeypatch, ns):
    """A complete graph of 1-3 ms, n = 1,100: all 1,099 entries of every row
    are hits; its ns twin writes the quantized entries (remainder | vertex) in
    the rows that are tested again."""
    case = LC.complete_over(ns)
    d = _three_builds_agree(monkeypatch, case, "level:u32 " if ns else "level:u16 ", lat16=not ns)
    row_ptr, col, lat, _ = LC.case_csr(case)
    if ns:
        assert f" g=1 q={LC.level_quantum(case)} " in d, d
    else:
        assert LC.lmax_of(d) == LC.probe_bound(LC.oracle_graph(case), case.nodes)
    g, _ = LC.units_of(lat)
    assert set(LC.short_counts(row_ptr, col, lat, LC.lmax_of(d) * g).tolist()) == {case.n_nodes - 1}


def test_row_of_more_than_65536_entries(monkeypatch):
    """66,000 parallel edges ahead of vertex 0's 63 short ones: few enough hits
    to stage, but their places do not fit 16 bits, so the row is tested again;
    the one-call build lists its needed losses past the LDS chunks (it runs
    first: after the plan's full upload of the same graph, a loss that was not
    uploaded could be found where the plan left it)."""
    case = LC.parallel_row_graph()
    err = _lib.SrtErr()
    assert _lib.lib().srt_init(0, err) == 0  # pins the staging the needed-loss upload uses
    _check(LC.network_graph(case).compute_shortest_paths(case.nodes, algo=LEVEL), case)
    p = _plan(monkeypatch, case)
    try:
        d = p.describe()
        assert d.startswith("level:u16 ") and LC.lmax_of(d) == 2 == case.bound, d
        _check(p.run().fetch(), case)
    finally:
        p.close()


# ------------------------------------------------------------ the estimate
@pytest.mark.parametrize("algo", [LEVEL, _lib.SRT_ALGO_AUTO], ids=["level", "auto"])
def test_entry_estimate_too_small(monkeypatch, algo):
    """~300k entries of 1-9 units and one edge of 3,000: the first probe's
    arrays are sized for ~68k entries, the count says 300k, they are sized
    again and the pass runs again; the bound is the one the whole class CSR
    gives."""
    case = LC.concentrated()
    p = _plan(monkeypatch, case, algo=algo)
    try:
        d = p.describe()
        assert d.startswith("level:u16 "), d
        assert LC.lmax_of(d) == LC.probe_bound(LC.oracle_graph(case), case.nodes), d
        _check(p.run().fetch(), case)
    finally:
        p.close()


# ------------------------------------------------------------ wide hub rows
def _check_off_diagonal(lat, loss, case):
    elat, eloss = _expected(case)
    off = ~np.eye(len(elat), dtype=bool)
    assert np.array_equal(lat[off], elat[off]) and np.array_equal(_bits(loss)[off], _bits(eloss)[off])


def test_needed_loss_index_past_the_lds_chunks(monkeypatch):
    """Hub graph, V = 16,500: the hub's row has 258 chunks of 64 entries, two
    more than lvl_index_kernel keeps ballots for.  The one-call builds upload
    only the listed losses; half the in-use nodes are heads of the hub's last
    entries."""
    err = _lib.SrtErr()
    assert _lib.lib().srt_init(0, err) == 0  # pins the staging the upload uses
    case = LC.hub_wide(16_500)
    g = LC.network_graph(case)
    _check(g.compute_shortest_paths(case.nodes, algo=LEVEL), case)
    a = RoutingInfo.build(g, case.nodes, algo=LEVEL, device=0)
    monkeypatch.setenv("SRT_LOSS_FULL", "1")
    b = RoutingInfo.build(g, case.nodes, algo=LEVEL, device=0)
    try:
        la, pa = a.table()
        lb, pb = b.table()
        assert np.array_equal(la, lb) and np.array_equal(_bits(pa), _bits(pb))
        _check_off_diagonal(la, pa, case)
        assert a.get_smallest_latency_ns() == int(_expected(case)[0].min())
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("ns", [False, True], ids=["units", "ns"])
def test_level_v_max(monkeypatch, ns):
    """V = LEVEL_V_MAX = 18,400: the largest LDS row, u16 member ids up to
    18,399 (the last 32 vertices are in use); ns: 15 vertex bits and 19
    remainder bits an entry."""
    case = LC.hub_wide(LC.LEVEL_V_MAX, ns)
    p = _plan(monkeypatch, case)
    try:
        d = p.describe()
        if ns:
            assert d.startswith("level:u32 ") and f" g=1 q={LC.level_quantum(case)} " in d and LC.level_quantum(case) == 1 << 19, d
        else:
            assert d.startswith("level:u16 ") and LC.lmax_of(d) == 2, d
        _check(p.run().fetch(), case)
    finally:
        p.close()


def test_level_v_max_plus_one_is_refused(monkeypatch):
    """V = 18,401: forced LEVEL is refused, AUTO takes another family with the
    oracle's table."""
    case = LC.hub_wide(LC.LEVEL_V_MAX + 1)
    g = LC.network_graph(case)
    with pytest.raises(_lib.SrtError) as e:
        RoutingPlan(g, case.nodes, algo=LEVEL, device=0)
    assert e.value.code == _lib.SRT_ERR_UNSUPPORTED
    p = _plan(monkeypatch, case, algo=_lib.SRT_ALGO_AUTO, graph=g)
    try:
        assert not p.describe().startswith("level:"), p.describe()
        _check(p.run().fetch(), case)
    finally:
        p.close()


# ------------------------------------------------------------ the bounds
def _bound_case(monkeypatch, case):
    p = _plan(monkeypatch, case)
    try:
        d = p.describe()
        assert d.startswith("level:u16 ") and LC.lmax_of(d) == case.bound, d
        _check(p.run().fetch(), case)
    finally:
        p.close()


@pytest.mark.parametrize("D", [15, 16, 31, 32, 63])
def test_bound_at_the_class_table_edges(monkeypatch, D):
    """Caterpillars of unit edges whose probe bound is exactly D: 16 / 32 / 64
    class offsets a vertex on either side of 15 | 16 and 31 | 32, and D = 63,
    whose last level ends in the last word of the level ends."""
    _bound_case(monkeypatch, LC.path_graph(D, D))


def test_bound_64_is_refused():
    case = LC.path_graph(64, 64)
    with pytest.raises(_lib.SrtError) as e:
        RoutingPlan(LC.network_graph(case), case.nodes, algo=LEVEL, device=0)
    assert e.value.code == _lib.SRT_ERR_UNSUPPORTED


@pytest.mark.parametrize("w", [14, 15, 30, 31, 62])
def test_two_cycle_largest_class(monkeypatch, w):
    """0 -> 1 of w units, 1 -> 0 of 1: the bound is w + 1, the long edge the
    largest class but one of its table."""
    _bound_case(monkeypatch, LC.two_cycle(w))


# ------------------------------------------------------------ reruns
def _rerun_case(kind):
    if kind == "quantized":
        edges = LC.random_edges(300, 47, 0.08, lat=(LC.MS, 10 * LC.MS - 1), unit=1)
        return LC._case(300, *edges, False, np.random.default_rng(47).permutation(300))
    if kind == "sym":
        return LC.complete_identity(400, 49, lat_ms=(1, 40))
    return LC.ragged("v303")


_RERUN_CASES = {}


@pytest.mark.parametrize("kind", ["integer", "quantized", "sym", "shard", "static-rows"])
def test_rerun_rebuilds_a_clobbered_table(monkeypatch, kind):
    """run(); both device tables filled with 0xA5 bytes; run() again: the table
    is the oracle's, three times over -- a second run that wrote nothing (the
    dynamic row counter left past its rows, the class CSR not rebuilt) shows.
    shard: srt_plan_shard_rows(3, 1), its own rows; static-rows: SRT_LVL_DYN=0."""
    import torch

    case = _RERUN_CASES.setdefault(kind, _rerun_case(kind))
    elat, eloss = _expected(case)
    n = len(case.nodes)
    p = _plan(monkeypatch, case, {"SRT_LVL_DYN": "0"} if kind == "static-rows" else None)
    try:
        d = p.describe()
        assert d.startswith("level:u32 " if kind == "quantized" else "level:u16 ") and ("rows=sym" in d) == (kind == "sym"), d
        r0, r1 = (n // 3, 2 * n // 3) if kind == "shard" else (0, n)
        if kind == "shard":
            p.shard_rows(3, 1)
        p.run()
        for _ in range(3):
            L, P, lb, pb = _tables(p)
            lb.fill_(0xA5)
            pb.fill_(0xA5)
            torch.cuda.synchronize()
            assert int(L[r0, 0].item()) == -0x5A5A5A5A5A5A5A5B
            p.run()
            L, P, _, _ = _tables(p)
            got_l, got_p = L[r0:r1].cpu().numpy().view(np.uint64), P[r0:r1].cpu().numpy().view(np.uint32)
            assert np.array_equal(got_l, elat[r0:r1]) and np.array_equal(got_p, _bits(eloss[r0:r1]))
            p.fetch(table=False)
            if kind != "shard":
                assert p.min_latency_ns == int(elat.min())
    finally:
        p.close()


# ------------------------------------------------------------ small and ragged
@pytest.mark.parametrize("name", list(LC.RAGGED))
def test_small_and_ragged_in_use_lists(monkeypatch, name):
    """V mod 4 of 2 and 3 with sources in the last partial quad; 1, 2, 7 and 9
    in-use nodes (the probe takes min(8, n) rows); 20 unused vertices that no
    edge reaches, so the solve never settles all V."""
    case = LC.ragged(name)
    p = _plan(monkeypatch, case)
    try:
        d = p.describe()
        assert d.startswith("level:u16 ") and LC.lmax_of(d) == LC.probe_bound(LC.oracle_graph(case), case.nodes), d
        _check(p.run().fetch(), case)
    finally:
        p.close()
