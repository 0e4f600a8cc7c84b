"""The graphs of the level solve's edge tests (tests/level_cases.py) reach the
branches they are named for: checked here on the CPU, with numpy and the
oracle only, so the GPU tests' "this graph runs that path" is proved and not
claimed.  Also pins the kernel constants the cases mirror: a retuned constant
fails here, which is the signal to move the edges.

Not built: a wave of lvl_out_kernel that serves an unstaged row and then a
staged one.  A wave takes rows u0 + wave + k * nwaves, and every launch has
min(8192, (rows + 3) / 4) workgroups of 4 waves, so a wave has a second row
only past 32,768 rows -- and a level plan has at most LEVEL_V_MAX = 18,400
(test_a_wave_of_the_out_rows_has_one_row)."""
import os
import re

import numpy as np
import pytest

import level_cases as LC
from oracle import oracle as O
from shadow_amd import NetworkGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shadow_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return int(m[0])


def test_constants_match_the_sources():
    lvl, fold, internal, api = _src("srt_level.hip"), _src("srt_rowfold.h"), _src("srt_internal.h"), _src("srt_api.cpp")
    assert _one(r"constexpr uint32_t OUT_SCAP = (\d+);", lvl) == LC.OUT_SCAP
    assert _one(r"const bool staged = cnt <= OUT_SCAP && e - b <= (\d+);", lvl) == LC.OUT_PLACE == 1 << 16
    assert len(re.findall(r"if \(j < OUT_SCAP\) stage\[wv\]\[j\] =", lvl)) == 2  # the u64 rows and the u16 copy
    assert _one(r"constexpr uint32_t TR_CH = (\d+);", fold) == LC.TR_CH
    assert "const uint64_t m = c < TR_CH ? bal[wv][c] : test(c);" in lvl
    assert _one(r"constexpr uint32_t LEVEL_V_MAX = (\d+);", internal) == LC.LEVEL_V_MAX
    assert "p->V <= srt::LEVEL_V_MAX" in api
    assert _one(r"constexpr uint32_t LWC = (\d+);", fold) == LC.LWC
    assert _one(r"constexpr uint32_t WC = (\d+);", fold) == LC.WC
    assert _one(r"constexpr size_t SOLVE_HIST = (\d+);", fold) == LC.SOLVE_HIST == 4 * (LC.LWC + 1)
    # the class-table rule, in both class-CSR builds
    assert lvl.count("const uint32_t cls = ncls < 16 ? 16 : ncls < 32 ? 32 : 64;") == 1
    assert lvl.count("const uint32_t cls = wmax < 16 ? 16 : wmax < 32 ? 32 : 64;") == 1
    assert [LC.class_table(b) for b in (0, 15, 16, 31, 32, 63)] == [16, 16, 32, 32, 64, 64]
    # the probe: its rows, its three integer bounds, its estimate
    assert _one(r"const uint32_t K = std::min<uint32_t>\((\d+), p->n\);", lvl) == LC.PROBE_ROWS
    assert "rows[k] = (uint32_t)((uint64_t)k * p->n / K);" in lvl
    assert tuple(int(a) for a, b in re.findall(r"probe\(std::min<uint64_t>\((\d+), maxu\), (\d+)\)", api)
                 if a == b) == LC.PROBE_WC
    assert _one(r"p->lvl_est = \(uint64_t\)\(\(double\)p->n_adj \* f\) \+ (\d+);", lvl) == LC.EST_SLACK
    assert "std::min(1.0, 2.0 * (double)wmax / (double)std::max<uint64_t>(maxu, 1))" in lvl
    # the largest LDS row (LEVEL_V_MAX vertices, 8 B each and the level ends) fits the launch's limit
    V = LC.LEVEL_V_MAX
    up16 = lambda b: (b + 15) & ~15
    assert LC.SOLVE_HIST + up16(2 * V) + 4 * V + up16(2 * V) <= 160 * 1024 - 1024 - 4096
    assert LC.level_vbits(V) == 15 and LC.level_vbits(1 << 14) == 14 and LC.level_vbits((1 << 14) + 1) == 15


def test_a_wave_of_the_out_rows_has_one_row():
    """Why no case mixes a staged and an unstaged row in one wave."""
    lvl = _src("srt_level.hip")
    assert _one(r"std::min<uint32_t>\((\d+), \(u1 - u0 \+ 3\) / 4\)", lvl) == LC.OUT_GRID
    assert "for (uint32_t u = u0 + wave; u < V; u += nwaves) {  // rows [u0, V)" in lvl
    for rows in (1, 2, 5, 1201, LC.LEVEL_V_MAX, 4 * LC.OUT_GRID):
        assert LC.out_rows_per_wave(rows) == 1
    assert LC.out_rows_per_wave(4 * LC.OUT_GRID + 1) == 2 and LC.LEVEL_V_MAX < 4 * LC.OUT_GRID


def test_short_counts_and_probe_rows():
    # rows: 0 -> {0 (loop, 1), 1 (5), 2 (6)}, 1 -> {}, 2 -> {0 (5), 0 (5), 2 (loop, 9)}
    row_ptr, col = [0, 3, 3, 6], [0, 1, 2, 0, 0, 2]
    lat = [1, 5, 6, 5, 5, 9]
    assert LC.short_counts(row_ptr, col, lat, 5).tolist() == [1, 0, 2]
    assert LC.short_counts(row_ptr, col, lat, 6).tolist() == [2, 0, 2]
    assert LC.short_counts(row_ptr, col, lat, 4).tolist() == [0, 0, 0]
    assert LC.probe_rows(1) == [0] and LC.probe_rows(2) == [0, 1] and LC.probe_rows(7) == list(range(7))
    assert LC.probe_rows(9) == [0, 1, 2, 3, 4, 5, 6, 7] and LC.probe_rows(20) == [0, 2, 5, 7, 10, 12, 15, 17]
    assert LC.units_of(np.array([6, 9, 300], np.uint64)) == (3, 100)
    assert LC.lvl_estimate(300_000, 15, 3000) == 3000 + 65536 and LC.lvl_estimate(10, 15, 20) == 10 + 65536


def _multiset_over_the_cap(counts):
    c = set(int(x) for x in counts)
    assert {LC.OUT_SCAP - 1, LC.OUT_SCAP, LC.OUT_SCAP + 1} <= c, sorted(c)[-8:]
    assert max(c) > LC.OUT_SCAP + 64


@pytest.mark.parametrize("directed", [False, True])
def test_hub_cap_rows_straddle_the_staging_cap(directed):
    case = LC.hub_cap(directed)
    og = LC.oracle_graph(case)
    assert case.n_nodes % 4 == 1 and len(case.nodes) == case.n_nodes and case.nodes[0] == 0
    assert LC.probe_bound(og, case.nodes) == 2 == case.bound
    row_ptr, col, lat, _ = LC.case_csr(case)
    g, maxu = LC.units_of(lat)
    assert g == LC.MS and maxu >= 40
    cnt = LC.short_counts(row_ptr, col, lat, 2 * g)
    _multiset_over_the_cap(cnt)
    for v, d in LC.CAP_DEGREES.items():
        assert cnt[v] == d
    assert cnt[0] == case.n_nodes - 1
    assert np.diff(row_ptr.astype(np.int64)).max() <= LC.OUT_PLACE
    # the in-rows: the same lists undirected, short ones for the chosen vertices when directed
    rows = np.repeat(np.arange(case.n_nodes), np.diff(row_ptr.astype(np.int64)))
    in_cnt = np.bincount(col[(lat <= np.uint64(2 * g)) & (col != rows)], minlength=case.n_nodes)
    if directed:
        assert all(in_cnt[v] == 1 for v in LC.CAP_DEGREES) and in_cnt.max() == case.n_nodes - 1
        assert sorted(in_cnt)[-2] <= 1 + len(LC.CAP_DEGREES)
    else:
        assert np.array_equal(in_cnt, cnt)
    # a 2-unit edge ties with the two hops through the hub, and the losses decide: both happen
    elat, eloss = O.compute_shortest_paths(og, case.nodes)
    assert int(elat[~np.eye(len(elat), dtype=bool)].max()) == 2 * g
    pos = np.empty(case.n_nodes, np.int64)
    pos[case.nodes] = np.arange(case.n_nodes)
    one = np.float32(1.0)
    direct = via = 0
    for e in np.nonzero((case.src == 4) & (case.lat == np.uint64(2 * g)))[0]:
        w = int(case.dst[e])
        h0 = case.loss[(case.src == 4) & (case.dst == 0)][0] if directed else case.loss[(case.src == 0) & (case.dst == 4)][0]
        h1 = case.loss[(case.src == 0) & (case.dst == w)][0]
        add = lambda a, b: one - (one - a) * (one - b)  # PathProperties' `+` on the losses
        two_hops, edge = add(add(np.float32(0), h0), h1), add(np.float32(0), case.loss[e])
        got = eloss[pos[4], pos[w]]
        assert got == min(two_hops, edge)
        direct += edge < two_hops
        via += two_hops < edge
    assert direct > 50 and via > 50


@pytest.mark.parametrize("V", [16_500, LC.LEVEL_V_MAX, LC.LEVEL_V_MAX + 1])
def test_hub_wide_row_and_in_use_list(V):
    case = LC.hub_wide(V)
    og = LC.oracle_graph(case)
    assert len(case.nodes) == 64 and case.nodes[0] == 0 and LC.probe_bound(og, case.nodes) == 2
    assert V - 1 in case.nodes and V - 2 in case.nodes and 7 in case.nodes
    row_ptr, col, lat, _ = LC.case_csr(case)
    b, e = int(row_ptr[0]), int(row_ptr[1])
    assert e - b == V > LC.TR_CH * 64
    # short entries past chunk TR_CH of the hub's row, whose heads are in use: their
    # losses are on the shortest paths of the table
    place = np.nonzero(lat[b:e] <= np.uint64(2 * LC.MS))[0]
    late = place[place >= LC.TR_CH * 64]
    assert len(late) >= 100 and np.isin(col[b:e][late], case.nodes).sum() >= 32
    cnt = LC.short_counts(row_ptr, col, lat, 2 * LC.MS)
    assert cnt[0] == V - 1 and cnt[7] == LC.OUT_SCAP + 1
    # in-use heads of vertex 7's 2-unit edges: the ties of the table
    heads = case.dst[(case.src == 7) & (case.lat == np.uint64(2 * LC.MS))]
    assert np.isin(heads, case.nodes).sum() >= 10


def test_hub_wide_ns_is_quantized_with_15_vertex_bits():
    case = LC.hub_wide(LC.LEVEL_V_MAX, True)
    g, maxu = LC.units_of(case.lat)
    assert g == 1 and LC.level_vbits(case.n_nodes) == 15
    assert LC.probe_bound(LC.oracle_graph(case), case.nodes) is None  # no bound within 63 ns
    q = LC.level_quantum(case)
    assert q == 1 << 19 and LC.MS <= int(case.lat[case.src != case.dst].min())
    # every shortest path (two hops through the hub, < 4 ms) within 31 buckets
    elat, _ = O.compute_shortest_paths(LC.oracle_graph(case), case.nodes)
    assert int(elat[~np.eye(64, dtype=bool)].max()) < 4 * LC.MS < 32 * q


@pytest.mark.parametrize("antipode", [False, True])
def test_circulant_rows_hold_exactly_the_cap(antipode):
    case = LC.circulant(antipode)
    n = case.n_nodes
    assert n == 1100 and n % 4 == 0 and case.hits == LC.OUT_SCAP + int(antipode)
    row_ptr, col, lat, loss = LC.case_csr(case)
    assert np.array_equal(row_ptr, np.arange(n + 1, dtype=np.uint64) * np.uint64(n))
    assert np.array_equal(col.reshape(n, n), np.tile(np.arange(n, dtype=np.uint32), (n, 1)))
    L, P = lat.reshape(n, n), loss.reshape(n, n)
    assert np.array_equal(L, L.T) and np.array_equal(P.view(np.uint32), P.T.view(np.uint32))  # rows=sym
    B = LC.probe_bound(LC.oracle_graph(case), case.nodes)
    assert B == 4
    for wmax in (B, 15):  # the run's bound and the first probe's
        assert set(LC.short_counts(row_ptr, col, lat, wmax * LC.MS).tolist()) == {case.hits}
    assert LC.units_of(lat)[1] < 0xffff  # the u16 copy applies


@pytest.mark.parametrize("ns", [False, True])
def test_complete_rows_are_all_over_the_cap(ns):
    case = LC.complete_over(ns)
    n = case.n_nodes
    row_ptr, col, lat, _ = LC.case_csr(case)
    g, maxu = LC.units_of(lat)
    if ns:
        q = LC.level_quantum(case)
        assert g == 1 and LC.probe_bound(LC.oracle_graph(case), case.nodes) is None
        assert LC.MS <= q < 2 * LC.MS and q < 1 << (34 - LC.level_vbits(n))
        wmax_ns = 32 * q - 1
    else:
        assert g == LC.MS and maxu == 3
        wmax_ns = LC.probe_bound(LC.oracle_graph(case), case.nodes) * g
        assert wmax_ns >= 3 * g
    assert set(LC.short_counts(row_ptr, col, lat, wmax_ns).tolist()) == {n - 1} and n - 1 > LC.OUT_SCAP + 64


@pytest.mark.parametrize("D", [15, 16, 31, 32, 63, 64])
def test_path_graph_bound_is_its_diameter(D):
    case = LC.path_graph(D, D)
    og = LC.oracle_graph(case)
    assert LC.units_of(case.lat) == (LC.MS, 1)
    elat, _ = O.compute_shortest_paths(og, case.nodes)
    off = ~np.eye(len(elat), dtype=bool)
    assert int(elat[off].max()) == D * LC.MS  # two vertices D apart: no bound below D
    assert int(elat[0][1:].max()) == (D + 1) // 2 * LC.MS and int(elat[:, 0][1:].max()) == D // 2 * LC.MS
    assert LC.probe_bound(og, case.nodes) == (D if D <= LC.LWC else None)
    assert LC.level_quantum(case) == 1  # no quantized solve either (q >= 2)


@pytest.mark.parametrize("w", [14, 15, 30, 31, 62, 63])
def test_two_cycle_bound_is_the_sum(w):
    case = LC.two_cycle(w)
    og = LC.oracle_graph(case)
    assert LC.units_of(case.lat) == (LC.MS, w)
    elat, _ = O.compute_shortest_paths(og, case.nodes)
    assert elat[0, 1] == w * LC.MS and elat[1, 0] == LC.MS
    B = LC.probe_bound(og, case.nodes)
    assert B == (w + 1 if w + 1 <= LC.LWC else None)
    if B is not None:
        # the edge 0 -> 1 is the last class the table of B classes has room for but one
        assert LC.class_table(B) == {15: 16, 16: 32, 31: 32, 32: 64, 63: 64}[B] and w == B - 1


def test_concentrated_count_exceeds_the_estimate():
    case = LC.concentrated()
    row_ptr, col, lat, _ = LC.case_csr(case)
    g, maxu = LC.units_of(lat)
    assert (g, maxu) == (LC.MS, 3000) and 290_000 < len(col) < 320_000
    wmax = min(LC.PROBE_WC[0], maxu)
    est = LC.lvl_estimate(len(col), wmax, maxu)
    count = int(LC.short_counts(row_ptr, col, lat, wmax * g).sum())
    assert est < 70_000 and count > 4 * est
    assert count == len(col) - case.n_nodes - 2  # everything but the self-loops and the long edge
    B = LC.probe_bound(LC.oracle_graph(case), case.nodes)
    assert B is not None and B <= 15  # the first probe (the one that sizes the arrays) finds it


def test_parallel_edges_are_kept_and_the_long_row_reaches_its_branch():
    """NetworkGraph.from_edges and the oracle both keep parallel edges, so a
    row of more than 65,536 entries can be built."""
    edges = ([0, 0, 0, 1, 2, 0, 1, 2], [1, 1, 1, 2, 0, 0, 1, 2], [9, 5, 7, 1, 1, 1, 1, 1],
             [0.5, 0.25, 0.125, 0, 0, 0, 0, 0])
    g = NetworkGraph.from_edges(3, *edges, directed=True)
    assert g.row_ptr.tolist() == [0, 4, 6, 8] and g.col[:4].tolist() == [1, 1, 1, 0] and g.lat_ns[:3].tolist() == [9, 5, 7]
    elat, eloss = O.compute_shortest_paths(O.Graph(True, np.arange(3), *edges), np.arange(3, dtype=np.uint32))
    assert elat[0, 1] == 5 and eloss[0, 1] == np.float32(0.25)  # the shortest of the three, with its loss
    case = LC.parallel_row_graph()
    row_ptr, col, lat, _ = LC.case_csr(case)
    b, e = int(row_ptr[0]), int(row_ptr[1])
    assert e - b > LC.OUT_PLACE and e - b > LC.TR_CH * 64
    B = LC.probe_bound(LC.oracle_graph(case), case.nodes)
    assert B == 2 == case.bound
    place = np.nonzero((lat[b:e] <= np.uint64(B * LC.MS)) & (col[b:e] != 0))[0]
    assert len(place) == case.n_nodes - 1 <= LC.OUT_SCAP and place.min() >= LC.OUT_PLACE
    assert LC.short_counts(row_ptr, col, lat, B * LC.MS)[0] == len(place)
    assert np.diff(row_ptr.astype(np.int64))[1:].max() < 64


@pytest.mark.parametrize("name", list(LC.RAGGED))
def test_ragged_cases(name):
    case = LC.ragged(name)
    V, isolated, _ = LC.RAGGED[name]
    n = len(case.nodes)
    assert case.n_nodes == V + isolated and len(np.unique(case.nodes)) == n
    B = LC.probe_bound(LC.oracle_graph(case), case.nodes)
    assert B is not None and (B == 0) == (n == 1)
    row_ptr, col, _, _ = LC.case_csr(case)
    deg = np.diff(row_ptr.astype(np.int64))
    if name in ("v302", "v303", "v303-source-last"):
        last_quad = V - V % 4
        assert V % 4 in (2, 3) and (case.nodes >= last_quad).sum() >= 2 and V - 1 in case.nodes
        assert case.nodes[-1] == V - 1 or case.nodes[0] == V - 1
    if name.startswith("n"):
        assert n == int(name[1:]) and len(LC.probe_rows(n)) == min(8, n)
    if isolated:
        # the unused vertices: their self-loop and nothing else, no edge reaches them
        assert (deg[V:] == 1).all() and (col[row_ptr[V:-1].astype(np.int64)] == np.arange(V, V + isolated)).all()
        assert not np.isin(col[: int(row_ptr[V])], np.arange(V, V + isolated)).any() and case.nodes.max() < V
