"""The kept class structure of symmetric integer-level plans (srt_level.hip:
level_keep at the create keeps the prefix "classes 1..B" of every row of the
probe's class rows, lvl_fill_kernel fills the run's losses into it).  Every
case creates the plan with SRT_LVL_KEEP=1 and with SRT_LVL_KEEP=0 (every run
builds the rows from the adjacency): one table bit for bit on the device
(latency, and the loss bits as i32), one minimum latency, one edge-visit count,
the oracle's table -- and the create's trace line `[srt] level keep: ...` in
the one and not in the other.

  sparse rows    the 200-vertex complete graph of 1-300 ms, every vertex in use
                 and 120 of them; and a graph whose 80 unused vertices have no
                 edge within the bound (empty kept rows: every in-use vertex has
                 one, being reached within B -- test_level_keep_cpu.py);
  entry forms    V = 255, 256, 257 on 4-byte entries, 8-byte entries and the
                 unpacked row;
  overflow       a loss that does not fit the 4-byte entry: the repeat fills the
                 8-byte form from the same kept structure;
  long rows      1,024 / 1,025 kept entries a row, and rows all over 1,024;
  strides        bounds of 24 (32 offsets a vertex) and 60 (64);
  three runs     of one plan;
  not eligible   general rows, SRT_LVL_SYM=0, a quantized plan: no line, the
                 same table;
  one call       srt_compute_shortest_paths with mirrored losses, and with a
                 pair whose losses do not mirror (the run builds in-rows)."""
import functools

import numpy as np
import pytest

import level_cases as LC
import test_gpu_level_ce4 as G
import test_gpu_level_edges as E
from shadow_amd import _lib, synth
from shadow_amd.graph import NetworkGraph

pytestmark = pytest.mark.gpu

TRACE = "[srt] level keep: "
CE4, CE8, NOPACK = G.CE4, G.CE8, G.NOPACK


# ------------------------------------------------------------ graphs
@functools.lru_cache(maxsize=None)
def complete200(in_use):
    """synth.complete_csr(200, 1) in identity rows; the first `in_use` of a seeded permutation in use."""
    edges = synth.complete_graph(200, 1)
    nodes = np.arange(200) if in_use == 200 else np.random.default_rng(3).permutation(200)[:in_use]
    return LC._case(200, *edges, False, nodes, csr=synth.complete_csr(200, 1, edges=edges))


USED, UNUSED = 120, 80


@functools.lru_cache(maxsize=None)
def empty_rows_case():
    """200 vertices, the first 120 in use: a ring of unit pairs over them and each
    pair of them at 1-3 units with probability 0.03; every pair with an unused
    vertex is 40-300 units, past any bound the probe proves: 80 empty kept rows."""
    rng = np.random.default_rng(77)
    short = {}
    iu, ju = np.nonzero(np.triu(rng.random((USED, USED)) < 0.03, 1))
    for a, b, u in zip(iu, ju, rng.integers(1, 4, size=len(iu))):
        short[(int(a), int(b))] = int(u)
    for i in range(USED):
        short[(min(i, (i + 1) % USED), max(i, (i + 1) % USED))] = 1
    case = G.sym_case(USED + UNUSED, short, {}, 77)
    case.nodes = np.arange(USED, dtype=np.uint32)
    return case


@functools.lru_cache(maxsize=None)
def ring_case(n):
    """A ring of n unit pairs inside a complete graph of 40-300-unit pairs: every
    eccentricity is n / 2, the probe's bound n."""
    return G.sym_case(n, {(min(i, (i + 1) % n), max(i, (i + 1) % n)): 1 for i in range(n)}, {}, 500 + n)


@functools.lru_cache(maxsize=None)
def identity_ns():
    """test_gpu_auto.py's identity_ns graph: 1-20 ms plus a sub-ms offset, gcd 1 ns (the quantized solve)."""
    return LC.complete_identity(200, 2, lat_ms=(1, 20), ns=True)


@functools.lru_cache(maxsize=None)
def sym257(over):
    return G.random_sym(257, 9057, {(0, 1): G.over_min(9)} if over else None)


# ------------------------------------------------------------ the comparison
def _create(monkeypatch, capfd, case, keep, extra=None):
    """(plan, the create said it kept a structure)."""
    capfd.readouterr()
    p = E._plan(monkeypatch, case, dict(extra or {}, SRT_LVL_KEEP=keep, SRT_TRACE="1"))
    return p, TRACE in capfd.readouterr().err


def _same(monkeypatch, capfd, case, extra=None, eligible=True, runs=1, overflow=False, oracle=True):
    """KEEP=1 and KEEP=0: the trace line, the table, the minimum, the visits, the oracle."""
    import torch

    a, said_a = _create(monkeypatch, capfd, case, "1", extra)
    b, said_b = _create(monkeypatch, capfd, case, "0", extra)
    try:
        assert said_a == eligible and not said_b
        assert a.describe() == b.describe() and a.describe().startswith("level:"), (a.describe(), b.describe())
        ce4 = G.CE_TOKEN in a.describe()
        assert ce4 or not overflow
        b.run()
        Lb, Pb, _, _ = E._tables(b)
        for _ in range(runs):
            a.run()
            La, Pa, la, pa = E._tables(a)
            assert torch.equal(La, Lb) and torch.equal(Pa, Pb), a.describe()
            assert a.timing()["edge_visits"] == b.timing()["edge_visits"] > 0
            la.zero_()
            pa.zero_()
        assert a.describe() == b.describe()
        assert (G.CE_TOKEN in a.describe()) == (ce4 and not overflow)
        a.run()  # (after an overflow: on 8-byte entries from its start)
        La, Pa, _, _ = E._tables(a)
        assert torch.equal(La, Lb) and torch.equal(Pa, Pb)
        assert a.timing()["edge_visits"] == b.timing()["edge_visits"]
        ta, tb = a.fetch(), b.fetch()
        assert ta.min_latency_ns == tb.min_latency_ns
        if oracle:
            E._check(ta, case)
        return a.describe()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------ sparse rows
@pytest.mark.parametrize("in_use", [200, 120])
def test_complete_graph_of_200(monkeypatch, capfd, in_use):
    d = _same(monkeypatch, capfd, complete200(in_use))
    assert "rows=sym" in d, d


def test_rows_that_keep_nothing(monkeypatch, capfd):
    d = _same(monkeypatch, capfd, empty_rows_case())
    assert "rows=sym" in d and LC.lmax_of(d) < 40, d


# ------------------------------------------------------------ vertex bits, entry forms
@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("env", [CE4, CE8, NOPACK], ids=["ce4", "ce8", "unpacked"])
def test_vertex_bits_and_entry_forms(monkeypatch, capfd, n, env):
    d = _same(monkeypatch, capfd, G.random_sym(n, 8800 + n), env)
    assert (G.CE_TOKEN in d) == (env is CE4), d


# ------------------------------------------------------------ overflow
def test_overflow_repeats_on_the_kept_structure(monkeypatch, capfd):
    """Through srt_plan_run: the repeat is the fill's 8-byte form, the plan leaves ' ce=4', the next run is right."""
    case = sym257(True)
    assert case.units[0, 1] == 1 and G.delta_of(case.loss[(case.src == 0) & (case.dst == 1)][0]) == 1 << 23
    d = _same(monkeypatch, capfd, case, CE4, overflow=True)
    assert G.CE_TOKEN not in d


def test_overflow_through_run_async_and_fetch(monkeypatch, capfd):
    import torch

    case = sym257(True)
    a, said = _create(monkeypatch, capfd, case, "1", CE4)
    b, _ = _create(monkeypatch, capfd, case, "0", CE4)
    try:
        assert said and G.CE_TOKEN in a.describe()
        a.run_async()
        t = a.fetch()
        assert G.CE_TOKEN not in a.describe()
        E._check(t, case)
        b.run()
        La, Pa, _, _ = E._tables(a)
        Lb, Pb, _, _ = E._tables(b)
        assert torch.equal(La, Lb) and torch.equal(Pa, Pb)
        E._check(a.run().fetch(), case)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------ long rows
@pytest.mark.parametrize("which", ["1024", "1025", "all-over", "all-over-lat16"])
def test_long_rows(monkeypatch, capfd, which):
    case = LC.complete_over(False) if which.startswith("all") else LC.circulant(which == "1025")
    _same(monkeypatch, capfd, case, {"SRT_LAT16": "1"} if which.endswith("lat16") else None)


# ------------------------------------------------------------ other strides
@pytest.mark.parametrize("n", [24, 60])
def test_bounds_past_16_offsets(monkeypatch, capfd, n):
    d = _same(monkeypatch, capfd, ring_case(n))
    assert LC.lmax_of(d) == n and LC.class_table(n) == (32 if n == 24 else 64), d


# ------------------------------------------------------------ three runs
def test_three_runs_of_one_plan(monkeypatch, capfd):
    _same(monkeypatch, capfd, sym257(False), CE4, runs=3)


# ------------------------------------------------------------ not eligible
@pytest.mark.parametrize("which", ["general-rows", "sym-off", "quantized"])
def test_not_eligible_plans_keep_nothing(monkeypatch, capfd, which):
    if which == "general-rows":
        case, extra = LC.ragged("v303"), None
    elif which == "sym-off":
        case, extra = complete200(200), {"SRT_LVL_SYM": "0"}
    else:
        case, extra = identity_ns(), None
    d = _same(monkeypatch, capfd, case, extra, eligible=False)
    assert ("rows=sym" in d) == (which == "quantized") and d.startswith("level:u32 " if which == "quantized" else "level:u16 "), d


# ------------------------------------------------------------ the one-call build
@pytest.mark.parametrize("mirrored", [True, False], ids=["mirrored", "one-pair-not"])
def test_one_call_build(monkeypatch, mirrored):
    """srt_compute_shortest_paths uploads only the needed losses (listed from the
    kept structure) and checks their mirrors: a pair that differs sends the run
    to the in-rows path."""
    err = _lib.SrtErr()
    assert _lib.lib().srt_init(0, err) == 0  # pins the staging the needed-loss upload uses
    case = sym257(False)
    row_ptr, col, lat, loss = LC.case_csr(case)
    if not mirrored:
        loss = loss.copy()
        assert case.units[3, 4] == 1 and loss[3 * 257 + 4] == loss[4 * 257 + 3]
        loss[3 * 257 + 4] = np.float32(0.25)  # 3 -> 4 only: 4 -> 3 keeps its loss
    g = NetworkGraph(257, np.arange(257, dtype=np.uint32), row_ptr, col, lat, loss, directed=False)
    out = []
    for keep in ("1", "0"):
        monkeypatch.setenv("SRT_LVL_KEEP", keep)
        out.append(g.compute_shortest_paths(case.nodes, algo=E.LEVEL))
    monkeypatch.delenv("SRT_LVL_KEEP")
    assert np.array_equal(out[0].latency_ns, out[1].latency_ns)
    assert np.array_equal(E._bits(out[0].packet_loss), E._bits(out[1].packet_loss))
    assert out[0].min_latency_ns == out[1].min_latency_ns
    if mirrored:
        E._check(out[0], case)
    else:
        elat, _ = E._expected(case)
        assert np.array_equal(out[0].latency_ns, elat)
        assert not np.array_equal(E._bits(out[0].packet_loss), E._bits(E._expected(case)[1]))  # the changed loss is read
