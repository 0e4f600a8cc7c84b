"""GPU test of the AUTO family chooser (srt_choose.cpp price_fw / price_sparse):
priced from the measured rates per key type and symmetry, it must pick the
faster family on a mid-density graph the old flat pricing (Vp^3 / 1.2e13
against 64 B per source-edge at 3e12 B/s) sent to the sparse sweeps."""
import json
import os

import numpy as np
import pytest

from shadow_amd import NetworkGraph, _lib, synth
from shadow_amd.plan import RoutingPlan

pytestmark = pytest.mark.gpu


def _device_ms(g, nodes, algo):
    p = RoutingPlan(g, nodes, algo=algo, device=0)
    try:
        best = float("inf")
        for _ in range(2):
            p.run()
            best = min(best, p.kernel_stats()[3])
        return best, p.describe()
    finally:
        p.close()


def test_auto_picks_faster_family_mid_density():
    # 16k-node BA graph, m = 16 (mean degree 32): old prices fw 366 ms vs
    # sparse 189 ms (picked sparse); measured-rate prices fw ~58 vs ~105 ms
    n = 16384
    src, dst, lat, loss = synth.barabasi_albert(n, 16, 5)
    g = NetworkGraph.from_edges(n, src, dst, lat, loss)
    nodes = np.arange(n, dtype=np.uint32)
    t = {}
    for algo in (_lib.SRT_ALGO_FW, _lib.SRT_ALGO_SSSP):
        t[algo], _ = _device_ms(g, nodes, algo)
    p = RoutingPlan(g, nodes, algo=_lib.SRT_ALGO_AUTO, device=0)
    desc = p.describe()
    p.close()
    assert "auto-price=" in desc, desc
    picked = _lib.SRT_ALGO_FW if desc.startswith("fw") else _lib.SRT_ALGO_SSSP
    assert t[picked] <= 1.15 * min(t.values()), (desc, t)


# every create-time knob (CreateKnobs in srt_choose.h): unset unless a case sets it
_CREATE_KNOBS = ("SRT_FW_NO_ECC", "SRT_LEVEL", "SRT_LVL_SYM", "SRT_LEVEL_Q", "SRT_FW_P1", "SRT_FW_EMULATE_RANKS",
                 "SRT_FW_BAND", "SRT_FW_KEY", "SRT_SSSP_KEY", "SRT_SSSP_ORDER", "SRT_SSSP_DELTA", "SRT_SSSP_ACT",
                 "SRT_SSSP_FR_NB", "SRT_SSSP_FR_GRID", "SRT_SSSP_SYM", "SRT_FR_FIRST")
_DESC_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_desc.json")


def create_desc_cases():
    """(name, graph, nodes, algo, env) of every pinned create.  Each field of
    the strings is capped by the graph (<= 64 frontier blocks, path state far
    below the packed sweep's budget), never by the free HBM."""
    AUTO, FW, SSSP, LEVEL = _lib.SRT_ALGO_AUTO, _lib.SRT_ALGO_FW, _lib.SRT_ALGO_SSSP, _lib.SRT_ALGO_LEVEL
    cases = []

    def add(name, g, nodes, algo, **env):
        cases.append((name, g, np.asarray(nodes, np.uint32), algo, env))

    # complete, 200 nodes, 1-20 ms: shortest paths within the level probe's bound
    n = 200
    g = NetworkGraph.from_edges(n, *synth.complete_graph(n, 2, lat_ms=(1, 20)))
    every = np.arange(n)
    add("complete/auto", g, every, AUTO)
    add("complete/auto lvl_sym=0", g, every, AUTO, SRT_LVL_SYM="0")
    add("complete/auto level=0", g, every, AUTO, SRT_LEVEL="0")
    add("complete/fw", g, every, FW)
    for key in ("u16", "u32", "f64", "u64"):
        add(f"complete/fw key={key}", g, every, FW, SRT_FW_KEY=key)
    # a strict subset of the in-use nodes in shuffled order (ident_nodes false)
    add("complete/auto subset", g, np.random.default_rng(11).permutation(n)[:120], AUTO)
    # the same graph at ns resolution (gcd 1 ns): only the quantized level solve applies
    gn = NetworkGraph.from_edges(n, *synth.complete_graph_ns(n, 2, lat_ms=(1, 20)))
    add("complete_ns/level", gn, every, LEVEL)
    add("complete_ns/level q=0", gn, every, LEVEL, SRT_LEVEL_Q="0")
    # the same two graphs as identity rows (row u lists 0 .. V-1 in order): the scan
    # proves them complete, so the longest edge bounds the keys and the level
    # plans check the rows' symmetry
    gi = NetworkGraph(n, every, *synth.complete_csr(n, 2, lat_ms=(1, 20)), False)
    add("identity/auto", gi, every, AUTO)
    add("identity/auto lvl_sym=0", gi, every, AUTO, SRT_LVL_SYM="0")
    add("identity/fw", gi, every, FW)
    add("identity/level", gi, every, LEVEL)
    add("identity/level lvl_sym=0", gi, every, LEVEL, SRT_LVL_SYM="0")
    gin = NetworkGraph(n, every, *synth.complete_csr(n, 2, edges=synth.complete_graph_ns(n, 2, lat_ms=(1, 20))),
                       False)
    add("identity_ns/level", gin, every, LEVEL)
    # dense, not complete: the key width comes from the eccentricity proof
    n = 300
    gd = NetworkGraph.from_edges(n, *synth.dense_graph(n, 3, drop=0.3, lat_ms=(1, 20)))
    add("dense/fw", gd, np.arange(n), FW)
    add("dense/fw no_ecc", gd, np.arange(n), FW, SRT_FW_NO_ECC="1")
    # sparse, 100 of 500 nodes in use
    n = 500
    gb = NetworkGraph.from_edges(n, *synth.barabasi_albert(n, 3, 9))
    some = np.arange(0, n, 5)
    add("ba500/sssp", gb, some, SSSP)
    add("ba500/sssp key=64", gb, some, SSSP, SRT_SSSP_KEY="64")
    add("ba500/sssp key=64 delta=0.25", gb, some, SSSP, SRT_SSSP_KEY="64", SRT_SSSP_DELTA="0.25")
    for order in ("0", "2", "3"):
        add(f"ba500/sssp order={order}", gb, some, SSSP, SRT_SSSP_ORDER=order)
    # three frontier blocks: the launch geometry
    n = 1300
    gf = NetworkGraph.from_edges(n, *synth.barabasi_albert(n, 3, 21))
    add("ba1300/sssp fr_nb=1", gf, np.arange(n), SSSP, SRT_SSSP_FR_NB="1")
    add("ba1300/sssp fr_nb=2 first=1", gf, np.arange(n), SSSP, SRT_SSSP_FR_NB="2", SRT_FR_FIRST="1")
    add("ba1300/sssp fr_nb=1 sym=0", gf, np.arange(n), SSSP, SRT_SSSP_FR_NB="1", SRT_SSSP_SYM="0")
    # directed
    n = 300
    gdir = NetworkGraph.from_edges(n, *synth.random_graph(n, 92, p_edge=0.05, directed=True, lat_range_ns=(1, 9)),
                                   directed=True)
    add("directed/auto", gdir, np.arange(n), AUTO)
    add("directed/sssp", gdir, np.arange(n), SSSP)
    return cases


def create_desc_record(case, setenv, delenv):
    """describe() of the case's plan, or the code and text of its refusal."""
    _, g, nodes, algo, env = case
    for k in _CREATE_KNOBS:
        delenv(k)
    for k, v in env.items():
        setenv(k, v)
    try:
        p = RoutingPlan(g, nodes, algo=algo, device=0)
    except _lib.SrtError as e:
        return {"code": e.code, "msg": str(e)}
    try:
        return {"desc": p.describe()}
    finally:
        p.close()


def test_create_descriptions_pinned(monkeypatch):
    """What plan creation decides -- family, key type and its proof, prices,
    bucket width, groups, launch geometry, source order, seeding -- as
    describe() reports it, or the refusal's code and text, equal to the strings
    recorded before creation was split into stages (tests/golden/create_desc.json)."""
    with open(_DESC_GOLDEN) as f:
        golden = json.load(f)
    cases = create_desc_cases()
    assert sorted(golden) == sorted(c[0] for c in cases)
    got = {c[0]: create_desc_record(c, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
           for c in cases}
    for name in golden:
        print(name, got[name])
    assert got == golden
