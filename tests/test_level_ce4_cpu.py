"""CPU proofs for tests/test_gpu_level_ce4.py: the 4-byte class entry's
arithmetic (srt_level.hip: v | (0x3f800000 - bits(1f32 - e)) << vb) and that
each graph reaches the branch it is named for, with numpy and the oracle only."""
import numpy as np
import pytest

import level_cases as LC
import test_gpu_level_ce4 as G
import test_level_walk_resources as WR
from oracle import oracle as O


def _encode(v, e, vb):
    d = G.delta_of(e)
    assert 0 <= d < 1 << (32 - vb)
    return (v | d << vb) & 0xFFFFFFFF


def _decode(x, vb):
    return x & ((1 << vb) - 1), G.ONE - (x >> vb)


@pytest.mark.parametrize("vb", [8, 9, 14, 15])  # V from 129 to 18,400
def test_entry_round_trip(vb):
    """Every loss that fits decodes to the bits of 1f32 - e, beside any vertex."""
    rng = np.random.default_rng(vb)
    big, dmax = G.fit_max(vb)
    top = 1.0 - float(np.uint32(G.ONE - dmax).view(np.float32))
    losses = [np.float32(0), big] + list(rng.uniform(0, top, 200).astype(np.float32))
    for e in losses:
        want = int((np.float32(1) - np.float32(e)).view(np.uint32))
        for v in (0, 1, (1 << vb) - 1):
            assert _decode(_encode(v, e, vb), vb) == (v, want)


def test_field_edges():
    # an f32 in [0.5, 1] is a contiguous range of integers: differences up to 2^23 exist one by one
    assert G.fit_max(9) == (np.float32(0.5) - np.float32(2.0 ** -24), (1 << 23) - 1)
    assert G.fit_max(14)[1] == (1 << 18) - 1 and float(G.fit_max(14)[0]) == ((1 << 18) - 1) * 2.0 ** -24
    # below 0.5 the loss is coarser than 1 - e: the odd differences past 2^23 have no loss
    assert G.loss_with_delta((1 << 24) - 1) is None and G.fit_max(8)[1] == (1 << 24) - 2
    assert float(G.over_min(9)) == 0.5 and float(G.over_min(8)) == 0.75
    for vb in (8, 9, 14):
        assert G.delta_of(G.over_min(vb)) == 1 << (32 - vb)
    # a loss past 1, and a NaN, wrap the u32 difference past every field
    for bad in (np.float32(1.5), np.float32(np.nan)):
        assert (G.ONE - int((np.float32(1) - bad).view(np.uint32))) & 0xFFFFFFFF >= 1 << 24


def _oracle_units(case):
    lat, _ = O.compute_shortest_paths(LC.oracle_graph(case), case.nodes, src_count=1)
    return (lat[0] // np.uint64(LC.MS)).astype(np.int64)


def test_walker_case_levels():
    case = G.walker_case()
    assert G.level_sizes(case, 0) == [1, G.NA, G.NB, G.NC, G.ND]
    u = _oracle_units(case)
    u[0] = 0  # (the diagonal is the self-loop)
    assert np.bincount(u).tolist() == [1, G.NA, G.NB, G.NC, G.ND]  # no long pair shortens a path
    lists = sorted(int(np.sum(case.units[a] == 1)) for a in range(1, 5))
    assert lists == sorted(G.LISTS)
    row_ptr, col, lat, loss = LC.case_csr(case)
    n = case.n_nodes
    L, P = lat.reshape(n, n), loss.view(np.uint32).reshape(n, n)
    assert np.array_equal(L, L.T) and np.array_equal(P, P.T)  # a symmetric plan
    assert LC.probe_bound(LC.oracle_graph(case), case.nodes) <= 14  # the packed row's levels


@pytest.mark.parametrize("n", [255, 256, 257])
def test_random_sym_reaches_the_field_edges(n):
    case = G.random_sym(n, 8800 + n)
    d = G._deltas(case)
    assert d.min() == 0 and d.max() == G.fit_max(case.vb)[1]
    assert LC.probe_bound(LC.oracle_graph(case), case.nodes) <= 14
    over = G.random_sym(n, 8800 + n, {(0, 1): G.over_min(case.vb)})
    assert int(np.sum(G._deltas(over) >= 1 << (32 - case.vb))) == 1


@WR.needs_hipcc
def test_ce4_instantiations_hold_two_workgroups_a_cu():
    """level_ce4_kernel<NT>: no scratch, and the waves a SIMD of two PACK_NT-thread workgroups a CU."""
    ks = {k: v for k, v in WR.KR._resources("srt_level.hip").items() if "level_ce4_kernel" in k}
    assert len(ks) == 2, sorted(ks)
    need = 2 * (WR._pack_nt() // 64) // 4
    for k, v in ks.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["Occupancy [waves/SIMD]"] >= need, (k, v, need)
