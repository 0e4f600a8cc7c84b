"""CPU proofs for tests/test_gpu_level_keep.py: each graph reaches the shape it
is named for (bounds, class-offset strides, kept entries a row, empty rows),
with numpy and the oracle only; and the source keeps the contract the GPU
tests lean on (the knob, the trace line)."""
import os

import numpy as np
import pytest

import level_cases as LC
import test_gpu_level_keep as K

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "shadow_amd", "csrc")


def _bound(case):
    return LC.probe_bound(LC.oracle_graph(case), case.nodes)


def _kept(case, B):
    """Kept entries a row: the entries within B units that are no self-loop."""
    row_ptr, col, lat, _ = LC.case_csr(case)
    g, _ = LC.units_of(lat)
    return LC.short_counts(row_ptr, col, lat, B * g)


@pytest.mark.parametrize("in_use", [200, 120])
def test_complete_graph_of_200_has_a_bound_and_sparse_rows(in_use):
    """1-300 ms over 200 vertices: the probe proves a bound within 63 units (this
    seed: past 31, so 64 offsets a vertex), and a row keeps about a tenth of its
    entries.  With every vertex in use no kept row can be empty: the probe row
    reaches every in-use vertex within B, by a last edge of at most B units."""
    case = K.complete200(in_use)
    B = _bound(case)
    assert B is not None and 6 < B <= 63
    c = _kept(case, B)
    assert 0 < c.mean() < 60 and (in_use < 200 or c.min() >= 1)


def test_unused_vertices_keep_empty_rows():
    case = K.empty_rows_case()
    B = _bound(case)
    assert B is not None and B < 40
    c = _kept(case, B)
    assert (c[: K.USED] >= 2).all() and (c[K.USED:] == 0).all() and len(c) == K.USED + K.UNUSED
    assert c[: K.USED].mean() < 8  # sparse rows


@pytest.mark.parametrize("n", [24, 60])
def test_ring_bounds_and_strides(n):
    """Each eccentricity is n / 2 and the sum n: n = 24 is refused by the 15-unit
    probe and proved by the 31-unit one (32 offsets); n = 60 by the 63-unit one
    (64 offsets), whose kept rows hold chords of 40-60 units in the high classes."""
    case = K.ring_case(n)
    assert _bound(case) == n
    assert LC.class_table(n) == (32 if n == 24 else 64)
    c = _kept(case, n)
    if n == 24:
        assert (c == 2).all()
    else:
        row_ptr, col, lat, _ = LC.case_csr(case)
        u = lat // np.uint64(LC.MS)
        assert (c > 2).any() and ((u >= 40) & (u <= 60)).any()


def test_long_rows_keep_1024_1025_and_every_entry():
    for antipode in (False, True):
        case = LC.circulant(antipode)
        assert set(_kept(case, 4).tolist()) == {LC.OUT_SCAP + int(antipode)}
    case = LC.complete_over(False)
    assert set(_kept(case, _bound(case)).tolist()) == {case.n_nodes - 1} and case.n_nodes - 1 > LC.OUT_SCAP


def test_overflow_case_is_a_shortest_path_edge():
    case = K.sym257(True)
    e = case.loss[(case.src == 0) & (case.dst == 1)][0]
    assert case.units[0, 1] == 1 and K.G.delta_of(e) == 1 << (32 - case.vb)


def test_source_contract():
    """The knob takes the Knob<int> route, and the create prints the line the GPU tests read."""
    choose = open(os.path.join(CSRC, "srt_choose.h")).read()
    api = open(os.path.join(CSRC, "srt_api.cpp")).read()
    level = open(os.path.join(CSRC, "srt_level.hip")).read()
    assert "Knob<int> lvl_keep;" in choose and 'read("SRT_LVL_KEEP", k.lvl_keep, as_int);' in api
    assert '"[srt] level keep: %llu of %llu entries, classes <= %llu\\n"' in level
    assert K.TRACE == "[srt] level keep: "
