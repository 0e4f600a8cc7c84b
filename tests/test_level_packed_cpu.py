"""The packed LDS row of the level solve (srt_rowfold.h, srt_level.hip
level_solve_kernel PK), restated on the CPU: its layout and the sizes at which
a plan chooses it, derived from the layout functions; and, from the oracle's
distances alone, that the graphs tests/test_gpu_level_packed.py runs reach the
pull side of the walk and the last level the 4-bit field holds.  Nothing here
needs a GPU."""
import os
import re

import numpy as np

import level_cases as LC
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shadow_amd", "csrc")

PACK_LMAX = 14       # srt_rowfold.h: the largest level beside 0xF in 4 bits
CU_LDS = 160 * 1024  # srt_level.hip level_rows_per_cu: a CU's LDS
WG_SLACK = 2048      # ... and what a workgroup takes beside its row
WCN = 15             # classes of the 16-offset class table (CLSN - 1)


def _up16(b):
    return (b + 15) & ~15


def unpacked_bytes(V):
    """solve_lds_bytes(V, false, false): level ends, u16 levels, f32 losses, u16 members."""
    return LC.SOLVE_HIST + _up16(2 * V) + 4 * V + _up16(2 * V)


def packed_bytes(V):
    """solve_lds_bytes(V, false, true): level ends, u32 keys, a u16 of four 4-bit levels a quad."""
    return LC.SOLVE_HIST + _up16(4 * V) + _up16((V + 3) // 4 * 2)


def rows_per_cu(row_bytes):
    return CU_LDS // (row_bytes + WG_SLACK)


def packed_by_default(V):
    """choose_row_packed with the knob unset, for a valid plan."""
    return rows_per_cu(unpacked_bytes(V)) < 2 and rows_per_cu(packed_bytes(V)) >= 2


def default_edges():
    """(lo, hi): the plan sizes lo < V <= hi take the packed row unforced."""
    vs = [V for V in range(2, LC.LEVEL_V_MAX + 1) if packed_by_default(V)]
    assert vs == list(range(vs[0], vs[-1] + 1))
    return vs[0] - 1, vs[-1]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_layout_matches_the_sources():
    fold, lvl, choose = _src("srt_rowfold.h"), _src("srt_level.hip"), _src("srt_choose.cpp")
    assert re.findall(r"constexpr uint32_t PACK_LMAX = (\d+);", fold) == [str(PACK_LMAX)]
    assert "constexpr uint32_t PACK_NT = 512;" in fold
    assert "pack_lev_off(size_t V) { return SOLVE_HIST + up16(V * 4); }" in fold
    assert ": packed ? pack_lev_off(V) + up16((V + 3) / 4 * 2)" in fold
    assert "return (int)((160 * 1024) / (solve_lds_bytes(V, quant, packed) + 2048));" in lvl
    assert "const bool valid = !quant && lmax <= 14 && sp && fit_rt >= 2;" in choose
    assert "return rows_unpacked < 2 && rows_packed >= 2;" in choose


def test_row_sizes_and_default_edges():
    # the 16k row: 256 + 65,536 + 8,192, twice a CU with the static LDS; the
    # 8-byte row once; a 5-byte row (u8 level, f32 loss) would not fit twice
    assert packed_bytes(16384) == 73_984 and 2 * (73_984 + 544) <= CU_LDS
    assert unpacked_bytes(16384) == 131_328
    assert 2 * (256 + 5 * 16384 + 544) == 165_440 > CU_LDS
    lo, hi = default_edges()
    assert (lo, hi) == (9_952, 17_692)
    assert [packed_by_default(V) for V in (lo, lo + 1, hi, hi + 1)] == [False, True, True, False]
    assert hi < LC.LEVEL_V_MAX and packed_bytes(LC.LEVEL_V_MAX) <= 160 * 1024 - 1024 - 4096
    # V mod 4 = 1, 2, 3: the last quad's word is there
    assert [packed_bytes(V) - LC.SOLVE_HIST - _up16(4 * V) for V in (1, 4, 5, 29, 32, 33)] == [16, 16, 16, 16, 16, 32]


# the RAGGED graphs of level_cases.py whose probe bound is past PACK_LMAX:
# forcing the packed row must leave them unpacked
RAGGED_PAST_THE_CAP = {"ragged-v302": 18, "ragged-v303": 18, "ragged-v303-source-last": 16, "ragged-n7": 16,
                       "ragged-n9": 16, "ragged-isolated20": 18}
_SHORT = {}


def ragged_short(name):
    """LC.ragged(name)'s size, unused vertices and in-use list over edges of 1-5
    units: a probe bound the packed row holds."""
    if name not in _SHORT:
        V, isolated, pick = LC.RAGGED[name]
        edges = LC.random_edges(V, 41, 0.04, lat=(1, 5), isolated=isolated)
        _SHORT[name] = LC._case(V + isolated, *edges, False, pick(np.random.default_rng(43)))
    return _SHORT[name]


def test_ragged_bounds():
    for name in LC.RAGGED:
        case = LC.ragged(name)
        b = LC.probe_bound(LC.oracle_graph(case), case.nodes)
        assert b == RAGGED_PAST_THE_CAP.get(f"ragged-{name}", b) and (b > PACK_LMAX) == (f"ragged-{name}" in RAGGED_PAST_THE_CAP)
        short = ragged_short(name)
        assert LC.probe_bound(LC.oracle_graph(short), short.nodes) <= 12
        assert np.array_equal(short.nodes, case.nodes) and short.n_nodes == case.n_nodes


def levels_of_rows(case, rows):
    """Distances in units from the in-use nodes at places `rows` to EVERY vertex
    of the graph that is reachable (the solve's LDS row covers all V), as one
    sorted array a row."""
    og = LC.oracle_graph(case)
    g, _ = LC.units_of(og.lat)
    out = []
    for r in rows:
        s = int(case.nodes[r])
        others = np.setdiff1d(np.arange(case.n_nodes), [s])
        lat, _ = O.compute_shortest_paths(og, np.concatenate([[s], others]).astype(np.uint32), src_count=1)
        d = lat[0].copy()
        d[0] = 0
        out.append(np.sort(d // np.uint64(g)).astype(np.int64))
    return out


def pull_levels(dist, V):
    """The kernel's rule for one row: building level l, class w <= min(l, 15)
    is walked from the unsettled side when level l - w holds more vertices
    than remain unsettled.  [(l, w)] of every such pair."""
    hist = np.bincount(dist)
    settled, out = 1, []
    for l in range(1, len(hist)):
        U = V - settled
        if U == 0:
            break
        for w in range(1, min(l, WCN) + 1):
            if hist[l - w] > U:
                out.append((l, w))
        settled += int(hist[l])
    return out


def test_the_complete_graph_takes_the_pull_side():
    case = LC.complete_identity(400, 49, lat_ms=(1, 40))
    rows = [0, 133, 399]
    pulls = [pull_levels(d, case.n_nodes) for d in levels_of_rows(case, rows)]
    assert all(pulls), pulls
    assert max(int(d.max()) for d in levels_of_rows(case, rows)) <= PACK_LMAX


def test_the_cap_cases_reach_level_14_and_15():
    for case, top in ((LC.path_graph(14, 14), 14), (LC.two_cycle(13), 13), (LC.path_graph(15, 15), 15),
                      (LC.two_cycle(14), 14)):
        n = len(case.nodes)
        assert n == case.n_nodes
        dist = levels_of_rows(case, range(n))
        assert max(int(d.max()) for d in dist) == top, case.bound
    assert LC.path_graph(14, 14).bound == LC.two_cycle(13).bound == PACK_LMAX
    assert LC.path_graph(15, 15).bound == LC.two_cycle(14).bound == PACK_LMAX + 1
