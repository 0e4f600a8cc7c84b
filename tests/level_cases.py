"""Graphs that sit on the level solve's kernel constants (srt_level.hip), and
the checkers the GPU edge tests share (tests/test_gpu_level_edges.py).  Plain
numpy generators with explicit seeds; tests/test_level_cases_cpu.py proves on
the CPU, with the oracle only, that every graph reaches the branch it is named
for.  Nothing here needs a GPU.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from shadow_amd import synth
from shadow_amd.graph import NetworkGraph, _csr_from_edges

# ---- the constants the cases are built around (test_level_cases_cpu.py reads
# the sources and fails when one of them is retuned)
OUT_SCAP = 1024      # srt_level.hip: constexpr uint32_t OUT_SCAP = 1024 (hits of a row lvl_out_kernel stages)
OUT_PLACE = 65536    # srt_level.hip: `e - b <= 65536` (a staged hit keeps its place in the row in 16 bits)
OUT_GRID = 8192      # srt_level.hip: launch_lvl_out, min(8192, (rows + 3) / 4) workgroups of 4 waves
TR_CH = 256          # srt_rowfold.h: constexpr uint32_t TR_CH = 256 (64-entry chunks lvl_index_kernel keeps)
LEVEL_V_MAX = 18400  # srt_internal.h: constexpr uint32_t LEVEL_V_MAX = 18400
LWC = 63             # srt_rowfold.h: the level solve's classes / levels at most
WC = 31              # srt_rowfold.h: weight classes at most of the level fold
SOLVE_HIST = 256     # srt_rowfold.h: bytes of level ends (u32 each: hist[63] is the last word)
EST_SLACK = 65536    # srt_level.hip level_probe: lvl_est = n_adj * min(1, 2 wmax / maxu) + 65536
PROBE_ROWS = 8       # srt_level.hip level_probe: K = min(8, n)
PROBE_WC = (15, 31, 63)  # srt_api.cpp run_level_probes: the integer probes, in turn

MS = synth.MS        # one latency unit of the integer cases


def class_table(ncls):
    """Class offsets a vertex (level_csr): < 16 -> 16, < 32 -> 32, else 64."""
    return 16 if ncls < 16 else 32 if ncls < 32 else 64


def lvl_estimate(n_adj, wmax, maxu):
    """level_probe's estimate of the class CSR's entries at `wmax` units."""
    f = min(1.0, 2.0 * float(wmax) / float(max(maxu, 1)))
    return int(float(n_adj) * f) + EST_SLACK


def out_rows_per_wave(rows):
    """Rows the busiest wave of lvl_out_kernel serves over `rows` rows."""
    nwaves = 4 * max(1, min(OUT_GRID, (rows + 3) // 4))
    return -(-rows // nwaves)


# ------------------------------------------------------------------ cases
def _case(n_nodes, src, dst, lat, loss, directed, nodes, csr=None, **kw):
    return SimpleNamespace(n_nodes=int(n_nodes), src=np.asarray(src, np.uint32), dst=np.asarray(dst, np.uint32),
                           lat=np.asarray(lat, np.uint64), loss=np.asarray(loss, np.float32), directed=bool(directed),
                           nodes=np.ascontiguousarray(nodes, np.uint32), csr=csr, **kw)


def case_csr(case):
    """(row_ptr, col, lat, loss): the adjacency the library is given."""
    if case.csr is not None:
        return case.csr
    return _csr_from_edges(case.n_nodes, case.src, case.dst, case.lat, case.loss, case.directed)


def network_graph(case):
    row_ptr, col, lat, loss = case_csr(case)
    return NetworkGraph(case.n_nodes, np.arange(case.n_nodes, dtype=np.uint32), row_ptr, col, lat, loss,
                        directed=case.directed)


def oracle_graph(case):
    return O.Graph(case.directed, np.arange(case.n_nodes), case.src, case.dst, case.lat, case.loss)


def units_of(lat):
    """(g, maxu): the gcd of every latency (self-loops too) and the longest in
    units of it, as the host scan's CsrStats."""
    lat = np.asarray(lat, np.uint64)
    g = int(np.gcd.reduce(lat)) if len(lat) else 1
    g = g or 1
    return g, (int(lat.max()) // g if len(lat) else 0)


def short_counts(row_ptr, col, lat, wmax_ns):
    """Per row: the entries that are no self-loop and of latency <= wmax_ns --
    lvl_out_kernel's `cnt`."""
    row_ptr = np.asarray(row_ptr, np.int64)
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    hit = (np.asarray(lat, np.uint64) <= np.uint64(wmax_ns)) & (np.asarray(col, np.int64) != rows)
    return np.bincount(rows[hit], minlength=n)


def _losses(rng, m, loss_max=0.05):
    return np.round(rng.uniform(0.0, loss_max, size=m), 6).astype(np.float32)


def _ns(rng, lat_units):
    """Integer-ms latencies plus a seeded sub-ms offset: g = 1 ns (the quantized solve)."""
    lat = np.asarray(lat_units, np.uint64) * np.uint64(MS)
    return lat + rng.integers(0, MS, size=len(lat), dtype=np.uint64)


def hub_graph(V, degrees, seed, directed=False, ns=False, nodes=None):
    """Vertex 0 joined to every vertex at 1 unit (both ways), so every pair is
    within 2 units and the probe row of the hub proves B = 2.  `degrees`
    {vertex: d}: the vertex gets d - 1 edges of 2 units to vertices that are
    neither the hub nor in `degrees`, its row then holding exactly d short
    entries (directed: on the out side only, the heads' in-rows growing
    instead).  The 2-unit edges tie with the two hops through the hub, at other
    losses.  Filler edges of 40-59 units (v -> the next vertex) are never hits
    and make the longest edge long; self-loops of 3 units.
    nodes: the in-use list (default: the hub, then the rest permuted)."""
    rng = np.random.default_rng(seed)
    others, hub = np.arange(1, V, dtype=np.int64), np.zeros(V - 1, np.int64)
    src, dst, lat = [], [], []

    def add(s, d, units):
        src.append(s)
        dst.append(d)
        lat.append(np.broadcast_to(np.asarray(units, np.int64), s.shape))

    add(hub, others, 1)
    if directed:
        add(others, hub, 1)
    pool = np.setdiff1d(others, np.fromiter(degrees, np.int64, len(degrees)))
    for c, d in degrees.items():
        assert 1 <= c < V and 1 <= d - 1 <= len(pool), (c, d)
        add(np.full(d - 1, c, np.int64), rng.permutation(pool)[: d - 1], 2)
    nxt = others % (V - 1) + 1  # 1 -> 2 -> ... -> V-1 -> 1
    keep = nxt != others
    add(others[keep], nxt[keep], 40 + others[keep] % 20)
    add(np.arange(V, dtype=np.int64), np.arange(V, dtype=np.int64), 3)
    src, dst, lat = np.concatenate(src), np.concatenate(dst), np.concatenate(lat)
    lat = _ns(rng, lat) if ns else lat.astype(np.uint64) * np.uint64(MS)
    if nodes is None:
        nodes = np.concatenate([[0], 1 + rng.permutation(V - 1)])
    assert int(nodes[0]) == 0
    return _case(V, src, dst, lat, _losses(rng, len(src)), directed, nodes, hub=0, bound=None if ns else 2,
                 degrees=dict(degrees))


def circulant_identity(n, seed, half=OUT_SCAP // 2, antipode=False):
    """A complete undirected graph in identity rows (row u = columns 0 .. n-1):
    the pairs at cyclic offset 1 .. half either way are 1 unit (2 half hits a
    row), `antipode` adds the offset n / 2 (one hit more), every other pair is
    40-300 units; latencies and losses mirror exactly (a symmetric plan).
    Every vertex in use, in node order."""
    assert n % 2 == 0 and 2 * half < n - 1
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 0)
    d = (ju - iu) % n
    short = ((d >= 1) & (d <= half)) | (d >= n - half)
    if antipode:
        short |= d == n // 2
    lat = rng.integers(40, 301, size=len(iu), dtype=np.uint64)
    lat[short] = 1
    lat *= np.uint64(MS)
    edges = (iu.astype(np.uint32), ju.astype(np.uint32), lat, _losses(rng, len(iu)))
    csr = synth.complete_csr(n, seed, edges=edges)
    return _case(n, *edges, False, np.arange(n), csr=csr, hits=2 * half + int(antipode))


def complete_identity(n, seed, lat_ms=(1, 3), ns=False):
    """synth.complete_graph(n, seed, lat_ms) (ns: complete_graph_ns) in identity
    rows, every vertex in use in node order: every row well over OUT_SCAP hits."""
    edges = synth.complete_graph_ns(n, seed, lat_ms) if ns else synth.complete_graph(n, seed, lat_ms)
    return _case(n, *edges, False, np.arange(n), csr=synth.complete_csr(n, seed, edges=edges))


def path_graph(D, seed, legs=True):
    """Unit edges; the centre (vertex 0, nodes[0]) has out-eccentricity
    ceil(D / 2) and in-eccentricity floor(D / 2) and two vertices are D apart, so
    the probe's bound is D exactly.  Two arms of floor(D / 2) and ceil(D / 2)
    vertices hang off the centre, their edges both ways; D odd: the longer arm's
    last edge points outward only and its tip returns by one edge to the arm's
    vertex two nearer the centre.  legs (a caterpillar): a leaf on the centre
    and on every arm vertex but the tips.  Directed edge list; every vertex in
    use, the centre first, the rest permuted."""
    a, b = D // 2, (D + 1) // 2
    assert a >= 1
    rng = np.random.default_rng(seed)
    depth_a = np.arange(1, a + 1)           # arm A: vertices 1 .. a
    arm_b = a + np.arange(1, b + 1)         # arm B: vertices a+1 .. a+b
    prev_a = np.concatenate([[0], depth_a[:-1]])
    prev_b = np.concatenate([[0], arm_b[:-1]])
    src, dst = [prev_a, depth_a], [depth_a, prev_a]
    if b == a:
        src += [prev_b, arm_b]
        dst += [arm_b, prev_b]
    else:
        tip, back = arm_b[-1], (arm_b[a - 2] if a >= 2 else 0)  # the vertex at depth a - 1
        src += [prev_b, arm_b[:-1], [tip]]
        dst += [arm_b, prev_b[:-1], [back]]
    n = 1 + a + b
    if legs:
        stems = np.concatenate([[0], depth_a[:-1], arm_b[: a - 1]])
        leaves = n + np.arange(len(stems))
        src += [stems, leaves]
        dst += [leaves, stems]
        n += len(stems)
    src.append(np.arange(n)), dst.append(np.arange(n))
    src, dst = np.concatenate(src), np.concatenate(dst)
    lat = np.full(len(src), MS, np.uint64)
    nodes = np.concatenate([[0], 1 + rng.permutation(n - 1)])
    return _case(n, src, dst, lat, _losses(rng, len(src)), True, nodes, bound=D)


def two_cycle(w01, w10=1):
    """Two vertices, 0 -> 1 of w01 units and 1 -> 0 of w10: B = w01 + w10, the
    edge 0 -> 1 in the class w01."""
    src, dst = [0, 1, 0, 1], [1, 0, 0, 1]
    lat = np.array([w01, w10, 1, 1], np.uint64) * np.uint64(MS)
    loss = np.array([0.015625, 0.03125, 0.5, 0.25], np.float32)
    return _case(2, src, dst, lat, loss, True, [0, 1], bound=w01 + w10)


def random_edges(n, seed, p_edge, lat=(1, 9), directed=False, isolated=0, unit=MS):
    """A ring (both ways when directed) plus each pair with probability p_edge,
    latencies U{lat} units, one self-loop a vertex; `isolated` more vertices
    n .. n + isolated - 1 with their self-loop only.  (src, dst, lat, loss)."""
    rng = np.random.default_rng(seed)
    ring = np.arange(n)
    iu, ju = np.nonzero(rng.random((n, n)) < p_edge)
    keep = (iu != ju) if directed else (iu < ju)
    src = [ring, iu[keep]] + ([(ring + 1) % n] if directed else [])
    dst = [(ring + 1) % n, ju[keep]] + ([ring] if directed else [])
    loops = np.arange(n + isolated)
    src, dst = np.concatenate(src + [loops]), np.concatenate(dst + [loops])
    l = rng.integers(lat[0], lat[1] + 1, size=len(src)).astype(np.uint64) * np.uint64(unit)
    perm = rng.permutation(len(src))
    return src[perm].astype(np.uint32), dst[perm].astype(np.uint32), l[perm], _losses(rng, len(src))[perm]


def ragged_graph(V, seed, nodes, isolated=0, directed=False):
    """random_edges over V vertices (p 0.04, 1-9 units) with the in-use list `nodes`."""
    return _case(V + isolated, *random_edges(V, seed, 0.04, directed=directed, isolated=isolated), directed, nodes)


def concentrated_graph(n, seed, p_edge=0.3, long_units=3000):
    """An undirected random graph whose ~n^2 p adjacency entries are all 1-9
    units, and one edge of `long_units`: level_probe's estimate (latencies
    spread evenly up to the longest edge) is a fraction of the entries its
    first pass counts.  Every vertex in use, permuted."""
    src, dst, lat, loss = random_edges(n, seed, p_edge)
    rng = np.random.default_rng(seed + 1)
    src = np.concatenate([src, [0]]).astype(np.uint32)
    dst = np.concatenate([dst, [n // 2]]).astype(np.uint32)
    lat = np.concatenate([lat, [np.uint64(long_units) * np.uint64(MS)]]).astype(np.uint64)
    loss = np.concatenate([loss, [np.float32(0.5)]]).astype(np.float32)
    return _case(n, src, dst, lat, loss, False, rng.permutation(n))


def parallel_row_graph(V=64, copies=66_000, seed=5):
    """Directed: vertex 0's row is `copies` parallel edges 0 -> 1 of 50 units,
    THEN its V - 1 unit edges to every vertex and its self-loop, so the row has
    more than 65,536 entries, at most OUT_SCAP short ones, every short one past
    place 65,535.  Every vertex returns to 0 by a unit edge; a few 2-unit edges
    tie with the two hops through 0.  Every vertex in use, 0 first."""
    assert copies >= OUT_PLACE and V - 1 <= OUT_SCAP
    rng = np.random.default_rng(seed)
    others = np.arange(1, V)
    a, b = rng.integers(1, V, 3 * V), rng.integers(1, V, 3 * V)
    a, b = a[a != b], b[a != b]
    src = np.concatenate([np.zeros(copies, np.int64), np.zeros(V - 1, np.int64), others, a, np.arange(V)])
    dst = np.concatenate([np.ones(copies, np.int64), others, np.zeros(V - 1, np.int64), b, np.arange(V)])
    lat = np.concatenate([np.full(copies, 50), np.ones(2 * (V - 1)), np.full(len(a), 2), np.full(V, 3)])
    nodes = np.concatenate([[0], 1 + rng.permutation(V - 1)])
    return _case(V, src, dst, lat.astype(np.uint64) * np.uint64(MS), _losses(rng, len(src)), True, nodes, bound=2)


# ------------------------------------------------------------------ the probe
def probe_rows(n):
    """The in-use list's places level_probe takes its rows from."""
    K = min(PROBE_ROWS, n)
    return [k * n // K for k in range(K)]


def _ecc(og, order, K, g):
    """Largest distance (units) from each of the first K of `order` to every
    node of it; None: one is unreachable."""
    try:
        lat, _ = O.compute_shortest_paths(og, order, src_count=K)
    except O.OracleError as e:
        if e.code != O.DISCONNECTED:
            raise
        return None
    off = lat[:K].copy()
    off[np.arange(K), np.arange(K)] = 1  # the diagonal is the raw self-loop (or, of fewer rows than nodes, unset)
    if (off == 0).any():  # fewer rows than nodes: an unreached pair stays 0 (no edge has latency 0)
        return None
    off[np.arange(K), np.arange(K)] = 0
    return (off // np.uint64(g)).max(axis=1)


def probe_bound(og, nodes):
    """The bound level_probe must prove for the integer-unit solve, restated
    with the oracle: wc = 15, 31, 63 in turn; the graph pruned to its edges <=
    min(wc, longest edge) units; from the K rows k n / K of the in-use list the
    out- plus the in-eccentricity over the in-use nodes, kept when each is <= wc
    and so is the sum; the smallest such sum.  None: no bound within 63 units."""
    nodes = np.asarray(nodes, np.uint32)
    n = len(nodes)
    if n == 0:
        return None
    g, maxu = units_of(og.lat)
    rows = probe_rows(n)
    K = len(rows)
    rest = np.setdiff1d(np.arange(n), rows)
    order = nodes[np.concatenate([rows, rest]).astype(np.int64)]
    for wc in PROBE_WC:
        wmax = min(wc, maxu)
        keep = (og.lat <= np.uint64(wmax * g)) | (og.src == og.dst)
        fwd = O.Graph(og.directed, og.ids, og.src[keep], og.dst[keep], og.lat[keep], og.loss[keep])
        rev = O.Graph(og.directed, og.ids, og.dst[keep], og.src[keep], og.lat[keep], og.loss[keep])
        eo, ei = _ecc(fwd, order, K, g), _ecc(rev, order, K, g)
        if eo is None or ei is None:
            continue
        sums = [int(a) + int(b) for a, b in zip(eo, ei) if a <= wc and b <= wc and int(a) + int(b) <= wc]
        if sums:
            return min(sums)
    return None


def lmax_of(desc):
    """The bound a level plan's describe() reports."""
    return int(desc.split(" lmax=")[1].split("(")[0])


def level_vbits(V):
    """Bits of a vertex id in a quantized entry (srt_level.hip level_vbits)."""
    vb = 1
    while (1 << vb) < V:
        vb += 1
    return vb


def level_quantum(case):
    """The quantized solve's bucket width in units of g (srt_choose.cpp
    level_quantum): the shortest edge that is no self-loop, at most 2^(34 - vb)
    and 2^25."""
    g, _ = units_of(case.lat)
    mn = int(case.lat[case.src != case.dst].min()) // g
    return min(mn, 1 << (34 - level_vbits(case.n_nodes)), 1 << 25)


# ------------------------------------------------------------------ the named cases
CAP_DEGREES = {3: OUT_SCAP - 1, 4: OUT_SCAP, 5: OUT_SCAP + 1, 6: 1150}  # short entries of four rows of hub_cap


@functools.lru_cache(maxsize=None)
def hub_cap(directed):
    """V = 1,201 (V mod 4 = 1), every vertex in use: rows of 1,023 / 1,024 /
    1,025 / 1,150 short entries and the hub's 1,200."""
    return hub_graph(1201, CAP_DEGREES, 11 + int(directed), directed=directed)


def _in_use_64(case, seed, low_hi):
    """64 in-use nodes: the hub, vertex 7 (a row of 1,025 short entries) and 14
    heads of its 2-unit edges, 16 vertices below `low_hi`, the last 32 vertices."""
    rng = np.random.default_rng(seed)
    V = case.n_nodes
    two = (case.src == 7) & (case.dst != 0) & (case.dst != 7) & (case.lat < np.uint64(3 * MS))
    heads = np.unique(case.dst[two])
    heads = heads[heads < V - 32][:14]
    low = np.setdiff1d(np.arange(8, low_hi), heads)
    pick = np.concatenate([[7], heads, rng.choice(low, 16, replace=False), np.arange(V - 32, V)])
    case.nodes = np.concatenate([[0], rng.permutation(pick)]).astype(np.uint32)
    assert len(np.unique(case.nodes)) == 64
    return case


@functools.lru_cache(maxsize=None)
def hub_wide(V, ns=False):
    """The hub graph with a hub row of V entries (V = 16,500: past
    lvl_index_kernel's TR_CH chunks; V = LEVEL_V_MAX: the largest LDS row) and
    64 in-use nodes, half of them the last 32 vertices."""
    return _in_use_64(hub_graph(V, {7: OUT_SCAP + 1}, 13 + int(ns), ns=ns), 17, 2000)


@functools.lru_cache(maxsize=None)
def circulant(antipode):
    return circulant_identity(1100, 21 + int(antipode), antipode=antipode)


@functools.lru_cache(maxsize=None)
def complete_over(ns):
    return complete_identity(1100, 23, ns=ns)


@functools.lru_cache(maxsize=None)
def concentrated():
    return concentrated_graph(1000, 31)


RAGGED = {
    # name: (V, isolated, in-use list)
    "v302": (302, 0, lambda r: np.concatenate([r.permutation(300)[:150], [300, 301]])),
    "v303": (303, 0, lambda r: np.concatenate([r.permutation(300)[:150], [300, 302]])),
    "v303-source-last": (303, 0, lambda r: np.concatenate([[302, 301, 300], r.permutation(300)[:40]])),
    "n1": (300, 0, lambda r: np.array([123])),
    "n2": (300, 0, lambda r: np.array([299, 5])),
    "n7": (300, 0, lambda r: r.permutation(300)[:7]),
    "n9": (300, 0, lambda r: r.permutation(300)[:9]),
    "isolated20": (300, 20, lambda r: r.permutation(300)[:120]),
}


@functools.lru_cache(maxsize=None)
def ragged(name):
    V, isolated, pick = RAGGED[name]
    return ragged_graph(V, 41, pick(np.random.default_rng(43)), isolated=isolated)
