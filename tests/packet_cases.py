"""Inputs that sit on the packet stage's kernel constants, and the checkers
the GPU edge tests share (tests/test_gpu_packet_edges.py,
tests/test_gpu_events_edges.py).  Plain numpy generators with explicit seeds;
tests/test_packet_cases_cpu.py proves on the CPU, with the oracle only, that
every case reaches the branch it is named for.  The two run_* checkers import
torch when called, nothing here needs a GPU to import.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O
from shadow_amd import synth

# ---- the constants the cases are built around (test_packet_cases_cpu.py reads
# the .hip files and fails when one of them is retuned)
RT = 256            # srt_packet.hip: constexpr int RT = 256
HB = 16             # srt_packet.hip: #define SRT_PKT_HB 16 (constexpr int HB = SRT_PKT_HB)
DCAP = 3072         # srt_packet.hip: constexpr uint32_t DCAP = 3072
KP = 8              # srt_packet.hip: constexpr int KP = 8
PF = 16             # srt_packet.hip: constexpr int PF = 16
BLOCK_PKTS = RT * KP  # 2048: packets past it take round_kernel's tail loops
EV_WAVE = 64        # srt_events.hip: event_id_kernel, `p0 += 64` (one ballot a step)
EV_ID_HOSTS = 4     # srt_events.hip: event_id_kernel launch, dim3((n_hosts + 3) / 4) waves of 64
EV_SMALL = 256      # srt_events.hip: constexpr uint32_t EV_SMALL = 256
EV_CAP = 1024       # srt_events.hip: constexpr uint32_t EV_CAP = 1024
EV_BIG_GRID = 512   # srt_events.hip: event_big_group_sort_kernel launch, std::min<uint32_t>(n_dst_hosts, 512)
EV_CHUNK = 4096     # srt_events.hip: constexpr uint32_t EV_CHUNK = 4096
EV_COL_LANES = 4    # srt_events.hip: event_col_scan_kernel, `per = (chunks + 3) / 4`
EV_COL_STEP = 16    # srt_events.hip: event_col_scan_kernel, `c += 16`
EV_LDS_DST = 15872  # srt_events.hip: EV_LDS_DST = 15872

MS = synth.MS
U64_MAX = np.iinfo(np.uint64).max
LOSS_ZERO_BITS = 0x00000000
LOSS_ONE_BITS = 0x3F800000

# the round every packet case lives in
R0 = 1_000_000_000
R1 = R0 + 5 * MS
N_ROWS = 40
GRAPH_SEED = 11


# ------------------------------------------------------------------ packets
def extremes_graph(n, seed):
    """synth.complete_graph(n, seed, loss_max=0.25) with every 7th edge lossless
    and every 7th (from the 4th) losing everything."""
    src, dst, lat, loss = synth.complete_graph(n, seed, loss_max=0.25)
    loss = loss.copy()
    loss[0::7] = 0.0
    loss[3::7] = 1.0
    return src, dst, lat, loss


@functools.lru_cache(maxsize=None)
def extremes_table(n=N_ROWS, seed=GRAPH_SEED):
    """The oracle's own table of extremes_graph(n, seed): (latency, loss)."""
    src, dst, lat, loss = extremes_graph(n, seed)
    nodes = np.arange(n, dtype=np.uint32)
    o_lat, o_loss = O.compute_shortest_paths(O.Graph(False, np.arange(n), src, dst, lat, loss), nodes)
    o_lat.setflags(write=False)
    o_loss.setflags(write=False)
    return o_lat, o_loss


def round_from_counts(counts, n_rows, seed, r0, r1, pins=(), zero_payload=0.1):
    """One round with exactly counts[h] packets from host h (zeros anywhere).
    Hosts sit round-robin on the table rows, destinations are uniform over the
    other hosts, payload is 0 with p=zero_payload else U{1..1460}, send times
    are uniform in [r0, r1) and non-decreasing within a host.

    pins: dicts {"host": h, "k": index within the host (negative: from its
    end), and any of "t_ns", "payload_size", "rows": (src_row, dst_row)}.  A
    pinned send time keeps the host's order: its earlier packets are lowered to
    it, its later ones raised to it.
    Returns (pkts O.PKT_DTYPE, host_ptr u32[n_hosts+1], host_row u32)."""
    counts = np.asarray(counts, np.int64)
    assert (counts >= 0).all()
    n_hosts, n = len(counts), int(counts.sum())
    rng = np.random.default_rng(seed)
    host_row = (np.arange(n_hosts) % n_rows).astype(np.uint32)
    host_ptr = np.zeros(n_hosts + 1, np.uint32)
    np.cumsum(counts, out=host_ptr[1:])
    src_host = np.repeat(np.arange(n_hosts), counts).astype(np.uint32)
    if n_hosts > 1:
        dst_host = rng.integers(0, n_hosts - 1, size=n).astype(np.uint32)
        dst_host = np.where(dst_host >= src_host, dst_host + 1, dst_host).astype(np.uint32)
    else:
        dst_host = np.zeros(n, np.uint32)
    payload = rng.integers(1, 1461, size=n).astype(np.uint32)
    payload[rng.random(n) < zero_payload] = 0
    t = rng.integers(r0, r1, size=n).astype(np.uint64)
    t = t[np.lexsort((t, src_host))]  # src_host is sorted already: orders the times within each host
    pk = np.zeros(n, O.PKT_DTYPE)
    pk["src_host"] = src_host
    pk["src_row"] = host_row[src_host]
    pk["dst_row"] = host_row[dst_host]
    pk["payload_size"] = payload
    pinned_t = {}
    for pin in pins:
        h, k = pin["host"], pin["k"]
        b, e = int(host_ptr[h]), int(host_ptr[h + 1])
        p = (b if k >= 0 else e) + k
        assert b <= p < e, pin
        if "t_ns" in pin:
            v = np.uint64(pin["t_ns"])
            t[b:p] = np.minimum(t[b:p], v)
            t[p + 1:e] = np.maximum(t[p + 1:e], v)
            t[p] = v
            pinned_t[p] = v
        if "payload_size" in pin:
            pk["payload_size"][p] = pin["payload_size"]
        if "rows" in pin:
            pk["src_row"][p], pk["dst_row"][p] = pin["rows"]
    pk["t_ns"] = t
    for p, v in pinned_t.items():
        assert t[p] == v, "a later pin moved an earlier one"
    same_host = src_host[1:] == src_host[:-1]
    assert (t[1:][same_host] >= t[:-1][same_host]).all()
    return pk, host_ptr, host_row


def pin_index(host_ptr, pin):
    """Batch index of a pin's packet."""
    h, k = pin["host"], pin["k"]
    return int(host_ptr[h] if k >= 0 else host_ptr[h + 1]) + k


def split_total(total, parts, seed):
    """`parts` positive counts that add up to `total`."""
    rng = np.random.default_rng(seed)
    return 1 + rng.multinomial(total - parts, np.ones(parts) / parts)


def block_totals(host_ptr):
    """Packets per round_kernel workgroup (HB consecutive hosts)."""
    hp = host_ptr.astype(np.int64)
    edges = hp[np.minimum(np.arange(0, len(hp) - 1 + HB, HB), len(hp) - 1)]
    return np.diff(edges)


def _case(name, pk, host_ptr, host_row, bootstrap_end, sim_end, round_end=R1, **extra):
    for a in (pk, host_ptr, host_row):
        a.setflags(write=False)
    return SimpleNamespace(name=name, pk=pk, host_ptr=host_ptr, host_row=host_row, n_hosts=len(host_ptr) - 1,
                           round_end=round_end, bootstrap_end=bootstrap_end, sim_end=sim_end, **extra)


def table_pairs(bits, loss=None):
    """Off-diagonal (row, column) pairs of the table whose loss has these bits."""
    loss = extremes_table()[1] if loss is None else loss
    i, j = np.nonzero(loss.view(np.uint32) == np.uint32(bits))
    keep = i != j
    return np.stack([i[keep], j[keep]], axis=1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def case_extremes(bootstrap_past_round=False):
    """~200 hosts, ~20k packets on the table with losses of exactly 0 and 1;
    the first ms of the round is bootstrap (or, bootstrap_past_round, all of it)."""
    counts = np.random.default_rng(21).multinomial(20_000, np.ones(200) / 200)
    pk, host_ptr, host_row = round_from_counts(counts, N_ROWS, 21, R0, R1)
    return _case("extremes", pk, host_ptr, host_row, bootstrap_end=R1 + 1 if bootstrap_past_round else R0 + MS,
                 sim_end=2**62)


@functools.lru_cache(maxsize=None)
def case_scratch_completed():
    """48 hosts, 60,000 packets (3 workgroups of ~20k: the draws live in the
    global scratch) and sim_end 2 ms into the 5 ms round: every host has
    completed packets, so every walk is redone exactly on the scratch."""
    pk, host_ptr, host_row = synth.packet_round(48, N_ROWS, 60_000, 3, R0, R1)
    pk = pk.view(O.PKT_DTYPE)
    return _case("scratch_completed", pk, host_ptr, host_row, bootstrap_end=0, sim_end=R0 + 2 * MS)


EDGE_SIM_END = R0 + 4 * MS
ALL_DONE_HOST = 5  # block 0: every packet of this host is completed


def _edge_counts(last_block, empty_block):
    b0 = np.zeros(HB, np.int64)
    live0 = [h for h in range(HB) if h not in (0, 7, 8)]     # empty: a block's first host, two neighbours
    b0[live0] = split_total(BLOCK_PKTS, len(live0), 31)
    b1 = np.zeros(HB, np.int64)
    b1[:HB - 1] = split_total(BLOCK_PKTS + 1, HB - 1, 32)    # empty: a block's last host
    b2 = np.zeros(3, np.int64)
    b2[:2] = split_total(last_block, 2, 33)                  # empty: the last host overall
    blocks = [b0] + ([np.zeros(HB, np.int64)] if empty_block else []) + [b1, b2]
    return np.concatenate(blocks)


@functools.lru_cache(maxsize=None)
def case_block_totals(last_block=DCAP, empty_block=False):
    """Workgroup totals of exactly 2048, 2049 and `last_block` (3072: the
    last total whose draws stay in LDS; 3073: the first in the scratch); with
    empty_block a workgroup of 16 empty hosts after the first.  In the 2049
    block and the last block the only completed packet is the block's last
    one (past index 2048, owned by the block's last non-empty host); in block
    0 one host has every packet completed."""
    counts = _edge_counts(last_block, empty_block)
    shift = HB if empty_block else 0
    last1, last2 = HB + shift + HB - 2, 2 * HB + shift + 1  # the last non-empty hosts of the two blocks
    pins = [{"host": ALL_DONE_HOST, "k": k, "t_ns": EDGE_SIM_END + k} for k in range(int(counts[ALL_DONE_HOST]))]
    tail_pins = [{"host": last1, "k": -1, "t_ns": EDGE_SIM_END}, {"host": last2, "k": -1, "t_ns": EDGE_SIM_END}]
    pk, host_ptr, host_row = round_from_counts(counts, N_ROWS, 34 + last_block + shift, R0, EDGE_SIM_END,
                                               pins=pins + tail_pins)
    totals = [BLOCK_PKTS] + ([0] if empty_block else []) + [BLOCK_PKTS + 1, last_block]
    return _case(f"block_totals_{last_block}{'_empty_block' if empty_block else ''}", pk, host_ptr, host_row,
                 bootstrap_end=R0 + MS, sim_end=EDGE_SIM_END, totals=totals, tail_pins=tail_pins,
                 tail_blocks=[len(totals) - 2, len(totals) - 1])


EQ_BOOTSTRAP_END = R0 + MS
EQ_SIM_END = R0 + 4 * MS


@functools.lru_cache(maxsize=None)
def case_equalities():
    """A small round with packets pinned on every comparison of the decision:
    t against sim_end and bootstrap_end, t + delay against round_end."""
    lat, _ = extremes_table()
    one = table_pairs(LOSS_ONE_BITS)
    # a pair whose t = round_end - delay falls inside the round, past bootstrap
    i, j = np.nonzero((lat >= 2 * MS) & (lat <= 3 * MS))
    assert len(i), "no table entry with a delay of 2..3 ms"
    near = (int(i[0]), int(j[0]))
    delay = int(lat[near])
    lossy = (int(one[0][0]), int(one[0][1]))
    pins = [
        {"host": 2, "k": -1, "t_ns": EQ_SIM_END, "name": "t == sim_end"},
        {"host": 3, "k": -1, "t_ns": EQ_SIM_END - 1, "name": "t == sim_end - 1"},
        {"host": 4, "k": 0, "t_ns": EQ_BOOTSTRAP_END, "payload_size": 100, "rows": lossy,
         "name": "t == bootstrap_end"},
        {"host": 5, "k": 0, "t_ns": EQ_BOOTSTRAP_END - 1, "payload_size": 100, "rows": lossy,
         "name": "t == bootstrap_end - 1"},
        {"host": 6, "k": 3, "t_ns": R1 - delay, "payload_size": 0, "rows": near, "name": "t + delay == round_end"},
        {"host": 7, "k": 3, "t_ns": R1 - delay - 1, "payload_size": 0, "rows": near,
         "name": "t + delay == round_end - 1"},
    ]
    counts = np.full(20, 20)
    pk, host_ptr, host_row = round_from_counts(counts, N_ROWS, 41, R0, R1, pins=pins)
    return _case("equalities", pk, host_ptr, host_row, bootstrap_end=EQ_BOOTSTRAP_END, sim_end=EQ_SIM_END,
                 pins=pins, delay=delay)


@functools.lru_cache(maxsize=None)
def case_sends_nothing():
    """Every packet carries payload on a pair that loses everything, outside
    bootstrap: all dropped."""
    counts = np.random.default_rng(51).multinomial(3000, np.ones(35) / 35)
    pk, host_ptr, host_row = round_from_counts(counts, N_ROWS, 51, R0, R1, zero_payload=0.0)
    pk = pk.copy()
    one = table_pairs(LOSS_ONE_BITS)
    pick = one[np.random.default_rng(52).integers(0, len(one), size=len(pk))]
    pk["src_row"], pk["dst_row"] = pick[:, 0], pick[:, 1]
    return _case("sends_nothing", pk, host_ptr, host_row, bootstrap_end=0, sim_end=2**62)


@functools.lru_cache(maxsize=None)
def case_two_rounds():
    """Two rounds of the same 35 hosts: ~500 packets, then a round whose last
    workgroup overflows its LDS (the plan's draws scratch grows in between)."""
    first = np.random.default_rng(61).multinomial(500, np.ones(35) / 35)
    pk1, hp1, host_row = round_from_counts(first, N_ROWS, 61, R0, R1)
    second = _edge_counts(DCAP + 1, False)
    pk2, hp2, _ = round_from_counts(second, N_ROWS, 62, R1, R1 + 5 * MS)
    return (_case("two_rounds_first", pk1, hp1, host_row, bootstrap_end=0, sim_end=2**62),
            _case("two_rounds_second", pk2, hp2, host_row.copy(), bootstrap_end=0, sim_end=2**62,
                  round_end=R1 + 5 * MS))


BAD_HOST = 16 + 13  # a host of workgroup 1 whose last packet lies past the block's first 2048


@functools.lru_cache(maxsize=None)
def case_late_unresolved():
    """48 hosts, workgroup 1 with 2,600 packets; the packet to give an
    unassigned address is the last one of BAD_HOST (block index >= 2048), sent
    later than every other packet of the round."""
    counts = np.concatenate([split_total(300, HB, 71), split_total(2600, HB, 72), split_total(300, HB, 73)])
    t_bad = R1 - 1000
    pin = {"host": BAD_HOST, "k": -1, "t_ns": t_bad}
    pk, host_ptr, host_row = round_from_counts(counts, N_ROWS, 74, R0, t_bad, pins=[pin])
    return _case("late_unresolved", pk, host_ptr, host_row, bootstrap_end=0, sim_end=2**62, pin=pin, t_bad=t_bad)


def run_round(plan, table, case, rng=None, stats_init=None, by_ip=None, sim_end=None):
    """The checking pattern of test_gpu_packet._run on a prepared case: the
    round on the GPU (by row, or by address when by_ip = (resolver, packets
    by address)) against O.packet_batch on the oracle's own table.  Flags,
    deliver times, RNG states after the round, counters and both stats must be
    bit-equal (stats are min-combined with stats_init, default UINT64_MAX).
    Returns the GPU's outputs; `rng` is the state to continue from."""
    import torch

    o_lat, o_loss = table
    n_nodes, n_hosts, n_pkts = o_lat.shape[0], case.n_hosts, len(case.pk)
    sim_end = case.sim_end if sim_end is None else sim_end
    rng = synth.host_rng_states(n_hosts, general_seed=1) if rng is None else rng
    init = np.array([U64_MAX, U64_MAX] if stats_init is None else stats_init, np.uint64)
    rng_o = rng.copy()
    cnt_o = np.zeros((n_nodes, n_nodes), np.uint64)
    f_o, d_o, mn_o, ne_o = O.packet_batch(o_lat, o_loss, case.pk, rng_o, case.round_end, case.bootstrap_end,
                                          sim_end, counters=cnt_o)
    dev = torch.device("cuda:0")
    t_pk = torch.from_numpy((case.pk if by_ip is None else by_ip[1]).view(np.uint8).copy()).to(dev)
    t_hp = torch.from_numpy(case.host_ptr.view(np.int32).copy()).to(dev)
    t_rng = torch.from_numpy(rng.view(np.int64).copy()).to(dev)
    t_f = torch.full((n_pkts,), -1, dtype=torch.int32, device=dev)
    t_d = torch.full((n_pkts,), -1, dtype=torch.int64, device=dev)
    t_c = torch.zeros(n_nodes * n_nodes, dtype=torch.int64, device=dev)
    t_s = torch.from_numpy(init.view(np.int64).copy()).to(dev)
    if by_ip is None:
        plan.packet_batch(t_pk, t_hp, t_rng, case.round_end, case.bootstrap_end, sim_end, t_f, t_d, t_c, t_s)
    else:
        plan.packet_batch_ip(by_ip[0], t_pk, t_hp, t_rng, case.round_end, case.bootstrap_end, sim_end, t_f, t_d,
                             t_c, t_s)
    out = SimpleNamespace(flags=t_f.cpu().numpy().view(np.uint32), deliver=t_d.cpu().numpy().view(np.uint64),
                          rng=t_rng.cpu().numpy().view(np.uint64).reshape(n_hosts, 4),
                          counters=t_c.cpu().numpy().view(np.uint64).reshape(n_nodes, n_nodes),
                          stats=t_s.cpu().numpy().view(np.uint64), oracle_stats=(mn_o, ne_o))
    assert np.array_equal(out.flags, f_o), case.name
    assert np.array_equal(out.deliver, d_o), case.name
    assert np.array_equal(out.rng, rng_o), case.name
    assert np.array_equal(out.counters, cnt_o), case.name
    assert int(out.stats[0]) == min(int(init[0]), mn_o) and int(out.stats[1]) == min(int(init[1]), ne_o), case.name
    return out


# ------------------------------------------------------------------- events
LADDER = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 1023, 1024)
LADDER_TIMES = {LADDER.index(1024): "equal", LADDER.index(1023): "descending"}
T_EVENTS = 1_000_000


def events_from_sizes(sizes, n_dst, n_hosts, unsent_frac, seed, times=None, counts=None):
    """A batch in which destination d receives exactly sizes[d] SENT packets,
    at random batch positions, among DROPPED / NONE packets (unsent_frac of the
    batch) with random destinations, some of them the zero-size destinations.
    times: {destination: "ties" | "equal" | "descending"}, default "ties" (3
    distinct deliver times a group); "equal": one time; "descending": strictly
    decreasing in batch index.  Hosts get multinomial shares of the batch
    (or `counts`); event bases are 2**63 + host.
    Returns (host_ptr, flags, deliver, dst, n_dst, base)."""
    sizes = np.asarray(sizes, np.int64)
    assert len(sizes) == n_dst and (sizes >= 0).all() and 0 <= unsent_frac < 1
    times = times or {}
    rng = np.random.default_rng(seed)
    n_sent = int(sizes.sum())
    n = int(counts.sum()) if counts is not None else int(round(n_sent / (1.0 - unsent_frac)))
    n_unsent = n - n_sent
    assert n_unsent >= 0
    perm = rng.permutation(n)
    sent_at, unsent_at = perm[:n_sent], perm[n_sent:]
    flags = np.empty(n, np.uint32)
    flags[sent_at] = O.PDS_INET_SENT
    flags[unsent_at] = rng.choice([O.PDS_INET_DROPPED, O.PDS_NONE], size=n_unsent)
    dst = np.empty(n, np.uint32)
    dst[sent_at] = np.repeat(np.arange(n_dst), sizes)
    dst[unsent_at] = rng.integers(0, max(n_dst, 1), size=n_unsent)
    empty = np.nonzero(sizes == 0)[0]
    if len(empty) and n_unsent:  # every third unsent packet names a destination that receives nothing
        third = unsent_at[::3]
        dst[third] = empty[rng.integers(0, len(empty), size=len(third))]
    deliver = (T_EVENTS + rng.integers(0, 3, size=n)).astype(np.uint64)
    for d, kind in times.items():
        at = np.nonzero((dst == d) & (flags == O.PDS_INET_SENT))[0]
        if kind == "equal":
            deliver[at] = T_EVENTS + 1
        elif kind == "descending":
            deliver[at] = (T_EVENTS + n - at).astype(np.uint64)
        else:
            assert kind == "ties", kind
    if counts is None:
        counts = rng.multinomial(n, np.ones(n_hosts) / n_hosts)
    assert len(counts) == n_hosts
    host_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    base = (np.uint64(2**63) + np.arange(n_hosts, dtype=np.uint64)).astype(np.uint64)
    return host_ptr, flags, deliver, dst, n_dst, base


def events_lexsort(host_ptr, flags, deliver, dst, n_dst, base):
    """The statement of test_packet_events.test_oracle_heap_order_is_lexicographic
    as a reference of its own: event ids per host, consecutive from its base in
    send order; the sent packets by (destination, time, source host, event id).
    Returns (event_id, order, dst_ptr, advanced base)."""
    hp = host_ptr.astype(np.int64)
    n_hosts = len(hp) - 1
    sent = flags == O.PDS_INET_SENT
    host_of = np.repeat(np.arange(n_hosts), np.diff(hp))
    before = np.concatenate([[0], np.cumsum(sent)]).astype(np.int64)  # sent packets below index p
    eid = np.full(len(flags), U64_MAX, np.uint64)
    idx = np.nonzero(sent)[0]
    eid[idx] = base[host_of[idx]] + (before[idx] - before[hp[host_of[idx]]]).astype(np.uint64)
    order = idx[np.lexsort((eid[idx], host_of[idx], deliver[idx], dst[idx]))]
    dst_ptr = np.searchsorted(dst[order], np.arange(n_dst + 1)).astype(np.uint32)
    new_base = base + (before[hp[1:]] - before[hp[:-1]]).astype(np.uint64)
    return eid, order.astype(np.uint32), dst_ptr, new_base


def _frozen(batch):
    """A cached batch is shared: read-only (O.packet_events advances the base it is given, pass a copy)."""
    for a in batch:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return batch


def group_sizes(flags, dst, n_dst):
    return np.bincount(dst[flags == O.PDS_INET_SENT], minlength=n_dst)


def n_chunks(n_pkts):
    return (n_pkts + EV_CHUNK - 1) // EV_CHUNK


@functools.lru_cache(maxsize=None)
def ladder_sizes(extra=()):
    """The ladder, `extra` group sizes, and 20 random small groups."""
    small = np.random.default_rng(81).integers(1, 200, size=20)
    return np.concatenate([LADDER, np.asarray(extra, np.int64), small]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def events_ladder(extra=()):
    """Section 4.1 (and 4.4 with extra=(1025,)): every ladder size as one
    destination's group, in one chunked batch of 60 hosts."""
    sizes = ladder_sizes(extra)
    return _frozen(events_from_sizes(sizes, len(sizes), 60, 0.2, 82, times=LADDER_TIMES))


@functools.lru_cache(maxsize=None)
def events_ladder_spread(n_dst):
    """The ladder among n_dst destinations: its groups at indices spread over
    the range, 0 and n_dst - 1 among them; every 97th other destination
    receives one event, the rest none.  Returns (batch, ladder indices)."""
    at = np.unique(np.linspace(0, n_dst - 1, len(LADDER)).astype(np.int64))
    assert len(at) == len(LADDER) and at[0] == 0 and at[-1] == n_dst - 1
    sizes = np.zeros(n_dst, np.int64)
    sizes[5::97] = 1
    sizes[at] = LADDER
    times = {int(at[k]): v for k, v in LADDER_TIMES.items()}
    return _frozen(events_from_sizes(sizes, n_dst, 60, 0.2, 83, times=times)), at


@functools.lru_cache(maxsize=None)
def events_many_big():
    """600 groups of 300..449 events (all on the big-list sort, more than its
    512 workgroups), ~285k packets: more than 64 chunks."""
    sizes = 300 + np.arange(600) % 150
    return _frozen(events_from_sizes(sizes, 600, 300, 0.21, 84))


def events_random(counts, n_dst, seed, p_sent=0.7):
    """A batch with counts[h] packets from host h, each SENT with p_sent, to
    uniform destinations, deliver times from 5 values."""
    counts = np.asarray(counts, np.int64)
    rng = np.random.default_rng(seed)
    n = int(counts.sum())
    host_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    flags = rng.choice([O.PDS_INET_SENT, O.PDS_INET_DROPPED, O.PDS_NONE], size=n,
                       p=[p_sent, (1 - p_sent) / 2, (1 - p_sent) / 2]).astype(np.uint32)
    deliver = (T_EVENTS + rng.integers(0, 5, size=n)).astype(np.uint64)
    dst = rng.integers(0, n_dst, size=n).astype(np.uint32)
    base = (np.uint64(2**63) + np.arange(len(counts), dtype=np.uint64)).astype(np.uint64)
    return host_ptr, flags, deliver, dst, n_dst, base


class EventsRun:
    """srt_packet_events on one batch with check=False; read() copies the
    outputs as they stand, status() is srt_packet_events_status."""

    def __init__(self, plan, batch):
        import torch

        host_ptr, flags, deliver, dst, n_dst, base = batch
        dev = torch.device("cuda:0")
        n = len(flags)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
        self.plan = plan
        self.inputs = (t(host_ptr, np.int32), t(flags, np.int32), t(deliver, np.int64), t(dst, np.int32))
        self.base = t(base, np.int64)
        self.eid = torch.zeros(n, dtype=torch.int64, device=dev)
        self.order = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        self.ptr = torch.full((n_dst + 1,), -1, dtype=torch.int32, device=dev)
        plan.packet_events(*self.inputs, n_dst, self.base, self.eid, self.order, self.ptr, check=False)

    def read(self):
        ptr = self.ptr.cpu().numpy().view(np.uint32)
        return (self.eid.cpu().numpy().view(np.uint64), self.order.cpu().numpy().view(np.uint32)[:ptr[-1]], ptr,
                self.base.cpu().numpy().view(np.uint64))

    def status(self):
        self.plan.packet_events_status()
