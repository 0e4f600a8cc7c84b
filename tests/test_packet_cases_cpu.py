"""The inputs of the packet-stage edge tests (tests/packet_cases.py) reach the
branches they are named for: checked here on the CPU, with the oracle only,
so the GPU tests' "this case runs that path" is proved and not claimed.  Also
pins the kernel constants the cases mirror: a retuned constant fails here,
which is the signal to move the edges."""
import os
import re

import numpy as np
import pytest

import packet_cases as P
from oracle import oracle as O
from shadow_amd import synth

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shadow_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return int(m[0])


def test_constants_match_the_kernels():
    pkt, ev = _src("srt_packet.hip"), _src("srt_events.hip")
    assert _one(r"constexpr int RT = (\d+);", pkt) == P.RT
    assert _one(r"#define SRT_PKT_HB (\d+)", pkt) == P.HB
    assert "constexpr int HB = SRT_PKT_HB;" in pkt
    assert _one(r"constexpr uint32_t DCAP = (\d+);", pkt) == P.DCAP
    assert _one(r"constexpr int KP = (\d+);", pkt) == P.KP
    assert _one(r"constexpr int PF = (\d+);", pkt) == P.PF
    assert P.BLOCK_PKTS == P.RT * P.KP == 2048
    assert _one(r"constexpr uint32_t EV_CAP = (\d+);", ev) == P.EV_CAP
    assert _one(r"constexpr uint32_t EV_SMALL = (\d+);", ev) == P.EV_SMALL
    assert _one(r"constexpr uint32_t EV_CHUNK = (\d+),", ev) == P.EV_CHUNK
    assert _one(r"EV_LDS_DST = (\d+);", ev) == P.EV_LDS_DST
    assert _one(r"event_big_group_sort_kernel, dim3\(std::min<uint32_t>\(n_dst_hosts, (\d+)\)\)", ev) == P.EV_BIG_GRID
    assert _one(r"p0 < e; p0 \+= (\d+)\)", ev) == P.EV_WAVE
    assert _one(r"event_id_kernel, dim3\(\(n_hosts \+ 3\) / (\d+)\), dim3\(256\)", ev) == P.EV_ID_HOSTS
    assert _one(r"per = \(chunks \+ 3\) / (\d+),", ev) == P.EV_COL_LANES
    assert set(re.findall(r"c < c1; c \+= (\d+)\)", ev)) == {str(P.EV_COL_STEP)}
    # the largest dynamic-LDS launch: the cursors and the 64-destination block prefixes
    assert 4 * P.EV_LDS_DST + 4 * ((P.EV_LDS_DST + 63) // 64) == 63_488 + 992 <= 64 * 1024


# ------------------------------------------------------------------ packets
def _oracle(case, sim_end=None):
    lat, loss = P.extremes_table()
    rng = synth.host_rng_states(case.n_hosts, general_seed=1)
    before = rng.copy()
    cnt = np.zeros(lat.shape, np.uint64)
    f, d, mn, ne = O.packet_batch(lat, loss, case.pk, rng, case.round_end, case.bootstrap_end,
                                  case.sim_end if sim_end is None else sim_end, counters=cnt)
    return f, d, mn, ne, before, rng, cnt


def _advance(state, k):
    s = state.copy()
    for _ in range(k):
        O.xoshiro_next(s)
    return s


def _loss_bits(pk):
    _, loss = P.extremes_table()
    return loss.view(np.uint32)[pk["src_row"], pk["dst_row"]]


def test_extremes_graph_table():
    lat, loss = P.extremes_table(40, 11)
    bits = loss.view(np.uint32)[~np.eye(40, dtype=bool)]
    assert (bits == P.LOSS_ZERO_BITS).sum() == 32
    assert (bits == P.LOSS_ONE_BITS).sum() == 590
    assert ((bits != P.LOSS_ZERO_BITS) & (bits != P.LOSS_ONE_BITS)).sum() == 938
    src, dst, lat_e, loss_e = P.extremes_graph(40, 11)
    s0, d0, l0, p0 = synth.complete_graph(40, 11, loss_max=0.25)
    assert np.array_equal(src, s0) and np.array_equal(dst, d0) and np.array_equal(lat_e, l0)
    assert (loss_e[0::7] == 0.0).all() and (loss_e[3::7] == 1.0).all()
    rest = np.ones(len(p0), bool)
    rest[0::7] = rest[3::7] = False
    assert np.array_equal(loss_e[rest], p0[rest])


def test_round_from_counts_shape():
    counts = [0, 3, 0, 0, 5, 1, 0]
    pins = [{"host": 4, "k": 2, "t_ns": 77, "payload_size": 9, "rows": (3, 1)}, {"host": 1, "k": -1, "t_ns": 10**12}]
    pk, host_ptr, host_row = P.round_from_counts(counts, 4, 1, 100, 200, pins=pins)
    assert pk.dtype == O.PKT_DTYPE and np.array_equal(np.diff(host_ptr.astype(np.int64)), counts)
    assert np.array_equal(host_row, np.arange(7) % 4)
    assert np.array_equal(pk["src_host"], np.repeat(np.arange(7), counts))
    p = P.pin_index(host_ptr, pins[0])
    assert p == 3 + 2 and pk["t_ns"][p] == 77 and pk["payload_size"][p] == 9
    assert (pk["src_row"][p], pk["dst_row"][p]) == (3, 1)
    assert pk["t_ns"][P.pin_index(host_ptr, pins[1])] == 10**12
    for h in range(7):
        assert (np.diff(pk["t_ns"][host_ptr[h]:host_ptr[h + 1]].astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("past_round", [False, True])
def test_case_extremes(past_round):
    case = P.case_extremes(past_round)
    f, d, _, _, before, after, _ = _oracle(case)
    pk = case.pk
    assert case.n_hosts == 200 and len(pk) == 20_000
    bits = _loss_bits(pk)
    boot = pk["t_ns"] < case.bootstrap_end
    one, zero, pay = bits == P.LOSS_ONE_BITS, bits == P.LOSS_ZERO_BITS, pk["payload_size"] > 0
    # both extremes are addressed with and without payload, in and out of bootstrap
    for sel in (one, zero):
        assert (sel & pay).sum() > 100 and (sel & ~pay).sum() > 10
    if past_round:
        assert boot.all() and (f == O.PDS_INET_SENT).all()
    else:
        assert (one & pay & boot).sum() > 100 and (one & pay & ~boot).sum() > 1000
        assert (f[one & pay & ~boot] == O.PDS_INET_DROPPED).all()
        assert (f[one & pay & boot] == O.PDS_INET_SENT).all()
        assert (f[one & ~pay] == O.PDS_INET_SENT).all()
        assert (f[zero] == O.PDS_INET_SENT).all()
        assert (f == O.PDS_INET_DROPPED).sum() > (one & pay & ~boot).sum()  # and partial losses drop too
    # one draw per live packet, dropped or not (no packet is completed here)
    counts = np.diff(case.host_ptr.astype(np.int64))
    for h in (0, 57, 199):
        assert np.array_equal(after[h], _advance(before[h], int(counts[h])))
    sent = f == O.PDS_INET_SENT
    assert (d[sent] == case.round_end).any() and (d[sent] > case.round_end).any()


def test_case_scratch_completed():
    case = P.case_scratch_completed()
    f, d, _, _, before, after, _ = _oracle(case)
    totals = P.block_totals(case.host_ptr)
    assert case.n_hosts == 48 and len(totals) == 3 and totals.sum() == 60_000
    assert (totals > P.DCAP).all() and (np.abs(totals - 20_000) < 1000).all()
    assert ((f == O.PDS_NONE).sum(), (f == O.PDS_INET_SENT).sum(), (f == O.PDS_INET_DROPPED).sum()) == (
        36_126, 12_889, 10_985)
    sent = f == O.PDS_INET_SENT
    assert ((d[sent] == case.round_end).sum(), (d[sent] > case.round_end).sum()) == (416, 12_473)
    done = case.pk["t_ns"] >= case.sim_end
    assert np.array_equal(done, f == O.PDS_NONE)
    # every host has completed packets (all 48 walks are redone), and a draw for the live ones only
    live = np.add.reduceat((~done).astype(np.int64), case.host_ptr[:-1].astype(np.int64))
    counts = np.diff(case.host_ptr.astype(np.int64))
    assert (live < counts).all() and (live > 0).all()
    for h in (0, 16, 47):
        assert np.array_equal(after[h], _advance(before[h], int(live[h])))
    bits = _loss_bits(case.pk)
    assert (bits[~done] == P.LOSS_ZERO_BITS).any() and (bits[~done] == P.LOSS_ONE_BITS).any()


@pytest.mark.parametrize("last_block,empty_block", [(P.DCAP, False), (P.DCAP + 1, False), (P.DCAP + 1, True)])
def test_case_block_totals(last_block, empty_block):
    case = P.case_block_totals(last_block, empty_block)
    hp = case.host_ptr.astype(np.int64)
    counts = np.diff(hp)
    totals = P.block_totals(case.host_ptr)
    assert totals.tolist() == case.totals
    assert case.totals == [2048] + ([0] if empty_block else []) + [2049, last_block]
    assert case.n_hosts == (51 if empty_block else 35) and len(counts) % P.HB == 3
    # empty hosts: a block's first host, two neighbours, a block's last host, the last host overall
    shift = P.HB if empty_block else 0
    for h in (0, 7, 8, P.HB + shift + P.HB - 1, case.n_hosts - 1):
        assert counts[h] == 0
    assert (counts == 0).sum() == 5 + shift
    f, d, _, _, before, after, _ = _oracle(case)
    done = case.pk["t_ns"] >= case.sim_end
    host_of = np.repeat(np.arange(case.n_hosts), counts)
    # block 0: exactly one host has completed packets, and all of its packets are
    b0 = done[:hp[P.HB]]
    assert set(host_of[:hp[P.HB]][b0]) == {P.ALL_DONE_HOST} and b0.sum() == counts[P.ALL_DONE_HOST] > 0
    assert np.array_equal(after[P.ALL_DONE_HOST], before[P.ALL_DONE_HOST])
    # the 2049 block and the last block: the only completed packet is the block's
    # last, past the lanes' first 2048, owned by the block's last non-empty host
    for blk, pin in zip(case.tail_blocks, case.tail_pins):
        pb, pe = hp[blk * P.HB], hp[min((blk + 1) * P.HB, case.n_hosts)]
        at = np.nonzero(done[pb:pe])[0]
        assert at.tolist() == [pe - pb - 1] and at[0] >= P.BLOCK_PKTS
        assert P.pin_index(case.host_ptr, pin) == pe - 1
        owner = pin["host"]
        assert host_of[pe - 1] == owner and (counts[owner + 1:min((blk + 1) * P.HB, case.n_hosts)] == 0).all()
        assert owner % P.HB > 0 and counts[owner] > 1
        assert np.array_equal(after[owner], _advance(before[owner], int(counts[owner]) - 1))
    assert done.sum() == counts[P.ALL_DONE_HOST] + 2
    sent = f == O.PDS_INET_SENT
    assert (d[sent] == case.round_end).any() and (d[sent] > case.round_end).any()
    assert (f == O.PDS_INET_DROPPED).any()


def test_case_equalities():
    case = P.case_equalities()
    f, d, _, _, _, _, _ = _oracle(case)
    lat, _ = P.extremes_table()
    got = {}
    for pin in case.pins:
        p = P.pin_index(case.host_ptr, pin)
        assert case.pk["t_ns"][p] == pin["t_ns"]
        got[pin["name"]] = (int(f[p]), int(d[p]))
    assert case.pins[0]["t_ns"] == case.sim_end and case.pins[1]["t_ns"] == case.sim_end - 1
    assert case.pins[2]["t_ns"] == case.bootstrap_end and case.pins[3]["t_ns"] == case.bootstrap_end - 1
    assert int(lat[case.pins[4]["rows"]]) == case.delay
    assert case.pins[4]["t_ns"] + case.delay == case.round_end
    assert case.pins[5]["t_ns"] + case.delay == case.round_end - 1
    assert case.bootstrap_end <= case.pins[5]["t_ns"] < case.pins[4]["t_ns"] < case.sim_end
    assert got["t == sim_end"] == (O.PDS_NONE, 0)                      # completed
    assert got["t == sim_end - 1"][0] != O.PDS_NONE                     # live
    assert got["t == bootstrap_end"] == (O.PDS_INET_DROPPED, 0)         # not bootstrapping: loss 1.0 drops
    assert got["t == bootstrap_end - 1"][0] == O.PDS_INET_SENT          # bootstrapping: never dropped
    assert got["t + delay == round_end"] == (O.PDS_INET_SENT, case.round_end)       # no clamp needed
    assert got["t + delay == round_end - 1"] == (O.PDS_INET_SENT, case.round_end)   # clamped up by 1 ns
    # the unclamped side of the same comparison
    sent = f == O.PDS_INET_SENT
    assert (d[sent] > case.round_end).any()


def test_case_sends_nothing():
    case = P.case_sends_nothing()
    f, d, mn, ne, before, after, cnt = _oracle(case)
    assert len(case.pk) == 3000 and (case.pk["payload_size"] > 0).all()
    assert (_loss_bits(case.pk) == P.LOSS_ONE_BITS).all()
    assert (f == O.PDS_INET_DROPPED).all() and (d == 0).all()
    assert mn == ne == int(P.U64_MAX)   # the caller's stats stay as initialised
    assert not cnt.any()
    assert not np.array_equal(before, after)  # the draws were still taken


def test_case_two_rounds():
    first, second = P.case_two_rounds()
    assert first.n_hosts == second.n_hosts == 35 and len(first.pk) == 500
    assert (P.block_totals(first.host_ptr) <= P.BLOCK_PKTS).all()
    assert P.block_totals(second.host_ptr).tolist() == [2048, 2049, P.DCAP + 1]
    assert len(second.pk) > len(first.pk)  # the draws scratch has to grow
    assert second.pk["t_ns"].min() >= first.round_end


def test_case_late_unresolved():
    case = P.case_late_unresolved()
    hp = case.host_ptr.astype(np.int64)
    assert case.n_hosts == 48 and P.block_totals(case.host_ptr).tolist() == [300, 2600, 300]
    p = P.pin_index(case.host_ptr, case.pin)
    assert p - hp[P.HB] >= P.BLOCK_PKTS and hp[P.HB] <= p < hp[2 * P.HB]
    # the only packet at or after t_bad: with sim_end = t_bad it alone is completed
    assert (np.nonzero(case.pk["t_ns"] >= case.t_bad)[0] == [p]).all()
    f = _oracle(case, sim_end=case.t_bad)[0]
    assert np.nonzero(f == O.PDS_NONE)[0].tolist() == [p]


# ------------------------------------------------------------------- events
def _in(lo, hi, sizes):
    return int(((sizes > lo) & (sizes <= hi)).sum())


def test_events_from_sizes_shape():
    sizes = [0, 5, 0, 7, 300]
    host_ptr, flags, deliver, dst, n_dst, base = P.events_from_sizes(
        sizes, 5, 9, 0.25, 1, times={1: "equal", 3: "descending"})
    assert P.group_sizes(flags, dst, n_dst).tolist() == sizes
    assert len(flags) == 416 and host_ptr[-1] == 416 and len(host_ptr) == 10
    unsent = flags != O.PDS_INET_SENT
    assert set(flags[unsent]) == {O.PDS_INET_DROPPED, O.PDS_NONE}
    assert (dst[unsent] == 0).any() and (dst[unsent] == 2).any() and (dst[unsent] == 4).any()
    sent_at = np.nonzero(~unsent)[0]
    assert not np.array_equal(dst[sent_at], np.sort(dst[sent_at]))  # spread over the batch, not grouped
    assert len(set(deliver[(dst == 1) & ~unsent])) == 1
    assert (np.diff(deliver[(dst == 3) & ~unsent].astype(np.int64)) < 0).all()
    assert len(set(deliver[(dst == 4) & ~unsent])) == 3
    assert np.array_equal(base, 2**63 + np.arange(9, dtype=np.uint64))


def _check_ladder(batch, at, extra=()):
    host_ptr, flags, deliver, dst, n_dst, base = batch
    sizes = P.group_sizes(flags, dst, n_dst)
    assert sizes[at].tolist() == list(P.LADDER)
    sent = flags == O.PDS_INET_SENT
    g1024, g1023 = at[P.LADDER.index(1024)], at[P.LADDER.index(1023)]
    assert len(set(deliver[sent & (dst == g1024)])) == 1
    assert (np.diff(deliver[sent & (dst == g1023)].astype(np.int64)) < 0).all()
    for k, d in enumerate(at):  # "ties": 3 values wherever a group has room for them
        if d not in (g1024, g1023) and P.LADDER[k] >= 63:
            assert len(set(deliver[sent & (dst == d)])) == 3
    assert sizes[at[0]] == 0 and (sizes[dst[~sent]] == 0).any()  # unsent packets name destinations that receive nothing
    assert np.array_equal(base, 2**63 + np.arange(len(base), dtype=np.uint64))
    return sizes


def test_events_ladder_case():
    batch = P.events_ladder()
    sizes = _check_ladder(batch, np.arange(len(P.LADDER)))
    assert batch[4] == 32 <= P.EV_LDS_DST and (sizes[len(P.LADDER):] >= 1).all() and sizes.max() == P.EV_CAP
    assert P.n_chunks(len(batch[1])) == 2
    assert _in(P.EV_SMALL, P.EV_CAP, sizes) == 4 and _in(P.EV_CAP, 10**9, sizes) == 0


def test_events_ladder_with_1025_case():
    batch = P.events_ladder((1025,))
    sizes = _check_ladder(batch, np.arange(len(P.LADDER)))
    assert sizes[len(P.LADDER)] == P.EV_CAP + 1
    assert _in(P.EV_SMALL, P.EV_CAP, sizes) == 4 and _in(P.EV_CAP, 10**9, sizes) == 1
    assert P.n_chunks(len(batch[1])) == 2


@pytest.mark.parametrize("n_dst", [P.EV_LDS_DST, P.EV_LDS_DST + 1])
def test_events_ladder_spread_case(n_dst):
    batch, at = P.events_ladder_spread(n_dst)
    assert batch[4] == n_dst and at[0] == 0 and at[-1] == n_dst - 1
    sizes = _check_ladder(batch, at)
    assert sizes.sum() == sum(P.LADDER) + (sizes == 1).sum() - 1 and (sizes == 1).sum() > 100
    assert P.n_chunks(len(batch[1])) == 2
    assert _in(P.EV_SMALL, P.EV_CAP, sizes) == 4 and _in(P.EV_CAP, 10**9, sizes) == 0


def test_events_many_big_case():
    host_ptr, flags, deliver, dst, n_dst, base = P.events_many_big()
    sizes = P.group_sizes(flags, dst, n_dst)
    assert np.array_equal(sizes, 300 + np.arange(600) % 150)
    assert n_dst == 600 > P.EV_BIG_GRID and _in(P.EV_SMALL, P.EV_CAP, sizes) == 600
    chunks = P.n_chunks(len(flags))
    assert chunks >= P.EV_COL_LANES * P.EV_COL_STEP + 1 == 65 and len(flags) <= 300_000
    # a lane's quarter of the chunks is longer than one 16-chunk step
    assert (chunks + P.EV_COL_LANES - 1) // P.EV_COL_LANES > P.EV_COL_STEP


@pytest.mark.parametrize("extra", [(), (1025,)])
def test_oracle_equals_lexsort_on_the_ladder(extra):
    host_ptr, flags, deliver, dst, n_dst, base = P.events_ladder(extra)
    ob = base.copy()
    eid_o, ord_o, ptr_o = O.packet_events(host_ptr, flags, deliver, dst, n_dst, ob)
    eid, order, ptr, nb = P.events_lexsort(host_ptr, flags, deliver, dst, n_dst, base)
    assert np.array_equal(eid, eid_o) and np.array_equal(order, ord_o) and np.array_equal(ptr, ptr_o)
    assert np.array_equal(nb, ob)
    # the statement of test_oracle_heap_order_is_lexicographic, spelled out
    sent = np.nonzero(flags == O.PDS_INET_SENT)[0]
    host_of = np.repeat(np.arange(len(host_ptr) - 1), np.diff(host_ptr.astype(np.int64)))
    lex = sent[np.lexsort((eid_o[sent], host_of[sent], deliver[sent], dst[sent]))]
    assert np.array_equal(ord_o, lex.astype(np.uint32))
    assert np.array_equal(ptr_o, np.searchsorted(dst[lex], np.arange(n_dst + 1)).astype(np.uint32))
