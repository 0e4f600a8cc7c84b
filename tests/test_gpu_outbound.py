"""Outbound relay stage on the device (srt_outbound over a plan): the CPU
tests' scenario bit-equal to the model and to the host-only form in both
qdiscs, a wave wider than the LDS window, ring overflow reported without a
fault, and the chain outbound -> send order -> srt_packet_batch against the
oracle fed with the model's send times and order."""
import numpy as np
import pytest

import outbound_model as M
import outbound_scenario as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu
QDISCS = pytest.mark.parametrize("qdisc", [M.FIFO, M.RR], ids=["fifo", "rr"])
SPLIT = pytest.mark.parametrize("split", [False, True], ids=["one_call", "split"])


@pytest.fixture(scope="module")
def plan():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    yield p
    p.close()


@QDISCS
@SPLIT
def test_gpu_outbound_equals_model_and_host_only(plan, qdisc, split):
    """max_sockets 320: the cursors and socket queues stay in HBM / L2, the packets in the LDS window"""
    sc = S.scenario()
    calls, mouts, m = S.model_results(qdisc, split=split)
    outs, state, stats = S.run_lib(sc, calls, qdisc, plan=plan)
    S.assert_same(outs, mouts, state, m)
    assert stats[-1] == (0, m.pending())
    h_outs, h_state, h_stats = S.run_lib(sc, calls, qdisc)
    assert stats == h_stats
    for d, h in zip(outs, h_outs):
        assert d["base"] == h["base"] and d["late"] == h["late"] and d["late_count"] == h["late_count"]
        for f in ("status", "send", "rank"):
            assert d[f].tobytes() == h[f].tobytes(), f
    assert state.tobytes() == h_state.tobytes()


@QDISCS
def test_gpu_outbound_wave_wider_than_the_lds_window(plan, qdisc):
    """A wave whose 64 hosts send more packets than its LDS window holds (2,048)
    walks them from HBM with the links in the HBM array; the remainder wave
    beside it from LDS.  max_sockets 4: both keep their cursors in LDS.  Two
    calls, so both forms also take packets back out of the ring."""
    n_hosts, n_pkts = 70, 2400
    rng = np.random.default_rng(11)
    sc = S.make_scenario(rng, n_hosts, n_pkts, rng.integers(1, 5, size=n_hosts),
                         rng.choice(np.array([60_000, 125_000_000], np.uint64), size=n_hosts), 300 * M.MS)
    calls = S.calls_of(sc, [300 * M.MS, 400 * M.MS])
    assert 2048 < calls[0]["host_ptr"][64] < 2048 + 256 and len(calls[0]["ids"]) == n_pkts
    assert 0 < n_pkts - calls[0]["host_ptr"][64] <= 2048
    mouts, m = S.run_model(sc, calls, qdisc, max_sockets=4)
    assert len(mouts[1]["late"]) > 100 and m.pending() > 0
    outs, state, stats = S.run_lib(sc, calls, qdisc, plan=plan, max_sockets=4, queue_cap=256)
    S.assert_same(outs, mouts, state, m)
    assert stats[-1] == (0, m.pending())


@QDISCS
def test_gpu_ring_overflow_reported_not_faulted(plan, qdisc):
    """queue_cap 4: the capacity check precedes every ring write; host 1 is
    flagged and marked, hosts 0 and 2 still equal the model"""
    from shadow_amd import _lib

    sc, calls, mouts, m = S.overflow_case(qdisc)
    outs, state, stats = S.run_lib(sc, calls, qdisc, plan=plan, max_sockets=4, queue_cap=4, bootstrap_end=0,
                                   check=False)
    assert stats[0][0] & _lib.OUTBOUND_RING_OVERFLOW
    assert state["overflow"].tolist() == [0, 1, 0]
    S.assert_same(outs, mouts, state, m, calls=calls, sc=sc, hosts={0, 2})
    _, h_state, _ = S.run_lib(sc, calls, qdisc, max_sockets=4, queue_cap=4, bootstrap_end=0, check=False)
    assert state.tobytes() == h_state.tobytes()


def test_gpu_outbound_then_packet_batch():
    """The chain on a 50-node plan, 200 hosts, 20,000 packets: outbound (round
    robin, a third of the hosts throttled, in two windows so that late records
    take part), srt_pkt built from send_ns in the helper's rank order,
    srt_packet_batch -- against the oracle's packet_batch fed with the MODEL's
    send times and order.  The RNG draws follow the send order, so a wrong rank
    or grouping changes flags and deliver times even where the times agree."""
    import torch

    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import OUTBOUND_LATE_DTYPE, OutboundRelay, RoutingPlan, outbound_send_order

    n_nodes, n_hosts, n_pkts, seed = 50, 200, 20_000, 5
    src, dst, lat, loss = synth.complete_graph(n_nodes, seed, loss_max=0.25)
    r0, r1 = 1_000_000_000, 1_000_000_000 + 5 * synth.MS
    pk, host_ptr, _ = synth.packet_round(n_hosts, n_nodes, n_pkts, seed, r0, r1)
    rng = np.random.default_rng(seed)
    host = pk["src_host"]
    op = np.zeros(n_pkts, S.OUT_PKT_DTYPE)
    op["ready_ns"] = pk["t_ns"]
    op["total_size"] = pk["payload_size"] + 40
    op["socket"] = rng.integers(0, 4, size=n_pkts)
    op["flags"] = rng.random(n_pkts) < 0.02
    for h in range(n_hosts):
        b, e = int(host_ptr[h]), int(host_ptr[h + 1])
        op["priority"][b:e] = 7 + rng.permutation(e - b)
    bw = np.where(np.arange(n_hosts) % 3 == 0, 125_000, 125_000_000).astype(np.uint64)
    # window 1: the round's arrivals; window 2: nothing new, the throttled hosts go on draining
    u1, u2 = r1, r1 + 300 * synth.MS
    empty = np.zeros(0, S.OUT_PKT_DTYPE)
    zero_ptr = np.zeros(n_hosts + 1, np.uint32)
    # ---- model
    m = M.OutboundModel(bw, M.RR, 4)
    st1, sn1, rk1, late1, _ = m.run(op, host_ptr, u1, 0)
    _, _, _, late2, _ = m.run(empty, zero_ptr, u2, 0)
    assert late1 == [] and len(late2) > 1000 and m.pending() > 0
    assert ((st1 & M.CACHED) != 0).sum() > 0

    def expected(sel_idx, sel_host, sel_rank, sel_send):
        """the model's packets of one round in send order -> srt_pkt records, grouping"""
        keep = sel_rank != M.U64
        idx, hh, rr, ss = sel_idx[keep], sel_host[keep], sel_rank[keep], sel_send[keep]
        o = np.lexsort((rr, hh))
        out = pk[idx[o]].copy()
        out["t_ns"] = ss[o]
        return out, np.searchsorted(hh[o], np.arange(n_hosts + 1)).astype(np.uint32), idx[o]

    e1 = expected(np.arange(n_pkts), host, rk1, sn1)
    l2 = np.array(late2, dtype=np.uint64).reshape(-1, 5)
    e2 = expected(l2[:, 0].astype(np.int64), l2[:, 4].astype(np.uint32), l2[:, 2], l2[:, 1])
    # ---- device
    rp = RoutingPlan(NetworkGraph.from_edges(n_nodes, src, dst, lat, loss), np.arange(n_nodes, dtype=np.uint32)).run()
    table = rp.fetch()
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    t_pk = t(pk.view(np.uint8), np.uint8).view(n_pkts, 24)
    t_hp = t(host_ptr, np.int32)
    t_st = torch.zeros(n_pkts, dtype=torch.int32, device=dev)
    t_sn = torch.zeros(n_pkts, dtype=torch.int64, device=dev)
    t_rk = torch.zeros(n_pkts, dtype=torch.int64, device=dev)
    t_late = torch.zeros(n_pkts * 32, dtype=torch.uint8, device=dev)
    t_cnt = torch.ones(1, dtype=torch.int32, device=dev)
    t_rng = t(synth.host_rng_states(n_hosts, 1), np.int64)
    rng_o = synth.host_rng_states(n_hosts, 1)
    ob = OutboundRelay(rp, bw, M.RR, 4, 256)
    rounds = []
    try:
        for k, until in enumerate((u1, u2)):
            if k == 0:
                ob.run(t(op, np.uint8), t_hp, until, 0, t_st, t_sn, t_rk, t_late, t_cnt)
                order, send_ptr = outbound_send_order(t_hp, t_rk)
                src_idx, send = order, t_sn[order]
            else:
                none = torch.zeros(0, dtype=torch.int64, device=dev)
                ob.run(torch.zeros(32, dtype=torch.uint8, device=dev), t(zero_ptr, np.int32), until, 0,
                       none.to(torch.int32), none, none, t_late, t_cnt)
                n_late = int(t_cnt.item())
                recs = t_late[:n_late * 32].view(torch.int64).view(n_late, 4)  # seq, send_ns, send_rank, status|host
                order, send_ptr = outbound_send_order(t(zero_ptr, np.int32), none, recs[:, 3] >> 32, recs[:, 2])
                src_idx, send = recs[order, 0], recs[order, 1]  # base 0: a first call's seq is its batch index
            assert ob.status()[0] == 0
            # srt_pkt of the round's sends, in the send order: the packet's record with t_ns = send_ns
            spk = t_pk[src_idx].clone()
            spk[:, 16:24] = send.view(-1, 1).view(torch.uint8).view(-1, 8)
            n_sent = spk.shape[0]
            t_f = torch.zeros(n_sent, dtype=torch.int32, device=dev)
            t_d = torch.zeros(n_sent, dtype=torch.int64, device=dev)
            rp.packet_batch(spk.contiguous().view(-1), send_ptr, t_rng, until, 0, 2**62, t_f, t_d)
            rounds.append((src_idx.cpu().numpy(), send_ptr.cpu().numpy().view(np.uint32),
                           spk.cpu().numpy().reshape(-1).view(O.PKT_DTYPE), t_f.cpu().numpy().view(np.uint32),
                           t_d.cpu().numpy().view(np.uint64)))
        pending = ob.status()[1]
        late_recs = t_late[:32 * int(t_cnt.item())].cpu().numpy().view(OUTBOUND_LATE_DTYPE)
    finally:
        ob.close()
        rp.close()
    assert pending == m.pending() and len(late_recs) == len(late2)
    for (idx, ptr, spk, f, d), (e_pk, e_ptr, e_idx), until in zip(rounds, (e1, e2), (u1, u2)):
        assert np.array_equal(idx, e_idx) and np.array_equal(ptr, e_ptr)
        assert spk.tobytes() == e_pk.view(O.PKT_DTYPE).tobytes()
        f_o, d_o, _, _ = O.packet_batch(table.latency_ns, table.packet_loss, e_pk.view(O.PKT_DTYPE), rng_o, until, 0,
                                        2**62)
        assert (f_o == O.PDS_INET_SENT).sum() > 0 and (f_o == O.PDS_INET_DROPPED).sum() > 0
        assert np.array_equal(f, f_o) and np.array_equal(d, d_o)


def test_gpu_closing_the_plan_closes_its_relays():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import OutboundRelay, RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    ob = OutboundRelay(p, [1000, 1000], M.FIFO, 4, 4)
    try:
        p.close()
        closed = not ob._h
    finally:
        ob.close()
        p.close()
    assert closed
