"""Send-batch gather on the device (srt_sendbatch over a plan): real outbound
windows bit-equal to the host-only form and to the model with the host count
on and across a wave, the hand-made edge cases, the chain srt_outbound_run ->
srt_sendbatch_run -> srt_packet_batch against the oracle without torch glue,
and the plan closing its instance."""
import numpy as np
import pytest

import outbound_model as M
import outbound_scenario as S
import sendbatch_model as SM
import sendbatch_scenario as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plan():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    yield p
    p.close()


@pytest.mark.parametrize("shape", [B.DENSE, B.SPARSE])
@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 130])
def test_gpu_equals_host_only_and_model(plan, n_hosts, shape):
    """dense: 0 to about 200 packets a host, a wave a host (segments over 64 loop); sparse: about one
    packet a host, eight hosts a wave.  Three windows; the third has a late list only."""
    qdisc = M.RR if n_hosts % 2 else M.FIFO
    ws, _ = B.windows(n_hosts, shape, qdisc)
    if shape == B.DENSE and n_hosts > 1:
        per_host = np.diff(ws[0]["host_ptr"].astype(np.int64))
        assert per_host.max() > 64 and (per_host == 0).any()
    assert sum(len(w["late"]) for w in ws) > 0
    outs = B.run_windows(plan, n_hosts, shape, qdisc)
    h_outs = B.run_windows(None, n_hosts, shape, qdisc)
    for k, (o, h, m) in enumerate(zip(outs, h_outs, B.model_windows(n_hosts, shape, qdisc))):
        B.assert_same(o, m, (k, "model"))
        B.assert_same(o, h, (k, "host-only"))


@pytest.mark.parametrize("case", B.CASES, ids=[c.__name__[5:] for c in B.CASES])
def test_gpu_hand_made(plan, case):
    case(lambda n_hosts, log_cap: B.Runner(plan, n_hosts, log_cap))


def test_gpu_error_paths(plan):
    B.error_paths(plan.handle)


def test_gpu_outbound_sendbatch_packet_batch():
    """The chain on a 50-node plan, 130 hosts, 2,000 packets, two rounds (the second a late list
    only): srt_outbound_run, srt_sendbatch_run, srt_packet_batch on device arrays handed on as they
    are.  The gather's output equals the records built from the MODEL's send times and order; flags,
    deliver times and RNG states equal the oracle's packet_batch on them.  Each round's send decision
    runs twice, once told n_sent and once, on a copy of the RNG states, told out_cap: the same."""
    import torch

    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import OutboundRelay, RoutingPlan, SendBatch

    n_nodes, n_hosts, n_pkts, seed = 50, 130, 2000, 5
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
    meta = np.zeros(n_pkts, SM.META_DTYPE)
    for f in ("src_row", "dst_row", "payload_size"):
        meta[f] = pk[f]
    meta["user"] = rng.integers(0, n_hosts, size=n_pkts)
    bw = np.where(np.arange(n_hosts) % 3 == 0, 125_000, 125_000_000).astype(np.uint64)
    u1, u2 = r1, r1 + 40 * synth.MS  # the throttled hosts drain some 320 packets late and keep some 220
    zero_ptr = np.zeros(n_hosts + 1, np.uint32)
    # ---- model
    m = M.OutboundModel(bw, M.RR, 4)
    st1, sn1, rk1, late1, _ = m.run(op, host_ptr, u1, 0)
    _, _, _, late2, _ = m.run(np.zeros(0, S.OUT_PKT_DTYPE), zero_ptr, u2, 0)
    assert late1 == [] and len(late2) > 100 and m.pending() > 0

    def expected(sel_idx, sel_host, sel_rank, sel_send):
        keep = sel_rank != M.U64
        idx, hh, rr, ss = sel_idx[keep], sel_host[keep], sel_rank[keep], sel_send[keep]
        o = np.lexsort((rr, hh))
        out = pk[idx[o]].copy()
        out["t_ns"] = ss[o]
        return out, np.searchsorted(hh[o], np.arange(n_hosts + 1)).astype(np.uint32), idx[o]

    l2 = np.array(late2, dtype=np.uint64).reshape(-1, 5)
    exp = [expected(np.arange(n_pkts), host, rk1, sn1),
           expected(l2[:, 0].astype(np.int64), l2[:, 4].astype(np.uint32), l2[:, 2], l2[:, 1])]
    # ---- device
    rp = RoutingPlan(NetworkGraph.from_edges(n_nodes, src, dst, lat, loss), np.arange(n_nodes, dtype=np.uint32)).run()
    table = rp.fetch()
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    out_cap = n_pkts
    t_late, t_cnt = z(n_pkts * 32, torch.uint8), z(1, torch.int32)
    o_pk, o_hp, o_us, o_sq = z(out_cap * 24, torch.uint8), z(n_hosts + 1, torch.int32), z(out_cap, torch.int32), z(
        out_cap, torch.int64)
    t_rng = t(synth.host_rng_states(n_hosts, 1), np.int64)
    rng_o = synth.host_rng_states(n_hosts, 1)
    batches = [(t(op, np.uint8), t(host_ptr, np.int32), t(meta, np.uint8), n_pkts),
               (z(32, torch.uint8), t(zero_ptr, np.int32), z(16, torch.uint8), 0)]
    ob = OutboundRelay(rp, bw, M.RR, 4, 256)
    sb = SendBatch(rp, n_hosts, n_pkts)
    rounds = []
    try:
        for (t_op, t_hp, t_meta, n), until in zip(batches, (u1, u2)):
            t_st, t_sn, t_rk = z(n, torch.int32), z(n, torch.int64), z(n, torch.int64)
            base = ob.run(t_op, t_hp, until, 0, t_st, t_sn, t_rk, t_late, t_cnt)
            sb.run(t_hp, t_meta, t_sn, t_rk, base, t_late, t_cnt, o_pk, o_hp, o_us, o_sq)
            # the send decision told out_cap, straight behind the gather: no host round trip before it
            rng_b = t_rng.clone()
            f_b, d_b = z(out_cap, torch.int32), z(out_cap, torch.int64)
            rp.packet_batch(o_pk, o_hp, rng_b, until, 0, 2**62, f_b, d_b)
            assert ob.status()[0] == 0
            flags, n_sent = sb.status()
            f_a, d_a = z(n_sent, torch.int32), z(n_sent, torch.int64)
            rp.packet_batch(o_pk, o_hp, t_rng, until, 0, 2**62, f_a, d_a)
            assert torch.equal(f_a, f_b[:n_sent]) and torch.equal(d_a, d_b[:n_sent]) and torch.equal(t_rng, rng_b)
            rounds.append((n_sent, o_hp.cpu().numpy().view(np.uint32), o_pk.cpu().numpy()[:24 * n_sent].view(
                O.PKT_DTYPE), o_us.cpu().numpy().view(np.uint32)[:n_sent], o_sq.cpu().numpy().view(np.uint64)[:n_sent],
                f_a.cpu().numpy().view(np.uint32), d_a.cpu().numpy().view(np.uint64),
                t_rng.cpu().numpy().view(np.uint64)))
        pending = ob.status()[1]
    finally:
        sb.close()
        ob.close()
        rp.close()
    assert pending == m.pending()
    for (n_sent, ptr, spk, user, seq, f, d, rng_d), (e_pk, e_ptr, e_idx), until in zip(rounds, exp, (u1, u2)):
        assert n_sent == len(e_idx) and np.array_equal(ptr, e_ptr)
        assert spk.tobytes() == e_pk.view(O.PKT_DTYPE).tobytes()
        assert np.array_equal(seq, e_idx.astype(np.uint64)) and np.array_equal(user, meta["user"][e_idx])
        f_o, d_o, _, _ = O.packet_batch(table.latency_ns, table.packet_loss, e_pk.view(O.PKT_DTYPE), rng_o, until, 0,
                                        2**62)
        assert (f_o == O.PDS_INET_SENT).sum() > 0 and (f_o == O.PDS_INET_DROPPED).sum() > 0
        assert np.array_equal(f, f_o) and np.array_equal(d, d_o)
        assert np.array_equal(rng_d.reshape(-1), np.asarray(rng_o, np.uint64).reshape(-1))


def test_gpu_closing_the_plan_closes_its_sendbatch():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan, SendBatch

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    sb = SendBatch(p, 2, 4)
    try:
        p.close()
        closed = not sb._h
    finally:
        sb.close()
        p.close()
    assert closed
