"""pcap capture stage on the device (srt_pcap over a plan): the multi-call
scenarios byte-equal to the host-only form and to the model with the host count
on and across a wave, at several capture lengths and both tie rules; the
hand-made flag cases; the write pass at its tile edges (T =
srt_pcap_tile_bytes(): totals around T, records that start and end next to a
tile boundary, a full segment across the boundary at every alignment, d_out
misaligned, only the last host capturing, empty lists), the buffer behind the
total still poisoned after each; the error paths on a plan; the chain
srt_deliver_run -> srt_pcap_run through the index array with no host
synchronisation between the two; and the plan closing its instance."""
import numpy as np
import pytest

import deliver_model as DM
import deliver_scenario as D
import pcap_model as PM
import pcap_scenario as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plan():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    yield p
    p.close()


@pytest.mark.parametrize("shape", [P.DENSE, P.SPARSE])
@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 130])
def test_gpu_equals_host_only_and_model(plan, n_hosts, shape):
    """dense: a wave a host, segments over 64 loop, some hosts empty; sparse: eight hosts a wave.  Three
    calls in a row on one instance; d_out misaligned by 5 bytes."""
    if n_hosts >= 63:
        P.assert_scenario_is_not_empty(n_hosts, shape)
    want, w_st = P.model_scenario(n_hosts, shape, 65535)
    got, st = P.run_scenario(plan, n_hosts, shape, 65535, misalign=5)
    host, h_st = P.run_scenario(None, n_hosts, shape, 65535, misalign=5)
    P.same_outputs(got, want, "model")
    P.same_outputs(got, host, "host-only")
    assert st == h_st == w_st and st[0] == 0


@pytest.mark.parametrize("capture_len", [0, 19, 28, 43, 64, 100])
def test_gpu_capture_lengths_and_tie_rules(plan, capture_len):
    for n_hosts, shape, tx_first in ((65, P.SPARSE, False), (64, P.DENSE, True)):
        want, w_st = P.model_scenario(n_hosts, shape, capture_len, tx_first)
        got, st = P.run_scenario(plan, n_hosts, shape, capture_len, tx_first)
        P.same_outputs(got, want, (n_hosts, shape))
        assert st == w_st and st[0] == 0


@pytest.mark.parametrize("case", P.CASES, ids=[c.__name__[5:] for c in P.CASES])
def test_gpu_hand_made(plan, case):
    case(lambda *a: P.Runner(plan, *a))


@pytest.mark.parametrize("case", P.EDGES, ids=[c.__name__[5:] for c in P.EDGES])
def test_gpu_tile_edges(plan, case):
    case(lambda *a: P.Runner(plan, *a))


def test_gpu_error_paths(plan):
    P.error_paths(plan.handle)


def test_gpu_outbound_and_deliver_feed_pcap_without_a_sync(plan):
    """65 hosts.  Sent side: one srt_outbound_run window; its send times become the records' times with one
    device copy and outbound_send_order's permutation is the index array.  Received side: the deliver
    scenario's seven windows through srt_deliver_run, each list handed to srt_pcap_run as it is -- the
    records are indexed by flight tag, the receive times scattered into them on the device, n_rx the
    arrays' capacity, far past the delivered count.  No status call and no read-back between the stages;
    everything is read back after the last call and compared with the model, fed the deliver model's lists
    and a numpy restatement of the send order."""
    import torch

    from shadow_amd import PcapCapture, _lib
    from shadow_amd.plan import OUT_PKT_DTYPE, DeliverStage, OutboundRelay, outbound_send_order

    n_hosts, shape, capture_len = 65, D.DENSE, 200
    sc, lists = D.scenario(n_hosts, shape), D.model_scenario(n_hosts, shape)
    rng = np.random.default_rng(9)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
    payload = rng.integers(0, 256, P.POOL).astype(np.uint8)
    total, out_cap = sc["total"], 2 * (sc["cap"] + sc["late_cap"]) + 777
    # the sent side: 1,000 packets in the first window, hosts at 300 kB/s, so not all are sent by its end
    n_tx = 1000
    h = np.sort(rng.integers(0, n_hosts, n_tx))
    tx_ptr = np.searchsorted(h, np.arange(n_hosts + 1)).astype(np.int32)
    tx_recs = P.rand_recs(rng, np.zeros(n_tx, np.uint64))
    ready = rng.integers(0, D.W_NS // 2, n_tx)
    pk = np.zeros(n_tx, OUT_PKT_DTYPE)
    pk["ready_ns"] = ready[np.lexsort((ready, h))]
    pk["priority"] = np.arange(n_tx)
    pk["total_size"] = 44 + tx_recs["payload_len"].astype(np.uint32)
    pk["socket"] = rng.integers(0, 2, n_tx)
    # the received side: a record a flight tag, one more that takes the writes of the unused entries
    rx_recs = P.rand_recs(rng, np.zeros(total + 1, np.uint64))
    ob = OutboundRelay(plan, np.full(n_hosts, 300_000, np.uint64), _lib.QDISC_FIFO, 2, 256)
    ds = DeliverStage(plan, n_hosts, 8, total, (D.N_WIN + 1) * sc["cap"])
    pc = PcapCapture(plan, n_hosts, capture_len, n_tx + out_cap)
    outs, k = [], 0
    try:
        d_tx, d_rx, d_pay = t(tx_recs.view(np.uint8), np.uint8), t(rx_recs.view(np.uint8), np.uint8), t(payload, np.uint8)
        d_tx_ptr, o_st, o_sn, o_rk = t(tx_ptr, np.int32), z(n_tx, torch.int32), z(n_tx, torch.int64), z(n_tx, torch.int64)
        ob.run(t(pk.view(np.uint8), np.uint8), d_tx_ptr, D.W_NS, 0, o_st, o_sn, o_rk, z(32 * n_tx, torch.uint8),
               z(1, torch.int32))
        d_tx.view(torch.int64).view(-1, 6)[:, 0] = o_sn  # a packet not sent keeps UINT64_MAX and is in no list
        order, send_ptr = outbound_send_order(d_tx_ptr, o_rk)
        tx_idx = order.to(torch.int32)
        no_tx = z(n_hosts + 1, torch.int32)
        for st in sc["steps"]:
            if st[0] == "assoc":
                ds.associate(st[1])
            elif st[0] == "disassoc":
                ds.disassociate(st[1])
            elif st[0] == "note":
                ds.note(t(st[1].view(np.uint8), np.uint8), st[2])
            else:
                a = st[1]
                late = np.zeros(sc["late_cap"], DM.LATE)
                late[:len(a["late"])] = a["late"]
                o_hp = z(n_hosts + 1, torch.int32)
                o_sock, o_user, o_stat = (z(out_cap, torch.int32) for _ in range(3))
                o_fw, o_tag = z(out_cap, torch.int64), z(out_cap, torch.int64)  # tag 0, time 0: would be written
                ds.run(t(a["dst_ptr"], np.int32), t(a["tag"], np.int64), t(a["status"], np.int32),
                       t(a["forward"], np.int64), a["seq_base"], t(late.view(np.uint8), np.uint8),
                       t(np.array([len(a["late"])], np.uint32), np.int32), o_hp, o_sock, o_fw, o_tag, o_user, o_stat)
                used = torch.arange(out_cap, device=dev) < o_hp[n_hosts]
                rx_idx = torch.where(used, o_tag, torch.full_like(o_tag, total))
                d_rx.view(torch.int64).view(-1, 6)[:, 0].index_copy_(0, rx_idx, o_fw)
                out = torch.full((1 << 22,), P.POISON, dtype=torch.uint8, device=dev)
                ho = z(n_hosts + 1, torch.int64)
                if k == 0:
                    pc.run(d_tx, send_ptr, d_rx, o_hp, d_pay, out, ho, tx_idx=tx_idx, rx_idx=rx_idx.to(torch.int32))
                else:
                    pc.run(None, no_tx, d_rx, o_hp, d_pay, out, ho, rx_idx=rx_idx.to(torch.int32))
                outs.append((ho, out))
                k += 1
        status = pc.status(check=False)
        d_flags = ds.status()[0]
        o_flags = ob.status()[0]
        send_ns, send_rank = o_sn.cpu().numpy().view(np.uint64), o_rk.cpu().numpy().view(np.uint64)
        outs = [(ho.cpu().numpy().view(np.uint64), out.cpu().numpy()) for ho, out in outs]
    finally:
        pc.close()
        ds.close()
        ob.close()
    assert k == 7 and d_flags == 0 and o_flags == 0
    # the send order restated: the packets with a rank, a host's by rank
    host_of = np.repeat(np.arange(n_hosts), np.diff(tx_ptr))
    sent = np.nonzero(send_rank != np.uint64(DM.NONE64))[0]
    sent = sent[np.lexsort((send_rank[sent], host_of[sent]))]
    assert len(sent) > 100
    tx_list = tx_recs[sent].copy()
    tx_list["time_ns"] = send_ns[sent]
    m_tx_ptr = np.searchsorted(host_of[sent], np.arange(n_hosts + 1))
    m = PM.PcapModel(n_hosts, capture_len)
    for j, ((ho, out), mo) in enumerate(zip(outs, lists)):
        rx_list = rx_recs[mo["tag"].astype(np.int64)].copy()
        rx_list["time_ns"] = mo["forward"]
        first = j == 0
        w_off, want = m.run(tx_list if first else None, m_tx_ptr if first else np.zeros(n_hosts + 1, np.int64),
                            rx_list, mo["host_ptr"], payload, 1 << 22)
        assert np.array_equal(ho, w_off), j
        n = int(w_off[-1])
        assert n > 100000 and out[:n].tobytes() == want and (out[n:] == P.POISON).all(), j
    assert status == m.status() and status[1] > 20000


def test_gpu_closing_the_plan_closes_its_instance():
    from shadow_amd import NetworkGraph, PcapCapture, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    pc = PcapCapture(p, 2, 64, 4)
    try:
        p.close()
        closed = not pc._h
    finally:
        pc.close()
        p.close()
    assert closed
