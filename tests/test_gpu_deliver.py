"""Interface receive stage on the device (srt_deliver over a plan): the
scenarios bit-equal to the host-only form and to the model with the host count
on and across a wave, the hand-made edge cases (the probe chain that wraps the
table's end among them), the chain srt_flight_pop -> srt_inbound_run ->
srt_deliver_run with n_pkts = out_cap and no host synchronisation between the
three calls, and the plan closing its instance."""
import numpy as np
import pytest

import deliver_model as DM
import deliver_scenario as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plan():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    yield p
    p.close()


@pytest.mark.parametrize("shape", [D.DENSE, D.SPARSE])
@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 130])
def test_gpu_equals_host_only_and_model(plan, n_hosts, shape):
    """dense: 0 to 200 packets a host and window, a wave a host (segments over 64 loop), some hosts
    empty; sparse: about one packet a host, eight hosts a wave.  Seven inbound calls with late lists,
    CoDel drops, associations added and removed between them."""
    mo = D.model_scenario(n_hosts, shape)
    outs = D.run_scenario(plan, n_hosts, shape)
    h_outs = D.run_scenario(None, n_hosts, shape)
    assert sum(m["n_delivered"] for m in mo) > 0
    for k, (o, h, m) in enumerate(zip(outs, h_outs, mo)):
        D.assert_same(o, m, (k, "model"))
        D.assert_same(o, h, (k, "host-only"))


@pytest.mark.parametrize("case", D.CASES, ids=[c.__name__[5:] for c in D.CASES])
def test_gpu_hand_made(plan, case):
    case(lambda *a: D.Runner(plan, *a))


def test_gpu_error_paths(plan):
    D.error_paths(plan.handle)


def test_gpu_pop_inbound_deliver_chain(plan):
    """130 hosts, three rounds of 3,000 packets pushed into srt_flight with their metas noted; each
    window is srt_flight_pop -> srt_inbound_run -> srt_deliver_run on device arrays handed on as they
    are, n_pkts = out_cap, no status call and no read-back between the three.  The delivery lists
    equal the model fed from the same calls' (read back afterwards) inbound results."""
    import torch

    from shadow_amd.plan import INBOUND_LATE_DTYPE, DeliverStage, FlightStore, InboundRouter

    n_hosts, n_pkts, n_rounds = 130, 3000, 3
    rng = np.random.default_rng(17)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    bw = np.where(np.arange(n_hosts) % 3 == 0, 200_000, 125_000_000).astype(np.uint64)
    out_cap = late_cap = n_rounds * n_pkts
    fs, ib = FlightStore(plan, n_hosts, out_cap), InboundRouter(plan, bw, 1024)
    ds = DeliverStage(plan, n_hosts, 8, n_rounds * n_pkts, (n_rounds + 2) * out_cap)
    m = DM.DeliverModel(n_hosts, n_rounds * n_pkts, (n_rounds + 2) * out_cap)
    taken = set()
    wins = []
    try:
        for k in range(n_rounds + 1):
            new = D.rand_assoc(rng, n_hosts, 2 * n_hosts, taken, 1000 * k)
            ds.associate(new)
            assert m.associate(new)
            if k < n_rounds:
                per = rng.multinomial(n_pkts, np.ones(n_hosts) / n_hosts)
                host_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
                t0 = 1_000_000_000 + k * 10 * D.MS
                deliver = (t0 + 10 * D.MS + rng.integers(0, 64, size=n_pkts) * (20 * D.MS // 64)).astype(np.uint64)
                dst = rng.integers(0, n_hosts, size=n_pkts).astype(np.uint32)
                dst[rng.random(n_pkts) < 0.1] = 3 * rng.integers(0, 5)  # bursts at slow hosts
                eid = (1000 * k + np.arange(n_pkts) - host_ptr[np.repeat(np.arange(n_hosts), per)]).astype(np.uint64)
                meta = D.rand_meta(rng, n_pkts)
                base = fs.push(t(host_ptr, np.int32), torch.full((n_pkts,), 1 << 8, dtype=torch.int32,  # INET_SENT
                                                                 device=dev), t(deliver, np.int64),
                               t(dst, np.int32), t(eid, np.int64), t(rng.integers(40, 1501, size=n_pkts).astype(np.uint32),
                                                                     np.int32))
                ds.note(t(meta.view(np.uint8), np.uint8), base)
                m.note(meta, base)
            until = 1_000_000_000 + (k + 2) * 10 * D.MS if k < n_rounds else 1_000_000_000 + 10_000 * D.MS
            w = dict(order=z(out_cap, torch.int32), dst_ptr=z(n_hosts + 1, torch.int32), deliver=z(out_cap, torch.int64),
                     size=z(out_cap, torch.int32), src=z(out_cap, torch.int32), eid=z(out_cap, torch.int64),
                     tag=z(out_cap, torch.int64), status=z(out_cap, torch.int32), forward=z(out_cap, torch.int64),
                     late=z(late_cap * 24, torch.uint8), late_count=z(1, torch.int32),
                     o_hp=z(n_hosts + 1, torch.int32), o_sock=z(2 * out_cap, torch.int32),
                     o_fw=z(2 * out_cap, torch.int64), o_tag=z(2 * out_cap, torch.int64),
                     o_user=z(2 * out_cap, torch.int32), o_st=z(2 * out_cap, torch.int32))
            fs.pop(until, w["order"], w["dst_ptr"], w["deliver"], w["size"], w["src"], w["eid"], w["tag"])
            w["base"] = ib.run(w["order"], w["dst_ptr"], w["deliver"], w["size"], until, 0, w["status"], w["forward"],
                               w["late"], w["late_count"])
            ds.run(w["dst_ptr"], w["tag"], w["status"], w["forward"], w["base"], w["late"], w["late_count"], w["o_hp"],
                   w["o_sock"], w["o_fw"], w["o_tag"], w["o_user"], w["o_st"])
            wins.append(w)
        f_flags = fs.status()[0]
        i_flags, _ = ib.status()
        d_flags = ds.status()[0]
    finally:
        ds.close()
        fs.close()
        ib.close()
    assert (f_flags, i_flags, d_flags) == (0, 0, 0)
    u4, u8 = (lambda a: a.cpu().numpy().view(np.uint32)), (lambda a: a.cpu().numpy().view(np.uint64))
    n_late = n_del = 0
    m2 = DM.DeliverModel(n_hosts, n_rounds * n_pkts, (n_rounds + 2) * out_cap)
    m2.ring, m2.note_end = m.ring, m.note_end  # every note precedes the tags a later window reads
    taken2 = sorted(m.assoc.items())
    for k, w in enumerate(wins):
        # the associations as they stood at call k: those with sockets below 1000 * (k + 1)
        m2.assoc = {key: s for key, s in taken2 if s < 1000 * (k + 1)}
        c = int(u4(w["late_count"])[0])
        late = w["late"].cpu().numpy().view(INBOUND_LATE_DTYPE)[:c].astype(DM.LATE)
        mo = m2.run(u4(w["dst_ptr"]), out_cap, u8(w["tag"]), u4(w["status"]), u8(w["forward"]), w["base"], late,
                    2 * out_cap)
        n = mo["n_delivered"]
        assert mo["flags"] == 0 and np.array_equal(u4(w["o_hp"]), mo["host_ptr"]), k
        for a, b in (("o_sock", "socket"), ("o_user", "user"), ("o_st", "status")):
            assert np.array_equal(u4(w[a])[:n], mo[b]), (k, a)
        assert np.array_equal(u8(w["o_fw"])[:n], mo["forward"]) and np.array_equal(u8(w["o_tag"])[:n], mo["tag"]), k
        n_late += c
        n_del += n
    assert n_late > 300 and n_del > 5000


def test_gpu_closing_the_plan_closes_its_instance():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import DeliverStage, RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    ds = DeliverStage(p, 2, 8, 4, 4)
    try:
        p.close()
        closed = not ds._h
    finally:
        ds.close()
        p.close()
    assert closed
