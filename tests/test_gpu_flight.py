"""In-flight store on the device (srt_flight over a plan): the scenarios
bit-equal to the host-only form and to the model with the destination count on
and across a wave, the hand-made edge cases, one window against the path the
documentation prescribed before (srt_packet_events over the gathered set), the
chain srt_packet_batch -> srt_packet_events -> srt_flight_push ... srt_flight_pop
-> srt_inbound_run without a host round trip between the pop and the inbound
call, and the plan closing its store."""
import numpy as np
import pytest

import flight_model as FM
import flight_scenario as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plan():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    yield p
    p.close()


@pytest.mark.parametrize("shape", [F.DENSE, F.SPARSE])
@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 130])
def test_gpu_equals_host_only_and_model(plan, n_hosts, shape):
    """dense: 0 to 200 packets a source host, a wave a host (segments over 64 loop), some hosts
    empty; sparse: about one packet a host, eight hosts a wave.  Three pushes, four windows, every
    pop mixes pushes, the last one drains."""
    steps, _ = F.scenario(n_hosts, shape)
    if shape == F.DENSE:
        per_host = np.diff(steps[0][1]["host_ptr"].astype(np.int64))
        assert per_host.max() > 64 and (n_hosts == 1 or (per_host == 0).any())
    mo = F.model_scenario(n_hosts, shape)
    assert mo[-1]["status"][2] == 0
    outs = F.run_scenario(plan, n_hosts, shape)
    h_outs = F.run_scenario(None, n_hosts, shape)
    for k, (o, h, m) in enumerate(zip(outs, h_outs, mo)):
        F.assert_same(o, m, (k, "model"))
        F.assert_same(o, h, (k, "host-only"))


@pytest.mark.parametrize("case", F.CASES, ids=[c.__name__[5:] for c in F.CASES])
def test_gpu_hand_made(plan, case):
    case(lambda n_dst, pool_cap: F.Runner(plan, n_dst, pool_cap))


def test_gpu_error_paths(plan):
    F.error_paths(plan.handle)


def test_gpu_window_equals_packet_events_over_the_gathered_set(plan):
    """The joining as the documentation prescribed it before: the window's set gathered on the host,
    grouped by source host in send order, ordered by a second srt_packet_events call over a scratch
    event_base.  Its dst_ptr and the (deliver, source host, event id) sequence of every group equal
    the pop's."""
    import torch

    n_hosts = 130
    steps, total = F.scenario(n_hosts, F.DENSE)
    r = F.Runner(plan, n_hosts, total)
    try:
        for kind, arg in steps[:4]:  # two pushes, a pop, a push
            if kind == "push":
                r.push(*[arg[k] for k in F.PUSH_KEYS])
            else:
                r.pop(arg, total)
        # what the store holds now, from the model, and the window the next pop must give
        m = FM.FlightModel(n_hosts, total)
        for kind, arg in steps[:4]:
            m.push(*[arg[k] for k in F.PUSH_KEYS]) if kind == "push" else m.pop(arg, total)
        until = steps[4][1]
        due = m.recs[m.recs["deliver"] < np.uint64(until)]
        out = r.pop(until, total)
    finally:
        r.close()
    assert out["status"][0] == 0 and out["status"][1] == len(due) > 1000
    # send order within a source host is event-id order
    g = due[np.lexsort((due["event_id"], due["src"]))]
    host_ptr = np.searchsorted(g["src"], np.arange(n_hosts + 1)).astype(np.int32)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    n = len(g)
    t_f = torch.full((n,), FM.SENT, dtype=torch.int32, device=dev)
    t_d = t(g["deliver"], np.int64)
    t_base = torch.zeros(n_hosts, dtype=torch.int64, device=dev)  # scratch: the ids it hands out are not used
    t_eid = torch.zeros(n, dtype=torch.int64, device=dev)
    t_ord = torch.zeros(n, dtype=torch.int32, device=dev)
    t_ptr = torch.zeros(n_hosts + 1, dtype=torch.int32, device=dev)
    plan.packet_events(t(host_ptr, np.int32), t_f, t_d, t(g["dst"], np.int32), n_hosts, t_base, t_eid, t_ord, t_ptr)
    order = t_ord.cpu().numpy()
    assert np.array_equal(t_ptr.cpu().numpy().view(np.uint32), out["dst_ptr"])
    assert np.array_equal(g["deliver"][order], out["deliver"])
    assert np.array_equal(g["src"][order], out["src"])
    assert np.array_equal(g["event_id"][order], out["event_id"])
    assert np.array_equal(g["tag"][order], out["tag"]) and np.array_equal(g["size"][order], out["size"])


def test_gpu_batch_events_flight_inbound_chain():
    """A 50-node plan, 130 hosts, three rounds of 2,000 packets: srt_packet_batch, srt_packet_events,
    srt_flight_push each round; srt_flight_pop -> srt_inbound_run once per window (the round that
    follows each push, then one window that drains) on device arrays handed on as they are, with
    n_pkts = out_cap and no status call between the two.  Statuses, forward times, late lists and
    the hosts' final states equal a host-only srt_inbound fed from the MODEL's windows; no call
    raises AFTER_UNTIL or TIME_REGRESSION."""
    import torch

    from oracle import oracle as O
    from shadow_amd import NetworkGraph, _lib, synth
    from shadow_amd.plan import INBOUND_LATE_DTYPE, FlightStore, InboundRouter, RoutingPlan

    n_nodes, n_hosts, n_pkts, seed = 50, 130, 2000, 5
    round_ns = 2 * synth.MS
    src, dst, lat, loss = synth.complete_graph(n_nodes, seed, lat_ms=(1, 14), loss_max=0.25)
    rp = RoutingPlan(NetworkGraph.from_edges(n_nodes, src, dst, lat, loss), np.arange(n_nodes, dtype=np.uint32)).run()
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    bw = np.where(np.arange(n_hosts) % 3 == 0, 125_000, 125_000_000).astype(np.uint64)
    out_cap, late_cap = 3 * n_pkts, 3 * n_pkts
    t_rng = t(synth.host_rng_states(n_hosts, 1), np.int64)
    t_base = z(n_hosts, torch.int64)
    starts = [1_000_000_000 + k * round_ns for k in range(3)]
    untils = [s + 2 * round_ns for s in starts] + [starts[2] + 100 * round_ns]
    fs, ib = FlightStore(rp, n_hosts, 3 * n_pkts), InboundRouter(rp, bw, 256)
    rounds, wins, bases = [], [], []
    try:
        for k in range(4):
            if k < 3:
                pk, host_ptr, _ = synth.packet_round(n_hosts, n_nodes, n_pkts, seed + k, starts[k], starts[k] + round_ns)
                dst_host = ((pk["dst_row"].astype(np.uint32) + n_nodes * (np.arange(n_pkts) % 4)) % n_hosts
                            ).astype(np.uint32)
                size = (pk["payload_size"] + 40).astype(np.uint32)
                t_hp, t_f, t_d, t_eid = t(host_ptr, np.int32), z(n_pkts, torch.int32), z(n_pkts, torch.int64), z(
                    n_pkts, torch.int64)
                t_ord, t_ptr = z(n_pkts, torch.int32), z(n_hosts + 1, torch.int32)
                rp.packet_batch(t(pk.view(np.uint8), np.uint8), t_hp, t_rng, starts[k] + round_ns, 0, 2**62, t_f, t_d,
                                sync=False)
                rp.packet_events(t_hp, t_f, t_d, t(dst_host, np.int32), n_hosts, t_base, t_eid, t_ord, t_ptr,
                                 check=False)
                fs.push(t_hp, t_f, t_d, t(dst_host, np.int32), t_eid, t(size, np.int32))
                rounds.append((host_ptr, t_f, t_d, dst_host, t_eid, size))
            w = dict(order=z(out_cap, torch.int32), dst_ptr=z(n_hosts + 1, torch.int32), deliver=z(out_cap, torch.int64),
                     size=z(out_cap, torch.int32), src=z(out_cap, torch.int32), eid=z(out_cap, torch.int64),
                     tag=z(out_cap, torch.int64), status=z(out_cap, torch.int32), forward=z(out_cap, torch.int64),
                     late=z(late_cap * 24, torch.uint8), late_count=z(1, torch.int32))
            fs.pop(untils[k], w["order"], w["dst_ptr"], w["deliver"], w["size"], w["src"], w["eid"], w["tag"])
            bases.append(ib.run(w["order"], w["dst_ptr"], w["deliver"], w["size"], untils[k], 0, w["status"],
                                w["forward"], w["late"], w["late_count"]))
            wins.append(w)
        f_flags, _, f_stored, f_lost = fs.status()
        i_flags, i_pending = ib.status()
        i_state = ib.state()
        rp.packet_events_status()
    finally:
        fs.close()
        ib.close()
        rp.close()
    assert (f_flags, f_stored, f_lost) == (0, 0, 0) and i_flags == 0
    # ---- the model's windows from the rounds' device results, into a host-only srt_inbound
    m = FM.FlightModel(n_hosts, 3 * n_pkts)
    hb = InboundRouter(None, bw, 256)
    u4, u8 = (lambda a: a.cpu().numpy().view(np.uint32)), (lambda a: a.cpu().numpy().view(np.uint64))
    n_late = n_drop = 0
    try:
        for k in range(4):
            if k < 3:
                host_ptr, t_f, t_d, dst_host, t_eid, size = rounds[k]
                assert (u4(t_f) == O.PDS_INET_SENT).sum() > 1000 and (u4(t_f) == O.PDS_INET_DROPPED).sum() > 100
                m.push(host_ptr, u4(t_f), u8(t_d), dst_host, u8(t_eid), size)
            mo = m.pop(untils[k], out_cap)
            n = len(mo["tag"])
            stored = m.status()
            assert stored[0] == 0 and n > 300 and (k == 3 or stored[2] > 300)
            w = wins[k]
            assert np.array_equal(u4(w["dst_ptr"]), mo["dst_ptr"]) and np.array_equal(u4(w["order"])[:n], mo["order"])
            for a, b in (("deliver", "deliver"), ("eid", "event_id"), ("tag", "tag")):
                assert np.array_equal(u8(w[a])[:n], mo[b]), (k, a)
            assert np.array_equal(u4(w["size"])[:n], mo["size"]) and np.array_equal(u4(w["src"])[:n], mo["src"])
            pad = lambda a: np.concatenate([a, np.zeros(out_cap - n, a.dtype)])  # noqa: E731
            st, fw = np.zeros(out_cap, np.uint32), np.zeros(out_cap, np.uint64)
            late, cnt = np.zeros(late_cap * 24, np.uint8), np.zeros(1, np.uint32)
            base = hb.run(pad(mo["order"]), mo["dst_ptr"], pad(mo["deliver"]), pad(mo["size"]), untils[k], 0, st, fw,
                          late, cnt)
            assert base == bases[k] == k * out_cap
            assert np.array_equal(u4(w["status"]), st) and np.array_equal(u8(w["forward"]), fw), k
            c = int(cnt[0])
            assert int(u4(w["late_count"])[0]) == c
            key = lambda a: np.sort(a.view(INBOUND_LATE_DTYPE)[:c], order=["seq"]).tobytes()  # noqa: E731
            assert key(w["late"].cpu().numpy()) == key(late), k
            n_late += c
            n_drop += int(((st & _lib.PDS_ROUTER_DROPPED) != 0).sum()) + int(
                ((late.view(INBOUND_LATE_DTYPE)[:c]["status"] & _lib.PDS_ROUTER_DROPPED) != 0).sum())
        assert hb.status() == (0, i_pending)
        assert hb.state().tobytes() == i_state.tobytes()
    finally:
        hb.close()
    # packets that left in a later call than they came in, CoDel drops, every window a mix of rounds
    assert n_late > 1000 and n_drop > 10 and len(m.recs) == 0


def test_gpu_closing_the_plan_closes_its_store():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import FlightStore, RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    fs = FlightStore(p, 2, 4)
    try:
        p.close()
        closed = not fs._h
    finally:
        fs.close()
        p.close()
    assert closed
