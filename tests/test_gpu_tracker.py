"""Tracker stage on the device (srt_tracker over a plan): the seven-window
scenarios bit-equal to the host-only form and to the model with the host count
on and across a wave (the output side through srt_outbound_run ->
srt_outbound_cached_seq -> srt_tracker_tx on device arrays), the hand-made cases
(the pop-time rule, one packet a class, the 64-bit carry, the socket slots, the
flags), the chain srt_deliver_run -> srt_tracker_rx with out_cap past the
delivered count and no host synchronisation between the two, and the plan
closing its instance."""
import numpy as np
import pytest

import deliver_model as DM
import deliver_scenario as D
import tracker_model as TM
import tracker_scenario as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plan():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    yield p
    p.close()


@pytest.mark.parametrize("shape", [T.DENSE, T.SPARSE])
@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 130])
def test_gpu_equals_host_only_and_model(plan, n_hosts, shape):
    """dense: 0 to 200 packets a host and window, a wave a host (segments over 64 loop), some hosts
    empty; sparse: about one packet a host, eight hosts a wave.  Seven windows of outbound -> tracker tx
    and deliver list -> tracker rx, throttled hosts (late lists, packets cached across a call boundary),
    a heartbeat after windows 3 and 7 on a subset of hosts and slots, then on all."""
    if n_hosts >= 63:
        T.assert_scenario_is_not_empty(n_hosts, shape)
    m_beats, m_st, _ = T.model_scenario(n_hosts, shape)
    beats, st = T.run_scenario(plan, n_hosts, shape)
    h_beats, h_st = T.run_scenario(None, n_hosts, shape)
    assert st == h_st == m_st and len(beats) == len(h_beats) == len(m_beats) == 4
    for k, (a, h, m) in enumerate(zip(beats, h_beats, m_beats)):
        T.same_records(a, m, (k, "model"))
        T.same_records(a, h, (k, "host-only"))


@pytest.mark.parametrize("case", T.CASES, ids=[c.__name__[5:] for c in T.CASES])
def test_gpu_hand_made(plan, case):
    case(lambda *a: T.Runner(plan, *a))


def test_gpu_error_paths(plan):
    T.error_paths(plan.handle)


def test_gpu_deliver_then_tracker_without_a_sync(plan):
    """130 hosts: the deliver scenario's windows through srt_deliver_run on the device, each list handed to
    srt_tracker_rx as it is -- out_cap the arrays' capacity, far past the delivered count, the arrays
    behind the list filled with records that would count -- with no status call and no read-back
    between the two.  The records equal the model's, fed the deliver model's lists."""
    import torch

    from shadow_amd import Tracker
    from shadow_amd.plan import DeliverStage

    n_hosts, shape = 130, D.DENSE
    sc, lists = D.scenario(n_hosts, shape), D.model_scenario(n_hosts, shape)
    rng = np.random.default_rng(4)
    metas = T.rand_meta(rng, sc["total"])
    n_sockets = 12 * n_hosts
    out_cap = 2 * (sc["cap"] + sc["late_cap"]) + 777
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    ds = DeliverStage(plan, n_hosts, 8, sc["total"], (D.N_WIN + 1) * sc["cap"])
    trk = Tracker(plan, n_hosts, n_sockets, sc["total"], 0)
    m = TM.TrackerModel(n_hosts, n_sockets, sc["total"], 0)
    k = 0
    try:
        for st in sc["steps"]:
            if st[0] == "assoc":
                ds.associate(st[1])
            elif st[0] == "disassoc":
                ds.disassociate(st[1])
            elif st[0] == "note":
                ds.note(t(st[1].view(np.uint8), np.uint8), st[2])
                part = metas[st[2]:st[2] + len(st[1])]
                trk.note(t(part.view(np.uint8), np.uint8), st[2])
                m.note(part, st[2])
            else:
                a = st[1]
                late = np.zeros(sc["late_cap"], DM.LATE)
                late[:len(a["late"])] = a["late"]
                o_hp = torch.zeros(n_hosts + 1, dtype=torch.int32, device=dev)
                o_sock = torch.zeros(out_cap, dtype=torch.int32, device=dev)  # socket 0, tag 0, a hit: would count
                o_tag = torch.zeros(out_cap, dtype=torch.int64, device=dev)
                o_st = torch.full((out_cap,), T.RX_HIT, dtype=torch.int32, device=dev)
                o_fw = torch.zeros(out_cap, dtype=torch.int64, device=dev)
                o_user = torch.zeros(out_cap, dtype=torch.int32, device=dev)
                ds.run(t(a["dst_ptr"], np.int32), t(a["tag"], np.int64), t(a["status"], np.int32),
                       t(a["forward"], np.int64), a["seq_base"], t(late.view(np.uint8), np.uint8),
                       t(np.array([len(a["late"])], np.uint32), np.int32), o_hp, o_sock, o_fw, o_tag, o_user, o_st)
                trk.rx(o_hp, o_sock, o_tag, o_st)
                mo = lists[k]
                m.rx(mo["host_ptr"], mo["socket"], mo["tag"], mo["status"])
                k += 1
        got = trk.heartbeat()
        flags = trk.status()
        d_flags = ds.status()[0]
    finally:
        trk.close()
        ds.close()
    want = m.heartbeat()
    assert k == 7 and d_flags == 0 and flags == m.status() and flags[0] == 0 and flags[2] > 5000
    T.same_records(got, want)
    assert all(int(want[0][f].sum()) > 0 for f in TM.FIELDS)


def test_gpu_closing_the_plan_closes_its_instance():
    from shadow_amd import NetworkGraph, Tracker, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    trk = Tracker(p, 2, 2, 4, 4)
    try:
        p.close()
        closed = not trk._h
    finally:
        trk.close()
        p.close()
    assert closed
