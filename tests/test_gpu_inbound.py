"""Inbound router stage on the device (srt_inbound over a plan): the CPU
tests' scenario bit-equal to the model and to the host-only form, a real
packet_batch -> packet_events -> inbound round against oracle + model, the
control law's f64 path against the host's, and ring overflow reported without
a fault."""
import numpy as np
import pytest

import inbound_model as M
import inbound_scenario as S
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


@pytest.mark.parametrize("split", [False, True])
def test_gpu_inbound_equals_model(plan, split):
    calls, mouts, m = S.model_results(split=split)
    outs, state, stats = S.run_lib(S.scenario(), calls, plan=plan)
    S.assert_same(outs, mouts, state, m)
    assert stats[-1] == (0, m.pending())


@pytest.mark.parametrize("split", [False, True])
def test_gpu_inbound_equals_host_only(plan, split):
    sc = S.scenario()
    calls = S.split_calls(sc) if split else S.one_call(sc)
    d_outs, d_state, d_stats = S.run_lib(sc, calls, plan=plan)
    h_outs, h_state, h_stats = S.run_lib(sc, calls)
    assert d_stats == h_stats
    for d, h in zip(d_outs, h_outs):
        assert d["base"] == h["base"] and d["late"] == h["late"] and d["late_count"] == h["late_count"]
        assert np.array_equal(d["status"], h["status"]) and np.array_equal(d["forward"], h["forward"])
    assert d_state.tobytes() == h_state.tobytes()


def test_gpu_inbound_wave_wider_than_the_lds_window(plan):
    """A wave whose 64 hosts receive more records than its LDS window holds
    (8,192) walks them from HBM; the remainder wave beside it from LDS.  Two
    calls, so both forms also take packets back out of the ring."""
    n_hosts, n_pkts = 70, 10_000
    rng = np.random.default_rng(11)
    sc = dict(bw=rng.choice(np.array([60_000, 125_000_000], np.uint64), size=n_hosts),
              dst=rng.integers(0, n_hosts, size=n_pkts).astype(np.uint32),
              deliver=(rng.integers(0, 1000, size=n_pkts) * M.MS + rng.integers(0, 2, size=n_pkts) * 1234
                       ).astype(np.uint64),
              size=rng.integers(40, 1501, size=n_pkts).astype(np.uint32), sent=rng.random(n_pkts) < 0.97)
    calls = S.calls_of(sc, [1001 * M.MS, 1100 * M.MS], n_hosts)
    assert calls[0]["dst_ptr"][64] > 8192 and len(calls[0]["ids"]) == n_pkts
    mouts, m = S.run_model(sc, calls)
    assert len(mouts[1]["late"]) > 100 and m.pending() > 0
    outs, state, stats = S.run_lib(sc, calls, plan=plan, queue_cap=512)
    S.assert_same(outs, mouts, state, m)
    assert stats[-1] == (0, m.pending())


def test_gpu_inbound_after_packet_round(plan):
    """batch -> events -> inbound on a small plan: flags and deliver times of a
    real srt_packet_batch round, srt_packet_events' order, then the inbound
    call, against the oracle's event order fed to the model."""
    import torch

    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import InboundRouter, RoutingPlan

    n_nodes, n_hosts, n_pkts = 50, 200, 20_000
    src, dst, lat, loss = synth.complete_graph(n_nodes, 5, loss_max=0.25)
    rp = RoutingPlan(NetworkGraph.from_edges(n_nodes, src, dst, lat, loss), np.arange(n_nodes, dtype=np.uint32)).run()
    r0, r1 = 1_000_000_000, 1_000_000_000 + 5 * synth.MS
    pk, host_ptr, _ = synth.packet_round(n_hosts, n_nodes, n_pkts, 5, r0, r1)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    t_hp = t(host_ptr, np.int32)
    t_f = torch.zeros(n_pkts, dtype=torch.int32, device=dev)
    t_d = torch.zeros(n_pkts, dtype=torch.int64, device=dev)
    rp.packet_batch(t(pk.view(np.uint8), np.uint8), t_hp, t(synth.host_rng_states(n_hosts, 1), np.int64), r1, 0, 2**62,
                    t_f, t_d)
    dst_host = ((pk.view(O.PKT_DTYPE)["dst_row"].astype(np.uint32) + n_nodes * (np.arange(n_pkts) % 4)) % n_hosts
                ).astype(np.uint32)
    t_base = torch.zeros(n_hosts, dtype=torch.int64, device=dev)
    t_eid = torch.zeros(n_pkts, dtype=torch.int64, device=dev)
    t_ord = torch.zeros(n_pkts, dtype=torch.int32, device=dev)
    t_ptr = torch.zeros(n_hosts + 1, dtype=torch.int32, device=dev)
    rp.packet_events(t_hp, t_f, t_d, t(dst_host, np.int32), n_hosts, t_base, t_eid, t_ord, t_ptr)
    # payload plus TCP/IP headers, as the caller knows them
    size = (pk["payload_size"] + 40).astype(np.uint32)
    bw = np.where(np.arange(n_hosts) % 3 == 0, 125_000_000, 125_000).astype(np.uint64)
    f = t_f.cpu().numpy().view(np.uint32)
    d = t_d.cpu().numpy().view(np.uint64)
    # the window ends just past the batch's last arrival (paths here reach 300 ms)
    until = int(d[f == O.PDS_INET_SENT].max()) + 1
    t_st = torch.zeros(n_pkts, dtype=torch.int32, device=dev)
    t_fw = torch.zeros(n_pkts, dtype=torch.int64, device=dev)
    t_cnt = torch.ones(1, dtype=torch.int32, device=dev)
    ib = InboundRouter(rp, bw, 256)
    try:
        base = ib.run(t_ord, t_ptr, t_d, t(size, np.int32), until, 0, t_st, t_fw, None, t_cnt)
        flags, pending = ib.status()
        state = ib.state()
    finally:
        ib.close()
        rp.close()
    # oracle + model
    _, ord_o, ptr_o = O.packet_events(host_ptr, f, d, dst_host, n_hosts, np.zeros(n_hosts, np.uint64))
    m = M.InboundModel(bw)
    st_m, fw_m, late_m, base_m = m.run(ord_o, ptr_o, d, size, until, 0)
    assert m.not_taken == 0
    assert base == base_m == 0 and late_m == [] and int(t_cnt.item()) == 0 and flags == 0
    assert np.array_equal(t_st.cpu().numpy().view(np.uint32), st_m)
    assert np.array_equal(t_fw.cpu().numpy().view(np.uint64), fw_m)
    assert ((st_m & M.DROPPED) != 0).sum() > 0 and ((st_m & M.CACHED) != 0).sum() > 0 and pending == m.pending() > 0
    for h, ms in enumerate(m.state()):
        for k in S.STATE_FIELDS:
            assert int(state[k][h]) == ms[k], (h, k)
    # every scheduled forward task took one of the host's event ids
    assert int(state["tasks_scheduled"].sum()) == sum(x.tasks for x in m.hosts) > 0


def test_gpu_control_law_equals_host(plan):
    """round(1e8 / sqrt(count)) in f64: the device's sqrt and divide against
    the host's IEEE evaluation, and the table path against both."""
    from shadow_amd.plan import InboundRouter

    p2 = 2 ** np.arange(0, 41, dtype=np.uint64)
    counts = np.concatenate([np.arange(0, 70_001, dtype=np.uint64), p2, p2 + np.uint64(1), p2 - np.uint64(1)])
    dev, host = InboundRouter(plan, [1000], 4), InboundRouter(None, [1000], 4)
    try:
        want = host.control_law(counts, use_table=False)
        got = dev.control_law(counts, use_table=False)
        got_tab, want_tab = dev.control_law(counts, use_table=True), host.control_law(counts, use_table=True)
    finally:
        dev.close()
        host.close()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (counts[bad][:10], got[bad][:10], want[bad][:10])
    assert np.array_equal(got_tab, want) and np.array_equal(want_tab, want)


def test_gpu_ring_overflow_reported_not_faulted(plan):
    """queue_cap 4: the capacity check precedes every ring write; the hosts
    that overflow are marked and every other host's results stand"""
    from shadow_amd import _lib

    sc = S.scenario()
    calls, mouts, m = S.model_results(split=True)
    outs, state, stats = S.run_lib(sc, calls, plan=plan, queue_cap=4, check=False)
    assert any(f & _lib.INBOUND_RING_OVERFLOW for f, _ in stats)
    over = set(np.nonzero(state["overflow"])[0].tolist())
    assert any(sc["bw"][h] == 1_000 for h in over)
    good = set(range(S.N_HOSTS)) - over
    S.assert_same(outs, mouts, state, m, hosts=good)
    for c, o, mo in zip(calls, outs, mouts):
        keep = np.isin(sc["dst"][c["ids"]], sorted(good))
        assert np.array_equal(o["status"][keep], mo["status"][keep])
        assert np.array_equal(o["forward"][keep], mo["forward"][keep])
    h_outs, h_state, _ = S.run_lib(sc, calls, queue_cap=4, check=False)
    assert np.array_equal(h_state["overflow"], state["overflow"])


def test_gpu_arrivals_at_or_after_until_are_flagged(plan):
    """the window rule on the device: arrivals at 5, 6, 7 ms, until 6 ms"""
    import torch

    from shadow_amd import _lib
    from shadow_amd.plan import InboundRouter

    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)  # noqa: E731
    ib = InboundRouter(plan, [125_000_000], 8)
    st, fw = t([7, 7, 7], torch.int32), t([0, 0, 0], torch.int64)
    try:
        ib.run(t([0, 1, 2], torch.int32), t([0, 3], torch.int32), t([5 * M.MS, 6 * M.MS, 7 * M.MS], torch.int64),
               t([100, 100, 100], torch.int32), 6 * M.MS, 0, st, fw)
        first, second = ib.status(check=False), ib.status()
    finally:
        ib.close()
    assert first == (_lib.INBOUND_AFTER_UNTIL, 0) and second == (0, 0)
    assert st.tolist() == [M.ENQUEUED | M.DEQUEUED | M.FORWARDED, 0, 0] and fw.tolist() == [5 * M.MS, -1, -1]


def test_gpu_closing_the_plan_closes_its_routers():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import InboundRouter, RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    ib = InboundRouter(p, [1000, 1000], 4)
    try:
        p.close()
        closed = not ib._h
    finally:
        ib.close()
        p.close()
    assert closed
