"""Loopback stage on the device (srt_loopback over a plan): the CPU tests'
scenario bit-equal to the model and to the host-only form in both qdiscs, one
call and split; the shapes on either side of the constants the kernel switches
on (8 or 64 lanes a host at an average of 16 packets a host, 32 or 4 hosts a
workgroup, spans and instants longer than a lane group); one instant many times
a wave beside empty hosts; flagged hosts reported without a fault;
srt_deliver_lookup_flat against the host lookup; and the chain outbound ->
lookup_flat -> tracker rx_flat beside a loopback run, local and remote counters
apart."""
import numpy as np
import pytest

import loopback_model as LM
import loopback_scenario as S

pytestmark = pytest.mark.gpu
QDISCS = pytest.mark.parametrize("qdisc", [LM.FIFO, LM.RR], ids=["fifo", "rr"])
WIDE_AVG, LANES_NARROW, LANES_WIDE, BT = 16, 8, 64, 256  # srt_stage.h (the lane groups: 8 or 64)


@pytest.fixture(scope="module")
def plan():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    yield p
    p.close()


def three_way(sc, qdisc, plan, n_slots=None):
    """device == model and device == host-only, byte for byte"""
    m_outs, m_beats, m_stats, m = S.run_model(sc, qdisc, n_slots)
    dev = S.run_lib(sc, qdisc, plan, n_slots)
    S.assert_same(dev, (m_outs, m_beats, m_stats), "device vs model")
    S.assert_same(dev, S.run_lib(sc, qdisc, None, n_slots), "device vs host-only")
    return dev, m


@QDISCS
@pytest.mark.parametrize("split", [False, True], ids=["one_call", "split"])
def test_gpu_equals_model_and_host_only(plan, qdisc, split):
    sc = S.main_scenario()
    dev, m = three_way(S.split_scenario(sc) if split else sc, qdisc, plan)
    assert all(st[0][0] == 0 for st in dev[2]) and sum(st[0][1] for st in dev[2]) > 500


def _counts(n_hosts, total, seed, big=None):
    """n_hosts counts that sum to `total`, a few hosts empty, host `big[0]` with big[1] packets"""
    rng = np.random.default_rng(seed)
    c = np.zeros(n_hosts, np.int64)
    c[::9] = 0
    free = [h for h in range(n_hosts) if h % 9]
    if big:
        c[big[0]] = big[1]
        free.remove(big[0])
    left = total - int(c.sum())
    assert left >= 0
    for h in rng.choice(free, size=left):
        c[h] += 1
    return c


@QDISCS
@pytest.mark.parametrize("over", [0, 1], ids=["avg16_8lanes", "over16_64lanes"])
def test_gpu_either_side_of_the_lane_switch(plan, qdisc, over):
    """70 hosts (two workgroups of 32 and a rest of 6 at 8 lanes; 17 of 4 and a rest of 2 at 64) with
    exactly 16 packets a host on average, and one packet more; host 40 holds 150 packets, more than
    either lane group walks in one step, with instants that cross the steps"""
    n_hosts = 70
    total = WIDE_AVG * n_hosts + over
    counts = _counts(n_hosts, total, 3 + over, big=(40, 150))
    lanes = LANES_WIDE if total > WIDE_AVG * n_hosts else LANES_NARROW
    assert lanes == (LANES_WIDE if over else LANES_NARROW) and n_hosts % (BT // lanes) not in (0, 1)
    assert counts[40] > 2 * LANES_WIDE and (counts == 0).sum() >= 8 and counts.sum() == total
    sc = S.shape_scenario(17, n_hosts, 5, counts, group_max=40)
    pk = sc["steps"][1][1]["pkts"]
    b = int(sc["steps"][1][1]["host_ptr"][40])
    t = pk["ready_ns"][b:b + 150]
    starts = np.r_[0, np.nonzero(np.diff(t.astype(np.int64)))[0] + 1, 150]
    assert (np.diff(starts) > LANES_NARROW).any() and any(s // lanes != (e - 1) // lanes
                                                          for s, e in zip(starts[:-1], starts[1:]))
    three_way(sc, qdisc, plan)


@QDISCS
def test_gpu_one_long_instant_beside_empty_hosts(plan, qdisc):
    """host 2 of 9 sends 700 packets in one instant, eleven times a wave, over 5 sockets; the others
    nothing or a handful"""
    counts = [0, 3, 700, 0, 0, 9, 0, 1, 0]
    sc = S.shape_scenario(23, 9, 5, counts, single=True)
    assert sum(counts) > WIDE_AVG * 9
    dev, m = three_way(sc, qdisc, plan)
    assert max(m.pop_lens) == 700 and dev[2][0][1] == [0, 1, 1, 0, 0, 1, 0, 1, 0]
    # and at 8 lanes a host: the same long instant among enough hosts to bring the average down
    counts = [0] * 60
    counts[7], counts[8], counts[59] = 300, 2, 5
    sc = S.shape_scenario(24, 60, 5, counts, single=True)
    assert sum(counts) <= WIDE_AVG * 60
    three_way(sc, qdisc, plan)


@QDISCS
@pytest.mark.parametrize("kind", ["time", "time_inside", "socket"])
def test_gpu_flagged_hosts_reported_not_faulted(plan, qdisc, kind):
    """valid API input with a caller error in it: every write is range-checked, the neighbours stay exact"""
    dev, m = three_way(S.flag_scenario(kind), qdisc, plan)
    assert [st[0][0] for st in dev[2]] == [0, LM.BAD_SOCKET if kind == "socket" else LM.TIME_ORDER, 0]


@QDISCS
def test_gpu_slots_out_of_range_and_off(plan, qdisc):
    sc = S.flag_scenario("none")
    sc["steps"][2][1]["pkts"]["socket"][:] %= 4
    dev, m = three_way(sc, qdisc, plan, n_slots=6)
    assert all(st[0][0] == LM.BAD_SLOT for st in dev[2])
    dev, m = three_way(sc, qdisc, plan, n_slots=0)
    assert all(st[0][0] == 0 for st in dev[2])


def test_gpu_grouping_past_the_batch_is_walked_inside_it(plan):
    """host_ptr claims more packets than n_pkts: the walk is held below n_pkts on the device"""
    sc = S.shape_scenario(5, 6, 4, [4, 0, 7, 3, 5, 6])
    c = sc["steps"][1][1]
    n = len(c["pkts"]) - 4
    for k in ("pkts", "rx_meta", "trk_meta"):
        c[k] = c[k][:n].copy()
    assert int(c["host_ptr"][6]) == n + 4
    dev, m = three_way(sc, LM.FIFO, plan)
    assert dev[2][0][0][1] == n


def test_gpu_lookup_flat_equals_host_lookup(plan):
    """every key class of the deliver scenario's generator (specific, wildcard, peer 0:0, a protocol that
    matches nothing), hosts out of range, and a table change between two calls (the re-upload, the
    second time after the table has doubled)"""
    import torch

    import deliver_model as DM
    import deliver_scenario as D
    from shadow_amd.plan import DeliverStage

    n_hosts, n = 40, 3000
    rng = np.random.default_rng(8)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    taken = set()
    first = D.rand_assoc(rng, n_hosts, 60, taken, 0)
    second = D.rand_assoc(rng, n_hosts, 500, taken, 1000)
    metas = D.rand_meta(rng, n)
    hosts = rng.integers(0, n_hosts, size=n).astype(np.uint32)
    hosts[::50] = n_hosts + rng.integers(0, 5, size=len(hosts[::50]))
    hosts[7] = 0xFFFFFFFF
    ds, ref = DeliverStage(plan, n_hosts, 8, 0, 0), DeliverStage(None, n_hosts, 8, 0, 0)
    try:
        d_hosts, d_meta = t(hosts, np.int32), t(metas.view(np.uint8), np.uint8)
        seen = []
        for step in ("empty", first, second, ("drop", first[::2])):
            if isinstance(step, tuple):
                ds.disassociate(step[1]), ref.disassociate(step[1])
            elif not isinstance(step, str):
                ds.associate(step), ref.associate(step)
            out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            ds.lookup_flat(d_hosts, d_meta, out)
            got = out.cpu().numpy().view(np.uint32)
            want = ref.lookup(np.minimum(hosts, n_hosts), metas)  # a host the table cannot hold: no socket
            want[hosts >= n_hosts] = DM.NONE32
            assert got.tobytes() == want.tobytes(), step if isinstance(step, str) else len(step)
            seen.append(int((got != DM.NONE32).sum()))
        assert seen[0] == 0 and seen[0] < seen[1] < seen[2] and seen[3] < seen[2]
        assert ds.table_stats()[1] > 8 * 16  # the table doubled between calls
        hit = want != DM.NONE32
        wild = (metas["peer_ip_be"] == 0) & (metas["peer_port_be"] == 0)
        assert (hit & wild).any() and (hit & ~wild).any() and (~hit & (metas["protocol"] == 3)).any()
        assert ds.status()[0] == 0
    finally:
        ds.close()
        ref.close()


def test_gpu_chain_local_and_remote_counters_stay_apart(plan):
    """One round at 30 hosts.  Internet interface: an outbound call with SRT_OUT_LOCAL packets among the
    remote ones, srt_tracker_tx on its outputs, then the local packets through srt_deliver_lookup_flat
    and srt_tracker_rx_flat on device arrays, no read-back in between: the REMOTE records.  Loopback
    interface: a loopback run on its own packets and associations: the LOCAL records.  Each side equals
    its model fed the same packets and the two sets of records differ."""
    import torch

    import outbound_scenario as OS
    import tracker_model as TM
    from shadow_amd import LoopbackRelay, Tracker
    from shadow_amd.plan import DeliverStage, OutboundRelay

    n_hosts, ms, n_pkts = 30, 4, 900
    n_slots = n_hosts * ms
    rng = np.random.default_rng(12)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    osc = OS.make_scenario(rng, n_hosts, n_pkts, np.full(n_hosts, ms), np.full(n_hosts, 1 << 40, np.uint64),
                           50 * OS.MS, local_share=0.3)
    pk, hp, host = osc["pkts"], osc["host_ptr"], osc["host"]
    inet_assoc = S.associations(n_hosts, ms)
    g = S.Gen(31, n_hosts, ms)
    inet = g.call(np.diff(hp.astype(np.int64)))  # rx and trk metas for the internet interface's packets
    lo_sc = S.shape_scenario(32, n_hosts, ms, rng.integers(0, 25, size=n_hosts))
    lo_call = lo_sc["steps"][1][1]
    local = np.nonzero(pk["flags"] & 1)[0]
    assert 150 < len(local) < 450

    ob = OutboundRelay(plan, osc["bw"], LM.FIFO, ms, 64)
    inet_dl, lo_dl = DeliverStage(plan, n_hosts, 8, 0, 0), DeliverStage(plan, n_hosts, 8, 0, 0)
    trk = Tracker(plan, n_hosts, n_slots, 0, 0)
    lb = LoopbackRelay(plan, n_hosts, LM.FIFO, ms, n_slots)
    try:
        inet_dl.associate(inet_assoc)
        lo_dl.associate(lo_sc["steps"][0][1][::2])  # the loopback interface's own, different, table
        d_hp = t(hp, np.int32)
        d_st = torch.zeros(n_pkts, dtype=torch.int32, device=dev)
        d_sn, d_rk = torch.zeros(n_pkts, dtype=torch.int64, device=dev), torch.zeros(n_pkts, dtype=torch.int64, device=dev)
        d_cs = torch.zeros(n_hosts, dtype=torch.int64, device=dev)
        d_trk = t(inet["trk_meta"].view(np.uint8), np.uint8)
        base = ob.run(t(pk.view(np.uint8), np.uint8), d_hp, 60 * OS.MS, 0, d_st, d_sn, d_rk)
        ob.cached_seq(d_cs)
        trk.tx(d_cs, d_hp, d_trk, d_st, base)
        # the local packets: hosts and metas gathered on the device, looked up, counted
        d_local = t(local, np.int64)
        d_lhost = t(host, np.int32)[d_local].contiguous()
        d_lrx = t(inet["rx_meta"].view(np.uint8), np.uint8).view(n_pkts, 16)[d_local].contiguous().view(-1)
        d_ltrk = d_trk.view(n_pkts, 16)[d_local].contiguous().view(-1)
        d_lsock = torch.full((len(local),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        inet_dl.lookup_flat(d_lhost, d_lrx, d_lsock)
        trk.rx_flat(d_lhost, d_lsock, d_ltrk)
        # beside them, the loopback interface
        n_lo = len(lo_call["pkts"])
        o = [torch.zeros(n_lo, dtype=torch.int32, device=dev) for _ in range(2)] + \
            [torch.zeros(n_lo, dtype=torch.int64, device=dev)] + \
            [torch.zeros(n_lo, dtype=torch.int32, device=dev) for _ in range(2)]
        lb.run(lo_dl, t(lo_call["pkts"].view(np.uint8), np.uint8), t(lo_call["host_ptr"], np.int32),
               t(lo_call["rx_meta"].view(np.uint8), np.uint8), t(lo_call["trk_meta"].view(np.uint8), np.uint8), *o)
        remote, local_recs = trk.heartbeat(), lb.heartbeat()
        st = d_st.cpu().numpy().view(np.uint32)
        lsock = d_lsock.cpu().numpy().view(np.uint32)
        assert ob.status() == (0, 0) and trk.status()[0] == 0 and lb.status()[0] == 0
        assert inet_dl.status()[0] == 0 and lo_dl.status()[0] == 0
    finally:
        for x in (lb, trk, lo_dl, inet_dl, ob):
            x.close()
    assert (st & LM.SENT).all()  # unthrottled: every packet was popped in the call
    # the remote side against the tracker model and the host lookup's rules
    im = LM.LoopbackModel(n_hosts, LM.FIFO, ms, n_slots)  # its association dict and lookup only
    im.associate(inet_assoc)
    want_sock = np.array([im.lookup(int(host[i]), inet["rx_meta"][i]) for i in local], np.uint32)
    assert lsock.tobytes() == want_sock.tobytes() and 0 < (want_sock == LM.NONE32).sum() < len(local)
    tm = TM.TrackerModel(n_hosts, n_slots, 0, 0)
    tm.tx(np.full(n_hosts, TM.U64, np.uint64), hp, inet["trk_meta"], st, base)
    tm.rx_flat(host[local], want_sock, inet["trk_meta"][local])
    S.same_records(remote, tm.heartbeat(), "remote")
    # the local side against the loopback model
    lm = LM.LoopbackModel(n_hosts, LM.FIFO, ms, n_slots)
    lm.associate(lo_sc["steps"][0][1][::2])
    lm.run(lo_call["pkts"], lo_call["host_ptr"], lo_call["rx_meta"], lo_call["trk_meta"])
    S.same_records(local_recs, lm.heartbeat(), "local")
    for k in range(4):
        assert remote[k].tobytes() != local_recs[k].tobytes() and local_recs[k]["packets_data"].sum() > 0


def test_gpu_closing_the_plan_closes_its_instance():
    from shadow_amd import LoopbackRelay, NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    lb = LoopbackRelay(p, 2, LM.RR, 2, 4)
    try:
        p.close()
        closed = not lb._h
    finally:
        lb.close()
        p.close()
    assert closed
