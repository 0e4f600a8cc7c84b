"""UDP receive stage on the device (srt_udprecv over a plan): the seven-window
scenarios and the hand-worked cases byte-equal to the host-only form and to the
model, one call against the same window cut in two, a wave whose spans exceed
its LDS window beside one whose spans fit, the chain srt_inbound_run ->
srt_deliver_run -> srt_udprecv_run on device arrays with nothing read back in
between, a ring of four messages overflowing, reads outside the window, and the
plan closing its instance."""
import numpy as np
import pytest

import udprecv_model as M
import udprecv_scenario as T

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
@pytest.mark.parametrize("n_hosts", [1, 64, 65, 130])
def test_gpu_equals_host_only_and_model(plan, n_hosts, shape):
    """hosts with 0 to 70 slots, so waves that hold one host's slots, several hosts', and a host's tail
    with the next hosts' heads; dense: up to 130 records and 150 reads a host and window"""
    m_outs, m_st, m_status, _ = T.model_scenario(n_hosts, shape)
    outs, st, status = T.run_scenario(plan, n_hosts, shape)
    h_outs, h_st, h_status = T.run_scenario(None, n_hosts, shape)
    assert status == h_status == m_status and status[0] == 0 and len(outs) == 7
    for k, (a, h, m) in enumerate(zip(outs, h_outs, m_outs)):
        T.same_outputs(a, m, (k, "model"))
        T.same_outputs(a, h, (k, "host-only"))
    T.same_state(st, m_st)
    T.same_state(st, h_st)


@pytest.mark.parametrize("case", T.golden_cases(), ids=lambda c: c["name"])
def test_gpu_golden_case(plan, case):
    outs, st, status = T.run_scenario(plan, 0, None, T.golden_windows(case), case["socket_ptr"])
    assert status[0] == 0
    T.check_golden(case, outs, st)


def test_gpu_one_call_equals_split_calls(plan):
    T.one_call_against_split(plan)


@pytest.mark.parametrize("over", ["records", "reads", "both"])
def test_gpu_span_over_the_lds_window_beside_one_that_fits(plan, over):
    """70 hosts of two slots: the first wave's 32 hosts get just over the window's worth of records (walked in
    device memory, their few reads in LDS), or of reads (the other way round), or of both; the other waves'
    hosts get a few of each and are walked in LDS"""
    from shadow_amd.plan import UdpReceive

    n_hosts, win = 70, UdpReceive.window_bytes()
    sp = np.arange(n_hosts + 1, dtype=np.uint32) * 2
    rng = np.random.default_rng(5)
    per, rper = np.full(n_hosts, 6, np.int64), np.full(n_hosts, 5, np.int64)
    if over != "reads":
        per[:32] = win // 32 // 32 + 1  # 32 bytes a staged record, 32 hosts in the wave
    if over != "records":
        rper[:32] = win // 24 // 32 + 1  # 24 bytes a read
    hp = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    n = int(hp[-1])
    rp = np.concatenate([[0], np.cumsum(rper)]).astype(np.uint32)
    # asserted on the inputs: wave 0 (slots 0..63, hosts 0..31) has a list past the window -- by less than a
    # record or a read a host -- and the other list within it; waves 1 and 2 hold both lists
    rec_b, rd_b = int(hp[32]) * 32, int(rp[32]) * 24
    assert (rec_b > win >= rec_b - 32 * 32) == (over != "reads") and (rd_b > win >= rd_b - 32 * 24) == (over != "records")
    assert rec_b <= win or rd_b <= win or over == "both"
    assert (over == "records" and rd_b < win) or (over == "reads" and rec_b + rd_b > win > rec_b) or over == "both"
    assert (int(hp[64]) - int(hp[32])) * 32 + (int(rp[64]) - int(rp[32])) * 24 < win // 8
    fwd, sock = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    reads = np.zeros(int(rp[-1]), M.READ)
    for h in range(n_hosts):
        fwd[hp[h]:hp[h + 1]] = np.sort(rng.integers(0, 400, per[h])) * T.GRID
        sock[hp[h]:hp[h + 1]] = 2 * h + rng.integers(0, 2, per[h])
        reads["time_ns"][rp[h]:rp[h + 1]] = np.sort(rng.integers(0, 400, rper[h])) * T.GRID
        reads["slot"][rp[h]:rp[h + 1]] = 2 * h + rng.integers(0, 2, rper[h])
    reads["len"], reads["flags"] = 700, rng.choice([0, M.PEEK, M.TRUNC], len(reads))
    meta = np.zeros(n, M.META)
    meta["payload_size"], meta["src_ip_be"], meta["src_port_be"] = rng.integers(0, 1400, n), 9, 9
    meta["user"] = np.arange(n)
    ops = np.array([(M.OPEN, x, 20000) for x in range(2 * n_hosts)], M.OP)
    win0 = dict(ops=ops, meta=meta, tag_base=0, out_host_ptr=hp, out_socket=sock, out_forward_ns=fwd,
                out_tag=np.arange(n, dtype=np.uint64), out_status=np.full(n, T.HIT, np.uint32), read_host_ptr=rp,
                reads=reads, until_ns=400 * T.GRID)
    drain = dict(win0, ops=np.zeros(0, M.OP), meta=np.zeros(0, M.META), tag_base=n,
                 out_host_ptr=np.zeros(n_hosts + 1, np.uint32), read_host_ptr=rp, until_ns=800 * T.GRID,
                 reads=np.array([(500 * T.GRID, s, 9, 0, 0) for s in reads["slot"]], M.READ),
                 **{k: np.zeros(0, win0[k].dtype) for k in ("out_socket", "out_forward_ns", "out_tag", "out_status")})
    m_outs, m_st, m_status, stats = T.model_scenario(0, None, [win0, drain], sp)
    outs, st, status = T.run_scenario(plan, 0, None, [win0, drain], sp)
    h_outs, h_st, h_status = T.run_scenario(None, 0, None, [win0, drain], sp)
    assert status == h_status == m_status and status[0] == 0
    assert stats["read_same_call"] > 10 and stats["read_carried"] > 10, stats
    assert stats["drop_full"] > 10 or over != "records", stats
    for k in range(2):
        T.same_outputs(outs[k], m_outs[k], (k, "model"))
        T.same_outputs(outs[k], h_outs[k], (k, "host-only"))
    T.same_state(st, m_st)
    T.same_state(st, h_st)


def test_gpu_inbound_deliver_udprecv_chain_without_a_read_back(plan):
    """70 hosts, six windows and one that drains: srt_inbound_run, srt_deliver_run and srt_udprecv_run on
    device arrays, each taking the one before's outputs as they are (out_cap the arrays' capacity, no status
    call and no copy to the host in between), against inbound_model -> deliver_model -> udprecv_model
    chained the same way"""
    T.chain(plan)


def test_gpu_ring_of_four_overflows_for_its_sockets_only(plan):
    """ring_cap 4 on a scenario that leaves more than four messages in some sockets: the flag, the marked
    sockets equal the host-only form's, and every socket that was never marked has the model's results"""
    sc = T.scenario(65, T.DENSE)
    wins, sp = sc["windows"][:3], sc["socket_ptr"]
    r = T.Runner(plan, sp, 4)
    outs, ever = [], np.zeros(int(sp[-1]), bool)
    for w in wins:
        outs.append(r.window(w))
        ever |= r.ur.state()["overflow"] != 0  # reopening a socket clears its mark, not what it returned before
    st, status = r.finish()
    h_outs, h_st, h_status = T.run_scenario(None, 0, None, wins, sp, ring_cap=4)
    m_outs, m_st, _, _ = T.model_scenario(0, None, wins, sp)  # rings that hold everything
    assert status == h_status and status[0] & M.F_RING_OVERFLOW and not status[0] & ~(M.F_RING_OVERFLOW | M.F_ARMED_TWICE)
    for k, (a, h) in enumerate(zip(outs, h_outs)):
        T.same_outputs(a, h, k)
    T.same_state(st, h_st)
    marked = ever
    assert 10 < marked.sum() < len(marked) - 10 and set(st["overflow"]) == {0, M.MARK_RING}
    assert (st["n_msgs"] <= 4).all() and (st["n_msgs"][marked] == 4).any()
    ok = ~marked
    for k in ("len_bytes", "soft_limit", "n_msgs", "last_read_recv_ns", "armed_seq", "open"):
        assert np.array_equal(st[k][ok], m_st[k][ok]), k
    for w, o, mo in zip(wins, outs, m_outs):
        keep = (w["out_socket"] >= len(marked)) | ok[np.minimum(w["out_socket"], len(marked) - 1)]
        assert np.array_equal(o["rx_status"][keep], mo["rx_status"][keep])
        rkeep = ok[w["reads"]["slot"]]
        assert o["results"][rkeep].tobytes() == mo["results"][rkeep].tobytes() and rkeep.sum() > 100


def test_gpu_reads_outside_the_window_are_flagged_and_not_taken(plan):
    wins = T.golden_windows(dict(socket_ptr=[0, 1, 2], calls=[
        dict(ops=[[1, 0, 1000], [1, 1, 1000]], until=1000, pushes=[[0, 0, 10, 1, 1, 1], [1, 1, 10, 2, 1, 1]],
             reads=[[0, 1000, 0, 100, 0], [1, 500, 1, 100, 2], [1, 400, 1, 100, 0], [1, 500, 1, 100, 0]]),
        dict(ops=[], until=2000, pushes=[], reads=[[0, 999, 0, 100, 0], [0, 1000, 0, 100, 0]])]))
    for p in (plan, None):
        outs, st, status = T.run_scenario(p, 0, None, wins, [0, 1, 2])
        assert status[0] == M.F_READ_ORDER
        # at until_ns: not taken; 400 after 500 in its host's list: not taken, the reads around it are
        assert list(outs[0]["results"]["status"]) == [0, 1, 0, 1]
        assert list(outs[0]["results"]["return_val"]) == [0, 2, 0, 2]
        # below the previous until_ns: not taken; at it: taken
        assert list(outs[1]["results"]["status"]) == [0, 1] and outs[1]["results"]["return_val"][1] == 1
        assert list(st["n_msgs"]) == [0, 0]
    m_outs, _, m_status, _ = T.model_scenario(0, None, wins, [0, 1, 2])
    assert m_status[0] == M.F_READ_ORDER
    for a, b in zip(outs, m_outs):
        T.same_outputs(a, b)


def test_gpu_closing_the_plan_closes_its_instance():
    from shadow_amd import NetworkGraph, UdpReceive, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    ur = UdpReceive(p, [0, 2, 3], 4, 4)
    try:
        p.close()
        closed = not ur._h
    finally:
        ur.close()
        p.close()
    assert closed
