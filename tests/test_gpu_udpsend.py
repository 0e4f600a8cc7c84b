"""UDP send side on the device (srt_udpsend over a plan): the seven-window
scenarios and the hand-worked cases byte-equal to the host-only form and to the
model, one call against the same window cut in two, a wave whose call span is
just past its LDS window beside waves that fit, hosts with one slot more than
the in-LDS slot count beside hosts at it, a ring of four messages overflowing on
one host while its neighbours stay exact, the chain srt_udpsend_run ->
srt_sendbatch_run on device arrays with nothing read back in between, and the
plan closing its instance."""
import numpy as np
import pytest

import udpsend_model as M
import udpsend_scenario as T

pytestmark = pytest.mark.gpu

# the step kernel's LDS (include/srt.h, srt_udpsend_window_bytes): staged calls of 32 bytes, then slot records
# of 88 bytes with a 4-byte qdisc entry each
WIN_CAP, SLOT_LDS = 1536, 320


@pytest.fixture(scope="module")
def plan():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    yield p
    p.close()


def three_ways(plan, sc, ring_cap=T.RING_CAP):
    """device == host-only == model: outputs, state, status"""
    m_outs, m_st, m_status = T.model_scenario(sc, ring_cap)
    outs, st, status = T.run_scenario(plan, sc, ring_cap)
    h_outs, h_st, h_status = T.run_scenario(None, sc, ring_cap)
    assert status == h_status == m_status and len(outs) == len(sc["windows"])
    for k, (a, h, m) in enumerate(zip(outs, h_outs, m_outs)):
        T.same_outputs(a, m, (k, "model"))
        T.same_outputs(a, h, (k, "host-only"))
    T.same_state(st, m_st)
    T.same_state(st, h_st)
    return status


@pytest.mark.parametrize("qdisc", [M.FIFO, M.RR])
@pytest.mark.parametrize("shape", [T.FREE, T.THROTTLED])
@pytest.mark.parametrize("n_hosts", [1, 64, 65, 130])
def test_gpu_equals_host_only_and_model(plan, n_hosts, shape, qdisc):
    """hosts with 0 to 5 slots; FREE: nothing ever blocks; THROTTLED: 1,000 to 100,000 B/s and limits of 4,096,
    so sends arm, wake and carry across calls"""
    sc = T.scenario(n_hosts, shape, qdisc)
    status = three_ways(plan, sc)
    assert not status[0] & (M.F_RING_OVERFLOW | M.F_LATE_OVERFLOW | M.F_LATE_RESULT_OVERFLOW)
    if shape == T.FREE:
        assert status[3] == status[4] == 0
    elif n_hosts >= 64:
        st = T.scenario_stats(sc)
        assert st["woken_same_call"] > 20 and st["woken_later"] > 20 and st["late_pkts"] > 100


@pytest.mark.parametrize("case", T.golden_cases(), ids=lambda c: c["name"])
def test_gpu_golden_case(plan, case):
    outs, st, status = T.run_scenario(plan, T.golden_scenario(case))
    T.check_golden(case, outs, st, status)


def test_gpu_one_call_equals_split_calls(plan):
    T.one_call_against_split(plan)


def test_gpu_call_span_just_past_the_lds_window_beside_spans_that_fit(plan):
    """130 hosts of one slot: the first wave's 64 hosts make WIN_CAP + 1 calls a window (walked in device memory),
    the second wave's exactly WIN_CAP (staged in LDS), the third's two hosts a few"""
    from shadow_amd.plan import UdpSend

    assert UdpSend.window_bytes() == WIN_CAP * 32 + SLOT_LDS * (88 + 4) <= 80 * 1024
    assert WIN_CAP % 64 == 0
    per = [WIN_CAP // 64] * 128 + [5, 3]
    per[0] += 1
    sc = T.simple_scenario([1] * 130, per)
    hp = sc["windows"][0]["host_ptr"].astype(np.int64)
    assert hp[64] - hp[0] == WIN_CAP + 1 and hp[128] - hp[64] == WIN_CAP and hp[130] - hp[128] == 8
    status = three_ways(plan, sc)
    assert status[2] > 1000 and status[3] > 1000 and status[4] > 100 and not status[0] & ~M.F_ARMED_TWICE


def test_gpu_one_slot_past_the_lds_slot_count_beside_hosts_at_it(plan):
    """the first wave's 64 hosts own SLOT_LDS slots (their records sit in LDS), the second wave's one more (they
    stay in device memory), the third wave has two hosts"""
    assert SLOT_LDS % 64 == 0
    counts = [SLOT_LDS // 64] * 128 + [2, 0]
    counts[64] += 1
    sc = T.simple_scenario(counts, [25] * 130, qdisc=M.RR)
    sp = sc["socket_ptr"].astype(np.int64)
    assert sp[64] - sp[0] == SLOT_LDS and sp[128] - sp[64] == SLOT_LDS + 1
    status = three_ways(plan, sc)
    assert status[2] > 1000 and status[3] > 100 and status[4] > 100 and not status[0] & ~M.F_ARMED_TWICE


def test_gpu_ring_of_four_overflows_on_one_host_only(plan):
    """ring_cap 4.  Host 3 (1,000 B/s) sends payloads of 40 to 60 bytes: about eighty fit its limit of 4,096 and
    stay queued, so its ring overflows; every other host sends 1,400 to 1,472 bytes, of which a socket holds
    at most three.  The device agrees with the host-only form everywhere and with the model on every host."""
    n = 70
    lens = [(1400, 1473)] * n
    lens[3] = (40, 61)
    sc = T.simple_scenario([2] * n, [30] * n, lens=lens, bws=[1000 if h == 3 else 50000 for h in range(n)])
    status = three_ways(plan, sc, ring_cap=4)
    assert status[0] & M.F_RING_OVERFLOW
    from shadow_amd.plan import UdpSend  # noqa: F401

    outs, (hosts, socks), _ = T.run_scenario(plan, sc, ring_cap=4)
    assert list(np.flatnonzero(hosts["overflow"])) == [3] and set(np.flatnonzero(socks["overflow"])) <= {6, 7}
    assert socks["n_msgs"].max() <= 4


def test_gpu_chain_udpsend_to_sendbatch_nothing_read_back(plan):
    """srt_udpsend_run's send_ns / send_rank / late list feed srt_sendbatch_run as they lie on the device; the
    batch it builds is the model's send order: per host its non-local forwarded packets by rank"""
    import torch

    from shadow_amd.plan import SEND_META_DTYPE, SRT_PKT_DTYPE, SendBatch

    sc = T.scenario(65, T.THROTTLED, M.FIFO)
    n_hosts = 65
    m_outs, _, _ = T.model_scenario(sc)
    r = T.Runner(plan, sc)
    total = sum(len(w["calls"]) for w in sc["windows"])
    sb = SendBatch(plan, n_hosts, total + 1)
    cap = 4096
    got, want = [], []
    host_of = {}
    for w, mo in zip(sc["windows"], m_outs):
        calls, hp = w["calls"], w["host_ptr"]
        n = len(calls)
        meta = np.zeros(max(n, 1), SEND_META_DTYPE)
        meta["payload_size"][:n], meta["user"][:n] = calls["len"], calls["user"]
        d = r.window(w, keep_device=True)
        o_pk = torch.zeros(cap * 24, dtype=torch.uint8, device="cuda:0")
        o_hp = torch.zeros(n_hosts + 1, dtype=torch.int32, device="cuda:0")
        o_us = torch.zeros(cap, dtype=torch.int32, device="cuda:0")
        o_sq = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
        sb.run(d["host_ptr"], T._dev(meta, plan)[:16 * n], d["send_ns"], d["send_rank"], d["base"], d["late"],
               d["late_count"], o_pk, o_hp, o_us, o_sq)
        ohp = T._host(o_hp, np.uint32)
        n_sent = int(ohp[-1])
        pk = T._host(o_pk, SRT_PKT_DTYPE)[:n_sent]
        sq = T._host(o_sq, np.uint64)[:n_sent]
        got.append([(int(h), int(sq[k]), int(pk["t_ns"][k])) for h in range(n_hosts) for k in range(ohp[h], ohp[h + 1])])
        for h in range(n_hosts):
            for i in range(int(hp[h]), int(hp[h + 1])):
                host_of[mo["base"] + i] = h
        sent = [(host_of[mo["base"] + i], int(mo["send_rank"][i]), mo["base"] + i, int(mo["send_ns"][i]))
                for i in range(n) if mo["send_rank"][i] != M.U64]
        sent += [(h, rank, seq, t) for seq, t, rank, st, h in mo["late"] if rank != M.U64]
        want.append([(h, seq, t) for h, rank, seq, t in sorted(sent)])
    assert sb.status()[0] == 0
    assert got == want and sum(len(g) for g in got) > 1000
    r.finish()
    sb.close()


def test_gpu_plan_close_closes_the_instance():
    from shadow_amd import NetworkGraph, synth
    from shadow_amd.plan import RoutingPlan, UdpSend

    src, dst, lat, loss = synth.complete_graph(16, 1)
    p = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32)).run()
    us = UdpSend(p, [0, 2, 3], [T.ip_of(0), T.ip_of(1)], [1000, 1000], M.FIFO, 4)
    assert us._h
    p.close()
    assert not us._h
    us.close()
