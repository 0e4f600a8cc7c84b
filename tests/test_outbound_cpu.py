"""Outbound relay stage (srt_outbound: interface qdisc over per-socket queues +
upload token bucket per source host; network_interface.c,
network_queuing_disciplines.c, relay/mod.rs, relay/token_bucket.rs) without a
GPU: hand-computed pins on the model and on the host-only srt_outbound -- the
same per-host step the device kernel compiles -- and the host-only form against
the model, bit for bit.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import outbound_model as M
import outbound_scenario as S

MS = M.MS
SENT, CACHED, FWD = M.INTERFACE_SENT, M.CACHED, M.FORWARDED
QDISCS = [M.FIFO, M.RR]


def _pkts(rows):
    """rows: (ready_ms, socket, priority, size, local) of one host, in arrival order"""
    pk = np.zeros(len(rows), S.OUT_PKT_DTYPE)
    for i, (t, sock, prio, size, local) in enumerate(rows):
        pk[i] = (t * MS, prio, size, sock, int(local), 0)
    return pk


def _tiny(bw, rows, qdisc, untils, bootstrap_end=0, max_sockets=4, queue_cap=16, late_cap=16, lib=True, refeed=True):
    """one host fed `rows` (with refeed, those whose status was 0; without, nothing)
    call after call, through the host-only library or the model -> per call (status, send_ns, rank, late
    records, flags, pending), and the final state as a dict"""
    from shadow_amd.plan import OutboundRelay

    pk = _pkts(rows)
    outs, left = [], np.arange(len(rows))
    if lib:
        r = OutboundRelay(None, [bw], qdisc, max_sockets, queue_cap)
    else:
        m = M.OutboundModel([bw], qdisc, max_sockets)
    for until in untils:
        n = len(left)
        hp = np.array([0, n], np.uint32)
        if lib:
            st, sn, rk = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
            late, cnt = np.zeros(32 * late_cap, np.uint8), np.zeros(1, np.uint32)
            r.run(pk[left].view(np.uint8), hp, until * MS, bootstrap_end, st, sn, rk, late, cnt)
            flags, pending = r.status(check=False)
            recs = late[:32 * min(int(cnt[0]), late_cap)].view(S.LATE_DTYPE)
            lt = sorted((int(x["seq"]), int(x["send_ns"]), int(x["send_rank"]), int(x["status"]), int(x["src_host"]))
                        for x in recs)
        else:
            st, sn, rk, lt, _ = m.run(pk[left], hp, until * MS, bootstrap_end)
            flags, pending = None, m.pending()
        outs.append((st.tolist(), sn.tolist(), rk.tolist(), lt, flags, pending))
        left = left[st == 0] if refeed else left[:0]
    if lib:
        rec = r.state()
        state = {f: int(rec[f][0]) for f in rec.dtype.names}
        r.close()
    else:
        state = m.state()[0]
    return outs, state


BOTH = pytest.mark.parametrize("lib", [False, True], ids=["model", "host_only"])


# ------------------------------------------------------------ hand-computed pins
@BOTH
def test_pin_bucket_timing(lib):
    """1,000,000 B/s: refill 1000 a ms, capacity 2500; five 1500-byte packets at 0"""
    rows = [(0, 0, 10 + k, 1500, False) for k in range(5)]
    outs, state = _tiny(1_000_000, rows, M.FIFO, [100], lib=lib)
    st, sn, rk = outs[0][:3]
    assert sn == [0, 1 * MS, 2 * MS, 4 * MS, 5 * MS]
    assert rk == [0, 1, 2, 3, 4]
    assert st == [SENT | FWD] + [SENT | FWD | CACHED] * 4
    assert state["tasks_scheduled"] == 5 and state["sent_total"] == 5 and state["queue_len"] == 0
    assert state["task_ns"] == M.U64 and state["cached"] == 0


def _send_sequence(outs):
    st, sn, rk = outs[0][:3]
    return [i for _, i in sorted((r, i) for i, r in enumerate(rk) if r != M.U64)]


@BOTH
def test_pin_qdisc_order(lib):
    """sockets A (priorities 1, 2, 3) and B (4, 5), all ready at 0, during bootstrap"""
    rows = [(0, 0, 1, 100, False), (0, 0, 2, 100, False), (0, 0, 3, 100, False), (0, 1, 4, 100, False),
            (0, 1, 5, 100, False)]
    a0, a1, a2, b0, b1 = range(5)
    outs, _ = _tiny(1000, rows, M.FIFO, [10], bootstrap_end=10 * MS, lib=lib)
    assert _send_sequence(outs) == [a0, a1, a2, b0, b1] and outs[0][1] == [0] * 5
    outs, _ = _tiny(1000, rows, M.RR, [10], bootstrap_end=10 * MS, lib=lib)
    assert _send_sequence(outs) == [a0, b0, a1, b1, a2] and outs[0][1] == [0] * 5


@BOTH
def test_pin_fifo_compares_socket_heads(lib):
    """socket A lists priorities 5 then 1, socket B lists 3: B3, A5, A1 (heads, not the global minimum)"""
    rows = [(0, 0, 5, 100, False), (0, 0, 1, 100, False), (0, 1, 3, 100, False)]
    outs, _ = _tiny(1000, rows, M.FIFO, [10], bootstrap_end=10 * MS, lib=lib)
    assert _send_sequence(outs) == [2, 0, 1]


@BOTH
def test_pin_local_exemption(lib):
    """1000 B/s: refill 1, capacity 1501; 1500-byte packets at 0"""
    p = lambda prio, local=False: (0, 0, prio, 1500, local)  # noqa: E731
    outs, state = _tiny(1000, [p(1), p(2), p(3, True)], M.FIFO, [2000], lib=lib)
    st, sn, rk = outs[0][:3]
    assert sn == [0, 1499 * MS, 1499 * MS]  # the cached packet blocks the local one behind it
    assert rk == [0, 1, M.U64] and st == [SENT | FWD, SENT | FWD | CACHED, SENT | FWD]
    assert state["sent_total"] == 2 and state["balance"] == 0
    outs, state = _tiny(1000, [p(1), p(2, True), p(3)], M.FIFO, [2000], lib=lib)
    st, sn, rk = outs[0][:3]
    assert sn == [0, 0, 1499 * MS] and rk == [0, M.U64, 1]
    assert st == [SENT | FWD, SENT | FWD, SENT | FWD | CACHED]
    assert state["sent_total"] == 2 and state["balance"] == 0  # L took no tokens: 1501 - 1500 + 1499 - 1500


@BOTH
def test_pin_bootstrap_leaves_the_bucket_alone(lib):
    rows = [(k, 0, k + 1, 1500, False) for k in range(6)]
    outs, state = _tiny(1000, rows, M.FIFO, [50], bootstrap_end=50 * MS, lib=lib)
    assert outs[0][1] == [k * MS for k in range(6)] and outs[0][2] == list(range(6))
    assert state["balance"] == 1501 and state["last_refill_ns"] == 0 and state["tasks_scheduled"] == 6


@BOTH
def test_cached_packet_crosses_a_call_and_comes_back_late(lib):
    """1000 B/s, one socket, 1500 / 1500 / 100 bytes at 0: the second packet is cached at 0 with its
    task at 1499 ms, so the first call (until 1000 ms) reports it INTERFACE_SENT | RELAY_CACHED and the
    third still in its socket queue (status 0, pending); the second call forwards both as late records"""
    rows = [(0, 0, 1, 1500, False), (0, 0, 2, 1500, False), (0, 0, 3, 100, False)]
    outs, state = _tiny(1000, rows, M.FIFO, [1000, 1700], lib=lib, refeed=False)
    assert outs[0][:4] == ([SENT | FWD, SENT | CACHED, 0], [0, M.U64, M.U64], [0, M.U64, M.U64], [])
    assert outs[0][5] == 2 and outs[1][5] == 0
    assert outs[1][3] == [(1, 1499 * MS, 1, SENT | FWD | CACHED, 0), (2, 1599 * MS, 2, SENT | FWD | CACHED, 0)]
    assert state["tasks_scheduled"] == 3 and state["sent_total"] == 3


# ------------------------------------------------------------ scenario
def test_scenario_exercises_the_hard_paths():
    """asserted on the model's output alone"""
    sc = S.scenario()
    assert sc["n_hosts"] == 70 and set(sc["bw"].tolist()) == set(S.BANDWIDTHS)
    assert 5500 <= len(sc["pkts"]) <= 6500
    local = (sc["pkts"]["flags"] & 1) != 0
    assert 0.02 < local.mean() < 0.04
    b, e = sc["host_ptr"][S.WIDE_HOST], sc["host_ptr"][S.WIDE_HOST + 1]
    assert len(set(sc["pkts"]["socket"][b:e].tolist())) > 200 and sc["pkts"]["socket"].max() < S.WIDE_SOCKETS
    for h in range(sc["n_hosts"]):
        g = sc["pkts"][sc["host_ptr"][h]:sc["host_ptr"][h + 1]]
        assert (np.diff(g["ready_ns"].astype(np.int64)) >= 0).all() and len(set(g["priority"].tolist())) == len(g)
    # priorities do not increase within every socket
    g = sc["pkts"][sc["host_ptr"][0]:sc["host_ptr"][1]]
    assert any((np.diff(g["priority"][g["socket"] == s].astype(np.int64)) < 0).any() for s in set(g["socket"].tolist()))
    for qdisc in QDISCS:
        calls, outs, m = S.model_results(qdisc)
        st = outs[0]["status"]
        assert ((st & CACHED) != 0).sum() >= 100 and m.pending() > 0
        assert sum(h.ties for h in m.hosts) >= 50                # arrivals at the time of the one before
        assert sum(h.on_blocked_task for h in m.hosts) >= 3      # arrivals exactly on a pending task's time
        assert ((st & FWD) != 0)[local].any() and (outs[0]["rank"][local] == M.U64).all()
        _, souts, sm = S.model_results(qdisc, split=True)
        assert sm.pending() > 0 and sum(len(o["late"]) for o in souts) > 100
        assert any(st_ == SENT | CACHED for o in souts[:-1] for st_ in o["status"].tolist())  # cached across a call
    # the two disciplines really send in different orders
    assert not np.array_equal(S.model_results(M.FIFO)[1][0]["rank"], S.model_results(M.RR)[1][0]["rank"])


@pytest.mark.parametrize("qdisc", QDISCS, ids=["fifo", "rr"])
def test_host_only_one_call_equals_model(qdisc):
    calls, mouts, m = S.model_results(qdisc)
    outs, state, stats = S.run_lib(S.scenario(), calls, qdisc)
    S.assert_same(outs, mouts, state, m)
    assert stats[-1] == (0, m.pending())


@pytest.mark.parametrize("qdisc", QDISCS, ids=["fifo", "rr"])
def test_host_only_split_equals_model_and_one_call(qdisc):
    sc = S.scenario()
    calls, mouts, m = S.model_results(qdisc, split=True)
    outs, state, stats = S.run_lib(sc, calls, qdisc)
    S.assert_same(outs, mouts, state, m)
    assert stats[-1] == (0, m.pending())
    assert [o["late_count"] for o in outs] == [len(mo["late"]) for mo in mouts]
    # split invariance: what was forwarded (status, time, rank), and every host's final state
    c1, _, m1 = S.model_results(qdisc)
    o1, state1, _ = S.run_lib(sc, c1, qdisc)
    assert S.resolved(calls, outs) == S.resolved(c1, o1)
    assert state.tobytes() == state1.tobytes()
    assert m1.state() == m.state()


def test_host_only_ring_filled_to_its_last_slot():
    """queue_cap = the deepest backlog any host has at the end of any call"""
    sc = S.scenario()
    calls, mouts, m = S.model_results(M.RR, split=True)
    m2, deepest = M.OutboundModel(sc["bw"], M.RR, S.MAX_SOCKETS), 0
    for c in calls:
        m2.run(c["pkts"], c["host_ptr"], c["until"], S.BOOTSTRAP_END_NS)
        deepest = max(deepest, max(len(h.iface) for h in m2.hosts))
    assert deepest > 50
    outs, state, stats = S.run_lib(sc, calls, M.RR, queue_cap=deepest)
    S.assert_same(outs, mouts, state, m)
    assert not state["overflow"].any()


# ------------------------------------------------------------ conditions
def test_error_paths():
    from shadow_amd import _lib

    L = _lib.lib()
    err = _lib.SrtErr()
    h = C.c_void_p()
    bw = (C.c_uint64 * 2)(1000, 1000)
    assert L.srt_outbound_create(None, 2, None, 0, 4, 4, C.byref(h), C.byref(err)) == _lib.SRT_ERR_INVALID
    assert L.srt_outbound_create(None, 2, bw, 0, 4, 4, None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert L.srt_outbound_create(None, 2, bw, 2, 4, 4, C.byref(h), C.byref(err)) == _lib.SRT_ERR_INVALID  # qdisc
    assert L.srt_outbound_create(None, 2, bw, 0, 0, 4, C.byref(h), C.byref(err)) == _lib.SRT_ERR_INVALID  # no sockets
    assert L.srt_outbound_create(None, 2, bw, 0, 4, 4, C.byref(h), C.byref(err)) == _lib.SRT_OK
    pk = _pkts([(5, 0, 1, 100, False), (6, 0, 2, 100, False)])
    hp = np.array([0, 1, 2], np.uint32)
    st, sn, rk = np.zeros(2, np.uint32), np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731
    run = lambda hh, pp, until: L.srt_outbound_run(hh, pp, p(hp), 2, until, 0, p(st), p(sn), p(rk), None, 0, None,  # noqa
                                                   None, C.byref(err))
    assert run(None, p(pk), 10 * MS) == _lib.SRT_ERR_INVALID
    assert run(h, None, 10 * MS) == _lib.SRT_ERR_INVALID
    assert L.srt_outbound_status(None, None, None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert L.srt_outbound_state(h, None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert run(h, p(pk), 10 * MS) == _lib.SRT_OK
    assert L.srt_outbound_status(h, None, None, C.byref(err)) == _lib.SRT_OK
    assert (st == SENT | FWD).all() and sn.tolist() == [5 * MS, 6 * MS] and rk.tolist() == [0, 0]
    assert run(h, p(pk), 9 * MS) == _lib.SRT_ERR_INVALID  # a window that ends before the previous one
    # arrivals (5 and 6 ms) earlier than the previous call's until_ns (10 ms): TIME_REGRESSION at the status call
    assert run(h, p(pk), 20 * MS) == _lib.SRT_OK
    flags = C.c_uint32()
    assert L.srt_outbound_status(h, C.byref(flags), None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert flags.value == _lib.OUTBOUND_TIME_REGRESSION and b"earlier" in err.msg
    assert L.srt_outbound_status(h, C.byref(flags), None, C.byref(err)) == _lib.SRT_OK  # cleared with the report
    L.srt_outbound_destroy(h)
    L.srt_outbound_destroy(None)


def test_arrivals_at_or_after_until_are_flagged_not_lost():
    from shadow_amd import _lib

    rows = [(5, 0, 1, 100, False), (6, 1, 2, 100, False), (7, 0, 3, 100, False)]
    outs, state = _tiny(125_000_000, rows, M.FIFO, [1, 6, 8])
    done = SENT | FWD
    assert outs[0] == ([0, 0, 0], [M.U64] * 3, [M.U64] * 3, [], _lib.OUTBOUND_AFTER_UNTIL, 0)
    assert outs[1] == ([done, 0, 0], [5 * MS, M.U64, M.U64], [0, M.U64, M.U64], [], _lib.OUTBOUND_AFTER_UNTIL, 0)
    assert outs[2] == ([done, done], [6 * MS, 7 * MS], [1, 2], [], 0, 0)
    assert state["tasks_scheduled"] == 3 and state["queue_len"] == 0 and state["sent_total"] == 3
    mouts, _ = _tiny(125_000_000, rows, M.FIFO, [1, 6, 8], lib=False)
    assert [o[:4] for o in mouts] == [o[:4] for o in outs]


def test_bad_socket_is_flagged_and_not_taken():
    from shadow_amd import _lib

    rows = [(1, 0, 1, 100, False), (2, 4, 2, 100, False), (3, 3, 3, 100, False)]
    outs, state = _tiny(125_000_000, rows, M.RR, [10], max_sockets=4)
    done = SENT | FWD
    assert outs[0] == ([done, 0, done], [1 * MS, M.U64, 3 * MS], [0, M.U64, 1], [], _lib.OUTBOUND_BAD_SOCKET, 0)
    assert state["sent_total"] == 2 and state["tasks_scheduled"] == 2 and state["queue_len"] == 0


def test_oversize_packet_is_flagged_and_the_call_ends():
    """a non-local packet larger than the bucket's capacity (refill 1 + 1500) can never conform: its
    task is tried once a call, parked at until_ns, and the call is flagged; a local one is exempt"""
    from shadow_amd import _lib

    rows = [(5, 0, 1, 2000, True), (5, 0, 2, 2000, False), (6, 1, 3, 100, False)]
    outs, state = _tiny(1000, rows, M.FIFO, [10_000])
    assert outs[0][0] == [SENT | FWD, SENT | CACHED, 0] and outs[0][1] == [5 * MS, M.U64, M.U64]
    assert outs[0][4] == _lib.OUTBOUND_OVERSIZE and outs[0][5] == 2
    assert state["cached"] == 1 and state["queue_len"] == 1 and state["task_ns"] == 10_000 * MS
    assert state["balance"] == 1501
    # a packet of exactly the capacity does conform
    outs, state = _tiny(1000, [(5, 0, 1, 1501, False)], M.FIFO, [10_000])
    assert outs[0][:3] == ([SENT | FWD], [5 * MS], [0]) and outs[0][4:] == (0, 0)


def test_late_overflow_is_reported():
    from shadow_amd import _lib

    sc = S.scenario()
    calls, mouts, _ = S.model_results(M.FIFO, split=True)
    outs, _, stats = S.run_lib(sc, calls, M.FIFO, late_cap=2, check=False)
    assert any(f & _lib.OUTBOUND_LATE_OVERFLOW for f, _ in stats)
    assert [o["late_count"] for o in outs] == [len(mo["late"]) for mo in mouts]


@pytest.mark.parametrize("qdisc", QDISCS, ids=["fifo", "rr"])
def test_ring_overflow_is_reported_and_contained(qdisc):
    """queue_cap 4: host 1 overflows, is flagged and marked; hosts 0 and 2 still equal the model"""
    from shadow_amd import _lib

    sc, calls, mouts, m = S.overflow_case(qdisc)
    outs, state, stats = S.run_lib(sc, calls, qdisc, max_sockets=4, queue_cap=4, bootstrap_end=0, check=False)
    assert stats[0][0] & _lib.OUTBOUND_RING_OVERFLOW
    assert state["overflow"].tolist() == [0, 1, 0]
    S.assert_same(outs, mouts, state, m, calls=calls, sc=sc, hosts={0, 2})


# ------------------------------------------------------------- the kernel
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_outbound_kernels_use_no_scratch():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shadow_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
           os.path.join(csrc, "srt_outbound.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=csrc)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"remark:\s+Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]:\s+(\d+)", out.stderr)]
    assert any("outbound_step_kernel" in n for n in names) and len(names) == len(scratch) >= 2
    assert not any(scratch), dict(zip(names, scratch))
