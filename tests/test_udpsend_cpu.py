"""UDP send side (srt_udpsend: the sockets' send buffers fused with the outbound
relay) without a GPU: the host-only instance -- the same step the device kernel
compiles -- against the plain-Python model on the seven-window scenarios and the
hand-worked cases of tests/golden/udpsend_cases.json, one call against the same
window cut in two, a raw-only list against srt_outbound_run byte for byte, every
flag raised by its smallest input, the header's records against the Python
dtypes, and the step header under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/asan/udpsend_check.cpp, a stand-alone program)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import udpsend_model as M
import udpsend_scenario as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEEDS_HIPCC = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC),
                                 reason="hipcc not available")
A, B = T.ip_of(1), T.ip_of(2)


def test_scenarios_exercise_every_rule():
    """asserted on the generator and the model's output alone: an empty scenario cannot pass"""
    st = T.scenario_stats(T.scenario(130, T.THROTTLED, M.FIFO))
    for k in ("would_block", "armed", "woken_same_call", "woken_later", "late_pkts", "cached", "local", "first_writable"):
        assert st[k] > 50, (k, st)
    st = T.scenario_stats(T.scenario(130, T.FREE, M.FIFO))
    assert st["accepted"] > 5000 and not st["would_block"] and not st["armed"] and not st["cached"], st
    sc = T.scenario(130, T.THROTTLED, M.FIFO)
    per = np.diff(sc["socket_ptr"].astype(np.int64))
    assert set(per) == set(range(6)) and len(sc["windows"]) == T.N_WIN == 7
    assert (sc["bw"] >= 1000).all() and (sc["bw"] <= 100000).all()


@pytest.mark.parametrize("qdisc", [M.FIFO, M.RR])
@pytest.mark.parametrize("shape", [T.FREE, T.THROTTLED])
@pytest.mark.parametrize("n_hosts", [1, 64, 65, 130])
def test_host_only_equals_model(n_hosts, shape, qdisc):
    status = T.compare(None, T.scenario(n_hosts, shape, qdisc))
    assert not status[0] & (M.F_RING_OVERFLOW | M.F_LATE_OVERFLOW | M.F_LATE_RESULT_OVERFLOW)


@pytest.mark.parametrize("case", T.golden_cases(), ids=lambda c: c["name"])
def test_golden_case(case):
    sc = T.golden_scenario(case)
    outs, st, status = T.run_scenario(None, sc)
    T.check_golden(case, outs, st, status)
    m_outs, m_st, m_status = T.model_scenario(sc)
    T.check_golden(case, m_outs, m_st, m_status)
    for k, (a, b) in enumerate(zip(outs, m_outs)):
        T.same_outputs(a, b, k)
    T.same_state(st, m_st)
    assert status == m_status


def test_golden_cases_cover_the_issue():
    cases = T.golden_cases()
    names = " ".join(c["name"] for c in cases)
    for k in ("throttled_host", "soft_limit", "error_order", "unspecified_source", "fifo_two", "round_robin_two",
              "later_call", "close_with", "set_sndbuf", "raw_arrivals"):
        assert k in names
    assert all(len(c["comment"]) > 200 for c in cases)


def test_one_call_equals_split_calls():
    T.one_call_against_split(None)


def test_raw_only_list_equals_outbound_byte_for_byte():
    """the same arrivals through srt_outbound_run and, as raw arrivals, through srt_udpsend_run"""
    from shadow_amd.plan import OUTBOUND_LATE_DTYPE, OutboundRelay, UdpSend

    for qdisc in (M.FIFO, M.RR):
        sp, ips, bw, wins = T.raw_only()
        ob = OutboundRelay(None, bw, qdisc, 3, 4096)
        us = UdpSend(None, sp, ips, bw, qdisc, 4096)
        n_fwd = 0
        for w in wins:
            pk, hp = w["pkts"], w["host_ptr"]
            n = len(pk)
            a = [np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(4096, OUTBOUND_LATE_DTYPE),
                 np.zeros(1, np.uint32)]
            b = [np.ones(n, np.uint32), np.ones(n, np.uint64), np.ones(n, np.uint64), np.zeros(4096, OUTBOUND_LATE_DTYPE),
                 np.ones(1, np.uint32)]
            base_a = ob.run(pk.view(np.uint8), hp, w["until_ns"], 0, a[0], a[1], a[2], a[3].view(np.uint8), a[4])
            base_b = us.run(hp, T.raw_calls(pk, hp, sp), w["until_ns"], 0, np.zeros(40 * n, np.uint8), b[0], b[1], b[2],
                            b[3].view(np.uint8), b[4], None, None, np.zeros(len(sp) * 3, np.uint64))
            assert base_a == base_b and a[4][0] == b[4][0]
            for x, y in zip(a[:3], b[:3]):
                assert x.tobytes() == y.tobytes()
            k = int(a[4][0])
            assert np.sort(a[3][:k], order="seq").tobytes() == np.sort(b[3][:k], order="seq").tobytes()
            n_fwd += int((a[0] & M.FORWARDED != 0).sum()) + k
        sa = ob.state()
        hb, _ = us.state()
        for k in sa.dtype.names:
            assert sa[k].tobytes() == hb[k].tobytes(), k
        assert hb["next_priority"].tolist() == [1] * len(bw)
        assert ob.status() == us.status()[:2] and n_fwd > 1000
        seq_a, seq_b = np.zeros(len(bw), np.uint64), np.ones(len(bw), np.uint64)
        ob.cached_seq(seq_a), us.cached_seq(seq_b)
        assert seq_a.tobytes() == seq_b.tobytes()
        ob.close(), us.close()


def one_host(sends, ops=(), until=10 ** 9, ring_cap=8, late_cap=16, n_slots=2, bw=10 ** 9, calls2=None, ops2=(), late_cap2=None,
             until2=None):
    """one host A with n_slots slots, slot 0 open, bound and connected to B unless `ops` says otherwise; rows
    [time, slot, len, dst, flags, priority]; -> (outs, state, status)"""
    base_ops = [(M.OPEN, 0, 4096), (M.BIND, 0, A | 5000 << 32), (M.SET_PEER, 0, B | 5000 << 32)]
    wins = []
    for rows, o, unt in ((sends, base_ops + list(ops), until),) + (((calls2, list(ops2), until2 or 2 * until),) if calls2 is not None else ()):
        calls = np.zeros(len(rows), M.SEND)
        for k, r in enumerate(rows):
            r = list(r) + [0] * (6 - len(r))
            calls[k] = (r[0], r[5], r[1], r[2], r[3], 0, 0, r[4], k)
        wins.append(dict(ops=np.array(o, M.OP) if o else np.zeros(0, M.OP), calls=calls,
                         host_ptr=np.array([0, len(rows)], np.uint32), until_ns=unt))
    sc = dict(socket_ptr=np.array([0, n_slots], np.uint32), ips=np.array([A], np.uint32), bw=np.array([bw], np.uint64),
              qdisc=M.FIFO, windows=wins)
    r = T.Runner(None, sc, ring_cap, late_cap)
    outs = []
    for k, w in enumerate(wins):
        if k and late_cap2 is not None:
            r.late_cap = late_cap2
        outs.append(r.window(w))
    st, status = r.finish()
    m = M.UdpSendModel(sc["socket_ptr"], sc["ips"], sc["bw"], M.FIFO, ring_cap)
    for w, o in zip(wins, outs):
        m.config(w["ops"])
        mo = m.run(w["calls"], w["host_ptr"], w["until_ns"], 0)
        if not status[0] & (M.F_LATE_OVERFLOW | M.F_LATE_RESULT_OVERFLOW):
            T.same_outputs(o, mo)
    assert m.take_status()[0] == status[0] & ~(M.F_LATE_OVERFLOW | M.F_LATE_RESULT_OVERFLOW)  # the model has no caps
    return outs, st, status


def test_every_flag_is_raised_by_its_smallest_input():
    ok = [0, 0, 10, 0, 0]
    # nothing wrong: no flag
    outs, st, status = one_host([ok])
    assert status[0] == 0 and outs[0]["results"]["return_val"][0] == 10
    # RING_OVERFLOW: ring_cap 1 and two messages still queued at the end of the call (the host's bucket holds 1501)
    outs, st, status = one_host([[0, 0, 1000], [0, 0, 1000], [0, 0, 1000], [0, 0, 1000]], bw=1000, ring_cap=1, until=1000)
    assert status[0] == M.F_RING_OVERFLOW and st[1]["overflow"][0] == 1 and st[0]["overflow"][0] == 1
    assert st[1]["n_msgs"][0] == 1 and st[0]["queue_len"][0] == 1
    # LATE_OVERFLOW: two packets forwarded in the second call, late_cap 1 there
    outs, st, status = one_host([[0, 0, 1400], [0, 0, 1400], [0, 0, 1400]], bw=10 ** 6, until=500_000, calls2=[],
                                late_cap2=1, until2=10 ** 9)
    assert status[0] == M.F_LATE_OVERFLOW and len(outs[1]["late"]) == 1 and st[0]["sent_total"][0] == 3
    # LATE_RESULT_OVERFLOW: an armed send of the first call wakes in the second, which has room for no late result
    # (the relay is pending from t = 0 on, so the socket fills at t = 1000 without a pop in between)
    held = [[0, 0, 1472], [0, 0, 1472]]
    sends = held + [[1000, 0, 1472], [1000, 0, 1472], [1000, 0, 1472], [1000, 0, 100, 0, M.WAIT]]
    outs, st, status = one_host(sends, bw=10 ** 6, until=500_000, calls2=[], late_cap2=0, until2=10 ** 9)
    assert outs[0]["results"]["status"][5] == M.ARMED
    assert status[0] == M.F_LATE_OVERFLOW | M.F_LATE_RESULT_OVERFLOW and st[1]["armed_seq"][0] == M.U64
    assert st[0]["next_priority"][0] == 7  # the woken send was accepted; only its record was lost
    # TIME_REGRESSION: a call of the second window before the first one's until_ns; CALL_ORDER: a call before the one ahead
    outs, st, status = one_host([ok], until=1000, calls2=[[999, 0, 10]])
    assert status[0] == M.F_TIME_REGRESSION and outs[1]["results"]["status"][0] == M.NOT_TAKEN
    outs, st, status = one_host([[5, 0, 10], [4, 0, 10]])
    assert status[0] == M.F_CALL_ORDER and list(outs[0]["results"]["status"]) == [M.DONE, M.NOT_TAKEN]
    # AFTER_UNTIL
    outs, st, status = one_host([[1000, 0, 10]], until=1000)
    assert status[0] == M.F_AFTER_UNTIL and outs[0]["results"]["status"][0] == M.NOT_TAKEN and outs[0]["status"][0] == 0
    # OVERSIZE: a packet of 1502 bytes on a host whose bucket holds 1501
    outs, st, status = one_host([[0, 0, 1474]], bw=1000, until=10 ** 7)
    assert status[0] == M.F_OVERSIZE and st[0]["cached"][0] == 1 and st[0]["task_ns"][0] == 10 ** 7
    # BAD_SOCKET: a slot that is not open; a slot of no host; a raw arrival on an open slot
    for row, val, stt in (([0, 1, 10], -M.EBADF, M.DONE), ([0, 7, 10], -M.EBADF, M.DONE), ([0, 0, 10, 0, M.RAW, 3], 0, M.NOT_TAKEN)):
        outs, st, status = one_host([row])
        assert status[0] == M.F_BAD_SOCKET and outs[0]["results"]["return_val"][0] == val and \
            outs[0]["results"]["status"][0] == stt and st[0]["tasks_scheduled"][0] == 0
    # UNBOUND, LOOPBACK (by destination, by binding)
    outs, st, status = one_host([[0, 1, 10, B, M.HAS_ADDR]], ops=[(M.OPEN, 1, 4096)])
    assert status[0] == M.F_UNBOUND and outs[0]["results"]["status"][0] == M.NOT_TAKEN
    outs, st, status = one_host([[0, 0, 10, M.LOCALHOST, M.HAS_ADDR]])
    assert status[0] == M.F_LOOPBACK and outs[0]["results"]["status"][0] == M.NOT_TAKEN
    outs, st, status = one_host([ok], ops=[(M.BIND, 0, M.LOCALHOST | 5000 << 32)])
    assert status[0] == M.F_LOOPBACK
    # ARMED_TWICE
    sends = held + [[1000, 0, 4096], [1000, 0, 10, 0, M.WAIT], [1000, 0, 10, 0, M.WAIT]]
    outs, st, status = one_host(sends, bw=10 ** 6, until=500_000)
    assert status[0] == M.F_ARMED_TWICE and list(outs[0]["results"]["status"]) == [M.DONE] * 3 + [M.ARMED, M.DONE]
    assert outs[0]["results"]["return_val"][4] == -M.EWOULDBLOCK and st[1]["armed_seq"][0] == 3
    # REOPEN_BUSY
    outs, st, status = one_host([[0, 0, 1000], [0, 0, 1000], [0, 0, 1000]], bw=1000, until=1000, calls2=[], ops2=[(M.OPEN, 0, 9)])
    assert status[0] == M.F_REOPEN_BUSY and st[1]["soft_limit"][0] == 4096


def test_error_paths_on_raw_ctypes():
    from shadow_amd import _lib

    L = _lib.lib()
    err = _lib.SrtErr()
    h = C.c_void_p()
    sp = np.array([0, 2, 3], np.uint32)
    ips = np.array([A, B], np.uint32)
    bw = np.array([1000, 1000], np.uint64)
    INVALID = _lib.SRT_ERR_INVALID

    def create(ptr, qdisc=0, ring_cap=4, hint=0):
        return L.srt_udpsend_create(None, 2, ptr.ctypes.data, ips.ctypes.data, bw.ctypes.data, qdisc, ring_cap, hint,
                                    C.byref(h), C.byref(err))

    assert L.srt_udpsend_create(None, 2, None, ips.ctypes.data, bw.ctypes.data, 0, 4, 0, C.byref(h), C.byref(err)) == INVALID
    assert create(np.array([1, 2, 3], np.uint32)) == INVALID and not h.value
    assert create(np.array([0, 3, 2], np.uint32)) == INVALID and b"nondecreasing" in err.msg
    assert create(sp, qdisc=2) == INVALID and create(sp, hint=1 << 31) == INVALID and create(sp, ring_cap=(1 << 30)) == INVALID
    assert create(sp) == _lib.SRT_OK and h.value
    ops = np.array([(M.OPEN, 0, 100), (M.OPEN, 3, 100)], M.OP)
    assert L.srt_udpsend_config(h, ops.ctypes.data, 2, C.byref(err)) == INVALID and b"nothing was changed" in err.msg
    ops = np.array([(M.OPEN, 0, 100), (8, 1, 100)], M.OP)
    assert L.srt_udpsend_config(h, ops.ctypes.data, 2, C.byref(err)) == INVALID
    ops = np.array([(M.SET_NEXT_PRIORITY, 2, 100)], M.OP)  # the slot names a host
    assert L.srt_udpsend_config(h, ops.ctypes.data, 1, C.byref(err)) == INVALID
    hosts, socks = np.zeros(2, M.HOST_STATE), np.zeros(3, M.SOCK_STATE)
    assert L.srt_udpsend_state(h, hosts.ctypes.data, socks.ctypes.data, C.byref(err)) == _lib.SRT_OK
    assert not socks["open"].any() and (socks["armed_seq"] == M.U64).all() and list(hosts["next_priority"]) == [1, 1]
    assert list(hosts["balance"]) == [1501, 1501] and (hosts["task_ns"] == M.U64).all()
    ops = np.array([(M.SET_SNDBUF, 1, 9000), (M.OPEN, 0, 100), (M.SET_NEXT_PRIORITY, 1, 77)], M.OP)
    assert L.srt_udpsend_config(h, ops.ctypes.data, 3, C.byref(err)) == _lib.SRT_OK
    L.srt_udpsend_state(h, hosts.ctypes.data, socks.ctypes.data, C.byref(err))
    assert list(socks["open"]) == [1, 0, 0] and socks["soft_limit"][1] == 0 and list(hosts["next_priority"]) == [1, 77]
    hp = np.array([0, 0, 0], np.uint32)
    first = np.zeros(3, np.uint64)
    base = C.c_uint64(99)

    def run(until, host_ptr=hp.ctypes.data, first_p=first.ctypes.data, n=0, late_cap=0):
        return L.srt_udpsend_run(h, host_ptr, None, n, until, 0, None, None, None, None, None, late_cap, None, None, 0, None,
                                 first_p, C.byref(base), C.byref(err))

    assert run(100, host_ptr=None) == INVALID and run(100, first_p=None) == INVALID and run(100, n=1) == INVALID
    assert run(100, late_cap=1) == INVALID and base.value == 99
    assert run(100) == _lib.SRT_OK and base.value == 0 and list(first) == [M.U64] * 3
    assert run(99) == INVALID and b"until_ns" in err.msg
    flags = C.c_uint32(5)
    assert L.srt_udpsend_status(h, C.byref(flags), None, None, None, None, C.byref(err)) == _lib.SRT_OK and not flags.value
    L.srt_udpsend_destroy(h)
    L.srt_udpsend_destroy(None)
    z = np.zeros(1, np.uint32)
    assert L.srt_udpsend_create(None, 0, z.ctypes.data, None, None, 0, 0, 0, C.byref(h), C.byref(err)) == _lib.SRT_OK
    assert L.srt_udpsend_run(h, z.ctypes.data, None, 0, 5, 0, None, None, None, None, None, 0, None, None, 0, None, None,
                             None, C.byref(err)) == _lib.SRT_OK
    L.srt_udpsend_destroy(h)


def test_records_match_the_header():
    src = open(os.path.join(ROOT, "include", "srt.h")).read()
    from shadow_amd import _lib
    from shadow_amd import plan as P

    ctype = {"uint64_t": "<u8", "int64_t": "<i8", "uint32_t": "<u4", "uint16_t": "<u2", "uint8_t": "u1"}
    for name, dtype, model, size in (("srt_udp_send", P.UDP_SEND_DTYPE, M.SEND, 40),
                                     ("srt_udpsend_result", P.UDPSEND_RESULT_DTYPE, M.RESULT, 40),
                                     ("srt_udpsend_op", P.UDPSEND_OP_DTYPE, M.OP, 16),
                                     ("srt_udpsend_socket_state", P.UDPSEND_SOCKET_STATE_DTYPE, M.SOCK_STATE, 48),
                                     ("srt_udpsend_host_state", P.UDPSEND_HOST_STATE_DTYPE, M.HOST_STATE, 64)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, src).group(1)
        fields = [(f, ctype[t]) for t, f in re.findall(r"^\s*(u?int\d+_t) (\w+);", body, re.M)]
        assert np.dtype(fields) == dtype == model and dtype.itemsize == size, name
    assert P.UDPSEND_LATE_DTYPE.itemsize == 48 and P.UDPSEND_LATE_DTYPE == M.LATE_RESULT and M.LATE == P.OUTBOUND_LATE_DTYPE
    assert "SRT_PDS_SND_CREATED = 1u << 1" in src and _lib.PDS_SND_CREATED == M.SND_CREATED == 2
    for name in ("HAS_ADDR", "WAIT", "RAW", "LOCAL", "NOT_TAKEN", "DONE", "ARMED", "OPEN", "CLOSE", "BIND", "SET_PEER",
                 "SET_SNDBUF", "SHUT_WR", "SET_NEXT_PRIORITY", "F_RING_OVERFLOW", "F_LATE_OVERFLOW", "F_TIME_REGRESSION",
                 "F_OVERSIZE", "F_AFTER_UNTIL", "F_BAD_SOCKET", "F_UNBOUND", "F_LOOPBACK", "F_ARMED_TWICE", "F_REOPEN_BUSY",
                 "F_LATE_RESULT_OVERFLOW", "F_CALL_ORDER"):
        v = getattr(M, name)
        plain = name[2:] if name.startswith("F_") else name
        assert getattr(_lib, "UDPSEND_" + plain) == v, name
        assert int(re.search(r"#define SRT_UDPSEND_%s\s+(0x[0-9a-fA-F]+|\d+)u" % plain, src).group(1), 0) == v, name


@NEEDS_HIPCC
def test_step_header_under_asan_ubsan(tmp_path):
    """tests/asan/udpsend_check.cpp over srt_udpsend_step.h and its host-only entry points, host arrays sized
    exactly, built for the host with -fsanitize=address,undefined and run directly"""
    exe = str(tmp_path / "udpsend_check")
    cmd = [HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "asan", "udpsend_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "udpsend_check: clean" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
