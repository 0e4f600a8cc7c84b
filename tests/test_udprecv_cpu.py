"""UDP receive stage (srt_udprecv: the sockets' receive buffers and reads behind
srt_deliver_run) without a GPU: the host-only instance -- the same step the
device kernels compile -- against the plain-Python model on the seven-window
scenarios and the hand-worked cases of tests/golden/udprecv_cases.json, one call
against the same window cut in two, the error paths on raw ctypes, the header's
records against the Python dtypes, the kernels' resource report, and the step
header under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/asan/udprecv_check.cpp, a stand-alone program)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import udprecv_model as M
import udprecv_scenario as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEEDS_HIPCC = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC),
                                 reason="hipcc not available")


def test_scenario_exercises_every_rule():
    """asserted on the generator and the model's output alone: an empty scenario cannot pass"""
    st = T.assert_scenario_is_not_empty(130, T.DENSE)
    assert st["armed_same_call"] > 100 and st["armed_later_call"] > 100, st
    sc = T.scenario(130, T.DENSE)
    per = np.diff(sc["socket_ptr"].astype(np.int64))
    # a host with more sockets than a wave has lanes, one with none, one whose slots straddle a wave's end
    assert per.max() > 64 and (per == 0).any() and len(sc["windows"]) == T.N_WIN == 7
    sp = sc["socket_ptr"].astype(np.int64)
    assert any(sp[h] // 64 != (sp[h + 1] - 1) // 64 for h in range(130) if per[h] and per[h] <= 64)
    # the model flags nothing: the comparisons exclude no socket
    assert not sc["model"].state()["overflow"].any()
    for n_hosts in (63, 64, 65):
        T.assert_scenario_is_not_empty(n_hosts, T.DENSE)


@pytest.mark.parametrize("shape", [T.DENSE, T.SPARSE])
@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 130])
def test_host_only_equals_model(n_hosts, shape):
    outs, st, status = T.run_scenario(None, n_hosts, shape)
    m_outs, m_st, m_status, _ = T.model_scenario(n_hosts, shape)
    assert status == m_status and status[0] == 0 and len(outs) == len(m_outs) == 7
    for k, (a, b) in enumerate(zip(outs, m_outs)):
        T.same_outputs(a, b, k)
    T.same_state(st, m_st)


@pytest.mark.parametrize("case", T.golden_cases(), ids=lambda c: c["name"])
def test_golden_case(case):
    wins = T.golden_windows(case)
    outs, st, status = T.run_scenario(None, 0, None, wins, case["socket_ptr"])
    assert status[0] == 0
    T.check_golden(case, outs, st)
    m_outs, m_st, m_status, _ = T.model_scenario(0, None, wins, case["socket_ptr"])
    T.check_golden(case, m_outs, m_st)
    assert m_status == status


def test_golden_cases_cover_the_issue():
    names = " ".join(c["name"] for c in T.golden_cases())
    for k in ("soft_limit_9_5_1", "zero_length", "peer_mismatch", "trunc", "peek", "set_rcvbuf_0_1024_2pow30",
              "lowered", "blocked_read"):
        assert k in names


def test_one_call_equals_split_calls():
    T.one_call_against_split(None)


def test_chain_of_host_only_stages_equals_the_chained_models():
    """inbound router -> interface receive -> UDP sockets, host-only, each stage on the one before's arrays"""
    T.chain(None)


def test_error_paths_on_raw_ctypes():
    from shadow_amd import _lib

    L = _lib.lib()
    err = _lib.SrtErr()
    h = C.c_void_p()
    sp = np.array([0, 2, 3], np.uint32)
    INVALID = _lib.SRT_ERR_INVALID

    def create(ptr, n_hosts=2, ring_cap=4, note_cap=8, hint=0):
        return L.srt_udprecv_create(None, n_hosts, ptr.ctypes.data, ring_cap, note_cap, hint, C.byref(h), C.byref(err))

    assert L.srt_udprecv_create(None, 2, None, 4, 8, 0, C.byref(h), C.byref(err)) == INVALID
    assert L.srt_udprecv_create(None, 2, sp.ctypes.data, 4, 8, 0, None, C.byref(err)) == INVALID
    assert create(np.array([1, 2, 3], np.uint32)) == INVALID and not h.value  # not 0-based
    assert create(np.array([0, 3, 2], np.uint32)) == INVALID and b"nondecreasing" in err.msg
    assert create(np.array([0, 2, 1 << 31], np.uint32)) == INVALID
    assert create(sp, ring_cap=1 << 31) == INVALID and create(sp, note_cap=(1 << 31) + 1) == INVALID
    assert create(sp, hint=1 << 31) == INVALID
    assert create(sp) == _lib.SRT_OK and h.value
    state = np.zeros(3, M.STATE)
    ops = np.array([(M.OPEN, 0, 100), (M.OPEN, 3, 100)], M.OP)
    assert L.srt_udprecv_config(h, ops.ctypes.data, 2, C.byref(err)) == INVALID and b"nothing was changed" in err.msg
    ops = np.array([(M.OPEN, 0, 100), (9, 1, 100)], M.OP)
    assert L.srt_udprecv_config(h, ops.ctypes.data, 2, C.byref(err)) == INVALID
    assert L.srt_udprecv_config(h, None, 2, C.byref(err)) == INVALID
    assert L.srt_udprecv_state(h, state.ctypes.data, C.byref(err)) == _lib.SRT_OK and not state["open"].any()
    assert (state["armed_seq"] == M.U64).all() and (state["last_read_recv_ns"] == M.U64).all()
    # a step on a slot that is not open is ignored; OPEN then the rest in list order
    ops = np.array([(M.SET_RCVBUF, 1, 4000), (M.OPEN, 0, 100), (M.SET_PEER, 0, 7 | 9 << 32), (M.OPEN, 2, 5)], M.OP)
    assert L.srt_udprecv_config(h, ops.ctypes.data, 4, C.byref(err)) == _lib.SRT_OK
    L.srt_udprecv_state(h, state.ctypes.data, C.byref(err))
    assert list(state["open"]) == [1, 0, 1] and state["soft_limit"][1] == 0 and state["peer_ip_be"][0] == 7 and \
        state["peer_port_be"][0] == 9
    # note: the ring's rule
    meta = np.zeros(4, M.META)
    assert L.srt_udprecv_note(h, None, 4, 0, C.byref(err)) == INVALID
    assert L.srt_udprecv_note(h, meta.ctypes.data, 4, 10, C.byref(err)) == _lib.SRT_OK
    assert L.srt_udprecv_note(h, meta.ctypes.data, 4, 13, C.byref(err)) == INVALID and b"tag_base" in err.msg
    assert L.srt_udprecv_note(h, meta.ctypes.data, 1 << 31, 14, C.byref(err)) == INVALID
    # run: null arguments, the sizes, until_ns going back
    hp = np.array([0, 2, 3], np.uint32)
    sock = np.array([0, 1, 2], np.uint32)
    fwd = np.array([5, 6, 7], np.uint64)
    tag = np.array([10, 11, 2], np.uint64)  # tag 2: not in the ring
    status = np.full(3, T.HIT, np.uint32)
    rp = np.array([0, 3, 4], np.uint32)
    reads = np.array([(1, 0, 10, 0, 0), (50, 1, 10, 0, 0), (3, 9, 10, 0, 0), (200, 2, 10, M.WAIT, 0)], M.READ)
    rx = np.zeros(3, np.uint32)
    res = np.zeros(4, M.RESULT)
    late = np.zeros(1, M.LATE)
    n_late = np.zeros(1, np.uint32)
    first = np.zeros(3, np.uint64)
    base = C.c_uint64(99)

    def run(until, host_ptr=hp.ctypes.data, n_reads=4, first_p=first.ctypes.data, late_cap=1):
        return L.srt_udprecv_run(h, host_ptr, sock.ctypes.data, fwd.ctypes.data, tag.ctypes.data, status.ctypes.data, 3,
                                 rp.ctypes.data, reads.ctypes.data, n_reads, C.byref(base), until, rx.ctypes.data,
                                 res.ctypes.data, late.ctypes.data, late_cap, n_late.ctypes.data, first_p, C.byref(err))

    assert run(100, host_ptr=None) == INVALID and run(100, first_p=None) == INVALID
    assert run(100, n_reads=1 << 31) == INVALID and run(100, late_cap=1 << 31) == INVALID
    assert base.value == 99
    assert run(100) == _lib.SRT_OK and base.value == 0
    # slot 0 is connected to 7:9 and the packet comes from 0:0; slot 1 is not open: its record passes through
    # and its read is -EBADF; slot 9 does not exist; host 1's read at 200 lies past until_ns; slot 2's tag is
    # not in the ring
    assert list(rx) == [T.HIT | M.PROCESSED | M.DROPPED, T.HIT, T.HIT]
    assert list(res["return_val"]) == [-M.EWOULDBLOCK, -M.EBADF, -M.EBADF, 0]
    assert list(res["status"]) == [M.DONE, M.DONE, M.DONE, M.NOT_TAKEN]
    flags = C.c_uint32()
    n = [C.c_uint64(), C.c_uint64(), C.c_uint64()]
    assert L.srt_udprecv_status(h, C.byref(flags), *[C.byref(x) for x in n], C.byref(err)) == INVALID
    assert flags.value == M.F_NOTE_OVERRUN | M.F_BAD_SOCKET | M.F_READ_ORDER and [x.value for x in n] == [1, 0, 1]
    for word in (b"note overrun", b"bad socket", b"out of order"):
        assert word in err.msg, err.msg
    assert L.srt_udprecv_status(h, C.byref(flags), None, None, None, C.byref(err)) == _lib.SRT_OK and not flags.value
    L.srt_udprecv_state(h, state.ctypes.data, C.byref(err))
    assert state["overflow"][2] == M.MARK_NOTE and list(first) == [M.U64] * 3
    assert run(99) == INVALID and b"until_ns" in err.msg
    assert run(100, n_reads=0) == _lib.SRT_OK and base.value == 4
    L.srt_udprecv_destroy(h)
    L.srt_udprecv_destroy(None)
    # no hosts, no sockets
    z = np.zeros(1, np.uint32)
    assert L.srt_udprecv_create(None, 0, z.ctypes.data, 0, 0, 0, C.byref(h), C.byref(err)) == _lib.SRT_OK
    assert L.srt_udprecv_run(h, z.ctypes.data, None, None, None, None, 0, None, None, 0, None, 5, None, None, None, 0,
                             None, None, C.byref(err)) == _lib.SRT_OK
    assert L.srt_udprecv_status(h, C.byref(flags), None, None, None, C.byref(err)) == _lib.SRT_OK
    L.srt_udprecv_destroy(h)


def test_ring_overflow_marks_the_socket_only():
    """ring_cap 2: the third message still buffered at the end of a call is lost, its socket marked"""
    wins = T.golden_windows(dict(socket_ptr=[0, 2], calls=[dict(
        ops=[[1, 0, 1000], [1, 1, 1000]], until=1000,
        pushes=[[0, 0, 10, 1, 1, 1], [0, 0, 20, 2, 1, 1], [0, 0, 30, 3, 1, 1], [0, 0, 40, 4, 1, 1], [0, 1, 50, 5, 1, 1]],
        reads=[[0, 25, 0, 100, 0]])]))
    outs, st, status = T.run_scenario(None, 0, None, wins, [0, 2], ring_cap=2)
    m_outs, m_st, m_status, _ = T.model_scenario(0, None, wins, [0, 2], ring_cap=2)
    assert status == m_status and status[0] == M.F_RING_OVERFLOW
    T.same_outputs(outs[0], m_outs[0])
    T.same_state(st, m_st)
    assert list(st["overflow"]) == [M.MARK_RING, 0] and list(st["n_msgs"]) == [2, 1]
    assert outs[0]["results"]["return_val"][0] == 1  # inside the call the queue held three


def test_records_match_the_header():
    src = open(os.path.join(ROOT, "include", "srt.h")).read()
    from shadow_amd import plan as P

    ctype = {"uint64_t": "<u8", "int64_t": "<i8", "uint32_t": "<u4", "uint16_t": "<u2", "uint8_t": "u1"}
    for name, dtype, size in (("srt_udp_meta", P.UDP_META_DTYPE, 16), ("srt_udp_read", P.UDP_READ_DTYPE, 24),
                              ("srt_udp_result", P.UDP_RESULT_DTYPE, 56), ("srt_udprecv_op", P.UDP_OP_DTYPE, 16),
                              ("srt_udprecv_socket_state", P.UDP_STATE_DTYPE, 48)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, src).group(1)
        fields = [(f, ctype[t]) for t, f in re.findall(r"^\s*(u?int\d+_t) (\w+);", body, re.M)]
        assert np.dtype(fields) == dtype and dtype.itemsize == size, name
    assert P.UDP_LATE_DTYPE.itemsize == 64 and P.UDP_LATE_DTYPE == M.LATE
    for a, b in ((P.UDP_META_DTYPE, M.META), (P.UDP_READ_DTYPE, M.READ), (P.UDP_RESULT_DTYPE, M.RESULT),
                 (P.UDP_OP_DTYPE, M.OP), (P.UDP_STATE_DTYPE, M.STATE)):
        assert a == b
    from shadow_amd import _lib

    for k, v in (("SRT_PDS_RCV_SOCKET_PROCESSED = 1u << 15", _lib.PDS_RCV_SOCKET_PROCESSED == M.PROCESSED == 1 << 15),
                 ("SRT_PDS_RCV_SOCKET_DROPPED = 1u << 16", _lib.PDS_RCV_SOCKET_DROPPED == M.DROPPED == 1 << 16),
                 ("SRT_PDS_RCV_SOCKET_BUFFERED = 1u << 18", _lib.PDS_RCV_SOCKET_BUFFERED == M.BUFFERED == 1 << 18)):
        assert k in src and v
    for name, v in (("UDP_PEEK", M.PEEK), ("UDP_TRUNC", M.TRUNC), ("UDP_WAIT", M.WAIT),
                    ("UDPRECV_RING_OVERFLOW", M.F_RING_OVERFLOW), ("UDPRECV_LATE_OVERFLOW", M.F_LATE_OVERFLOW),
                    ("UDPRECV_NOTE_OVERRUN", M.F_NOTE_OVERRUN), ("UDPRECV_BAD_SOCKET", M.F_BAD_SOCKET),
                    ("UDPRECV_READ_ORDER", M.F_READ_ORDER), ("UDPRECV_ARMED_TWICE", M.F_ARMED_TWICE),
                    ("UDPRECV_OPEN", M.OPEN), ("UDPRECV_CLOSE", M.CLOSE), ("UDPRECV_SET_PEER", M.SET_PEER),
                    ("UDPRECV_SET_RCVBUF", M.SET_RCVBUF)):
        assert getattr(_lib, name) == v
        assert int(re.search(r"#define SRT_%s\s+(0x[0-9a-fA-F]+|\d+)u" % name, src).group(1), 0) == v, name


@NEEDS_HIPCC
def test_udprecv_kernels_use_no_scratch_and_half_a_cu_of_lds():
    csrc = os.path.join(ROOT, "shadow_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
           os.path.join(csrc, "srt_udprecv.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=csrc)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"remark:\s+Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]:\s+(\d+)", out.stderr)]
    lds = [int(x) for x in re.findall(r"remark:\s+LDS Size \[bytes/block\]:\s+(\d+)", out.stderr)]
    for k in ("udprecv_note_kernel", "udprecv_config_kernel", "udprecv_stage_kernel", "udprecv_step_kernel",
              "udprecv_sum_kernel"):
        assert any(k in n for n in names), (k, names)
    assert len(names) == len(scratch) == len(lds) == 5
    assert not any(scratch), dict(zip(names, scratch))
    # the step kernel's LDS is its window, asked for at launch: with its static part, within half of a CU's 160 KB
    from shadow_amd.plan import UdpReceive

    static = [v for n, v in zip(names, lds) if "udprecv_step_kernel" in n][0]
    assert static % 16 == 0 and 0 < static + UdpReceive.window_bytes() <= 80 * 1024
    assert UdpReceive.window_bytes() % 32 == 0


@NEEDS_HIPCC
def test_step_header_under_asan_ubsan(tmp_path):
    """tests/asan/udprecv_check.cpp over srt_udprecv_step.h and its host-only entry points, host arrays sized
    exactly, built for the host with -fsanitize=address,undefined and run directly"""
    exe = str(tmp_path / "udprecv_check")
    cmd = [HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "asan", "udprecv_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "udprecv_check: clean" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
