"""Inbound router stage (srt_inbound: CoDel queue + download token bucket per
destination host; router/codel_queue.rs, relay/mod.rs, relay/token_bucket.rs)
without a GPU: the Python model against the reference's own unit-test
scenarios, and the host-only srt_inbound -- the same per-host step the device
kernel compiles -- against the model, bit for bit.
"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import inbound_model as M
import inbound_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "inbound_reference_cases.json")))


# ------------------------------------------------------- the checker itself
def test_model_control_law_golden():
    cl = CASES["control_law"]
    got = [M.control_law_increment(c) for c in cl["counts"]]
    assert got == cl["expected_increment_ns"]
    assert got[0] == got[1] == M.INTERVAL


def _expect(q, want):
    for key, val in want.items():
        if key == "len":
            assert len(q) == val
        elif key == "mode":
            assert q.mode == val
        elif key == "interval_end":
            assert q.interval_end == val
        elif key == "bytes_gt_mtu":
            assert (q.bytes > M.MTU) == val
        elif key == "drop_next_is_some":
            assert (q.drop_next is not None) == val
        elif key in ("was_dropping_recently", "should_drop"):
            assert getattr(q, key)(val[0]) == val[1]
        else:
            assert getattr(q, key) == val, key


@pytest.mark.parametrize("name", sorted(CASES["codel"]))
def test_model_codel_golden(name):
    q, tag = M.CoDelQueue(), 0
    for op in CASES["codel"][name]:
        if op[0] == "push":
            q.push(tag, op[2], op[1])
            tag += 1
        elif op[0] == "pop":
            got = q.pop(op[1])
            if "returns" in op[2]:
                assert (got is not None) == op[2]["returns"]
        elif op[0] == "process_standing_delay":
            assert q.process_standing_delay(op[1], op[2]) == op[3]
        elif op[0] == "set_mode":
            q.mode = op[1]
        else:
            assert op[0] == "expect"
            _expect(q, op[1])


@pytest.mark.parametrize("name", sorted(CASES["token_bucket"]))
def test_model_token_bucket_golden(name):
    tb = None
    for op in CASES["token_bucket"][name]:
        if op[0] == "new":
            tb = M.TokenBucket(*op[1:])
        elif op[0] == "remove":
            verdict, val = tb.remove(op[1], op[2])
            assert {verdict: val} == op[3]
            if verdict == "ok":
                assert val == tb.balance
        else:
            assert op[0] == "expect_balance" and tb.balance == op[1]


def test_scenario_exercises_the_hard_paths():
    """asserted on the model's output alone"""
    sc = S.scenario()
    assert len(sc["bw"]) == 130 and set(sc["bw"].tolist()) == set(S.BANDWIDTHS)
    assert not (sc["dst"][sc["sent"]] == S.EMPTY_HOST).any()
    assert 0 < S.BOOTSTRAP_END_NS < S.SPAN_NS
    calls, outs, m = S.model_results()
    st = outs[0]["status"]
    assert ((st & M.DROPPED) != 0).sum() >= 50
    assert ((st & M.CACHED) != 0).sum() >= 50
    assert any(h.queue.drop_entries >= 2 for h in m.hosts)       # left Drop mode and entered it again
    assert any(h.queue.max_drop_count >= 3 for h in m.hosts)
    assert any(len(h.queue) + (h.cached is not None) > 0 for h in m.hosts) and m.pending() > 0
    assert sum(h.ties for h in m.hosts) >= 50                      # arrivals at the time of the one before
    assert sum(h.on_blocked_task for h in m.hosts) >= 3            # arrivals exactly on a pending task's time
    assert len(m.hosts[S.EMPTY_HOST].queue) == 0 and m.hosts[S.EMPTY_HOST].tasks == 0
    # the split run has packets that resolve in a later call than their own
    _, souts, _ = S.model_results(split=True)
    assert sum(len(o["late"]) for o in souts) >= 50


# ------------------------------------------------- host-only srt_inbound
def test_host_only_one_call_equals_model():
    calls, mouts, m = S.model_results()
    outs, state, stats = S.run_lib(S.scenario(), calls)
    S.assert_same(outs, mouts, state, m)
    assert stats[-1] == (0, m.pending())


def test_host_only_split_equals_model_and_one_call():
    sc = S.scenario()
    calls, mouts, m = S.model_results(split=True)
    outs, state, stats = S.run_lib(sc, calls)
    S.assert_same(outs, mouts, state, m)
    assert stats[-1] == (0, m.pending())
    # split invariance: what left the stage, and every host's final state
    c1, _, m1 = S.model_results()
    o1, state1, _ = S.run_lib(sc, c1)
    assert S.resolved(calls, outs) == S.resolved(c1, o1)
    for f in S.STATE_FIELDS:
        assert np.array_equal(state[f], state1[f]), f
    assert m1.state() == m.state()


def test_control_law_host_table_and_f64_agree_with_model():
    from shadow_amd.plan import InboundRouter

    r = InboundRouter(None, [1000], 4)
    counts = np.concatenate([np.arange(0, 3000), 2 ** np.arange(12, 41), 2 ** np.arange(12, 41) + 1,
                             2 ** np.arange(12, 41) - 1]).astype(np.uint64)
    want = np.array([M.control_law_increment(int(c)) for c in counts], np.uint64)
    assert np.array_equal(r.control_law(counts, use_table=True), want)
    assert np.array_equal(r.control_law(counts, use_table=False), want)
    r.close()


def test_error_paths():
    from shadow_amd import _lib

    L = _lib.lib()
    err = _lib.SrtErr()
    h = C.c_void_p()
    bw = (C.c_uint64 * 2)(1000, 1000)
    assert L.srt_inbound_create(None, 2, None, 4, C.byref(h), C.byref(err)) == _lib.SRT_ERR_INVALID
    assert L.srt_inbound_create(None, 2, bw, 4, None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert L.srt_inbound_create(None, 2, bw, 4, C.byref(h), C.byref(err)) == _lib.SRT_OK
    order = np.array([0, 1], np.uint32)
    dst_ptr = np.array([0, 1, 2], np.uint32)
    deliver = np.array([5 * M.MS, 6 * M.MS], np.uint64)
    size = np.array([100, 100], np.uint32)
    st, fw = np.zeros(2, np.uint32), np.zeros(2, np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731
    run = lambda hh, o, until: L.srt_inbound_run(hh, o, p(dst_ptr), p(deliver), p(size), 2, until, 0, p(st), p(fw),  # noqa
                                                 None, 0, None, None, C.byref(err))
    assert run(None, p(order), 10 * M.MS) == _lib.SRT_ERR_INVALID
    assert run(h, None, 10 * M.MS) == _lib.SRT_ERR_INVALID
    assert L.srt_inbound_status(None, None, None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert L.srt_inbound_state(h, None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert run(h, p(order), 10 * M.MS) == _lib.SRT_OK
    assert L.srt_inbound_status(h, None, None, C.byref(err)) == _lib.SRT_OK
    assert (st == M.ENQUEUED | M.DEQUEUED | M.FORWARDED).all() and fw.tolist() == deliver.tolist()
    # a window that ends before the previous one: refused at the call
    assert run(h, p(order), 9 * M.MS) == _lib.SRT_ERR_INVALID
    # arrivals (5 and 6 ms) earlier than the previous call's until_ns (10 ms): reported by the status call
    assert run(h, p(order), 20 * M.MS) == _lib.SRT_OK
    flags = C.c_uint32()
    assert L.srt_inbound_status(h, C.byref(flags), None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert flags.value & _lib.INBOUND_TIME_REGRESSION and b"earlier" in err.msg
    assert L.srt_inbound_status(h, C.byref(flags), None, C.byref(err)) == _lib.SRT_OK  # cleared with the report
    L.srt_inbound_destroy(h)
    L.srt_inbound_destroy(None)


def _tiny(bw, deliver_ms, size, calls, queue_cap=8):
    """one host-only host fed the same packets (those not yet taken) call after call
    -> per call (status, forward, flags, pending), and the final state"""
    from shadow_amd.plan import InboundRouter

    r = InboundRouter(None, [bw], queue_cap)
    n = len(deliver_ms)
    deliver = np.array(deliver_ms, np.uint64) * np.uint64(M.MS)
    sizes = np.full(n, size, np.uint32)
    outs, left = [], np.arange(n)
    for until in calls:
        st, fw = np.zeros(len(left), np.uint32), np.zeros(len(left), np.uint64)
        r.run(np.arange(len(left), dtype=np.uint32), np.array([0, len(left)], np.uint32), deliver[left], sizes[left],
              until * M.MS, 0, st, fw, np.zeros(24 * 16, np.uint8), np.zeros(1, np.uint32))
        flags, pending = r.status(check=False)
        outs.append((st.tolist(), fw.tolist(), flags, pending))
        left = left[st == 0]
    state = r.state()
    r.close()
    return outs, state


def test_arrivals_at_or_after_until_are_flagged_not_lost():
    """arrivals at 5, 6 and 7 ms against windows ending at 1, 6 and 8 ms: an
    arrival at or after until_ns is not taken (status 0, not pending), the call
    is flagged, and fed again with its own window it is handled as if in time"""
    from shadow_amd import _lib

    outs, state = _tiny(125_000_000, [5, 6, 7], 100, [1, 6, 8])
    done = M.ENQUEUED | M.DEQUEUED | M.FORWARDED
    assert outs[0] == ([0, 0, 0], [M.U64] * 3, _lib.INBOUND_AFTER_UNTIL, 0)
    assert outs[1] == ([done, 0, 0], [5 * M.MS, M.U64, M.U64], _lib.INBOUND_AFTER_UNTIL, 0)  # 6 ms is not < 6 ms
    assert outs[2] == ([done, done], [6 * M.MS, 7 * M.MS], 0, 0)
    assert int(state["tasks_scheduled"][0]) == 3 and int(state["queue_len"][0]) == 0
    # the model follows the same rule
    m = M.InboundModel([125_000_000])
    st, fw, _, _ = m.run(np.arange(3), [0, 3], np.array([5, 6, 7]) * M.MS, [100] * 3, 6 * M.MS, 0)
    assert st.tolist() == [done, 0, 0] and m.not_taken == 2 and m.pending() == 0
    # a pending task at or after until_ns does not let later arrivals through either
    outs, state = _tiny(1_000, [5, 5, 900, 901], 1500, [900, 2000])
    assert outs[0][2] == _lib.INBOUND_AFTER_UNTIL and outs[0][0][2:] == [0, 0] and outs[0][3] == 1
    assert outs[1][2] == 0 and all(x != 0 for x in outs[1][0])


def test_oversize_packet_is_flagged_and_the_call_ends():
    """a packet larger than the bucket's capacity (refill 1 + 1500) can never
    conform: the reference would reschedule its forward task for ever; here the
    task is tried once a call, parked at until_ns, and the call is flagged"""
    from shadow_amd import _lib

    outs, state = _tiny(1_000, [5, 6], 2000, [10_000, 20_000])
    for (st, fw, flags, pending), until in zip(outs, (10_000, 20_000)):
        assert flags == _lib.INBOUND_OVERSIZE and pending == 2
        assert int(state["cached"][0]) == 1 and int(state["queue_len"][0]) == 1
    assert outs[0][0] == [M.ENQUEUED | M.DEQUEUED | M.CACHED, M.ENQUEUED] and outs[0][1] == [M.U64, M.U64]
    assert int(state["task_ns"][0]) == 20_000 * M.MS and int(state["balance"][0]) == 1501
    # a packet of exactly the capacity does conform
    outs, state = _tiny(1_000, [5], 1501, [10_000])
    assert outs[0] == ([M.ENQUEUED | M.DEQUEUED | M.FORWARDED], [5 * M.MS], 0, 0)


def test_ring_overflow_is_reported_and_contained():
    """queue_cap 4: the 1,000 B/s hosts overflow; every other host's results stand"""
    from shadow_amd import _lib

    sc = S.scenario()
    calls, mouts, m = S.model_results(split=True)
    outs, state, stats = S.run_lib(sc, calls, queue_cap=4, check=False)
    assert any(f & _lib.INBOUND_RING_OVERFLOW for f, _ in stats)
    over = set(np.nonzero(state["overflow"])[0].tolist())
    assert any(sc["bw"][h] == 1_000 for h in over)
    good = set(range(S.N_HOSTS)) - over
    S.assert_same(outs, mouts, state, m, hosts=good)
    for c, o, mo in zip(calls, outs, mouts):
        keep = np.isin(sc["dst"][c["ids"]], sorted(good))
        assert np.array_equal(o["status"][keep], mo["status"][keep])
        assert np.array_equal(o["forward"][keep], mo["forward"][keep])
        assert [x for x in o["late"] if x[3] in good] == [x for x in mo["late"] if x[3] in good]


def test_late_overflow_is_reported():
    from shadow_amd import _lib

    sc = S.scenario()
    calls, mouts, _ = S.model_results(split=True)
    outs, _, stats = S.run_lib(sc, calls, late_cap=2, check=False)
    assert any(f & _lib.INBOUND_LATE_OVERFLOW for f, _ in stats)
    assert [o["late_count"] for o in outs] == [len(mo["late"]) for mo in mouts]


# ------------------------------------------------------------- the kernel
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_inbound_kernels_use_no_scratch():
    csrc = os.path.join(ROOT, "shadow_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
           os.path.join(csrc, "srt_inbound.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=csrc)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"remark:\s+Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]:\s+(\d+)", out.stderr)]
    assert any("inbound_step_kernel" in n for n in names) and len(names) == len(scratch) >= 3
    assert not any(scratch), dict(zip(names, scratch))
