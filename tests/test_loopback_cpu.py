"""Loopback stage (srt_loopback: the loopback interface's qdisc order, relay,
receive and local tracker counters) without a GPU: the host-only instance -- the
same step the device kernel compiles -- against the literal queue simulation of
loopback_model.py in both qdiscs, the flag cases, the error paths on raw ctypes,
srt_deliver_lookup_flat on a host-only instance, the kernels' resource report,
and the step header under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/asan/loopback_check.cpp, a stand-alone program)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import loopback_model as LM
import loopback_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEEDS_HIPCC = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC),
                                 reason="hipcc not available")
QDISCS = pytest.mark.parametrize("qdisc", [LM.FIFO, LM.RR], ids=["fifo", "rr"])


def test_main_scenario_has_what_it_claims():
    """asserted on the generator and the model alone: a weakened generator fails here"""
    sc = S.main_scenario()
    runs = [st[1] for st in sc["steps"] if st[0] == "run"]
    n_hosts, ms = sc["n_hosts"], sc["max_sockets"]
    assert len(runs) == 3 and 20 <= n_hosts <= 64 and 200 <= sum(len(c["pkts"]) for c in runs) <= 999
    three_sockets = several_a_socket = not_monotone = 0
    for c in runs:
        hp, pk = c["host_ptr"].astype(np.int64), c["pkts"]
        for h in range(n_hosts):
            b, e = hp[h], hp[h + 1]
            assert (np.diff(pk["ready_ns"][b:e].astype(np.int64)) >= 0).all()
            assert len(set(pk["priority"][b:e].tolist())) == e - b  # distinct within a host
            for t in np.unique(pk["ready_ns"][b:e]):
                g = pk[b:e][pk["ready_ns"][b:e] == t]
                socks = set(g["socket"].tolist())
                three_sockets += len(socks) >= 3
                for s in socks:
                    pr = g["priority"][g["socket"] == s].astype(object)
                    several_a_socket += len(pr) >= 2
                    not_monotone += any(pr[k + 1] < pr[k] for k in range(len(pr) - 1))
    assert three_sockets >= 5 and several_a_socket >= 20 and not_monotone >= 5
    assert any(np.diff(c["host_ptr"].astype(np.int64)).min() == 0 for c in runs)
    # specific, wildcard and missing associations; a protocol that matches nothing
    assoc = sc["steps"][0][1]
    assert (assoc["peer_ip_be"] != 0).any() and (assoc["peer_ip_be"] == 0).any() and ms % 3 != 0
    rx = np.concatenate([c["rx_meta"] for c in runs])
    assert (rx["protocol"] == 7).sum() >= 5 and ((rx["local_port_be"] - 1000) % 3 == 2).sum() >= 20
    trk = np.concatenate([c["trk_meta"] for c in runs])
    assert (trk["flags"] & 1).sum() >= 20 and (trk["payload_size"] == 0).sum() >= 20
    assert ((trk["flags"] & 1 == 1) & (trk["payload_size"] == 0)).any()
    # a heartbeat between calls on a subset, with a duplicate; a table change between calls
    kinds = [st[0] for st in sc["steps"]]
    assert kinds == ["assoc", "run", "beat", "disassoc", "run", "run", "beat"]
    sel = sc["steps"][2][1]
    assert 0 < len(set(sel.tolist())) < len(sel) < n_hosts
    # one instant continued across two calls: the task count does not move with it
    c1, c2 = runs[0], runs[1]
    cont = [h for h in range(n_hosts)
            if c1["host_ptr"][h + 1] > c1["host_ptr"][h] and c2["host_ptr"][h + 1] > c2["host_ptr"][h]
            and c1["pkts"]["ready_ns"][c1["host_ptr"][h + 1] - 1] == c2["pkts"]["ready_ns"][c2["host_ptr"][h]]]
    assert len(cont) >= 5
    for qdisc in (LM.FIFO, LM.RR):
        outs, beats, stats, m = S.run_model(sc, qdisc)
        h = cont[0]
        t1, t2 = stats[0][1][h], stats[1][1][h]
        distinct = len(set(c2["pkts"]["ready_ns"][c2["host_ptr"][h]:c2["host_ptr"][h + 1]].tolist()))
        assert t2 - t1 == distinct - 1
        sock = np.concatenate([o["socket"] for o in outs])
        assert (sock == LM.NONE32).sum() >= 50 and (sock != LM.NONE32).sum() >= 200
        assert max(m.pop_lens) >= 10 and all(int(beats[1][0][f].sum()) > 0 for f in LM.TM.FIELDS)
    # the two qdiscs really order differently
    a, b = S.run_model(sc, LM.FIFO)[0], S.run_model(sc, LM.RR)[0]
    assert any(x["index"].tobytes() != y["index"].tobytes() for x, y in zip(a, b))


@QDISCS
@pytest.mark.parametrize("split", [False, True], ids=["one_call", "split"])
def test_host_only_equals_model(qdisc, split):
    sc = S.main_scenario()
    got, want, m = S.check(S.split_scenario(sc) if split else sc, qdisc)
    outs, beats, stats = got
    assert all(st[0][0] == 0 for st in stats)
    for o, st in zip(outs, [s for s in (S.split_scenario(sc) if split else sc)["steps"] if s[0] == "run"]):
        hp = st[1]["host_ptr"].astype(np.int64)
        for h in range(sc["n_hosts"]):
            b, e = hp[h], hp[h + 1]
            assert sorted(o["index"][b:e].tolist()) == list(range(b, e))  # a permutation of the host's span
            assert (np.diff(o["recv_ns"][b:e].astype(np.int64)) >= 0).all()
    if split:  # cutting calls at instant boundaries changes neither the tasks nor the counters
        whole = S.run_lib(sc, qdisc)
        assert whole[2][-1][1] == stats[-1][1]  # the tasks; the received counts are a run's own
        assert sum(st[0][1] for st in whole[2]) == sum(st[0][1] for st in stats)
        for a, b in zip(whole[1], beats):
            S.same_records(a, b, "split")


@QDISCS
@pytest.mark.parametrize("n_hosts,counts,single", [
    (1, [0], False), (1, [1], False), (3, [0, 0, 0], False), (5, [0, 200, 0, 1, 0], True), (70, None, False)])
def test_shapes(qdisc, n_hosts, counts, single):
    """no packets at all, one packet, one long instant beside empty hosts, more hosts than a wave"""
    if counts is None:
        counts = np.random.default_rng(2).integers(0, 30, size=n_hosts)
    S.check(S.shape_scenario(3, n_hosts, 4, counts, single=single), qdisc)


@QDISCS
@pytest.mark.parametrize("kind", ["time", "time_inside", "socket"])
def test_flagged_host_leaves_state_and_neighbours_exact(qdisc, kind):
    sc = S.flag_scenario(kind)
    got, want, m = S.check(sc, qdisc)
    outs, beats, stats = got
    flag = LM.BAD_SOCKET if kind == "socket" else LM.TIME_ORDER
    assert [st[0][0] for st in stats] == [0, flag, 0]
    c2 = sc["steps"][2][1]
    b, e = int(c2["host_ptr"][2]), int(c2["host_ptr"][3])
    o = outs[1]
    assert e - b == 6 and o["index"][b:e].tolist() == list(range(b, e)) and not o["status"][b:e].any()
    assert (o["socket"][b:e] == LM.NONE32).all() and (o["recv_ns"][b:e] == LM.U64).all()
    assert o["user"][b:e].tolist() == c2["rx_meta"]["user"][b:e].tolist()
    assert stats[1][1][2] == stats[0][1][2]  # its task count did not move
    assert stats[1][0][1] == len(c2["pkts"]) - (e - b)  # and its packets are not received
    # its counters hold what calls 1 and 3 gave them, nothing of call 2: a model that never sees host 2's
    # span of call 2
    skip = dict(sc, steps=list(sc["steps"]))
    keep = np.r_[0:b, e:len(c2["pkts"])]
    hp = c2["host_ptr"].copy()
    hp[3:] -= e - b
    skip["steps"][2] = ("run", dict(pkts=c2["pkts"][keep], host_ptr=hp, rx_meta=c2["rx_meta"][keep],
                                    trk_meta=c2["trk_meta"][keep]))
    s_beats = S.run_model(skip, qdisc)[1]
    S.same_records(beats[0], s_beats[0], "flagged host skipped")
    assert int(beats[0][1]["packets_control"][2] + beats[0][1]["packets_data"][2]) > 0


@QDISCS
def test_bad_slot_counts_at_the_host_only(qdisc):
    """n_slots 6 of 20: most out and in slots are out of range"""
    sc = S.flag_scenario("none")
    sc["steps"][2][1]["pkts"]["socket"][:] %= 4  # no host flagged
    got, want, m = S.check(sc, qdisc, n_slots=6)
    assert all(st[0][0] == LM.BAD_SLOT for st in got[2])
    full = S.run_lib(sc, qdisc)
    for k in (0, 1):  # the hosts' records do not depend on n_slots; the slots that exist agree
        assert got[1][0][k].tobytes() == full[1][0][k].tobytes()
        assert got[1][0][2 + k].tobytes() == full[1][0][2 + k][:6].tobytes()
    off = S.run_lib(sc, qdisc, n_slots=0)  # slot counters off: no flag
    assert all(st[0][0] == 0 for st in off[2]) and off[1][0][0].tobytes() == full[1][0][0].tobytes()
    assert len(off[1][0][2]) == 0


def test_without_trk_meta_nothing_is_counted():
    sc = S.shape_scenario(4, 6, 4, [5, 0, 9, 3, 1, 7])
    del sc["steps"][1][1]["trk_meta"]
    got, want, m = S.check(sc, LM.FIFO)
    assert not any(got[1][0][k][f].any() for k in range(4) for f in LM.TM.FIELDS)
    assert got[2][0][0][1] == 25


def test_error_paths():
    from shadow_amd import _lib

    L = _lib.lib()
    err = _lib.SrtErr()
    mk = lambda fn, *a: (lambda h: (fn(*a, C.byref(h), C.byref(err)), h)[1])(C.c_void_p())  # noqa: E731
    assert L.srt_loopback_create(None, 4, 0, 4, 8, None, C.byref(err)) == _lib.SRT_ERR_INVALID
    for bad in ((4, 2, 4, 8), (4, 0, 0, 8), (1 << 31, 0, 4, 8)):
        h = C.c_void_p()
        assert L.srt_loopback_create(None, *bad, C.byref(h), C.byref(err)) == _lib.SRT_ERR_INVALID and not h
    lb = mk(L.srt_loopback_create, None, 4, 0, 4, 8)
    dl = mk(L.srt_deliver_create, None, 4, 8, 0, 0)
    dl5 = mk(L.srt_deliver_create, None, 5, 8, 0, 0)
    assert lb and dl and dl5
    try:
        n = 3
        pk, rx, trk = np.zeros(n, S.OUT_PKT), np.zeros(n, S.RX_META), np.zeros(n, S.TRK_META)
        hp = np.array([0, 1, 1, 2, 3], np.uint32)
        o = [np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint32),
             np.zeros(n, np.uint32)]
        p = lambda a: a.ctypes.data  # noqa: E731
        args = [lb, dl, p(pk), p(hp), n, p(rx), p(trk)] + [p(a) for a in o]
        assert L.srt_loopback_run(*args, C.byref(err)) == _lib.SRT_OK
        # a deliver instance of another n_hosts
        a5 = list(args)
        a5[1] = dl5
        assert L.srt_loopback_run(*a5, C.byref(err)) == _lib.SRT_ERR_INVALID and b"n_hosts" in err.msg
        # NULL arguments (trk_meta alone may be NULL)
        for k in (0, 1, 2, 3, 5, 7, 8, 9, 10, 11):
            a = list(args)
            a[k] = None
            assert L.srt_loopback_run(*a, C.byref(err)) == _lib.SRT_ERR_INVALID, k
        a = list(args)
        a[6] = None
        assert L.srt_loopback_run(*a, C.byref(err)) == _lib.SRT_OK
        a[4] = 1 << 31
        assert L.srt_loopback_run(*a, C.byref(err)) == _lib.SRT_ERR_INVALID
        assert L.srt_loopback_status(None, None, None, None, C.byref(err)) == _lib.SRT_ERR_INVALID
        assert L.srt_loopback_tasks(lb, None, C.byref(err)) == _lib.SRT_ERR_INVALID
        assert L.srt_loopback_heartbeat(None, None, 0, None, 0, None, None, None, None, C.byref(err)) == \
            _lib.SRT_ERR_INVALID
        # a heartbeat index out of range clears nothing; a duplicate is returned twice and cleared once
        trk["header_size"] = 40
        assert L.srt_loopback_run(*args, C.byref(err)) == _lib.SRT_OK
        out = np.zeros(4, LM.TM.COUNTERS)
        sel = np.array([0, 4, 0], np.uint32)
        assert L.srt_loopback_heartbeat(lb, p(sel), 3, None, 0, None, p(out), None, None, C.byref(err)) == \
            _lib.SRT_ERR_INVALID and b"nothing was cleared" in err.msg
        slot = np.array([8], np.uint32)
        assert L.srt_loopback_heartbeat(lb, None, 0, p(slot), 1, None, None, None, None, C.byref(err)) == \
            _lib.SRT_ERR_INVALID
        sel[1] = 3
        assert L.srt_loopback_heartbeat(lb, p(sel), 3, p(slot), 0, None, p(out), None, None, C.byref(err)) == _lib.SRT_OK
        assert out["packets_control"].tolist() == [2, 2, 2, 0] and out["bytes_control_header"][:3].tolist() == [40] * 3
        assert L.srt_loopback_heartbeat(lb, None, 0, p(slot), 0, None, p(out), None, None, C.byref(err)) == _lib.SRT_OK
        assert out["packets_control"].tolist() == [0, 0, 2, 0]  # hosts 0 and 3 were cleared, host 2 was not selected
        flags, a_, b_ = C.c_uint32(), C.c_uint64(), C.c_uint64()
        assert L.srt_loopback_status(lb, C.byref(flags), C.byref(a_), C.byref(b_), C.byref(err)) == _lib.SRT_OK
        assert (flags.value, a_.value, b_.value) == (0, 3, 3)
        # every flag is named
        pk["socket"][0] = 9
        pk["ready_ns"][1] = 5
        hp2 = np.array([0, 1, 3, 3, 3], np.uint32)
        trk["socket_slot"] = 99
        args[3] = p(hp2)
        pk["ready_ns"][2] = 4
        assert L.srt_loopback_run(*args, C.byref(err)) == _lib.SRT_OK
        assert L.srt_loopback_status(lb, C.byref(flags), None, None, C.byref(err)) == _lib.SRT_ERR_INVALID
        assert flags.value == 3 and b"previous arrival" in err.msg and b"max_sockets" in err.msg
        pk["ready_ns"][:] = 10
        pk["socket"][:] = 0
        assert L.srt_loopback_run(*args, C.byref(err)) == _lib.SRT_OK
        assert L.srt_loopback_status(lb, C.byref(flags), None, None, C.byref(err)) == _lib.SRT_ERR_INVALID
        assert flags.value == 4 and b"n_slots" in err.msg
        assert L.srt_loopback_status(lb, C.byref(flags), None, None, C.byref(err)) == _lib.SRT_OK and flags.value == 0
    finally:
        L.srt_loopback_destroy(lb)
        L.srt_deliver_destroy(dl)
        L.srt_deliver_destroy(dl5)
    L.srt_loopback_destroy(None)


def test_lookup_flat_on_a_host_only_instance_is_lookup():
    from shadow_amd.plan import DeliverStage

    sc = S.main_scenario()
    ds = DeliverStage(None, sc["n_hosts"], 8, 0, 0)
    try:
        ds.associate(sc["steps"][0][1])
        c = sc["steps"][1][1]
        hosts = np.repeat(np.arange(sc["n_hosts"], dtype=np.uint32), np.diff(c["host_ptr"].astype(np.int64)))
        hosts[::17] = sc["n_hosts"] + 5  # out of range
        want = ds.lookup(hosts, c["rx_meta"])
        got = np.full(len(hosts), 0x5A5A5A5A, np.uint32)
        ds.lookup_flat(hosts, c["rx_meta"].view(np.uint8), got)
        assert got.tobytes() == want.tobytes() and (want[::17] == LM.NONE32).all()
        assert (want != LM.NONE32).sum() > 50 and (want == LM.NONE32).sum() > 50
    finally:
        ds.close()


def test_records_match_the_header():
    from shadow_amd import _lib
    from shadow_amd.plan import OUT_PKT_DTYPE, RX_META_DTYPE

    src = open(os.path.join(ROOT, "include", "srt.h")).read()
    for name, val in (("TIME_ORDER", LM.TIME_ORDER), ("BAD_SOCKET", LM.BAD_SOCKET), ("BAD_SLOT", LM.BAD_SLOT)):
        assert int(re.search(rf"#define SRT_LOOPBACK_{name}\s+(\d+)u", src).group(1)) == val == \
            getattr(_lib, "LOOPBACK_" + name)
    assert OUT_PKT_DTYPE == S.OUT_PKT and RX_META_DTYPE == S.RX_META


@NEEDS_HIPCC
def test_loopback_kernels_use_no_scratch():
    csrc = os.path.join(ROOT, "shadow_amd", "csrc")
    for unit, kernels, at_least in (("srt_loopback.hip", ("loopback_run_kernel", "loopback_sum_kernel"), 3),
                                    ("srt_deliver.hip", ("deliver_lookup_kernel",), 1)):
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-c",
               os.path.join(csrc, unit), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=csrc)
        assert out.returncode == 0, out.stderr[-2000:]
        names = re.findall(r"remark:\s+Function Name: (\S+)", out.stderr)
        scratch = [int(x) for x in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]:\s+(\d+)", out.stderr)]
        for k in kernels:
            assert any(k in n for n in names), (k, names)
        assert len(names) == len(scratch) >= at_least
        assert not any(scratch), dict(zip(names, scratch))


@NEEDS_HIPCC
def test_step_header_under_asan_ubsan(tmp_path):
    """tests/asan/loopback_check.cpp over srt_loopback_step.h and the deliver step's host-only lookup, host
    arrays sized exactly, built for the host with -fsanitize=address,undefined and run directly"""
    exe = str(tmp_path / "loopback_check")
    cmd = [HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wall", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "asan", "loopback_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "loopback_check: clean" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
