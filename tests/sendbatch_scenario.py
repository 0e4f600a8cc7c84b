"""What the send-batch gather tests share: outbound windows produced by the
host-only srt_outbound on tests/outbound_scenario.py's generator, a runner that
feeds srt_sendbatch (host-only or on the device) from numpy arrays and keeps a
guard behind every output, and the hand-made cases both forms must pass.  The
windows are computed once per process."""
import ctypes as C
import functools

import numpy as np

import outbound_scenario as S
import sendbatch_model as SM
from outbound_model import MS, U64

GUARD = 4            # entries behind out_cap that no call may touch
FILL = 0xA5
SPAN_NS = 1000 * MS
DENSE, SPARSE = "dense", "sparse"  # about 100 packets a host (0 to 200) / about one


@functools.lru_cache(maxsize=None)
def windows(n_hosts, shape, qdisc, seed=7):
    """three windows of one scenario through a host-only srt_outbound: arrivals in the first two, the
    third only drains -> (list of window dicts, n_pkts of the scenario)"""
    from shadow_amd.plan import OutboundRelay

    rng = np.random.default_rng(seed + n_hosts)
    dense = shape == DENSE
    n_pkts = 100 * n_hosts if dense else n_hosts + 2
    slow = 60_000 if dense else 2_000
    bw = np.where(rng.random(n_hosts) < 0.4, slow, 125_000_000).astype(np.uint64)
    bw[0] = slow
    w = rng.uniform(0.0, 2.0, size=n_hosts)
    w[rng.random(n_hosts) < 0.15] = 0.0  # hosts that send nothing
    w[0] = 2.0
    sc = S.make_scenario(rng, n_hosts, n_pkts, rng.integers(1, 5, size=n_hosts), bw, SPAN_NS, w, local_share=0.05)
    meta = np.zeros(n_pkts, SM.META_DTYPE)
    for f in ("src_row", "dst_row", "payload_size", "user"):
        meta[f] = rng.integers(0, 1 << 32, size=n_pkts, dtype=np.uint64)
    calls = S.calls_of(sc, [SPAN_NS // 2, SPAN_NS, SPAN_NS + (300 if dense else 3000) * MS])
    late_cap = n_pkts + 1
    r = OutboundRelay(None, bw, qdisc, 8, n_pkts)
    out = []
    try:
        for c in calls:
            n = len(c["pkts"])
            st, sn, rk = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
            late, cnt = np.zeros(late_cap * 32, np.uint8), np.zeros(1, np.uint32)
            base = r.run(c["pkts"].view(np.uint8), c["host_ptr"], c["until"], 0, st, sn, rk, late, cnt)
            assert r.status()[0] == 0
            out.append(dict(host_ptr=c["host_ptr"], meta=meta[c["ids"]].copy(), send_ns=sn, send_rank=rk,
                            seq_base=base, late=late.view(SM.LATE_DTYPE)[:int(cnt[0])].copy(),
                            local=(c["pkts"]["flags"] & 1) != 0))
    finally:
        r.close()
    return out, n_pkts


class Runner:
    """srt_sendbatch fed from numpy arrays; plan=None: the host-only instance"""

    def __init__(self, plan, n_hosts, log_cap):
        from shadow_amd.plan import SendBatch

        self.plan, self.n_hosts = plan, n_hosts
        self.sb = SendBatch(plan, n_hosts, log_cap)

    def close(self):
        self.sb.close()

    def _in(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype.fields:
            a = a.view(np.uint8).reshape(-1)
        if self.plan is None:
            return a
        import torch

        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype)
        return torch.from_numpy(a.view(signed).copy()).to("cuda:0")

    def _out(self, n, width):
        if self.plan is None:
            return np.full(n * width, FILL, np.uint8)
        import torch

        return torch.full((n * width,), FILL, dtype=torch.uint8, device="cuda:0")

    def run(self, host_ptr, meta, send_ns, send_rank, seq_base, late, out_cap, late_count=None):
        """late: LATE_DTYPE records (the list's capacity is their number; late_count defaults to it) ->
        dict(pkts, host_ptr, user, seq: the first min(n_sent, out_cap) entries; flags; n_sent;
        untouched: every output byte behind those entries, the guard included, still holds the fill)"""
        cnt = np.array([len(late) if late_count is None else late_count], np.uint32)
        cap = out_cap + GUARD
        o_pk, o_us, o_sq = self._out(cap, 24), self._out(cap, 4), self._out(cap, 8)
        o_hp = self._out(self.n_hosts + 1 + GUARD, 4)
        self.sb.run(self._in(np.asarray(host_ptr, np.uint32)), self._in(meta), self._in(np.asarray(send_ns, np.uint64)),
                    self._in(np.asarray(send_rank, np.uint64)), seq_base, self._in(late), self._in(cnt),
                    o_pk[:24 * out_cap], o_hp[:4 * (self.n_hosts + 1)], o_us[:4 * out_cap], o_sq[:8 * out_cap])
        flags, n_sent = self.sb.status(check=False)
        host = (lambda a: a) if self.plan is None else (lambda a: a.cpu().numpy())
        o_pk, o_us, o_sq, o_hp = host(o_pk), host(o_us), host(o_sq), host(o_hp)
        k = min(n_sent, out_cap)
        tail = [o_pk[24 * k:], o_us[4 * k:], o_sq[8 * k:], o_hp[4 * (self.n_hosts + 1):]]
        return dict(pkts=o_pk[:24 * k].view(SM.PKT_DTYPE), user=o_us[:4 * k].view(np.uint32),
                    seq=o_sq[:8 * k].view(np.uint64), host_ptr=o_hp[:4 * (self.n_hosts + 1)].view(np.uint32),
                    flags=flags, n_sent=n_sent, untouched=all((t == FILL).all() for t in tail))


def assert_same(out, mo, what=""):
    """a runner's output against the model's (or another runner's), byte for byte"""
    assert out["flags"] == mo["flags"] and out["n_sent"] == mo["n_sent"], (what, out["flags"], mo["flags"])
    assert np.array_equal(out["host_ptr"], mo["host_ptr"]), what
    for f in ("pkts", "user", "seq"):
        assert out[f].tobytes() == mo[f].tobytes(), (what, f)
    assert out.get("untouched", True), what


def run_windows(plan, n_hosts, shape, qdisc, log_cap=None):
    """the scenario's three windows through a runner -> its outputs, out_cap = batch + late list"""
    ws, n_pkts = windows(n_hosts, shape, qdisc)
    r = Runner(plan, n_hosts, n_pkts if log_cap is None else log_cap)
    try:
        return [r.run(w["host_ptr"], w["meta"], w["send_ns"], w["send_rank"], w["seq_base"], w["late"],
                      len(w["send_rank"]) + len(w["late"])) for w in ws]
    finally:
        r.close()


@functools.lru_cache(maxsize=None)
def model_windows(n_hosts, shape, qdisc):
    ws, n_pkts = windows(n_hosts, shape, qdisc)
    m = SM.SendBatchModel(n_hosts, n_pkts)
    return [m.run(w["host_ptr"], w["meta"], w["send_ns"], w["send_rank"], w["seq_base"], w["late"],
                  len(w["send_rank"]) + len(w["late"])) for w in ws]


# ------------------------------------------------------------ hand-made cases
def _meta(n, start=1):
    m = np.zeros(n, SM.META_DTYPE)
    k = np.arange(n, dtype=np.uint32) + start
    m["src_row"], m["dst_row"], m["payload_size"], m["user"] = k * 3, k * 5 + 1, k * 7 + 2, k * 11 + 3
    return m


def _late(rows):
    """rows: (seq, send_ns, send_rank, src_host)"""
    a = np.zeros(len(rows), SM.LATE_DTYPE)
    for i, (seq, ns, rank, h) in enumerate(rows):
        a[i] = (seq, ns, rank, 0, h)
    return a


class _Pair:
    """the same calls through a runner and the model"""

    def __init__(self, make, n_hosts, log_cap):
        self.r, self.m = make(n_hosts, log_cap), SM.SendBatchModel(n_hosts, log_cap)

    def run(self, host_ptr, meta, send_ns, send_rank, seq_base, late, out_cap, late_count=None):
        hp, sn, rk = np.asarray(host_ptr, np.uint32), np.asarray(send_ns, np.uint64), np.asarray(send_rank, np.uint64)
        out = self.r.run(hp, meta, sn, rk, seq_base, late, out_cap, late_count)
        mo = self.m.run(hp, meta, sn, rk, seq_base, late[:len(late) if late_count is None else late_count], out_cap)
        return out, mo

    def close(self):
        self.r.close()


NO_LATE = np.zeros(0, SM.LATE_DTYPE)


def case_late_list_only(make):
    """n_pkts == 0: the first call only fills the log, the second gathers three hosts' late packets,
    host 1's none, one of them local (no rank: it takes no part)"""
    p = _Pair(make, 3, 8)
    try:
        out, mo = p.run([0, 2, 2, 5], _meta(5), [U64] * 5, [U64] * 5, 100, NO_LATE, 4)
        assert_same(out, mo)
        assert out["n_sent"] == 0 and out["host_ptr"].tolist() == [0, 0, 0, 0]
        late = _late([(104, 70, 41, 2), (100, 50, 8, 0), (102, 60, 40, 2), (101, 55, U64, 0), (103, 65, 42, 2)])
        out, mo = p.run([0, 0, 0, 0], _meta(0), [], [], 105, late, 4)
        assert_same(out, mo)
        assert out["flags"] == 0 and out["host_ptr"].tolist() == [0, 1, 1, 4]
        assert out["seq"].tolist() == [100, 102, 104, 103] and out["pkts"]["t_ns"].tolist() == [50, 60, 70, 65]
        assert out["user"].tolist() == _meta(5)["user"][[0, 2, 4, 3]].tolist()
    finally:
        p.close()


def case_one_host(make):
    p = _Pair(make, 1, 4)
    try:
        out, mo = p.run([0, 5], _meta(5), [10, 11, U64, 13, 14], [9, 7, U64, 8, 10], 0, NO_LATE, 4)
        assert_same(out, mo)
        assert out["flags"] == 0 and out["seq"].tolist() == [1, 3, 0, 4] and out["host_ptr"].tolist() == [0, 4]
    finally:
        p.close()


def case_rank_bases_need_u64(make):
    """host 0's ranks start above 2^32, host 1's run crosses 2^63: the differences are u64"""
    a, b = (1 << 32) + 5, (1 << 63) - 2
    p = _Pair(make, 2, 4)
    try:
        out, mo = p.run([0, 3, 7], _meta(7), np.arange(7) + 20, [a + 2, a, a + 1, b + 3, b, b + 2, b + 1], 40,
                        NO_LATE, 7)
        assert_same(out, mo)
        assert out["flags"] == 0 and out["seq"].tolist() == [41, 42, 40, 44, 46, 45, 43]
    finally:
        p.close()


def case_late_count_past_its_cap(make):
    """*d_late_count = 5 over a list of 2 records: two are used"""
    p = _Pair(make, 2, 8)
    try:
        p.run([0, 2, 4], _meta(4), [U64] * 4, [U64] * 4, 0, NO_LATE, 2)
        late = _late([(1, 30, 0, 0), (2, 31, 6, 1)])
        out = p.r.run([0, 0, 0], _meta(0), [], [], 4, late, 6, late_count=5)
        mo = p.m.run(np.zeros(3, np.uint32), _meta(0), [], np.zeros(0, np.uint64), 4, late, 6)
        assert_same(out, mo)
        assert out["flags"] == 0 and out["n_sent"] == 2 and out["seq"].tolist() == [1, 2]
    finally:
        p.close()


def case_out_cap_one_short(make):
    p = _Pair(make, 3, 4)
    try:
        args = ([0, 2, 3, 6], _meta(6), np.arange(6) + 5, [1, 0, 7, 4, 3, 5], 0, NO_LATE)
        out, mo = p.run(*args, 5)
        assert_same(out, mo)
        assert out["flags"] == SM.OUT_OVERFLOW and out["n_sent"] == 6 and len(out["seq"]) == 5 and out["untouched"]
        assert out["host_ptr"].tolist() == [0, 2, 3, 5]
        out, mo = p.run(*args, 6)  # and with room it is whole
        assert_same(out, mo)
        assert out["flags"] == 0 and out["seq"].tolist() == [1, 0, 2, 4, 3, 5]
    finally:
        p.close()


def case_rank_gap(make):
    """host 1's ranks 4, 5, 7: the packet of rank 7 has no place and is not written"""
    p = _Pair(make, 2, 4)
    try:
        out, mo = p.run([0, 1, 4], _meta(4), [1, 2, 3, 4], [0, 4, 7, 5], 0, NO_LATE, 4)
        assert out["flags"] == mo["flags"] == SM.RANK_GAP and out["n_sent"] == 4
        assert out["host_ptr"].tolist() == [0, 1, 4]
        assert out["seq"][:3].tolist() == [0, 1, 3] and out["untouched"]
        assert out["seq"][3:].view(np.uint8).tolist() == [FILL] * 8  # the place no rank named
    finally:
        p.close()


def case_late_host_out_of_range(make):
    p = _Pair(make, 2, 8)
    try:
        p.run([0, 1, 3], _meta(3), [U64] * 3, [U64] * 3, 0, NO_LATE, 2)
        late = _late([(0, 9, 3, 0), (1, 9, 0, 2), (2, 9, 5, 1), (1, 9, 0, 0xffffffff)])
        out, mo = p.run([0, 0, 0], _meta(0), [], [], 3, late, 4)
        assert_same(out, mo)
        assert out["flags"] == SM.BAD_HOST and out["n_sent"] == 2 and out["seq"].tolist() == [0, 2]
    finally:
        p.close()


def case_log_rule_at_its_edge(make):
    """log_cap 4.  Call 1 feeds seqs 0..5 (all stay queued): 0 and 1 are already out of the log's
    reach and are not written.  Call 2 (seq_base 6, two packets) ends the range at 8: seq 4 is
    exactly log_cap back and resolves, seq 3 is one more and comes out as the placeholder"""
    p = _Pair(make, 1, 4)
    try:
        p.run([0, 6], _meta(6), [U64] * 6, [U64] * 6, 0, NO_LATE, 2)
        late = _late([(4, 90, 0, 0), (3, 91, 1, 0)])
        out, mo = p.run([0, 2], _meta(2, start=50), [92, U64], [2, U64], 6, late, 4)
        assert_same(out, mo)
        assert out["flags"] == SM.LOG_OVERRUN and out["seq"].tolist() == [4, 3, 6]
        assert tuple(out["pkts"][0])[1:4] == tuple(_meta(6)[4])[:3] and out["user"][0] == _meta(6)["user"][4]
        assert tuple(out["pkts"][1]) == (0, 0, 0, 0, 91) and out["user"][1] == 0xffffffff
        # the status call cleared the flag; a clean call reports none.  seq 7 (written by call 2) and
        # seq 5 (by call 1, four back from the new end 9) both resolve
        out, mo = p.run([0, 1], _meta(1, start=70), [95], [5], 8, _late([(7, 93, 3, 0), (5, 94, 4, 0)]), 4)
        assert_same(out, mo)
        assert out["flags"] == 0 and out["seq"].tolist() == [7, 5, 8]
        assert out["user"].tolist() == [_meta(2, start=50)["user"][1], _meta(6)["user"][5], _meta(1, start=70)["user"][0]]
    finally:
        p.close()


CASES = [case_late_list_only, case_one_host, case_rank_bases_need_u64, case_late_count_past_its_cap,
         case_out_cap_one_short, case_rank_gap, case_late_host_out_of_range, case_log_rule_at_its_edge]


def error_paths(plan_handle=None):
    """null arguments and SRT_ERR_INVALID of the four entry points, on raw ctypes"""
    from shadow_amd import _lib

    L, err, h = _lib.lib(), _lib.SrtErr(), C.c_void_p()
    assert L.srt_sendbatch_create(plan_handle, 2, 4, None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert L.srt_sendbatch_create(plan_handle, 0xffffffff, 4, C.byref(h), C.byref(err)) == _lib.SRT_ERR_INVALID
    assert L.srt_sendbatch_status(None, None, None, C.byref(err)) == _lib.SRT_ERR_INVALID and b"null" in err.msg
    L.srt_sendbatch_destroy(None)
    if plan_handle is not None:
        return
    assert L.srt_sendbatch_create(None, 2, 4, C.byref(h), C.byref(err)) == _lib.SRT_OK
    hp, meta = np.array([0, 1, 2], np.uint32), _meta(2)
    sn, rk = np.array([5, 6], np.uint64), np.array([0, 0], np.uint64)
    late, cnt = _late([(0, 1, 1, 0)]), np.ones(1, np.uint32)
    o_pk, o_hp, o_us, o_sq = np.zeros(2, SM.PKT_DTYPE), np.zeros(3, np.uint32), np.zeros(2, np.uint32), np.zeros(
        2, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def run(sb=h, hp=hp, n=2, meta=meta, sn=sn, rk=rk, late=None, late_cap=0, cnt=None, o_pk=o_pk, o_hp=o_hp,
            o_us=o_us, o_sq=o_sq, out_cap=2):
        return L.srt_sendbatch_run(sb, p(hp), n, p(meta), p(sn), p(rk), 0, p(late), late_cap, p(cnt), p(o_pk),
                                   p(o_hp), p(o_us), p(o_sq), out_cap, C.byref(err))

    for bad in (dict(sb=None), dict(hp=None), dict(meta=None), dict(sn=None), dict(rk=None), dict(o_hp=None),
                dict(o_pk=None), dict(o_us=None), dict(o_sq=None), dict(late_cap=1, cnt=cnt),
                dict(late=late, late_cap=1), dict(n=1 << 31), dict(late=late, late_cap=1 << 31, cnt=cnt)):
        assert run(**bad) == _lib.SRT_ERR_INVALID, bad
        assert err.code == _lib.SRT_ERR_INVALID and err.msg
    assert run() == _lib.SRT_OK and o_sq.tolist() == [0, 1] and o_hp.tolist() == [0, 1, 2]
    assert run(o_pk=None, o_us=None, o_sq=None, out_cap=0) == _lib.SRT_OK  # nothing to write: no arrays needed
    flags, n_sent = C.c_uint32(), C.c_uint64()
    assert L.srt_sendbatch_status(h, C.byref(flags), C.byref(n_sent), C.byref(err)) == _lib.SRT_ERR_INVALID
    assert flags.value == _lib.SENDBATCH_OUT_OVERFLOW and n_sent.value == 2 and b"out_cap" in err.msg
    assert L.srt_sendbatch_status(h, C.byref(flags), None, C.byref(err)) == _lib.SRT_OK and flags.value == 0
    # every flag has its own words in the message: a gap and a bad host in one call
    late2 = _late([(0, 1, 1, 7)])
    rk[:] = [0, 5]
    hp[:] = [0, 2, 2]
    assert run(late=late2, late_cap=1, cnt=cnt) == _lib.SRT_OK
    assert L.srt_sendbatch_status(h, C.byref(flags), None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert flags.value == _lib.SENDBATCH_RANK_GAP | _lib.SENDBATCH_BAD_HOST
    assert b"contiguous" in err.msg and b"src_host" in err.msg and b"out_cap" not in err.msg
    L.srt_sendbatch_destroy(h)
