"""What the in-flight store tests share: a generator of rounds (three pushes
whose deliver times spread over four windows), a runner that feeds srt_flight
(host-only or on the device) from numpy arrays and keeps a guard behind every
output, and the hand-made cases both forms must pass."""
import ctypes as C
import functools

import numpy as np

import flight_model as FM

GUARD = 4            # entries behind out_cap that no call may touch
FILL = 0xA5
U64 = 0xFFFFFFFFFFFFFFFF
SENT, DROPPED = FM.SENT, 1 << 9
W_NS = 10_000_000    # one window
T0 = 1_000_000_000
DENSE, SPARSE = "dense", "sparse"  # about 100 packets a host (0 to 200) / about one
G = 256              # FL_CAP of srt_flight.hip: the keys a destination's run may hold for the one-pass LDS sort

OUT_FIELDS = (("order", np.uint32), ("deliver", np.uint64), ("size", np.uint32), ("src", np.uint32),
              ("event_id", np.uint64), ("tag", np.uint64))


def make_push(rng, n_src, n_dst, shape, event_base, t_lo, t_hi, sent_share=0.8):
    """one round's srt_packet_events arrays: packets grouped by source host, the sent ones numbered
    from event_base[h] (advanced in place), deliver times on a coarse grid so that ties happen"""
    if shape == DENSE:
        per = rng.integers(0, 201, size=n_src)
        per[rng.random(n_src) < 0.15] = 0
        per[0] = 150 + int(rng.integers(0, 50))
    else:
        per = rng.integers(0, 3, size=n_src)
    n = int(per.sum())
    host_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    src = np.repeat(np.arange(n_src), per)
    u = rng.random(n)
    flags = np.where(u < sent_share, SENT, np.where(u < sent_share + 0.1, DROPPED, 0)).astype(np.uint32)
    step = max(1, (t_hi - t_lo) // 64)
    deliver = (t_lo + rng.integers(0, 64, size=n) * step).astype(np.uint64)
    dst = rng.integers(0, n_dst, size=n).astype(np.uint32)
    size = rng.integers(40, 1541, size=n).astype(np.uint32)
    event_id = np.full(n, U64, np.uint64)
    for h in range(n_src):
        b, e = int(host_ptr[h]), int(host_ptr[h + 1])
        s = flags[b:e] == SENT
        event_id[b:e][s] = event_base[h] + np.arange(int(s.sum()), dtype=np.uint64)
        event_base[h] += np.uint64(s.sum())
    return dict(host_ptr=host_ptr, flags=flags, deliver=deliver, dst=dst, event_id=event_id, size=size, src=src)


@functools.lru_cache(maxsize=None)
def scenario(n_hosts, shape, seed=11):
    """-> (steps, total packets).  steps: ("push", arrays) / ("pop", until_ns): two pushes, the first
    window, a third push, three more windows; the last one drains the store"""
    rng = np.random.default_rng(seed + n_hosts)
    base = (rng.integers(0, 1000, size=n_hosts) + (1 << 32) * (np.arange(n_hosts) % 2)).astype(np.uint64)
    end = T0 + 4 * W_NS
    p0 = make_push(rng, n_hosts, n_hosts, shape, base, T0, end)
    p1 = make_push(rng, n_hosts, n_hosts, shape, base, T0, end)
    p2 = make_push(rng, n_hosts, n_hosts, shape, base, T0 + W_NS, end)
    steps = [("push", p0), ("push", p1), ("pop", T0 + W_NS), ("push", p2), ("pop", T0 + 2 * W_NS),
             ("pop", T0 + 3 * W_NS), ("pop", end)]
    return steps, len(p0["flags"]) + len(p1["flags"]) + len(p2["flags"])


class Runner:
    """srt_flight fed from numpy arrays; plan=None: the host-only instance"""

    def __init__(self, plan, n_dst, pool_cap):
        from shadow_amd.plan import FlightStore

        self.plan, self.n_dst = plan, n_dst
        self.fs = FlightStore(plan, n_dst, pool_cap)

    def close(self):
        self.fs.close()

    def _in(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
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

    def push(self, host_ptr, flags, deliver, dst, event_id, size, tag=None):
        u4, u8 = (lambda a: np.asarray(a, np.uint32)), (lambda a: np.asarray(a, np.uint64))
        return self.fs.push(self._in(u4(host_ptr)), self._in(u4(flags)), self._in(u8(deliver)), self._in(u4(dst)),
                            self._in(u8(event_id)), self._in(u4(size)), None if tag is None else self._in(u8(tag)))

    def status(self):
        """-> (flags, n_popped, n_stored, n_lost, message)"""
        from shadow_amd import _lib

        f, a, b, c, err = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64(), _lib.SrtErr()
        rc = _lib.lib().srt_flight_status(self.fs._h, C.byref(f), C.byref(a), C.byref(b), C.byref(c), C.byref(err))
        assert rc == (_lib.SRT_ERR_INVALID if f.value else _lib.SRT_OK), (rc, err.msg)
        return f.value, a.value, b.value, c.value, err.msg.decode()

    def pop(self, until_ns, out_cap):
        """-> dict(dst_ptr; order, deliver, size, src, event_id, tag: the popped entries; status;
        untouched: every output byte behind those entries, the guard included, still holds the fill)"""
        cap = out_cap + GUARD
        bufs = {k: self._out(cap, np.dtype(t).itemsize) for k, t in OUT_FIELDS}
        o_dp = self._out(self.n_dst + 1 + GUARD, 4)
        cut = lambda k, t: bufs[k][:np.dtype(t).itemsize * out_cap]  # noqa: E731
        self.fs.pop(until_ns, cut("order", np.uint32), o_dp[:4 * (self.n_dst + 1)], cut("deliver", np.uint64),
                    cut("size", np.uint32), cut("src", np.uint32), cut("event_id", np.uint64), cut("tag", np.uint64))
        st = self.status()
        host = (lambda a: a) if self.plan is None else (lambda a: a.cpu().numpy())
        o_dp = host(o_dp)
        dst_ptr = o_dp[:4 * (self.n_dst + 1)].view(np.uint32)
        k = int(dst_ptr[-1])
        assert k <= out_cap
        out = dict(dst_ptr=dst_ptr, status=st[:4], msg=st[4])
        ok = bool((o_dp[4 * (self.n_dst + 1):] == FILL).all())
        for name, t in OUT_FIELDS:
            a, w = host(bufs[name]), np.dtype(t).itemsize
            out[name] = a[:w * k].view(t)
            ok = ok and bool((a[w * k:] == FILL).all())
        out["untouched"] = ok
        return out


def assert_same(out, mo, what=""):
    """a runner's window against the model's (or another runner's), byte for byte"""
    assert tuple(out["status"]) == tuple(mo["status"]), (what, out["status"], mo["status"])
    assert np.array_equal(out["dst_ptr"], mo["dst_ptr"]), what
    for f, _ in OUT_FIELDS:
        assert out[f].tobytes() == mo[f].tobytes(), (what, f)
    assert out.get("untouched", True), what


PUSH_KEYS = ("host_ptr", "flags", "deliver", "dst", "event_id", "size")


def run_scenario(plan, n_hosts, shape):
    """the scenario through a runner -> the windows of its pops"""
    steps, total = scenario(n_hosts, shape)
    r = Runner(plan, n_hosts, total)
    try:
        outs = []
        for kind, arg in steps:
            if kind == "push":
                r.push(*[arg[k] for k in PUSH_KEYS])
            else:
                outs.append(r.pop(arg, total))
        return outs
    finally:
        r.close()


@functools.lru_cache(maxsize=None)
def model_scenario(n_hosts, shape):
    steps, total = scenario(n_hosts, shape)
    m = FM.FlightModel(n_hosts, total)
    outs = []
    for kind, arg in steps:
        if kind == "push":
            m.push(*[arg[k] for k in PUSH_KEYS])
        else:
            o = m.pop(arg, total)
            o["status"] = m.status()
            outs.append(o)
    return outs


# ------------------------------------------------------------ hand-made cases
class _Pair:
    """the same calls through a runner and the model"""

    def __init__(self, make, n_dst, pool_cap):
        self.r, self.m = make(n_dst, pool_cap), FM.FlightModel(n_dst, pool_cap)

    def push(self, host_ptr, flags, deliver, dst, event_id, size, tag=None):
        a = self.r.push(host_ptr, flags, deliver, dst, event_id, size, tag)
        b = self.m.push(host_ptr, flags, deliver, dst, event_id, size, tag)
        assert a == b
        return a

    def pop(self, until_ns, out_cap):
        out, mo = self.r.pop(until_ns, out_cap), self.m.pop(until_ns, out_cap)
        mo["status"] = self.m.status()
        assert_same(out, mo)
        return out

    def status(self):
        st, ms = self.r.status(), self.m.status()
        assert st[:4] == ms, (st, ms)
        return st

    def close(self):
        self.r.close()


def _sent(n):
    return [SENT] * n


def case_every_part_of_the_key_decides(make):
    """destination 0: equal deliver times across source hosts (the lower host first) and within one
    (the lower event id first), and a later time with a lower host and id that still comes last"""
    p = _Pair(make, 2, 16)
    try:
        #            host 0        host 1              host 2
        hp = [0, 2, 5, 7]
        deliver = [50, 70, 50, 50, 40, 50, 60]
        eid = [9, 1, 8, 3, 100, 0, 2]
        dst = [0, 0, 0, 0, 0, 0, 1]
        p.push(hp, _sent(7), deliver, dst, eid, [100 + k for k in range(7)])
        out = p.pop(100, 8)
        assert out["dst_ptr"].tolist() == [0, 6, 7] and out["order"].tolist() == list(range(7))
        assert out["tag"].tolist() == [4, 0, 3, 2, 5, 1, 6]
        assert out["src"].tolist() == [1, 0, 1, 1, 2, 0, 2] and out["event_id"].tolist() == [100, 9, 3, 8, 0, 1, 2]
        assert out["size"].tolist() == [104, 100, 103, 102, 105, 101, 106]
    finally:
        p.close()


def case_full_width_compares(make):
    """event ids above 2^32 that differ only there, deliver times above 2^63 that differ only in the
    low word or only in the top bit"""
    p = _Pair(make, 1, 8)
    try:
        hi, big = 1 << 63, 1 << 32
        deliver = [hi + 5, 5, hi + 5, hi + 4, hi + 5]
        eid = [2 * big + 1, 7, big + 1, 3, big + 2]
        p.push([0, 5], _sent(5), deliver, [0] * 5, eid, [1, 2, 3, 4, 5])
        out = p.pop(hi, 8)
        assert out["tag"].tolist() == [1]
        out = p.pop(U64, 8)
        assert out["tag"].tolist() == [3, 2, 4, 0] and out["status"][2] == 0
    finally:
        p.close()


def case_nothing_due_then_everything(make):
    p = _Pair(make, 3, 8)
    try:
        p.push([0, 2, 4], _sent(4), [30, 20, 20, 10], [2, 0, 2, 1], [0, 1, 0, 1], [9, 9, 9, 9], tag=[70, 71, 72, 73])
        out = p.pop(10, 4)  # deliver < until: the packet at 10 is not due at 10
        assert out["dst_ptr"].tolist() == [0, 0, 0, 0] and out["status"] == (0, 0, 4, 0) and out["untouched"]
        out = p.pop(31, 4)
        assert out["dst_ptr"].tolist() == [0, 1, 2, 4] and out["tag"].tolist() == [71, 73, 72, 70]
        assert out["status"] == (0, 4, 0, 0)
        out = p.pop(40, 4)  # the empty store
        assert out["dst_ptr"].tolist() == [0, 0, 0, 0] and out["status"] == (0, 0, 0, 0)
    finally:
        p.close()


def case_empty_pushes(make):
    """a push of zero packets, a batch with no SENT packet, then one that counts: tags run on"""
    p = _Pair(make, 2, 4)
    try:
        assert p.push([0, 0, 0], [], [], [], [], []) == 0
        assert p.push([0, 1, 3], [DROPPED, 0, SENT | DROPPED], [5, 5, 5], [0, 1, 0], [U64] * 3, [1, 1, 1]) == 0
        assert p.status()[:4] == (0, 0, 0, 0)
        assert p.push([0, 1, 2], [SENT, DROPPED], [5, 6], [1, 1], [0, U64], [7, 8]) == 3
        out = p.pop(9, 4)
        assert out["tag"].tolist() == [3] and out["dst_ptr"].tolist() == [0, 0, 1]
    finally:
        p.close()


def case_pool_exactly_full_then_one_more(make):
    p = _Pair(make, 2, 5)
    try:
        p.push([0, 3, 5], _sent(5), [10, 11, 12, 13, 14], [0, 1, 0, 1, 0], [0, 1, 2, 0, 1], [1] * 5)
        assert p.status()[:4] == (0, 0, 5, 0)
        p.push([0, 0, 1], _sent(1), [15], [0], [2], [1])
        st = p.status()
        assert st[:4] == (FM.POOL_OVERFLOW, 0, 5, 1) and "pool_cap" in st[4]
        out = p.pop(100, 5)  # the five that fitted, the guard intact
        assert out["tag"].tolist() == [0, 2, 4, 1, 3] and out["status"] == (0, 5, 0, 1) and out["untouched"]
        p.push([0, 0, 1], _sent(1), [115], [0], [3], [1])  # room again
        assert p.pop(200, 5)["tag"].tolist() == [6]
    finally:
        p.close()


def case_out_cap_exact_then_one_short(make):
    p = _Pair(make, 3, 8)
    try:
        p.push([0, 4, 6], _sent(6), [10, 20, 30, 40, 15, 25], [0, 1, 2, 0, 1, 2], [0, 1, 2, 3, 0, 1], [1] * 6)
        out = p.pop(21, 3)  # three due, room for three
        assert out["status"] == (0, 3, 3, 0) and out["tag"].tolist() == [0, 4, 1]
        out = p.pop(50, 2)  # three due, room for two: void
        assert out["status"] == (FM.OUT_OVERFLOW, 3, 3, 0) and "out_cap" in out["msg"]
        assert out["dst_ptr"].tolist() == [0, 0, 0, 0] and out["untouched"]
        out = p.pop(50, 3)  # the retry with room gives the whole window
        assert out["status"] == (0, 3, 0, 0) and out["tag"].tolist() == [3, 5, 2]
        assert out["dst_ptr"].tolist() == [0, 1, 1, 3]
    finally:
        p.close()


def case_flags_alone_and_together(make):
    p = _Pair(make, 2, 8)
    try:
        p.push([0, 3], _sent(3), [10, 11, 12], [0, 2, 0xffffffff], [0, 1, 2], [1] * 3)
        st = p.status()
        assert st[:4] == (FM.BAD_HOST, 0, 1, 0) and "dst_host" in st[4] and "until_ns" not in st[4]
        assert p.pop(20, 8)["tag"].tolist() == [0]
        p.push([0, 2], _sent(2), [19, 20], [1, 1], [3, 4], [1] * 2)  # 19 lies before the last pop
        st = p.status()
        assert st[:4] == (FM.LATE_PUSH, 1, 2, 0) and "before the last pop" in st[4] and "dst_host" not in st[4]
        out = p.r.pop(15, 8)  # a step back in time: flagged, and it takes what lies before it (nothing)
        mo = p.m.pop(15, 8)
        mo["status"] = p.m.status()
        assert_same(out, mo)
        assert out["status"] == (FM.TIME_REGRESSION, 0, 2, 0) and "backwards" in out["msg"]
        assert "dst_host" not in out["msg"] and "before the last pop" not in out["msg"]
        # two at once: a bad host and a late packet in one push, every flag with its own words
        p.push([0, 2], _sent(2), [5, 30], [1, 7], [5, 6], [1] * 2)
        st = p.status()
        assert st[:4] == (FM.BAD_HOST | FM.LATE_PUSH, 0, 3, 0)
        assert "dst_host" in st[4] and "before the last pop" in st[4] and "backwards" not in st[4]
        out = p.pop(21, 8)  # the late packets leave with the next pop
        assert out["status"] == (0, 3, 0, 0) and out["tag"].tolist() == [5, 3, 4]
    finally:
        p.close()


def case_all_five_flags_fit_one_message(make):
    p = _Pair(make, 1, 1)
    try:
        assert p.pop(20, 4)["status"] == (0, 0, 0, 0)
        p.push([0, 3], _sent(3), [3, 3, 3], [0, 5, 0], [0, 1, 2], [1] * 3)  # late; a bad host; one too many
        out = p.pop(10, 0)  # a step back, and one is due with no room
        assert out["status"] == (31, 1, 1, 1) and out["dst_ptr"].tolist() == [0, 0]
        for words in ("pool_cap", "out_cap", "dst_host", "before the last pop", "backwards"):
            assert words in out["msg"], (words, out["msg"])
    finally:
        p.close()


def case_groups_around_the_sort_capacity(make):
    """destination groups of G - 1, G, G + 1 and 3G + 5 packets (and an empty one), from 7 source
    hosts in shuffled order with tied deliver times"""
    sizes = [G - 1, 0, G, G + 1, 3 * G + 5]
    n = sum(sizes)
    rng = np.random.default_rng(3)
    dst = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.uint32)
    per = np.array([n // 7] * 6 + [n - 6 * (n // 7)])
    hp = np.concatenate([[0], np.cumsum(per)])
    eid = np.concatenate([(1 << 40) + np.arange(k, dtype=np.uint64) for k in per])
    deliver = 1000 + rng.integers(0, 40, size=n).astype(np.uint64)
    p = _Pair(make, len(sizes), n + 3)
    try:
        p.push(hp, _sent(n), deliver, dst, eid, rng.integers(40, 1500, size=n))
        out = p.pop(2000, n)
        assert np.diff(out["dst_ptr"].astype(np.int64)).tolist() == sizes and out["status"] == (0, n, 0, 0)
    finally:
        p.close()


def case_hosts_around_a_wave(make):
    """source hosts with 63, 64 and 65 sent packets in one push (unsent ones between them): the
    append's ballot at, below and above a wave"""
    rng = np.random.default_rng(4)
    flags = []
    for k in (63, 64, 65):
        f = np.array([SENT] * k + [DROPPED] * 5 + [0] * 3, np.uint32)
        flags.append(rng.permutation(f))
    per = [len(f) for f in flags]
    flags = np.concatenate(flags)
    n = len(flags)
    hp = np.concatenate([[0], np.cumsum(per)])
    eid = np.where(flags == SENT, np.arange(n, dtype=np.uint64), np.uint64(U64))
    p = _Pair(make, 4, 200)
    try:
        p.push(hp, flags, 500 + rng.integers(0, 9, size=n), rng.integers(0, 4, size=n), eid, [60] * n)
        assert p.status()[:4] == (0, 0, 192, 0)
        out = p.pop(600, 192)
        assert np.bincount(out["src"], minlength=3).tolist() == [63, 64, 65]
    finally:
        p.close()


CASES = [case_every_part_of_the_key_decides, case_full_width_compares, case_nothing_due_then_everything,
         case_empty_pushes, case_pool_exactly_full_then_one_more, case_out_cap_exact_then_one_short,
         case_flags_alone_and_together, case_all_five_flags_fit_one_message, case_groups_around_the_sort_capacity,
         case_hosts_around_a_wave]


def error_paths(plan_handle=None):
    """null arguments and SRT_ERR_INVALID of the five entry points, on raw ctypes"""
    from shadow_amd import _lib

    L, err, h = _lib.lib(), _lib.SrtErr(), C.c_void_p()
    inv = _lib.SRT_ERR_INVALID
    assert L.srt_flight_create(plan_handle, 2, 4, None, C.byref(err)) == inv and b"null" in err.msg
    assert L.srt_flight_create(plan_handle, 0xffffffff, 4, C.byref(h), C.byref(err)) == inv and not h
    assert L.srt_flight_create(plan_handle, 2, (1 << 31) + 1, C.byref(h), C.byref(err)) == inv and b"pool_cap" in err.msg
    assert L.srt_flight_status(None, None, None, None, None, C.byref(err)) == inv and b"null" in err.msg
    assert L.srt_flight_push(None, None, 0, 0, None, None, None, None, None, None, None, C.byref(err)) == inv
    assert L.srt_flight_pop(None, 0, None, None, None, None, None, None, None, 0, C.byref(err)) == inv
    L.srt_flight_destroy(None)
    if plan_handle is not None:
        return
    assert L.srt_flight_create(None, 2, 4, C.byref(h), C.byref(err)) == _lib.SRT_OK
    hp, fl = np.array([0, 1, 2], np.uint32), np.array([SENT, SENT], np.uint32)
    dl, ds = np.array([5, 6], np.uint64), np.array([1, 0], np.uint32)
    ei, sz = np.array([0, 0], np.uint64), np.array([50, 60], np.uint32)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def push(f=h, hp=hp, n=2, fl=fl, dl=dl, ds=ds, ei=ei, sz=sz):
        return L.srt_flight_push(f, p(hp), 2, n, p(fl), p(dl), p(ds), p(ei), p(sz), None, None, C.byref(err))

    for bad in (dict(f=None), dict(hp=None), dict(fl=None), dict(dl=None), dict(ds=None), dict(ei=None),
                dict(sz=None), dict(n=1 << 31)):
        assert push(**bad) == inv, bad
        assert err.code == inv and err.msg
    assert push(hp=np.zeros(3, np.uint32), n=0, fl=None, dl=None, ds=None, ei=None, sz=None) == _lib.SRT_OK
    assert push() == _lib.SRT_OK
    o4 = [np.zeros(2, np.uint32) for _ in range(3)]
    o8 = [np.zeros(2, np.uint64) for _ in range(3)]
    dp = np.full(3, 9, np.uint32)

    def pop(f=h, order=o4[0], dp=dp, dl=o8[0], sz=o4[1], src=o4[2], ei=o8[1], tag=o8[2], out_cap=2, until=10):
        return L.srt_flight_pop(f, until, p(order), p(dp), p(dl), p(sz), p(src), p(ei), p(tag), out_cap, C.byref(err))

    for bad in (dict(f=None), dict(order=None), dict(dp=None), dict(dl=None), dict(sz=None), dict(src=None),
                dict(ei=None), dict(tag=None)):
        assert pop(**bad) == inv, bad
        assert err.code == inv and b"null" in err.msg
    # nothing to write: no arrays needed; two are due, so the pop is void and says how many
    assert pop(order=None, dl=None, sz=None, src=None, ei=None, tag=None, out_cap=0) == _lib.SRT_OK
    flags, a, b, c = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.srt_flight_status(h, C.byref(flags), C.byref(a), C.byref(b), C.byref(c), C.byref(err)) == inv
    assert (flags.value, a.value, b.value, c.value) == (_lib.FLIGHT_OUT_OVERFLOW, 2, 2, 0) and b"out_cap" in err.msg
    assert dp.tolist() == [0, 0, 0]
    assert L.srt_flight_status(h, C.byref(flags), None, None, None, C.byref(err)) == _lib.SRT_OK and flags.value == 0
    assert pop() == _lib.SRT_OK and dp.tolist() == [0, 1, 2] and o8[2].tolist() == [1, 0] and o4[1].tolist() == [60, 50]
    assert L.srt_flight_status(h, None, C.byref(a), C.byref(b), None, None) == _lib.SRT_OK and (a.value, b.value) == (2, 0)
    L.srt_flight_destroy(h)
