"""Seeded multi-window scenarios for the UDP send side (srt_udpsend) and the
harness that runs them on an instance (host-only with plan=None, or on a
RoutingPlan's device) and on the plain-Python model (udpsend_model.py).

Seven windows of 100 ms over n_hosts hosts with 0 to 5 socket slots each.  About
one slot in six is never opened (a TCP socket: it hands raw packets to the
interface).  Two shapes: FREE, where bandwidth and limits are so large that
nothing ever blocks, and THROTTLED, where every host has 1,000 to 100,000 B/s
of upload and every socket a limit of 4,096 bytes, so that sends are refused,
arm, wake inside their call and across calls.  Between windows sockets are
connected, resized, shut, closed and reopened.  Call times lie on a coarse grid
so that instants repeat; the last window has no calls and drains.  The flags a
scenario raises (ARMED_TWICE, REOPEN_BUSY, ...) are compared like any output."""
import functools
import json
import os

import numpy as np

import udpsend_model as M
from udprecv_scenario import _dev, _host

N_WIN = 7
MS = 1_000_000
W = 100 * MS
GRID = 250_000
FREE, THROTTLED = "free", "throttled"
RING_CAP = 512
LATE_CAP = 4096
U64 = M.U64


def ip_of(h):
    """host h's address, big-endian bytes 11.x.y.z"""
    return int.from_bytes(bytes([11, (h >> 16) & 255, (h >> 8) & 255, h & 255]), "little")


def layout(n_hosts, shape, seed=5):
    rng = np.random.default_rng(seed * 1000 + n_hosts * 2 + (shape == FREE))
    counts = rng.integers(0, 6, n_hosts)
    if n_hosts > 2:
        counts[0], counts[1], counts[2] = 5, 0, 1
    sp = np.zeros(n_hosts + 1, np.uint32)
    sp[1:] = np.cumsum(counts)
    ips = np.array([ip_of(h) for h in range(n_hosts)], np.uint32)
    bw = np.full(n_hosts, 10 ** 10, np.uint64) if shape == FREE else \
        rng.choice([1000, 10000, 50000, 100000], n_hosts).astype(np.uint64)
    return rng, sp, ips, bw


@functools.lru_cache(maxsize=None)
def scenario(n_hosts, shape, qdisc=M.FIFO, per_host=None, seed=5):
    """-> dict(socket_ptr, ips, bw, qdisc, windows=[dict(ops, calls, host_ptr, until_ns, boot_end)])
    per_host: calls a host makes in a window (default: 0 to 40)"""
    rng, sp, ips, bw = layout(n_hosts, shape, seed)
    n_sock = int(sp[-1])
    udp = rng.random(n_sock) > 1 / 6
    is_open = np.zeros(n_sock, bool)
    has_peer = np.zeros(n_sock, bool)
    limit = 4096 if shape == THROTTLED else 1 << 24
    windows = []
    for w in range(N_WIN):
        ops = []
        for x in range(n_sock):
            if not udp[x]:
                continue
            if w == 0 or (not is_open[x] and rng.random() < .5):
                ops.append((M.OPEN, x, limit))
                is_open[x], has_peer[x] = True, False
                if rng.random() < .95:  # the rest stay unbound
                    ops.append((M.BIND, x, (0 if rng.random() < .5 else int(ips[np.searchsorted(sp, x, "right") - 1])) |
                                int(rng.integers(1, 1 << 16)) << 32))
                if rng.random() < .5:
                    ops.append((M.SET_PEER, x, ip_of(int(rng.integers(0, n_hosts))) | int(rng.integers(1, 1 << 16)) << 32))
                    has_peer[x] = True
            elif rng.random() < .05:
                ops.append((M.CLOSE, x, 0))
                is_open[x] = False
            elif rng.random() < .08:
                ops.append((M.SET_SNDBUF, x, int(rng.choice([1, 2048, 3000]) if shape == THROTTLED else 1 << 30)))
            elif rng.random() < .03:
                ops.append((M.SHUT_WR, x, 0))
            elif rng.random() < .03:
                ops.append((M.OPEN, x, limit))  # busy, or a fresh socket
                is_open[x], has_peer[x] = True, False
        if w == 3 and n_hosts:
            ops.append((M.SET_NEXT_PRIORITY, n_hosts - 1, 1 << 40))
        ops = np.array(ops, M.OP) if ops else np.zeros(0, M.OP)
        last = w == N_WIN - 1
        per = np.zeros(n_hosts, np.int64) if last else (
            rng.integers(0, 41, n_hosts) if per_host is None else np.full(n_hosts, per_host, np.int64))
        per[np.diff(sp.astype(np.int64)) == 0] = 0
        hp = np.zeros(n_hosts + 1, np.uint32)
        hp[1:] = np.cumsum(per)
        calls = np.zeros(int(hp[-1]), M.SEND)
        for h in range(n_hosts):
            b, e = int(hp[h]), int(hp[h + 1])
            lo, hi = int(sp[h]), int(sp[h + 1])
            calls["time_ns"][b:e] = w * W + np.sort(rng.integers(0, W // GRID, e - b)) * GRID
            for k in range(b, e):
                c = calls[k]
                x = int(rng.integers(lo, hi))
                c["slot"], c["user"] = x, rng.integers(0, 1 << 32)
                if not udp[x]:
                    c["flags"] = M.RAW | (M.LOCAL if rng.random() < .1 else 0)
                    c["len"], c["priority"] = rng.integers(40, 1501), rng.integers(1, 1 << 20)
                    continue
                c["len"] = 0 if rng.random() < .05 else rng.integers(1, 1473) if rng.random() < .98 else 70000
                fl = M.WAIT if rng.random() < .5 else 0
                if not has_peer[x] or rng.random() < .5:
                    if rng.random() < .97:
                        fl |= M.HAS_ADDR
                    r = rng.random()
                    c["dst_ip_be"] = int(ips[h]) if r < .1 else M.LOCALHOST if r < .12 else ip_of(int(rng.integers(0, n_hosts)))
                    c["dst_port_be"] = rng.integers(1, 1 << 16)
                c["flags"] = fl
        windows.append(dict(ops=ops, calls=calls, host_ptr=hp, until_ns=(w + 1) * W, boot_end=W // 2))
    return dict(socket_ptr=sp, ips=ips, bw=bw, qdisc=qdisc, windows=windows)


# ---- the model
def model_scenario(sc, ring_cap=RING_CAP):
    """-> (per-window outputs, (hosts, socks) state, status)"""
    m = M.UdpSendModel(sc["socket_ptr"], sc["ips"], sc["bw"], sc["qdisc"], ring_cap)
    outs = []
    for w in sc["windows"]:
        m.config(w["ops"])
        outs.append(m.run(w["calls"], w["host_ptr"], w["until_ns"], w.get("boot_end", 0)))
    return outs, m.state(), m.take_status()


def scenario_stats(sc):
    """what the model saw: asserted by the tests so that an empty scenario cannot pass"""
    outs, (hosts, socks), status = model_scenario(sc)
    st = dict(accepted=status[2], would_block=status[3], armed=status[4], woken_same_call=0, woken_later=0, late_pkts=0,
              cached=0, local=0, first_writable=0)
    for w, o in zip(sc["windows"], outs):
        r, c = o["results"], w["calls"]
        st["woken_same_call"] += int(((r["status"] == M.DONE) & (r["return_val"] >= 0) &
                                      (r["complete_ns"] > c["time_ns"])).sum())
        st["woken_later"] += len(o["late_results"])
        st["late_pkts"] += len(o["late"])
        st["cached"] += int((o["status"] & M.CACHED != 0).sum())
        st["local"] += int(((o["status"] & M.FORWARDED != 0) & (o["send_rank"] == U64)).sum())
        st["first_writable"] += int((o["first_writable"] != U64).sum())
    return st


# ---- the instance under test
class Runner:
    """a UdpSend instance fed window by window; outputs as the model returns them"""

    def __init__(self, plan, sc, ring_cap=RING_CAP, late_cap=LATE_CAP):
        from shadow_amd.plan import UdpSend

        self.plan, self.late_cap = plan, late_cap
        self.us = UdpSend(plan, sc["socket_ptr"], sc["ips"], sc["bw"], sc["qdisc"], ring_cap, late_cap)

    def window(self, win, keep_device=False):
        us, plan = self.us, self.plan
        us.config(win["ops"])
        calls = win["calls"]
        n = len(calls)
        dev = lambda a: _dev(a, plan)  # noqa: E731
        results = dev(np.full(max(n, 1) * 40, 0xEE, np.uint8))[:40 * n]
        status = dev(np.full(max(n, 1), 0xDEAD, np.uint32))[:n]
        send_ns = dev(np.full(max(n, 1), 7, np.uint64))[:n]
        rank = dev(np.full(max(n, 1), 7, np.uint64))[:n]
        late = dev(np.zeros(self.late_cap, M.LATE))
        late_count = dev(np.full(1, 77, np.uint32))
        late_res = dev(np.zeros(self.late_cap, M.LATE_RESULT))
        late_res_count = dev(np.full(1, 77, np.uint32))
        first = dev(np.zeros(max(us.n_sockets, 1), np.uint64))
        d_calls = dev(calls if n else np.zeros(1, M.SEND))[:40 * n] if plan is not None else calls
        d_hp = dev(win["host_ptr"])
        base = us.run(d_hp, d_calls, win["until_ns"], win.get("boot_end", 0), results, status, send_ns, rank, late,
                      late_count, late_res, late_res_count, first)
        if keep_device:
            return dict(host_ptr=d_hp, send_ns=send_ns, send_rank=rank, late=late, late_count=late_count, base=base)
        n_late = int(_host(late_count, np.uint32)[0])
        la = _host(late, M.LATE)[:min(n_late, self.late_cap)]
        n_lr = int(_host(late_res_count, np.uint32)[0])
        lr = _host(late_res, M.LATE_RESULT)[:min(n_lr, self.late_cap)].copy()
        return dict(results=_host(results, M.RESULT, n).copy(), status=_host(status, np.uint32, n).copy(),
                    send_ns=_host(send_ns, np.uint64, n).copy(), send_rank=_host(rank, np.uint64, n).copy(),
                    late=sorted(tuple(int(v) for v in x) for x in la.tolist()),
                    late_results=lr[np.argsort(lr["seq"], kind="stable")],
                    first_writable=_host(first, np.uint64, us.n_sockets).copy(), base=base)

    def cached(self):
        """srt_udpsend_cached_seq after the last window"""
        out = _dev(np.zeros(max(self.us.n_hosts, 1), np.uint64), self.plan)
        return _host(self.us.cached_seq(out), np.uint64, self.us.n_hosts).copy()

    def finish(self):
        st = self.us.state()
        status = self.us.status(check=False)
        self.us.close()
        return st, status


def run_scenario(plan, sc, ring_cap=RING_CAP):
    r = Runner(plan, sc, ring_cap)
    outs = [r.window(w) for w in sc["windows"]]
    return (outs,) + r.finish()


def same_outputs(a, b, where=""):
    """two windows' outputs, byte for byte"""
    for k in ("results", "status", "send_ns", "send_rank", "late_results", "first_writable"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (where, k, a[k].shape, b[k].shape)
        if a[k].tobytes() != b[k].tobytes():
            bad = np.flatnonzero(a[k] != b[k])[:5]
            raise AssertionError((where, k, bad, a[k][bad], b[k][bad]))
    assert a["late"] == b["late"], (where, a["late"][:5], b["late"][:5])
    assert a["base"] == b["base"], where


def same_state(a, b, skip_hosts=()):
    """(hosts, socks) twice; skip_hosts: (host, its slots) pairs left out"""
    for x, y, skip in ((a[0], b[0], [h for h, _ in skip_hosts]), (a[1], b[1], [s for _, ss in skip_hosts for s in ss])):
        keep = np.ones(len(x), bool)
        keep[skip] = False
        assert x[keep].tobytes() == y[keep].tobytes(), [(i, x[i], y[i]) for i in np.flatnonzero((x != y) & keep)[:5]]


def compare(plan, sc, ring_cap=RING_CAP):
    """the instance against the model on every window, the state and the status; returns the status"""
    outs, st, status = run_scenario(plan, sc, ring_cap)
    m_outs, m_st, m_status = model_scenario(sc, ring_cap)
    assert len(outs) == len(m_outs)
    for k, (a, b) in enumerate(zip(outs, m_outs)):
        same_outputs(a, b, k)
    same_state(st, m_st)
    assert status == m_status, (status, m_status)
    return status


# ---- one window cut in two at time t
def split_window(win, t):
    calls, hp = win["calls"], win["host_ptr"]
    early = calls["time_ns"] < t
    parts = []
    for keep in (early, ~early):
        p = np.zeros(len(hp), np.uint32)
        for h in range(len(hp) - 1):
            p[h + 1] = p[h] + keep[hp[h]:hp[h + 1]].sum()
        parts.append(p)
    first = dict(win, calls=calls[early], host_ptr=parts[0], until_ns=t)
    second = dict(win, ops=np.zeros(0, M.OP), calls=calls[~early], host_ptr=parts[1])
    return first, second, early


def merge_split(o1, o2, early, cached=(), raw=None):
    """the two calls' outputs as the one call over the whole window reports them; cached: the sequence numbers
    the relays hold after the second call (a packet of the first call that the second popped and still holds
    is in neither call's arrays), raw[i]: call i is a raw arrival"""
    n = len(early)
    res = np.zeros(n, M.RESULT)
    res[early], res[~early] = o1["results"], o2["results"]
    out = {}
    for k, dt in (("status", np.uint32), ("send_ns", np.uint64), ("send_rank", np.uint64)):
        out[k] = np.zeros(n, dt)
        out[k][early], out[k][~early] = o1[k], o2[k]
    idx1 = np.flatnonzero(early)
    late = []
    for seq, send_ns, rank, st, h in o2["late"]:  # a packet of the first call forwarded in the second
        i = seq - o1["base"]
        if 0 <= i < len(idx1):
            out["status"][idx1[i]], out["send_ns"][idx1[i]] = st, send_ns
            out["send_rank"][idx1[i]] = rank
        else:
            late.append((seq, send_ns, rank, st, h))
    for seq in cached:
        i = int(seq) - o1["base"]
        if seq != U64 and 0 <= i < len(idx1):
            out["status"][idx1[i]] = M.INTERFACE_SENT | M.CACHED | (0 if raw[idx1[i]] else M.SND_CREATED)
    late_res = []
    for l in o2["late_results"]:  # a send armed in the first call and woken in the second
        i = int(l["seq"]) - o1["base"]
        if 0 <= i < len(idx1):
            user = res[idx1[i]]["user"]
            res[idx1[i]] = l["result"]
            assert res[idx1[i]]["user"] == user
        else:
            late_res.append(l)
    out.update(results=res, late=sorted(o1["late"] + late),
               late_results=np.array(list(o1["late_results"]) + late_res, M.LATE_RESULT),
               first_writable=np.minimum(o1["first_writable"], o2["first_writable"]))
    return out


def one_call_against_split(plan, n_hosts=40):
    """every window of a throttled scenario once whole and once cut in two at a grid time.  The cut run numbers
    a window's calls differently (every host's early calls, then every host's late ones): remap[] takes its
    sequence numbers to the whole run's."""
    sc = scenario(n_hosts, THROTTLED, M.FIFO)
    whole, cut = Runner(plan, sc), Runner(plan, sc)
    n_cut = 0
    remap = np.zeros(0, np.uint64)
    for k, win in enumerate(sc["windows"]):
        t = k * W + (W // GRID // 3) * GRID
        a = whole.window(win)
        w1, w2, early = split_window(win, t)
        o1, o2 = cut.window(w1), cut.window(w2)
        b = merge_split(o1, o2, early, cut.cached(), win["calls"]["flags"] & M.RAW != 0)
        remap = np.concatenate([remap, a["base"] + np.flatnonzero(early), a["base"] + np.flatnonzero(~early)]).astype(np.uint64)
        n_cut += int(early.sum() and (~early).sum())
        for key in ("results", "status", "send_ns", "send_rank", "first_writable"):
            assert a[key].tobytes() == b[key].tobytes(), (k, key, np.flatnonzero(a[key] != b[key])[:5])
        assert a["late"] == sorted((int(remap[x[0]]),) + x[1:] for x in b["late"]), k
        lr = b["late_results"].copy()
        lr["seq"] = remap[lr["seq"].astype(np.int64)]
        assert a["late_results"].tobytes() == lr[np.argsort(lr["seq"])].tobytes(), k
    assert n_cut >= 5
    sa, fa = whole.finish()
    sb, fb = cut.finish()
    armed = sb[1]["armed_seq"] != U64
    sb[1]["armed_seq"][armed] = remap[sb[1]["armed_seq"][armed].astype(np.int64)]
    same_state(sa, sb)
    assert fa == fb


# ---- plain shapes for the kernel's edges: every slot an open, bound, connected UDP socket
def simple_scenario(counts, per, qdisc=M.FIFO, n_win=3, seed=11, lens=None, bws=None):
    """counts[h]: host h's slots; per[h]: its calls in each of n_win windows (a last window drains); lens[h]:
    (lo, hi) of its payloads; bws[h]: its upload bandwidth (default: a seeded pick of 20,000 to 10^6 B/s)"""
    rng = np.random.default_rng(seed)
    n_hosts = len(counts)
    sp = np.zeros(n_hosts + 1, np.uint32)
    sp[1:] = np.cumsum(counts)
    ips = np.array([ip_of(h) for h in range(n_hosts)], np.uint32)
    bw = rng.choice([20000, 100000, 10 ** 6], n_hosts).astype(np.uint64) if bws is None else np.array(bws, np.uint64)
    ops = []
    for x in range(int(sp[-1])):
        ops += [(M.OPEN, x, 4096), (M.BIND, x, (1 + x % 60000) << 32), (M.SET_PEER, x, ip_of((x * 7 + 1) % n_hosts) | 9 << 32)]
    hp = np.zeros(n_hosts + 1, np.uint32)
    hp[1:] = np.cumsum(np.where(np.array(counts) > 0, per, 0))
    windows = []
    for w in range(n_win + 1):
        if w == n_win:
            hp = np.zeros(n_hosts + 1, np.uint32)
        calls = np.zeros(int(hp[-1]), M.SEND)
        for h in range(n_hosts):
            b, e = int(hp[h]), int(hp[h + 1])
            if e == b:
                continue
            lo, hi = (1, 1473) if lens is None else lens[h]
            calls["time_ns"][b:e] = w * W + np.sort(rng.integers(0, W // GRID, e - b)) * GRID
            calls["slot"][b:e] = rng.integers(int(sp[h]), int(sp[h + 1]), e - b)
            calls["len"][b:e] = rng.integers(lo, hi, e - b)
            calls["flags"][b:e] = np.where(rng.random(e - b) < .5, M.WAIT, 0)
        calls["user"] = rng.integers(0, 1 << 32, len(calls))
        windows.append(dict(ops=np.array(ops if w == 0 else [], M.OP) if w == 0 else np.zeros(0, M.OP), calls=calls,
                            host_ptr=hp.copy(), until_ns=(w + 1) * W if w < n_win else 100 * W, boot_end=0))
    return dict(socket_ptr=sp, ips=ips, bw=bw, qdisc=qdisc, windows=windows)


# ---- raw arrivals only: the outbound relay's own list
def raw_only(n_hosts=70, max_sockets=3, seed=3):
    """-> (socket_ptr, ips, bw, windows as OUT_PKT arrays with host_ptr and until_ns) for both stages"""
    rng = np.random.default_rng(seed)
    sp = (np.arange(n_hosts + 1) * max_sockets).astype(np.uint32)
    bw = rng.choice([1000, 20000, 100000, 10 ** 9], n_hosts).astype(np.uint64)
    ips = np.array([ip_of(h) for h in range(n_hosts)], np.uint32)
    from shadow_amd.plan import OUT_PKT_DTYPE

    wins = []
    for w in range(4):
        per = rng.integers(0, 30, n_hosts) if w < 3 else np.zeros(n_hosts, np.int64)
        hp = np.zeros(n_hosts + 1, np.uint32)
        hp[1:] = np.cumsum(per)
        pk = np.zeros(int(hp[-1]), OUT_PKT_DTYPE)
        for h in range(n_hosts):
            b, e = int(hp[h]), int(hp[h + 1])
            pk["ready_ns"][b:e] = w * W + np.sort(rng.integers(0, W // GRID, e - b)) * GRID
        pk["priority"] = rng.permutation(len(pk)) + 1 + w * 100000
        pk["total_size"] = rng.integers(40, 1501, len(pk))
        pk["socket"] = rng.integers(0, max_sockets, len(pk))
        pk["flags"] = rng.random(len(pk)) < .1
        wins.append(dict(pkts=pk, host_ptr=hp, until_ns=(w + 1) * W))
    return sp, ips, bw, wins


def raw_calls(pk, hp, sp):
    """srt_out_pkt records as the raw arrivals of srt_udpsend"""
    c = np.zeros(len(pk), M.SEND)
    host = np.repeat(np.arange(len(hp) - 1), np.diff(hp.astype(np.int64)))
    c["time_ns"], c["priority"], c["len"] = pk["ready_ns"], pk["priority"], pk["total_size"]
    c["slot"] = sp[host] + pk["socket"]
    c["flags"] = M.RAW | np.where(pk["flags"] & 1, M.LOCAL, 0)
    return c


# ---- the hand-worked cases of tests/golden/udpsend_cases.json
def golden_cases():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "udpsend_cases.json")) as f:
        return json.load(f)["cases"]


def golden_scenario(case):
    """calls rows: [host, time_ns, slot, len, dst_ip, flags, priority]"""
    sp = np.array(case["socket_ptr"], np.uint32)
    nh = len(sp) - 1
    wins = []
    for c in case["calls"]:
        rows = sorted(c["sends"], key=lambda r: r[0])  # stable: by host, list order kept
        calls = np.zeros(len(rows), M.SEND)
        hp = np.zeros(nh + 1, np.uint32)
        for k, r in enumerate(rows):
            r = list(r) + [0] * (7 - len(r))
            calls[k] = (r[1], r[6], r[2], r[3], r[4], 0, 0, r[5], 1000 + k)
            hp[r[0] + 1:] += 1
        wins.append(dict(ops=np.array([tuple(o) for o in c.get("ops", [])], M.OP), calls=calls, host_ptr=hp,
                         until_ns=c["until"], boot_end=c.get("boot_end", 0)))
    return dict(socket_ptr=sp, ips=np.array(case["host_ip"], np.uint32), bw=np.array(case["bw_up"], np.uint64),
                qdisc=case.get("qdisc", M.FIFO), windows=wins)


def check_golden(case, outs, state, status):
    """the expectations the case states, against one implementation's outputs"""
    hosts, socks = state
    for k, (c, o) in enumerate(zip(case["calls"], outs)):
        ex = c.get("expect", {})
        for key in ("return_val", "status", "priority", "complete_ns", "src_ip_be", "src_port_be"):
            if key in ex:
                assert [int(v) for v in o["results"][key]] == ex[key], (case["name"], k, key, o["results"][key])
        for key, name in (("pds_status", "status"), ("send_ns", "send_ns"), ("send_rank", "send_rank"),
                          ("first_writable", "first_writable")):
            if key in ex:
                want = [U64 if v == -1 else v for v in ex[key]]
                assert [int(v) for v in o[name]] == want, (case["name"], k, key, o[name])
        if "late" in ex:  # [seq, send_ns, send_rank (-1: none)]
            assert [[a, b, -1 if r == U64 else r] for a, b, r, _, _ in o["late"]] == ex["late"], (case["name"], k, o["late"])
        if "late_results" in ex:  # [seq, return_val, complete_ns, priority]
            got = [[int(l["seq"]), int(l["result"]["return_val"]), int(l["result"]["complete_ns"]),
                    int(l["result"]["priority"])] for l in o["late_results"]]
            assert got == ex["late_results"], (case["name"], k, got)
    fin = case.get("final", {})
    for key, v in fin.get("hosts", {}).items():
        assert [int(x) for x in hosts[key]] == [U64 if y == -1 else y for y in v], (case["name"], key, hosts[key])
    for key, v in fin.get("socks", {}).items():
        assert [int(x) for x in socks[key]] == [U64 if y == -1 else y for y in v], (case["name"], key, socks[key])
    if "flags" in fin:
        assert status[0] == fin["flags"], (case["name"], status)
