"""Seeded multi-window scenarios for the UDP receive stage (srt_udprecv) and the
harness that runs them on an instance (host-only with plan=None, or on a
RoutingPlan's device) and on the plain-Python model (udprecv_model.py).

Seven windows of 20 ms over n_hosts hosts with 0 to 70 socket slots each: host 0
has 70 (more than a wave of 64, so its slots straddle a wave boundary and so do
its neighbours'), host 1 none, the others a seeded pick.  About one slot in seven
is never opened (foreign to the stage: a TCP socket).  Between windows sockets are
connected, resized, closed and reopened.  Every window has a delivery list as
srt_deliver_run emits it (grouped by host, forward_ns nondecreasing within a host,
on a coarse grid so that instants repeat; records without a socket and placeholder
records among them) and a list of reads on the same grid.  A read that would find
its socket with a blocked read already armed has its WAIT flag cleared (the model
decides), so no scenario raises a flag and the comparisons exclude nothing."""
import copy
import functools

import numpy as np

import udprecv_model as M

N_WIN = 7
MS = 1_000_000
W = 20 * MS
GRID = 50_000  # ns: event times are multiples, so pushes and reads meet at equal instants
DENSE, SPARSE = "dense", "sparse"
RING_CAP = 512
HIT = (1 << 22) | (1 << 13)  # RELAY_FORWARDED | RCV_INTERFACE_RECEIVED
MISS = HIT | (1 << 14)       # no socket: RCV_INTERFACE_DROPPED
PLACEHOLDER = 1 << 22        # deliver's placeholder record: never received


def socket_counts(n_hosts, rng):
    c = rng.choice([0, 1, 2, 3, 5, 8, 30, 70], size=n_hosts, p=[.1, .2, .2, .15, .15, .1, .05, .05])
    c[0] = 70
    if n_hosts > 1:
        c[1] = 0
    return c.astype(np.int64)


@functools.lru_cache(maxsize=None)
def scenario(n_hosts, shape, seed=7):
    """-> dict(socket_ptr, windows=[dict(ops, meta, tag_base, out_host_ptr, out_socket, out_forward_ns, out_tag,
    out_status, read_host_ptr, reads, until_ns)])"""
    rng = np.random.default_rng(seed * 1000 + n_hosts * 2 + (shape == DENSE))
    counts = socket_counts(n_hosts, rng)
    sp = np.zeros(n_hosts + 1, np.uint32)
    sp[1:] = np.cumsum(counts)
    n_sock = int(sp[-1])
    udp = rng.random(n_sock) > 1 / 7  # the rest stay foreign
    peer = {}                         # slot -> (ip, port) when connected
    is_open = np.zeros(n_sock, bool)
    model = M.Model(sp, RING_CAP, 1 << 20)
    windows = []
    tag_base = 0
    for w in range(N_WIN):
        ops = []
        for x in range(n_sock):
            if not udp[x]:
                continue
            if w == 0 or (not is_open[x] and rng.random() < .5):
                ops.append((M.OPEN, x, int(rng.choice([10, 300, 3000, 1 << 20]))))
                is_open[x] = True
                peer.pop(x, None)
                if rng.random() < .3:
                    peer[x] = (int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 16)))
                    ops.append((M.SET_PEER, x, peer[x][0] | peer[x][1] << 32))
            elif rng.random() < .06:
                ops.append((M.CLOSE, x, 0))
                is_open[x] = False
                peer.pop(x, None)
            elif rng.random() < .1:
                ops.append((M.SET_RCVBUF, x, int(rng.choice([0, 1024, 5000, 1 << 30]))))
            elif rng.random() < .05:
                peer.pop(x, None)
                ops.append((M.SET_PEER, x, 0))
        ops = np.array(ops, M.OP) if ops else np.zeros(0, M.OP)
        last = w == N_WIN - 1
        per = np.zeros(n_hosts, np.int64) if last else (
            rng.integers(0, 130, n_hosts) if shape == DENSE else rng.integers(0, 7, n_hosts))
        hp = np.zeros(n_hosts + 1, np.uint32)
        hp[1:] = np.cumsum(per)
        n = int(hp[-1])
        meta = np.zeros(n, M.META)
        sock = np.zeros(n, np.uint32)
        fwd = np.zeros(n, np.uint64)
        status = np.full(n, HIT, np.uint32)
        tag = (tag_base + rng.permutation(n)).astype(np.uint64)
        rper = np.zeros(n_hosts, np.int64)
        read_rows = []
        for h in range(n_hosts):
            b, e = int(hp[h]), int(hp[h + 1])
            fwd[b:e] = w * W + np.sort(rng.integers(0, W // GRID, e - b)) * GRID
            lo, hi = int(sp[h]), int(sp[h + 1])
            for k in range(b, e):
                r = rng.random()
                if hi == lo or r < .05:
                    sock[k], status[k] = M.NO_SOCKET, MISS
                elif r < .07:
                    sock[k], status[k] = M.NO_SOCKET, PLACEHOLDER
                else:
                    sock[k] = rng.integers(lo, hi)
                m = meta[k]  # the note is in list order here; the tags are a permutation of it
                x = int(sock[k])
                if x in peer and rng.random() < .8:
                    m["src_ip_be"], m["src_port_be"] = peer[x]
                    if rng.random() < .1:
                        m["src_port_be"] ^= 1  # the port alone differs
                else:
                    m["src_ip_be"], m["src_port_be"] = rng.integers(1, 1 << 32), rng.integers(1, 1 << 16)
                m["payload_size"] = 0 if rng.random() < .1 else rng.integers(1, 1401)
                m["user"] = rng.integers(0, 1 << 32)
            open_here = [x for x in range(lo, hi) if is_open[x]]
            if open_here:
                nr = int(rng.integers(0, 150)) if shape == DENSE else int(rng.integers(0, 9))
                ts = w * W + np.sort(rng.integers(0, W // GRID, nr)) * GRID
                for t in ts:
                    fl = (M.PEEK if rng.random() < .15 else 0) | (M.TRUNC if rng.random() < .25 else 0) | \
                        (M.WAIT if rng.random() < .4 else 0)
                    read_rows.append((int(t), int(rng.choice(open_here)), int(rng.choice([0, 16, 200, 2000])), fl,
                                      int(rng.integers(0, 1 << 32))))
                rper[h] = nr
        rp = np.zeros(n_hosts + 1, np.uint32)
        rp[1:] = np.cumsum(rper)
        reads = np.array(read_rows, M.READ) if read_rows else np.zeros(0, M.READ)
        # the note carries meta by tag: note[tag - tag_base] belongs to the record with that tag
        note = np.zeros(n, M.META)
        note[(tag - tag_base).astype(np.int64)] = meta
        until = (w + 1) * W
        win = dict(ops=ops, meta=note, tag_base=tag_base, out_host_ptr=hp, out_socket=sock, out_forward_ns=fwd,
                   out_tag=tag, out_status=status, read_host_ptr=rp, reads=reads, until_ns=until)
        # a read that would be the second blocked one of its socket does not wait
        trial = copy.deepcopy(model)
        out = run_window(trial, win)
        twice = (out["results"]["return_val"] == -M.EWOULDBLOCK) & ((reads["flags"] & M.WAIT) != 0)
        reads["flags"][twice] &= ~np.uint32(M.WAIT)
        run_window(model, win)
        assert model.status()[0] == 0
        windows.append(win)
        tag_base += n
    return dict(socket_ptr=sp, windows=windows, model=model)


def run_window(model, win):
    model.config(win["ops"])
    model.note(win["meta"], win["tag_base"])
    return model.run(win["out_host_ptr"], win["out_socket"], win["out_forward_ns"], win["out_tag"],
                     win["out_status"], win["read_host_ptr"], win["reads"], win["until_ns"])


def model_scenario(n_hosts, shape, windows=None, socket_ptr=None, ring_cap=RING_CAP):
    """-> (per-window outputs, final state, status, stats)"""
    if windows is None:
        sc = scenario(n_hosts, shape)
        windows, socket_ptr = sc["windows"], sc["socket_ptr"]
    m = M.Model(socket_ptr, ring_cap, 1 << 20)
    outs = [run_window(m, w) for w in windows]
    return outs, m.state(), m.status(), m.stats


def assert_scenario_is_not_empty(n_hosts, shape):
    """on the generator and the model alone"""
    sc = scenario(n_hosts, shape)
    st = sc["model"].stats
    for k in ("drop_full", "drop_peer", "read_same_call", "read_carried", "truncated", "peek", "ewouldblock",
              "armed_same_call", "armed_later_call", "zero_length", "foreign"):
        assert st[k] > 10, (k, dict(st))
    return dict(st)


# ---- the instance under test
def _dev(a, plan):
    """a numpy array as the instance takes it: itself, or a torch tensor on the plan's device (unsigned
    integers and records as their signed or byte views)"""
    if plan is None:
        return a
    import torch

    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    a = np.ascontiguousarray(a)
    a = a.view(view) if view is not None else a.view(np.uint8) if a.dtype.fields else a
    return torch.from_numpy(a.copy()).to("cuda:0")


def _host(t, dtype, n=None):
    a = t if isinstance(t, np.ndarray) else t.cpu().numpy()
    a = np.ascontiguousarray(a).view(np.uint8).view(dtype)
    return a if n is None else a[:n]


class Runner:
    """a UdpReceive instance fed window by window; outputs as the model returns them"""

    def __init__(self, plan, socket_ptr, ring_cap=RING_CAP, note_cap=1 << 20, late_cap=4096):
        from shadow_amd.plan import UdpReceive

        self.plan = plan
        self.ur = UdpReceive(plan, socket_ptr, ring_cap, note_cap, late_cap)
        self.late_cap = late_cap

    def window(self, win):
        ur, plan = self.ur, self.plan
        ur.config(win["ops"])
        if len(win["meta"]):
            ur.note(_dev(win["meta"], plan), win["tag_base"])
        n, n_reads = len(win["out_socket"]), len(win["reads"])
        pad = lambda a: a if len(a) else np.zeros(1, a.dtype)  # noqa: E731  (a tensor needs an address)
        rx = _dev(np.full(max(n, 1), 0xDEAD, np.uint32), plan)[:n]
        results = _dev(np.full(max(n_reads, 1), 0xEE, np.uint8).repeat(56), plan)[:56 * n_reads]
        late = _dev(np.zeros(self.late_cap, M.LATE), plan)
        late_count = _dev(np.full(1, 77, np.uint32), plan)
        first = _dev(np.zeros(max(ur.n_sockets, 1), np.uint64), plan)
        base = ur.run(_dev(win["out_host_ptr"], plan), _dev(pad(win["out_socket"]), plan)[:n],
                      _dev(pad(win["out_forward_ns"]), plan)[:n], _dev(pad(win["out_tag"]), plan)[:n],
                      _dev(pad(win["out_status"]), plan)[:n],
                      _dev(win["read_host_ptr"], plan) if n_reads else None,
                      _dev(win["reads"], plan) if n_reads else None, win["until_ns"], rx, results, late, late_count,
                      first)
        lim = min(int(win["out_host_ptr"][-1]), n)
        n_late = int(_host(late_count, np.uint32)[0])
        late_a = _host(late, M.LATE)[:min(n_late, self.late_cap)].copy()
        late_a = late_a[np.argsort(late_a["seq"], kind="stable")]
        return dict(rx_status=_host(rx, np.uint32, lim).copy(), results=_host(results, M.RESULT, n_reads).copy(),
                    late=late_a, first_readable=_host(first, np.uint64, ur.n_sockets).copy(), seq_base=base,
                    n_late=n_late)

    def finish(self):
        st = self.ur.state()
        status = self.ur.status(check=False)
        self.ur.close()
        return st, status


def run_scenario(plan, n_hosts, shape, windows=None, socket_ptr=None, ring_cap=RING_CAP):
    if windows is None:
        sc = scenario(n_hosts, shape)
        windows, socket_ptr = sc["windows"], sc["socket_ptr"]
    r = Runner(plan, socket_ptr, ring_cap)
    outs = [r.window(w) for w in windows]
    return (outs,) + r.finish()


def same_outputs(a, b, where=""):
    """two windows' outputs, byte for byte"""
    for k in ("rx_status", "results", "late", "first_readable"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (where, k, a[k].shape, b[k].shape)
        if a[k].tobytes() != b[k].tobytes():
            bad = np.flatnonzero(a[k] != b[k])[:5]
            raise AssertionError((where, k, bad, a[k][bad], b[k][bad]))
    assert a["seq_base"] == b["seq_base"], where


def same_state(a, b):
    assert a.tobytes() == b.tobytes(), [(i, a[i], b[i]) for i in np.flatnonzero(a != b)[:5]]


# ---- one window cut in two at time t
def split_window(win, t):
    """-> (first, second, read_map): the records and reads before t, then the rest; read_map[i] = (call, index)
    of read i of the whole window"""
    nh = len(win["out_host_ptr"]) - 1
    parts = []
    for sel in (lambda x: x < t, lambda x: x >= t):
        keep = sel(win["out_forward_ns"])
        rkeep = sel(win["reads"]["time_ns"]) if len(win["reads"]) else np.zeros(0, bool)
        hp = np.zeros(nh + 1, np.uint32)
        rp = np.zeros(nh + 1, np.uint32)
        for h in range(nh):
            hp[h + 1] = hp[h] + keep[win["out_host_ptr"][h]:win["out_host_ptr"][h + 1]].sum()
            rp[h + 1] = rp[h] + (rkeep[win["read_host_ptr"][h]:win["read_host_ptr"][h + 1]].sum() if len(rkeep) else 0)
        parts.append((keep, rkeep, hp, rp))
    first = dict(win, out_host_ptr=parts[0][2], read_host_ptr=parts[0][3], until_ns=t,
                 **{k: win[k][parts[0][0]] for k in ("out_socket", "out_forward_ns", "out_tag", "out_status")},
                 reads=win["reads"][parts[0][1]])
    second = dict(win, ops=np.zeros(0, M.OP), meta=np.zeros(0, M.META), tag_base=win["tag_base"] + len(win["meta"]),
                  out_host_ptr=parts[1][2], read_host_ptr=parts[1][3],
                  **{k: win[k][parts[1][0]] for k in ("out_socket", "out_forward_ns", "out_tag", "out_status")},
                  reads=win["reads"][parts[1][1]])
    return first, second, (parts[0][0], parts[0][1])


def merge_split(whole_win, o1, o2, keep, rkeep):
    """the two calls' outputs as the one call over the whole window reports them"""
    rx = np.zeros(len(keep), np.uint32)
    rx[keep], rx[~keep] = o1["rx_status"], o2["rx_status"]
    res = np.zeros(len(rkeep), M.RESULT)
    res[rkeep], res[~rkeep] = o1["results"], o2["results"]
    # a read armed in the first call and completed in the second is in the second's late list
    idx1 = np.flatnonzero(rkeep)
    for l in o2["late"]:
        i = int(l["seq"]) - o1["seq_base"]
        if 0 <= i < len(idx1) and res[idx1[i]]["status"] == M.ARMED:
            res[idx1[i]] = l["result"]
    first = np.minimum(o1["first_readable"], o2["first_readable"])
    return rx, res, first


# ---- the hand-worked cases of tests/golden/udprecv_cases.json
def golden_cases():
    import json
    import os

    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "udprecv_cases.json")))["cases"]


def golden_windows(case):
    """the case's calls as windows; a push's tag is its running index, its meta is noted under it"""
    nh = len(case["socket_ptr"]) - 1
    wins, tag = [], 0
    for call in case["calls"]:
        pushes, rds = call["pushes"], call["reads"]
        assert [p[0] for p in pushes] == sorted(p[0] for p in pushes) and [r[0] for r in rds] == sorted(r[0] for r in rds)
        hp = np.zeros(nh + 1, np.uint32)
        rp = np.zeros(nh + 1, np.uint32)
        for h in range(nh):
            hp[h + 1] = hp[h] + sum(p[0] == h for p in pushes)
            rp[h + 1] = rp[h] + sum(r[0] == h for r in rds)
        meta = np.zeros(len(pushes), M.META)
        for i, p in enumerate(pushes):
            meta[i]["payload_size"], meta[i]["src_ip_be"], meta[i]["src_port_be"], meta[i]["user"] = p[3], p[4], p[5], 1000 + tag + i
        reads = np.zeros(len(rds), M.READ)
        for i, r in enumerate(rds):
            reads[i] = (r[1], r[2], r[3], r[4], 5000 + i)
        wins.append(dict(ops=np.array([tuple(o) for o in call["ops"]], M.OP) if call["ops"] else np.zeros(0, M.OP),
                         meta=meta, tag_base=tag, out_host_ptr=hp,
                         out_socket=np.array([p[1] for p in pushes], np.uint32),
                         out_forward_ns=np.array([p[2] for p in pushes], np.uint64),
                         out_tag=np.arange(tag, tag + len(pushes), dtype=np.uint64),
                         out_status=np.full(len(pushes), HIT, np.uint32), read_host_ptr=rp, reads=reads,
                         until_ns=call["until"]))
        tag += len(pushes)
    return wins


def check_golden(case, outs, state):
    """a run's outputs against the case's expected statuses, results, late records and state"""
    bits = {"B": M.PROCESSED | M.BUFFERED, "D": M.PROCESSED | M.DROPPED, "-": 0}
    for call, o in zip(case["calls"], outs):
        assert [int(x) for x in o["rx_status"]] == [HIT | bits[b] for b in call["rx"]], (case["name"], o["rx_status"])
        got = [[int(r[k]) for k in ("status", "return_val", "msg_flags", "tag", "complete_ns")] for r in o["results"]]
        assert got == call["results"], (case["name"], got)
        late = [[int(l["seq"])] + [int(l["result"][k]) for k in ("status", "return_val", "msg_flags", "tag", "complete_ns")]
                for l in o["late"]]
        assert late == call["late"], (case["name"], late)
        for r in o["results"]:  # a message's user comes back with it
            if r["status"] == M.DONE and r["return_val"] >= 0:
                assert r["user"] == 1000 + r["tag"] and r["recv_ns"] <= r["complete_ns"]
    got = [[x, int(state[x]["len_bytes"]), int(state[x]["n_msgs"]), int(state[x]["soft_limit"])] for x in range(len(state))]
    assert got == case["state"], (case["name"], got)


def one_call_against_split(plan, n_hosts=65, shape=DENSE):
    """window 1 of a scenario in one call, and cut in two at its middle: the same statuses, results and state"""
    sc = scenario(n_hosts, shape)
    w0, w1 = sc["windows"][0], sc["windows"][1]
    cut = w1["until_ns"] - W // 2
    first, second, (keep, rkeep) = split_window(w1, cut)
    assert 0 < keep.sum() < len(keep) and 0 < rkeep.sum() < len(rkeep)
    whole, parts = Runner(plan, sc["socket_ptr"]), Runner(plan, sc["socket_ptr"])
    same_outputs(whole.window(w0), parts.window(w0))
    o = whole.window(w1)
    o1, o2 = parts.window(first), parts.window(second)
    rx, res, first_readable = merge_split(w1, o1, o2, keep, rkeep)
    assert np.array_equal(rx, o["rx_status"])
    assert res.tobytes() == o["results"].tobytes(), np.flatnonzero(res != o["results"])[:5]
    assert np.array_equal(first_readable, o["first_readable"])
    # reads armed before this window: late in whichever call completes them
    old = np.concatenate([o1["late"], o2["late"][o2["late"]["seq"] < o1["seq_base"]]])
    assert old[np.argsort(old["seq"])].tobytes() == o["late"].tobytes() and len(o["late"]) > 0
    assert (o2["late"]["seq"] >= o1["seq_base"]).sum() > 0  # and some armed in the first part, completed in the second
    (st, status), (st2, status2) = whole.finish(), parts.finish()
    assert status == status2 and status[0] == 0
    # a blocked read's number depends on how the reads were listed: mapped back to its place in the whole window
    idx = np.concatenate([np.flatnonzero(rkeep), np.flatnonzero(~rkeep)])
    armed = st2["armed_seq"] >= np.uint64(o1["seq_base"])
    armed &= st2["armed_seq"] != np.uint64(M.U64)
    st2 = st2.copy()
    st2["armed_seq"][armed] = o["seq_base"] + idx[(st2["armed_seq"][armed] - np.uint64(o1["seq_base"])).astype(np.int64)]
    same_state(st, st2)
    assert armed.sum() > 0


# ---- the real chain: inbound router -> interface receive -> UDP sockets
def chain(plan, n_hosts=70, n_win=6):
    """srt_inbound_run, srt_deliver_run and srt_udprecv_run on the instance's arrays (the device's with a
    plan), each call taking the one before's outputs as they are and nothing read in between, against
    inbound_model -> deliver_model -> udprecv_model chained the same way"""
    import deliver_model as DM
    import inbound_model as IM
    from shadow_amd.plan import DeliverStage, InboundRouter, UdpReceive

    rng = np.random.default_rng(12)
    counts = socket_counts(n_hosts, rng)
    sp = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    n_sock = int(sp[-1])
    host_of = np.repeat(np.arange(n_hosts), counts)
    udp = rng.random(n_sock) > 1 / 7
    bw = rng.choice(np.array([200_000, 5_000_000, 1_250_000_000], np.uint64), size=n_hosts)
    assoc = np.zeros(n_sock, DM.ASSOC)
    assoc["host"], assoc["socket"] = host_of, np.arange(n_sock)
    assoc["protocol"] = np.where(udp, DM.UDP, DM.TCP)
    assoc["local_port_be"] = 0x1000 + np.arange(n_sock) - sp[host_of]
    cap, late_cap, u_late_cap = 100 * n_hosts, 100 * n_hosts * n_win, 4096
    out_cap = 2 * cap + 99
    d = lambda a: _dev(a, plan)  # noqa: E731
    ib, ds = InboundRouter(plan, bw, 100 * (n_win + 1)), DeliverStage(plan, n_hosts, 8, 1 << 20, late_cap + cap)
    ur = UdpReceive(plan, sp, 1024, 1 << 20, u_late_cap)
    m_ib, m_ds, m_ur = IM.InboundModel(bw), DM.DeliverModel(n_hosts, 1 << 20, late_cap + cap), M.Model(sp, 1024, 1 << 20)
    ops = np.array([(M.OPEN, x, int(rng.choice([300, 3000, 1 << 20]))) for x in range(n_sock) if udp[x]], M.OP)
    try:
        ds.associate(assoc)
        assert m_ds.associate(assoc)
        ur.config(ops)
        m_ur.config(ops)
        tag_next = 0
        for w in range(n_win + 1):
            per = rng.integers(0, 100, n_hosts) if w < n_win else np.zeros(n_hosts, np.int64)
            n = int(per.sum())
            lo, until = w * W, (w + 1) * W if w < n_win else 400 * W
            dst_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
            deliver, size = np.zeros(n, np.uint64), rng.integers(28, 1429, n).astype(np.uint32)
            rxm, um = np.zeros(n, DM.RX_META), np.zeros(n, M.META)
            for h in range(n_hosts):
                b, e = int(dst_ptr[h]), int(dst_ptr[h + 1])
                deliver[b:e] = lo + np.sort(rng.integers(0, W // GRID, e - b)) * GRID
                rxm["local_port_be"][b:e] = 0x1000 + rng.integers(0, counts[h] + 1, e - b)  # one port past: no socket
            rxm["protocol"] = DM.UDP
            for h in range(n_hosts):  # a packet to a port of a slot that is not a UDP socket is a TCP packet
                b, e = int(dst_ptr[h]), int(dst_ptr[h + 1])
                x = np.minimum(sp[h] + rxm["local_port_be"][b:e].astype(np.int64) - 0x1000, max(n_sock - 1, 0))
                rxm["protocol"][b:e][(x < sp[h + 1]) & ~udp[x]] = DM.TCP
            rxm["protocol"][rng.random(n) < .05] = 3
            rxm["peer_ip_be"], rxm["peer_port_be"] = rng.integers(1, 1 << 32, n), rng.integers(1, 1 << 16, n)
            rxm["user"] = um["user"] = np.arange(tag_next, tag_next + n)
            um["src_ip_be"], um["src_port_be"], um["payload_size"] = rxm["peer_ip_be"], rxm["peer_port_be"], size - 28
            tag = (tag_next + np.arange(n)).astype(np.uint64)
            order = np.arange(n, dtype=np.uint32)
            # the models, chained
            m_st, m_fw, m_late, base = m_ib.run(order, dst_ptr, deliver, size, until, 0)
            m_ds.note(rxm, tag_next)
            m_ur.note(um, tag_next)
            late_a = np.array(m_late, DM.LATE) if m_late else np.zeros(0, DM.LATE)
            mo = m_ds.run(dst_ptr, n, tag, m_st, m_fw, base, late_a, out_cap)
            assert mo["flags"] == 0
            reads, rp = [], [0]
            for h in range(n_hosts):
                mine = [x for x in range(int(sp[h]), int(sp[h + 1])) if udp[x]]
                nr = int(rng.integers(0, 80)) if mine else 0
                for tm in lo + np.sort(rng.integers(0, W // GRID, nr)) * GRID:
                    reads.append((int(tm), int(rng.choice(mine)), int(rng.choice([16, 2000])),
                                  int(rng.choice([0, M.PEEK, M.TRUNC, M.WAIT, M.WAIT])), 7))
                rp.append(len(reads))
            reads, rp = np.array(reads, M.READ) if reads else np.zeros(0, M.READ), np.array(rp, np.uint32)
            run = lambda mdl: mdl.run(mo["host_ptr"], mo["socket"], mo["forward"], mo["tag"], mo["status"], rp,  # noqa: E731
                                      reads, until)
            trial = run(copy.deepcopy(m_ur))
            if len(reads):
                twice = (trial["results"]["return_val"] == -M.EWOULDBLOCK) & ((reads["flags"] & M.WAIT) != 0)
                reads["flags"][twice] &= ~np.uint32(M.WAIT)
            want = run(m_ur)
            # the instances, chained: nothing comes back until the window's three calls are made
            pad = max(n, 1)
            d_status, d_forward = d(np.zeros(pad, np.uint32))[:n], d(np.zeros(pad, np.uint64))[:n]
            d_late, d_cnt = d(np.zeros(late_cap * 24, np.uint8)), d(np.zeros(1, np.uint32))
            d_dst, d_tag = d(dst_ptr), d(np.resize(tag, pad))[:n]
            seq_base = ib.run(d(np.resize(order, pad))[:n], d_dst, d(np.resize(deliver, pad))[:n],
                              d(np.resize(size, pad))[:n], until, 0, d_status, d_forward, d_late, d_cnt)
            assert seq_base == base
            if n:
                ds.note(d(rxm), tag_next)
                ur.note(d(um), tag_next)
            o_hp = d(np.zeros(n_hosts + 1, np.uint32))
            o_sock = d(np.zeros(out_cap, np.uint32))  # past the list: slot 0, a hit, which would be pushed
            o_fw, o_tag, o_user = d(np.zeros(out_cap, np.uint64)), d(np.zeros(out_cap, np.uint64)), d(np.zeros(out_cap, np.uint32))
            o_st = d(np.full(out_cap, HIT, np.uint32))
            ds.run(d_dst, d_tag, d_status, d_forward, seq_base, d_late, d_cnt, o_hp, o_sock, o_fw, o_tag, o_user, o_st)
            rx = d(np.full(out_cap, 0x5A5A, np.uint32))
            res = d(np.zeros(56 * max(len(reads), 1), np.uint8))[:56 * len(reads)]
            u_late, u_cnt = d(np.zeros(u_late_cap, M.LATE)), d(np.full(1, 9, np.uint32))
            first = d(np.zeros(max(n_sock, 1), np.uint64))
            ur.run(o_hp, o_sock, o_fw, o_tag, o_st, d(rp) if len(reads) else None, d(reads) if len(reads) else None,
                   until, rx, res, u_late, u_cnt, first)
            # only now the window's results are read
            lim = int(mo["host_ptr"][-1])
            got_rx = _host(rx, np.uint32)
            assert np.array_equal(got_rx[:lim], want["rx_status"]) and (got_rx[lim:] == 0x5A5A).all(), w
            assert _host(res, M.RESULT, len(reads)).tobytes() == want["results"].tobytes(), w
            got_late = _host(u_late, M.LATE)[:int(_host(u_cnt, np.uint32)[0])]
            assert got_late[np.argsort(got_late["seq"])].tobytes() == want["late"].tobytes(), w
            assert np.array_equal(_host(first, np.uint64, n_sock), want["first_readable"]), w
            tag_next += n
        st, status = ur.state(), ur.status()
        assert ib.status()[0] == 0 and ds.status()[0] == 0
    finally:
        ur.close()
        ds.close()
        ib.close()
    same_state(st, m_ur.state())
    assert status == m_ur.status() and status[0] == 0 and status[1] > 5000 and status[3] > 100, status
    s = m_ur.stats
    assert s["foreign"] > 10 and s["armed_later_call"] > 10 and s["read_carried"] > 10 and s["drop_full"] > 10, s
