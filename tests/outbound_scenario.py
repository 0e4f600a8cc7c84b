"""The random scenario of the outbound relay tests and the plumbing to feed it
to the model (tests/outbound_model.py) and to srt_outbound (host-only or on
the device), in one call or split into windows.  The model's outputs are
computed once per process and shared by the tests that compare against them.
"""
import functools

import numpy as np

from outbound_model import FIFO, MS, RR, U64, OutboundModel

N_HOSTS = 70           # one wave of 64 hosts and a remainder of 6
N_PKTS = 6000
SPAN_NS = 1000 * MS
BOOTSTRAP_END_NS = 150 * MS
UNTIL_NS = SPAN_NS + 50 * MS
BANDWIDTHS = (60_000, 125_000_000)
WIDE_HOST = 37         # 300 sockets; every other host 1 to 5
WIDE_SOCKETS = 300
MAX_SOCKETS = 320
SEED = 5
SPLITS = 6
LATE_CAP = 8192
STATE_FIELDS = ("balance", "last_refill_ns", "task_ns", "tasks_scheduled", "sent_total", "queue_len", "cached")
OUT_PKT_DTYPE = np.dtype([("ready_ns", "<u8"), ("priority", "<u8"), ("total_size", "<u4"), ("socket", "<u4"),
                          ("flags", "<u4"), ("reserved", "<u4")])
LATE_DTYPE = np.dtype([("seq", "<u8"), ("send_ns", "<u8"), ("send_rank", "<u8"), ("status", "<u4"),
                       ("src_host", "<u4")])

assert (FIFO, RR) == (0, 1) and U64


def make_scenario(rng, n_hosts, n_pkts, n_sockets, bw, span_ns, host_weight=None, local_share=0.03):
    """packets grouped by host, each host's in arrival order: ready times on a
    1 ms grid (where a blocked relay's tasks fall) with a sub-ms jitter bit, so
    ties and arrivals exactly on a pending task's time occur; priorities from a
    per-host counter, distinct within the host and NOT increasing within a
    socket (they follow the arrival order only loosely)"""
    p = None if host_weight is None else host_weight / host_weight.sum()
    host = np.sort(rng.choice(n_hosts, size=n_pkts, p=p)).astype(np.uint32)
    ready = (rng.integers(0, span_ns // MS, size=n_pkts) * MS + rng.integers(0, 2, size=n_pkts) * 321_123)
    order = np.lexsort((ready, host))
    ready = ready[order].astype(np.uint64)
    host_ptr = np.searchsorted(host, np.arange(n_hosts + 1)).astype(np.uint32)
    pk = np.zeros(n_pkts, OUT_PKT_DTYPE)
    pk["ready_ns"] = ready
    pk["total_size"] = rng.integers(40, 1501, size=n_pkts)
    pk["total_size"][rng.random(n_pkts) < 0.3] = 1500
    pk["socket"] = (rng.integers(0, 1 << 30, size=n_pkts) % n_sockets[host]).astype(np.uint32)
    pk["flags"] = (rng.random(n_pkts) < local_share).astype(np.uint32)
    for h in range(n_hosts):
        b, e = int(host_ptr[h]), int(host_ptr[h + 1])
        pk["priority"][b:e] = 1000 + np.argsort(np.argsort(np.arange(e - b) + rng.uniform(0, 6, size=e - b)))
    return dict(bw=np.asarray(bw, np.uint64), pkts=pk, host=host, host_ptr=host_ptr, n_hosts=n_hosts)


@functools.lru_cache(maxsize=None)
def scenario(seed=SEED):
    rng = np.random.default_rng(seed)
    bw = rng.choice(np.array(BANDWIDTHS, np.uint64), size=N_HOSTS, p=[0.5, 0.5])
    n_sockets = rng.integers(1, 6, size=N_HOSTS)
    n_sockets[WIDE_HOST] = WIDE_SOCKETS
    bw[WIDE_HOST] = 60_000
    w = np.ones(N_HOSTS)
    w[WIDE_HOST] = 8.0
    return make_scenario(rng, N_HOSTS, N_PKTS, n_sockets, bw, SPAN_NS, w)


def calls_of(sc, untils):
    """the batch cut into one call per window: packets with ready time in
    [previous until, until), still grouped by host in arrival order; ids =
    their indices in the scenario"""
    calls, lo = [], 0
    ready = sc["pkts"]["ready_ns"]
    for u in untils:
        ids = np.nonzero((ready >= lo) & (ready < u))[0]
        host_ptr = np.searchsorted(sc["host"][ids], np.arange(sc["n_hosts"] + 1)).astype(np.uint32)
        calls.append(dict(ids=ids, pkts=sc["pkts"][ids].copy(), host_ptr=host_ptr, until=int(u)))
        lo = u
    return calls


def one_call(sc):
    return calls_of(sc, [UNTIL_NS])


def split_calls(sc):
    # every cut is on the 1 ms grid: arrivals and tasks exactly at a window's end
    return calls_of(sc, [UNTIL_NS * (k + 1) // SPLITS for k in range(SPLITS)])


def run_model(sc, calls, qdisc, max_sockets=MAX_SOCKETS, bootstrap_end=BOOTSTRAP_END_NS):
    m = OutboundModel(sc["bw"], qdisc, max_sockets)
    outs = []
    for c in calls:
        st, sn, rk, late, base = m.run(c["pkts"], c["host_ptr"], c["until"], bootstrap_end)
        outs.append(dict(status=st, send=sn, rank=rk, late=late, base=base))
    return outs, m


@functools.lru_cache(maxsize=None)
def model_results(qdisc, split=False, seed=SEED):
    sc = scenario(seed)
    calls = split_calls(sc) if split else one_call(sc)
    outs, m = run_model(sc, calls, qdisc)
    return calls, outs, m


def run_lib(sc, calls, qdisc, plan=None, max_sockets=MAX_SOCKETS, queue_cap=None, late_cap=LATE_CAP,
            bootstrap_end=BOOTSTRAP_END_NS, check=True):
    """the same calls through srt_outbound -> (outs, state record array, [(flags, pending)] per call)"""
    from shadow_amd.plan import OutboundRelay

    r = OutboundRelay(plan, sc["bw"], qdisc, max_sockets, len(sc["pkts"]) if queue_cap is None else queue_cap)
    outs, stats = [], []
    try:
        for c in calls:
            n = len(c["pkts"])
            if plan is None:
                st = np.full(n, 0xdeadbeef, np.uint32)
                sn, rk = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
                late = np.zeros(late_cap * 32, np.uint8)
                cnt = np.ones(1, np.uint32)
                base = r.run(c["pkts"].view(np.uint8), c["host_ptr"], c["until"], bootstrap_end, st, sn, rk, late, cnt)
                stats.append(r.status(check=check))
            else:
                import torch

                dev = torch.device("cuda:0")
                t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
                t_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
                t_sn = torch.zeros(n, dtype=torch.int64, device=dev)
                t_rk = torch.zeros(n, dtype=torch.int64, device=dev)
                t_late = torch.zeros(max(late_cap, 1) * 32, dtype=torch.uint8, device=dev)
                t_cnt = torch.ones(1, dtype=torch.int32, device=dev)
                t_pk = t(c["pkts"], np.uint8) if n else torch.zeros(32, dtype=torch.uint8, device=dev)
                base = r.run(t_pk, t(c["host_ptr"], np.int32), c["until"], bootstrap_end, t_st, t_sn, t_rk,
                             t_late if late_cap else None, t_cnt)
                stats.append(r.status(check=check))
                st = t_st.cpu().numpy().view(np.uint32)
                sn = t_sn.cpu().numpy().view(np.uint64)
                rk = t_rk.cpu().numpy().view(np.uint64)
                late = t_late.cpu().numpy()
                cnt = t_cnt.cpu().numpy().view(np.uint32)
            k = min(int(cnt[0]), late_cap)
            recs = late[:k * 32].view(LATE_DTYPE)
            outs.append(dict(status=st, send=sn, rank=rk, base=base, late_count=int(cnt[0]), late=sorted(
                (int(x["seq"]), int(x["send_ns"]), int(x["send_rank"]), int(x["status"]), int(x["src_host"]))
                for x in recs)))
        return outs, r.state(), stats
    finally:
        r.close()


def assert_same(outs, mouts, state, model, calls=None, sc=None, hosts=None):
    """every status word, send time, rank, late record (sorted by seq) and state field; with
    `hosts`, only those hosts' (calls and sc then name each packet's host)"""
    for k, (o, m) in enumerate(zip(outs, mouts)):
        assert o["base"] == m["base"], k
        if hosts is None:
            keep = slice(None)
            assert o["late"] == m["late"], k
        else:
            keep = np.isin(sc["host"][calls[k]["ids"]], sorted(hosts))
            assert [x for x in o["late"] if x[4] in hosts] == [x for x in m["late"] if x[4] in hosts], k
        for f in ("status", "send", "rank"):
            assert np.array_equal(o[f][keep], m[f][keep]), (k, f, np.nonzero(o[f] != m[f])[0][:10])
    for h, ms in enumerate(model.state()):
        if hosts is not None and h not in hosts:
            continue
        for f in STATE_FIELDS:
            assert int(state[f][h]) == ms[f], (h, f, int(state[f][h]), ms[f])


def resolved(calls, outs):
    """scenario packet index -> (status, send time, rank) of every packet that was forwarded"""
    from outbound_model import FORWARDED

    res = {}
    bases = [(o["base"], c["ids"]) for c, o in zip(calls, outs)]
    for c, o in zip(calls, outs):
        for i, g in enumerate(c["ids"]):
            if o["status"][i] & FORWARDED:
                res[int(g)] = (int(o["status"][i]), int(o["send"][i]), int(o["rank"][i]))
        for seq, sn, rk, st, _ in o["late"]:
            b, ids = [x for x in bases if x[0] <= seq < x[0] + len(x[1])][0]
            res[int(ids[seq - b])] = (st, sn, rk)
    return res


def overflow_case(qdisc):
    """three hosts over three calls -> (scenario, calls, model outputs, model): host 1 (1000 B/s) ends
    the first call with more than four packets queued, host 2 (450 kB/s) carries a few over, never more
    than four, host 0 none"""
    rng = np.random.default_rng(2)
    sc = make_scenario(rng, 3, 60, np.array([2, 3, 2]), [125_000_000, 1000, 450_000], 40 * MS)
    calls = calls_of(sc, [20 * MS, 45 * MS, 400 * MS])
    m, mouts, deepest = OutboundModel(sc["bw"], qdisc, 4), [], np.zeros(3, int)
    for c in calls:
        st, sn, rk, late, base = m.run(c["pkts"], c["host_ptr"], c["until"], 0)
        mouts.append(dict(status=st, send=sn, rank=rk, late=late, base=base))
        deepest = np.maximum(deepest, [len(h.iface) for h in m.hosts])
    assert deepest[1] > 4 and 0 < deepest[2] <= 4 and deepest[0] == 0, deepest
    return sc, calls, mouts, m
