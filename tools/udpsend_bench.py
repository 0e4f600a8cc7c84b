#!/usr/bin/env python3
"""Times srt_udpsend_run at the C5 size -- 1M sendmsg calls a window over 10k
hosts and 40k socket slots -- next to srt_outbound_run on the arrivals the
window accepted, with HIP events on the plan's stream around each call of a
warmed sequence (every repetition is the next 20 ms window: the call times
move on, on the device).  Three cases:

  free       10 GB/s of upload and 16 MB buffers: nothing blocks, every call
             is accepted and forwarded in its window;
  refused    every host throttled to 1,000 B/s with limits of 4,096 bytes and
             non-blocking calls: the warm-up windows fill every socket, the
             timed ones find them full and answer -EWOULDBLOCK;
  blocked    as refused with blocking (WAIT) calls and 5 MB/s of upload, about
             what a window's calls need: a call that finds its socket full arms
             and is woken by the pop that frees space (a further WAIT call on a
             socket that already has an armed one is answered -EWOULDBLOCK and
             flagged ARMED_TWICE: one blocked sender a socket).

The yardstick is the outbound call of the same run: srt_udpsend does that
call's work plus one slot-state update a call and a pop.  Its input is built
between the timed regions, with torch ops, from the window's results: the
accepted calls as srt_out_pkt records in (host, completion time) order.

Beside them the host-only instance through the same windows (wall clock, the
last --host-reps windows) and, for `free` only, a torch formulation of the
bookkeeping: a sort of the calls by (host, time) and per-socket cumulative sums
of the accepted bytes.  That formulation cannot express `refused` or `blocked`:
whether a call is accepted depends on the pops before it, which depend on the
qdisc and the bucket, which depend on what was accepted.

Writes the raw samples to profiles/udpsend_c5.json and prints a summary line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = 20_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1_000_000)
    ap.add_argument("--hosts", type=int, default=10_000)
    ap.add_argument("--slots-per-host", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-refs", action="store_true", help="the device calls alone (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "udpsend_c5.json"))
    args = ap.parse_args()
    if args.reps < 20 and not args.no_refs:
        ap.error("--reps must be at least 20 (the median of fewer samples is not reported)")

    import torch

    from shadow_amd import NetworkGraph, UdpSend, _lib, synth
    from shadow_amd.plan import (OUT_PKT_DTYPE, UDP_SEND_DTYPE, UDPSEND_OP_DTYPE, UDPSEND_RESULT_DTYPE, OutboundRelay,
                                 RoutingPlan)

    _lib.require_device()
    hosts, n, sph, seed = args.hosts, args.calls, args.slots_per_host, 5
    n_sock = hosts * sph
    src, dst, lat, loss = synth.complete_graph(16, seed)
    plan = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32),
                       device=0).run()
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(plan.stream_ptr(), device=dev)
    assert UDPSEND_RESULT_DTYPE.itemsize == 40 and UDP_SEND_DTYPE.itemsize == 40 and OUT_PKT_DTYPE.itemsize == 32

    # ---- one window's calls, grouped by host in time order, on a 1 us grid
    h = np.sort(rng.integers(0, hosts, size=n))
    host_ptr = np.searchsorted(h, np.arange(hosts + 1)).astype(np.uint32)
    when = 1000 * rng.integers(0, W // 1000, size=n)
    calls = np.zeros(n, UDP_SEND_DTYPE)
    calls["time_ns"] = when[np.lexsort((when, h))]
    calls["slot"] = h * sph + rng.integers(0, sph, size=n)
    calls["len"] = rng.integers(100, 1401, size=n)
    calls["user"] = np.arange(n)
    socket_ptr = (np.arange(hosts + 1) * sph).astype(np.uint32)
    ips = (11 | (np.arange(hosts, dtype=np.uint64) + 1) << 8).astype(np.uint32)  # 11.x.y.0, none of them a destination
    ops = np.zeros(3 * n_sock, UDPSEND_OP_DTYPE).reshape(n_sock, 3)
    ops["slot"] = np.arange(n_sock)[:, None]
    ops["op"] = [_lib.UDPSEND_OPEN, _lib.UDPSEND_BIND, _lib.UDPSEND_SET_PEER]
    ops["value"][:, 1] = (0x1000 + np.arange(n_sock) % sph) << 32
    ops["value"][:, 2] = 10 | 9 << 32  # 10.0.0.0:9
    late_cap = n // 2
    host_of = torch.from_numpy(h.astype(np.int64)).to(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        plan.sync()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def accepted_as_out_pkts(d):
        """the window's accepted calls as srt_outbound_run's input, by (host, completion time), list order kept"""
        res = d["res"].view(torch.int64).view(-1, 5)
        ok = ((res[:, 3] & 0xffffffff) == _lib.UDPSEND_DONE) & (res[:, 2] >= 0)
        idx = torch.nonzero(ok).flatten()
        idx = idx[torch.sort(res[idx, 0], stable=True).indices]
        idx = idx[torch.sort(host_of[idx], stable=True).indices]
        pk = torch.zeros((idx.numel(), 4), dtype=torch.int64, device=dev)
        pk[:, 0], pk[:, 1] = res[idx, 0], res[idx, 1]
        c = d["calls"].view(torch.int64).view(-1, 5)
        slot, length = c[idx, 2] & 0xffffffff, c[idx, 2] >> 32
        pk[:, 2] = (length + 28) | (slot % sph) << 32
        hp = torch.zeros(hosts + 1, dtype=torch.int64, device=dev)
        hp[1:] = torch.cumsum(torch.bincount(host_of[idx], minlength=hosts), 0)
        return pk.view(torch.uint8).flatten(), hp.to(torch.int32), idx.numel()

    def torch_formulation(d):
        """`free` only: the calls by (host, time), the bytes each socket has accepted up to each call"""
        c = d["calls"].view(torch.int64).view(-1, 5)
        order = torch.sort(c[:, 0], stable=True).indices
        order = order[torch.sort(host_of[order], stable=True).indices]
        slot, length = c[order, 2] & 0xffffffff, c[order, 2] >> 32
        by_slot = torch.sort(slot, stable=True).indices
        run = torch.cumsum(length[by_slot], 0)
        first = torch.searchsorted(slot[by_slot].contiguous(), torch.arange(n_sock, device=dev))
        before = torch.where(first > 0, run[(first - 1).clamp(min=0)], torch.zeros_like(first))
        return run - before[slot[by_slot]]

    cases = (("free", 10 ** 10, 1 << 24, 0), ("refused", 1000, 4096, 0), ("blocked", 5_000_000, 4096, _lib.UDPSEND_WAIT))
    runs, same = {}, True
    for case, bw, limit, flag in cases:
        calls["flags"] = flag
        ops["value"][:, 0] = limit
        bws = np.full(hosts, bw, np.uint64)
        us = UdpSend(plan, socket_ptr, ips, bws, 0, 64, late_cap)
        ob = OutboundRelay(plan, bws, 0, sph, 4096)
        us.config(ops.reshape(-1))
        z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
        d = dict(calls=torch.from_numpy(calls.view(np.uint8).copy()).to(dev), hp=torch.from_numpy(host_ptr.view(np.int32).copy()).to(dev),
                 res=z(40 * n, torch.uint8), st=z(n, torch.int32), sn=z(n, torch.int64), rk=z(n, torch.int64),
                 late=z(32 * late_cap, torch.uint8), cnt=z(1, torch.int32), lres=z(48 * late_cap, torch.uint8),
                 lcnt=z(1, torch.int32), first=z(n_sock, torch.int64), o_st=z(n, torch.int32), o_sn=z(n, torch.int64),
                 o_rk=z(n, torch.int64), o_late=z(32 * late_cap, torch.uint8), o_cnt=z(1, torch.int32))
        samples = {"udpsend_ms": [], "outbound_ms": [], "torch_ms": [], "host_only_ms": []}
        accepted_per_call, kept = [], {}
        hu = None
        if not args.no_refs:
            hu = UdpSend(None, socket_ptr, ips, bws, 0, 64, late_cap)
            hu.config(ops.reshape(-1))
            h_calls = calls.copy()
        for k in range(args.warmup + args.reps):
            until = (k + 1) * W
            plan.sync()
            ms_u = timed(lambda: us.run(d["hp"], d["calls"], until, 0, d["res"], d["st"], d["sn"], d["rk"], d["late"], d["cnt"],
                                        d["lres"], d["lcnt"], d["first"]))
            pk, o_hp, n_acc = accepted_as_out_pkts(d)
            torch.cuda.synchronize(dev)
            ms_o = timed(lambda: ob.run(pk, o_hp, until, 0, d["o_st"][:n_acc], d["o_sn"][:n_acc], d["o_rk"][:n_acc],
                                        d["o_late"], d["o_cnt"])) if n_acc else 0.0
            if k >= args.warmup:
                samples["udpsend_ms"].append(ms_u)
                samples["outbound_ms"].append(ms_o)
                accepted_per_call.append(n_acc)
                if case == "free" and not args.no_refs:
                    torch.cuda.synchronize(dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    torch_formulation(d)
                    e1.record()
                    torch.cuda.synchronize(dev)
                    samples["torch_ms"].append(e0.elapsed_time(e1))
            # the host-only form through the first warmup + host_reps windows, the last host_reps of them timed
            if hu is not None and k < args.warmup + args.host_reps:
                hr = [np.zeros(40 * n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64),
                      np.zeros(32 * late_cap, np.uint8), np.zeros(1, np.int32), np.zeros(48 * late_cap, np.uint8),
                      np.zeros(1, np.int32), np.zeros(n_sock, np.int64)]
                t0 = time.perf_counter()
                hu.run(host_ptr, h_calls, until, 0, *hr)
                if k >= args.warmup:
                    samples["host_only_ms"].append(1e3 * (time.perf_counter() - t0))
                same = same and hr[0].tobytes() == d["res"].cpu().numpy().tobytes() and \
                    np.array_equal(hr[1], d["st"].cpu().numpy()) and np.array_equal(hr[2], d["sn"].cpu().numpy()) and \
                    np.array_equal(hr[3], d["rk"].cpu().numpy())
                h_calls["time_ns"] += W
            d["calls"].view(torch.int64).view(-1, 5)[:, 0] += W  # the next window: the same calls 20 ms later
        kept = dict(zip(("flags", "pending", "accepted", "would_block", "armed"), us.status(check=False)))
        o_flags = ob.status(check=False)[0]
        us.close(), ob.close()
        if hu is not None:
            hu.close()
        med = {f: statistics.median(v) for f, v in samples.items() if v}
        runs[case] = {"bw_up_bytes_per_s": bw, "send_buf_size": limit, "wait": bool(flag), "udpsend_status": kept,
                      "outbound_flags": o_flags, "accepted_per_timed_call_median": statistics.median(accepted_per_call),
                      "median_ms": med,
                      "udpsend_over_outbound": med["udpsend_ms"] / med["outbound_ms"] if med["outbound_ms"] else None,
                      "samples": samples}
        if "host_only_ms" in med:
            runs[case]["host_only_over_device"] = med["host_only_ms"] / med["udpsend_ms"]
        if "torch_ms" in med:
            runs[case]["torch_over_device"] = med["torch_ms"] / med["udpsend_ms"]
    plan.close()
    out = {"what": "srt_udpsend_run at the C5 size, device ms per call (HIP events on the plan's stream around one call of "
                   "a warmed sequence, every repetition the next window), beside srt_outbound_run on the arrivals the "
                   "window accepted, the host-only instance through the same windows (wall clock) and, for `free`, a "
                   "torch sort plus per-socket cumulative sums of the same calls",
           "measured_on": "MI355X", "calls": n, "hosts": hosts, "slots": n_sock, "window_bytes": UdpSend.window_bytes(),
           "warmup": args.warmup, "reps": args.reps, "host_reps": args.host_reps,
           "outputs_equal_host_only": bool(same) and not args.no_refs, "runs": runs}
    if not args.no_refs:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for r in runs.values():
        r.pop("samples")
    print(json.dumps(out))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
