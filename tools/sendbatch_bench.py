#!/usr/bin/env python3
"""Times srt_sendbatch_run on the results of an outbound call of the C5 size
(bench.py's c5: 1M packets, 10k source hosts, 4 sockets a host, as in
tools/outbound_bench.py) with HIP events on the plan's stream, and beside it,
in the same process and on the same inputs, the path it replaces
(shadow_amd.plan.outbound_send_order plus the record gather by index) and the
yardstick, srt_outbound_run itself.  Cases: uncongested (125 MB/s a host:
every packet is forwarded in its own call, no late list) and throttled
(125 kB/s a host), once its first window (most packets stay queued and their
meta is logged) and once its second (no batch, only a late list); --case runs
one of them alone, for a profiler.  Every sample is one call on
a warmed instance; the gather is a pure function of its inputs (the log is only
written by a call's unforwarded packets), so it is repeated on the same arrays.
Before anything is timed the two paths' outputs are compared byte for byte.
Writes the raw samples to profiles/sendbatch_c5.json and prints a summary
line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--hosts", type=int, default=10_000)
    ap.add_argument("--sockets", type=int, default=4)
    ap.add_argument("--queue-cap", type=int, default=256)
    ap.add_argument("--case", default="all", help="all, or one of the three case names (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sendbatch_c5.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20 (the median of fewer samples is not reported)")

    import torch

    from shadow_amd import NetworkGraph, _lib, synth
    from shadow_amd.plan import (OUT_PKT_DTYPE, SEND_META_DTYPE, OutboundRelay, RoutingPlan, SendBatch,
                                 outbound_send_order)

    _lib.require_device()
    hosts, n_pkts, seed = args.hosts, args.packets, 5
    src, dst, lat, loss = synth.complete_graph(16, seed)
    plan = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32),
                       device=0).run()
    r0, r1 = 1_000_000_000, 1_000_000_000 + 5 * synth.MS
    pk, host_ptr, _ = synth.packet_round(hosts, 16, n_pkts, seed, r0, r1)
    rng = np.random.default_rng(seed)
    op = np.zeros(n_pkts, OUT_PKT_DTYPE)
    op["ready_ns"] = pk["t_ns"]
    op["total_size"] = pk["payload_size"] + 40
    op["socket"] = rng.integers(0, args.sockets, size=n_pkts)
    op["priority"] = np.arange(n_pkts) - np.repeat(host_ptr[:-1].astype(np.int64), np.diff(host_ptr.astype(np.int64)))
    meta = np.zeros(n_pkts, SEND_META_DTYPE)
    for f in ("src_row", "dst_row", "payload_size"):
        meta[f] = pk[f]
    meta["user"] = rng.integers(0, hosts, size=n_pkts)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    t_op, t_hp, t_meta, t_pk = t(op, np.uint8), t(host_ptr, np.int32), t(meta, np.uint8), t(pk, np.uint8).view(-1, 24)
    t_zero = z(hosts + 1, torch.int32)
    t_st, t_sn, t_rk = z(n_pkts, torch.int32), z(n_pkts, torch.int64), z(n_pkts, torch.int64)
    none64, none32 = z(0, torch.int64), z(0, torch.int32)
    t_late, t_cnt = z(32 * n_pkts, torch.uint8), z(1, torch.int32)
    out_cap = n_pkts
    o_pk, o_hp, o_us, o_sq = z(24 * out_cap, torch.uint8), z(hosts + 1, torch.int32), z(out_cap, torch.int32), z(
        out_cap, torch.int64)
    stream = torch.cuda.ExternalStream(plan.stream_ptr(), device=dev)
    until1, until2 = r1, r1 + 300 * synth.MS

    def timed(fn, on):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(on)
        fn()
        e1.record(on)
        plan.sync()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def samples_of(fn, on):
        xs = [timed(fn, on) for _ in range(args.warmup + args.reps)][args.warmup:]
        return {"median": statistics.median(xs), "samples": xs}

    def torch_path(hp, sn, rk, late_n, seq0):
        """outbound_send_order + the gather of the records by index; a late-only window gathers by
        seq - seq0 out of the caller's store (seq0: the seq_base of the call that fed the packets)"""
        if late_n:
            recs = t_late[:late_n * 32].view(torch.int64).view(late_n, 4)  # seq, send_ns, send_rank, status|host
            order, ptr = outbound_send_order(hp, rk, recs[:, 3] >> 32, recs[:, 2])
            idx, send = recs[order, 0] - seq0, recs[order, 1]
        else:
            order, ptr = outbound_send_order(hp, rk)
            idx, send = order, sn[order]
        spk = t_pk[idx].clone()
        spk[:, 16:24] = send.view(-1, 1).view(torch.uint8).view(-1, 8)
        return spk, ptr

    def case(bw_bytes, windows):
        """a fresh outbound instance through `windows` [(pkts, host_ptr, meta, n, until)]: the last
        window's gather, torch path and outbound call are the timed ones (a window is either the full
        batch or a late list only)"""
        bw = np.full(hosts, bw_bytes, np.uint64)
        arrays = lambda n: (t_st, t_sn, t_rk) if n else (none32, none64, none64)  # noqa: E731

        def outbound_to_last(sb):
            """-> (ms of the last window's call, its seq_base, flags, pending); with sb, the earlier
            windows are gathered too, which fills its log"""
            ob = OutboundRelay(plan, bw, _lib.QDISC_FIFO, args.sockets, args.queue_cap)
            ob.run(t_op, t_zero, 0, 0, t_st, t_sn, t_rk, t_late, t_cnt)  # no group holds a packet: sizes the links
            ob.status()
            bases = []
            for k, (w_op, w_hp, w_meta, n, until) in enumerate(windows):
                st, sn, rk = arrays(n)
                call = lambda: bases.append(ob.run(w_op, w_hp, until, 0, st, sn, rk, t_late, t_cnt))  # noqa: E731
                if k + 1 < len(windows):
                    call()
                    ob.status()
                    if sb is not None:
                        sb.run(w_hp, w_meta, sn, rk, bases[-1], t_late, t_cnt, o_pk, o_hp, o_us, o_sq)
                        sb.status()
                else:
                    ms = timed(call, stream)
                    flags, pending = ob.status()
            ob.close()
            return ms, bases, flags, pending

        sb = SendBatch(plan, hosts, n_pkts)
        _, bases, _, _ = outbound_to_last(sb)
        w_op, w_hp, w_meta, n, until = windows[-1]
        _, sn, rk = arrays(n)
        late_n = int(t_cnt.item())
        native = lambda: sb.run(w_hp, w_meta, sn, rk, bases[-1], t_late, t_cnt, o_pk, o_hp, o_us, o_sq)  # noqa: E731
        native()
        flags, n_sent = sb.status()
        spk, ptr = torch_path(w_hp, sn, rk, late_n, bases[0])
        same = bool(torch.equal(ptr, o_hp) and n_sent == spk.shape[0] and
                    torch.equal(spk.reshape(-1), o_pk[:24 * n_sent]))
        res = {"n_sent": n_sent, "late_records": late_n, "batch_packets": n, "sendbatch_flags": flags,
               "native_equals_torch_path": same,
               "sendbatch_ms": samples_of(native, stream),
               "torch_path_ms": samples_of(lambda: torch_path(w_hp, sn, rk, late_n, bases[0]),
                                           torch.cuda.current_stream(dev))}
        xs = []
        for _ in range(args.warmup + args.reps):
            ms, _, o_flags, pending = outbound_to_last(None)
            xs.append(ms)
        xs = xs[args.warmup:]
        res["outbound_ms"] = {"median": statistics.median(xs), "samples": xs}
        res["outbound_outcome"] = {"flags": o_flags, "pending": pending}
        res["sendbatch_over_outbound"] = res["sendbatch_ms"]["median"] / res["outbound_ms"]["median"]
        res["torch_path_over_sendbatch"] = res["torch_path_ms"]["median"] / res["sendbatch_ms"]["median"]
        sb.close()
        return res

    full = (t_op, t_hp, t_meta, n_pkts, until1)
    empty = (z(32, torch.uint8), t_zero, z(16, torch.uint8), 0, until2)
    out = {"what": "srt_sendbatch_run on the results of an outbound call of the C5 size, device ms per call (HIP "
                   "events on the plan's stream); beside it outbound_send_order + the record gather (torch ops, "
                   "events on torch's stream) and srt_outbound_run on the same inputs",
           "packets": n_pkts, "hosts": hosts, "sockets_per_host": args.sockets, "queue_cap": args.queue_cap,
           "log_cap": n_pkts, "out_cap": out_cap, "warmup": args.warmup, "reps": args.reps}
    cases = {"uncongested_125MBps": (125_000_000, [full]), "throttled_125kBps_first_window": (125_000, [full]),
             "throttled_125kBps_second_window_late_only": (125_000, [full, empty])}
    if args.case != "all" and args.case not in cases:
        ap.error("--case: all or one of " + ", ".join(cases))
    for name, (bw_bytes, windows) in cases.items():
        if args.case in ("all", name):
            out[name] = case(bw_bytes, windows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)

    def brief(v):
        if not isinstance(v, dict) or "sendbatch_ms" not in v:
            return v
        return {k: (x["median"] if isinstance(x, dict) and "median" in x else x) for k, x in v.items()}

    print(json.dumps({k: brief(v) for k, v in out.items()}))
    plan.close()
    ok = all(v["native_equals_torch_path"] and not v["sendbatch_flags"] for v in out.values()
             if isinstance(v, dict) and "sendbatch_ms" in v)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
