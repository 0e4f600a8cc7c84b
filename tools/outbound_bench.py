#!/usr/bin/env python3
"""Times srt_outbound_run on a batch of the C5 size (bench.py's c5: 1M packets,
10k source hosts, synth.packet_round's grouping and send times as the
socket-has-data times, 4 sockets a host) with HIP events on the plan's stream:
FIFO and round robin, once with 125 MB/s per host (nothing is held back) and
once with 125 kB/s per host (the relay blocks, packets stay queued).  Every
sample is one call on a fresh srt_outbound (the state is consumed by a call),
primed by an empty call of the same size so that the allocation of its link
buffer is outside the timed span; warm-up calls come first.  The span still
holds the two launches, the gap between them and the stream waits around the
call.  The yardstick, tools/inbound_bench.py, is run beside it in the same
session.  Writes the raw samples to profiles/outbound_c5.json and prints a
summary line.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outbound_c5.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20 (the median of fewer samples is not reported)")

    import torch

    from shadow_amd import NetworkGraph, _lib, synth
    from shadow_amd.plan import OUT_PKT_DTYPE, OutboundRelay, RoutingPlan

    _lib.require_device()
    hosts, n_pkts, seed = args.hosts, args.packets, 5
    # the stage needs a plan only for its device and stream
    src, dst, lat, loss = synth.complete_graph(16, seed)
    plan = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32),
                       device=0).run()
    r0, r1 = 1_000_000_000, 1_000_000_000 + 5 * synth.MS
    pk, host_ptr, _ = synth.packet_round(hosts, 16, n_pkts, seed, r0, r1)
    rng = np.random.default_rng(seed)
    op = np.zeros(n_pkts, OUT_PKT_DTYPE)
    op["ready_ns"] = pk["t_ns"]
    op["total_size"] = pk["payload_size"] + 40  # payload + TCP/IP headers
    op["socket"] = rng.integers(0, args.sockets, size=n_pkts)
    op["priority"] = np.arange(n_pkts) - np.repeat(host_ptr[:-1].astype(np.int64), np.diff(host_ptr.astype(np.int64)))
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    t_op, t_hp = t(op, np.uint8), t(host_ptr, np.int32)
    t_zero = torch.zeros(hosts + 1, dtype=torch.int32, device=dev)
    t_st = torch.zeros(n_pkts, dtype=torch.int32, device=dev)
    t_sn = torch.zeros(n_pkts, dtype=torch.int64, device=dev)
    t_rk = torch.zeros(n_pkts, dtype=torch.int64, device=dev)
    t_late = torch.zeros(32 * 1024, dtype=torch.uint8, device=dev)
    t_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.ExternalStream(plan.stream_ptr(), device=dev)
    until = r1 + 300 * synth.MS

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        plan.sync()
        return e0.elapsed_time(e1)

    def outbound(qdisc, bw_bytes):
        bw = np.full(hosts, bw_bytes, np.uint64)
        samples, last = [], None
        for k in range(args.warmup + args.reps):
            ob = OutboundRelay(plan, bw, qdisc, args.sockets, args.queue_cap)
            # an empty batch of the same size (no group holds a packet): sizes the link buffer
            ob.run(t_op, t_zero, 0, 0, t_st, t_sn, t_rk, t_late, t_cnt)
            ob.status()
            ms = timed(lambda: ob.run(t_op, t_hp, until, 0, t_st, t_sn, t_rk, t_late, t_cnt))
            flags, pending = ob.status()
            if k >= args.warmup:
                samples.append(ms)
            state = ob.state()
            last = {"pending": pending, "flags": flags,
                    "forwarded": int(((t_st & _lib.PDS_RELAY_FORWARDED) != 0).sum().item()),
                    "cached": int(((t_st & _lib.PDS_RELAY_CACHED) != 0).sum().item()),
                    "forward_tasks": int(state["tasks_scheduled"].sum()), "sent_total": int(state["sent_total"].sum())}
            ob.close()
        return {"median": statistics.median(samples), "samples": samples, "outcome": last}

    out = {"what": "srt_outbound_run on a batch of the C5 size, device ms per call (HIP events on the plan's stream)",
           "packets": n_pkts, "hosts": hosts, "sockets_per_host": args.sockets, "until_ns": until,
           "queue_cap": args.queue_cap, "warmup": args.warmup, "reps": args.reps,
           "timed_span": "HIP events around one srt_outbound_run: both launches, the gap between them and the stream "
                         "waits of the call; the link buffer is allocated by an untimed empty call before"}
    for name, qdisc in (("fifo", _lib.QDISC_FIFO), ("rr", _lib.QDISC_RR)):
        out[f"outbound_{name}_125MBps_ms"] = outbound(qdisc, 125_000_000)
        out[f"outbound_{name}_125kBps_ms"] = outbound(qdisc, 125_000)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {"median": v["median"], "outcome": v["outcome"]})
                      for k, v in out.items()}))
    plan.close()


if __name__ == "__main__":
    main()
