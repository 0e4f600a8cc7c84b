#!/usr/bin/env python3
"""Times srt_inbound_run on the C5 batch (bench.py's c5: 1M packets, 10k
destination hosts, the sent set of a real srt_packet_batch round) with HIP
events on the plan's stream: once with 125 MB/s per host (nothing queues) and
once with 125 kB/s per host (queues build, CoDel drops, the relay blocks).
The event push it follows (srt_packet_events) is timed in the same process on
the same batch as the yardstick.  Every sample is one call on a fresh
srt_inbound (the state is consumed by a call), primed by an empty call of the
same size so that the allocation of its record buffer is outside the timed
span; warm-up calls come first.  The span still holds the two launches, the
gap between them and the stream waits around the call.
Writes the raw samples to profiles/inbound_c5.json and prints a summary line.
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
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--queue-cap", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inbound_c5.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20 (the median of fewer samples is not reported)")

    import torch

    from shadow_amd import NetworkGraph, _lib, synth
    from shadow_amd.plan import InboundRouter, RoutingPlan

    _lib.require_device()
    n_nodes, hosts, n_pkts, seed = args.nodes, args.hosts, args.packets, 5
    src, dst, lat, loss = synth.complete_graph(n_nodes, seed, loss_max=0.25)
    plan = RoutingPlan(NetworkGraph.from_edges(n_nodes, src, dst, lat, loss), np.arange(n_nodes, dtype=np.uint32),
                       device=0).run()
    r0, r1 = 1_000_000_000, 1_000_000_000 + 5 * synth.MS
    pk, host_ptr, _ = synth.packet_round(hosts, n_nodes, n_pkts, seed, r0, r1)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    t_hp = t(host_ptr, np.int32)
    t_f = torch.zeros(n_pkts, dtype=torch.int32, device=dev)
    t_d = torch.zeros(n_pkts, dtype=torch.int64, device=dev)
    plan.packet_batch(t(pk.view(np.uint8), np.uint8), t_hp, t(synth.host_rng_states(hosts, 1), np.int64), r1, 0,
                      2**62, t_f, t_d)
    dst_host = ((pk["dst_row"].astype(np.int64) + n_nodes * (np.arange(n_pkts) % max(1, hosts // n_nodes)))
                % hosts).astype(np.int32)
    t_dh = torch.from_numpy(dst_host).to(dev)
    t_eid = torch.zeros(n_pkts, dtype=torch.int64, device=dev)
    t_ord = torch.zeros(n_pkts, dtype=torch.int32, device=dev)
    t_ptr = torch.zeros(hosts + 1, dtype=torch.int32, device=dev)
    stream = torch.cuda.ExternalStream(plan.stream_ptr(), device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        plan.sync()
        return e0.elapsed_time(e1)

    t_base = torch.zeros(hosts, dtype=torch.int64, device=dev)

    def push():
        plan.packet_events(t_hp, t_f, t_d, t_dh, hosts, t_base, t_eid, t_ord, t_ptr, check=False)

    for _ in range(args.warmup):
        push()
    plan.packet_events_status()
    ev_ms = [timed(push) for _ in range(args.reps)]
    plan.packet_events_status()
    sent = int(t_ptr[-1].item())

    t_size = t((pk["payload_size"] + 40).astype(np.uint32), np.int32)  # payload + TCP/IP headers
    t_st = torch.zeros(n_pkts, dtype=torch.int32, device=dev)
    t_fw = torch.zeros(n_pkts, dtype=torch.int64, device=dev)
    t_late = torch.zeros(24 * 1024, dtype=torch.uint8, device=dev)
    t_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    until = r1 + 300 * synth.MS
    t_zero = torch.zeros(hosts + 1, dtype=torch.int32, device=dev)

    def inbound(bw_bytes):
        bw = np.full(hosts, bw_bytes, np.uint64)
        samples, last = [], None
        for k in range(args.warmup + args.reps):
            ib = InboundRouter(plan, bw, args.queue_cap)
            # an empty batch of the same size (no group holds a packet): sizes the record buffer
            ib.run(t_ord, t_zero, t_d, t_size, 0, 0, t_st, t_fw, t_late, t_cnt)
            ib.status()
            ms = timed(lambda: ib.run(t_ord, t_ptr, t_d, t_size, until, 0, t_st, t_fw, t_late, t_cnt))
            flags, pending = ib.status()
            if k >= args.warmup:
                samples.append(ms)
            st = t_st.view(torch.int32)
            last = {"pending": pending, "flags": flags,
                    "forwarded": int(((st & _lib.PDS_RELAY_FORWARDED) != 0).sum().item()),
                    "dropped": int(((st & _lib.PDS_ROUTER_DROPPED) != 0).sum().item()),
                    "cached": int(((st & _lib.PDS_RELAY_CACHED) != 0).sum().item()),
                    "forward_tasks": int(ib.state()["tasks_scheduled"].sum())}
            ib.close()
        return samples, last

    fast_ms, fast = inbound(125_000_000)
    slow_ms, slow = inbound(125_000)
    med = statistics.median
    out = {"what": "srt_inbound_run on the C5 batch, device ms per call (HIP events on the plan's stream)",
           "packets": n_pkts, "hosts": hosts, "sent": sent, "until_ns": until, "queue_cap": args.queue_cap,
           "warmup": args.warmup, "reps": args.reps,
           "timed_span": "HIP events around one srt_inbound_run: both launches, the gap between them and the stream "
                         "waits of the call; the record buffer is allocated by an untimed empty call before",
           "packet_events_ms": {"median": med(ev_ms), "samples": ev_ms},
           "inbound_125MBps_ms": {"median": med(fast_ms), "samples": fast_ms, "outcome": fast},
           "inbound_125kBps_ms": {"median": med(slow_ms), "samples": slow_ms, "outcome": slow},
           "congested_over_uncongested": med(slow_ms) / med(fast_ms),
           "uncongested_over_event_push": med(fast_ms) / med(ev_ms)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) or "samples" not in v else
                          {"median": v["median"], **({"outcome": v["outcome"]} if "outcome" in v else {})})
                      for k, v in out.items()}))
    plan.close()


if __name__ == "__main__":
    main()
