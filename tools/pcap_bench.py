#!/usr/bin/env python3
"""Times srt_pcap_run at the C5 size -- 1M records over 10k hosts, half of them
sent and half received, every record with a 512-byte payload of its own -- with
HIP events on the plan's stream around one call on a warmed instance, in two
runs: a header-only capture (capture_len 64) and a full capture (capture_len
65535; the stream, 0.57 GB, and the payload, 0.51 GB, are past the caches).
Beside each, in the same process and on the same inputs:

  * a torch formulation of the same output: a stable sort of the records by
    time and host, a cumsum of the sizes, the header bytes built column by
    column and scattered, the payload bytes scattered through a per-byte index;
    device ms by HIP events on torch's stream.  Its bytes are compared with the
    stage's, outside the timed regions;
  * the floor: a plain device-to-device copy of as many bytes as the call
    writes, HIP events on torch's stream.

Writes the raw samples to profiles/pcap_c5.json and prints a summary line.
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
    ap.add_argument("--ref-reps", type=int, default=5, help="timed runs of the torch formulation (it is slow)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--hosts", type=int, default=10_000)
    ap.add_argument("--payload", type=int, default=512)
    ap.add_argument("--no-refs", action="store_true", help="the stage alone (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcap_c5.json"))
    args = ap.parse_args()
    if args.reps < 20 and not args.no_refs:
        ap.error("--reps must be at least 20 (the median of fewer samples is not reported)")

    import torch

    from shadow_amd import NetworkGraph, PcapCapture, _lib, synth
    from shadow_amd.plan import PCAP_REC_DTYPE, RoutingPlan

    _lib.require_device()
    hosts, n, plen, seed = args.hosts, args.records, args.payload, 5
    src, dst, lat, loss = synth.complete_graph(16, seed)
    plan = RoutingPlan(NetworkGraph.from_edges(16, src, dst, lat, loss), np.arange(16, dtype=np.uint32),
                       device=0).run()
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)  # noqa: E731
    stream = torch.cuda.ExternalStream(plan.stream_ptr(), device=dev)
    cur = torch.cuda.current_stream(dev)

    # ---- the workload: two lists grouped by host, each in time order, times on a 1 us grid (ties are common)
    def side(k, first_payload):
        h = np.sort(rng.integers(0, hosts, size=k))
        ptr = np.searchsorted(h, np.arange(hosts + 1)).astype(np.int32)
        when = 1_000_000_000 + 1000 * rng.integers(0, 5000, size=k)
        r = np.zeros(k, PCAP_REC_DTYPE)
        r["time_ns"] = when[np.lexsort((when, h))]
        kind = rng.integers(0, 3, size=k)
        r["protocol"] = np.where(kind == 0, 17, 6)
        r["wscale_set"] = kind == 2
        r["wscale"] = 7
        r["payload_len"] = plen
        r["payload_off"] = (first_payload + np.arange(k, dtype=np.uint64)) * np.uint64(plen)
        for f, bits in (("src_ip_be", 32), ("dst_ip_be", 32), ("src_port_be", 16), ("dst_port_be", 16), ("seq", 32),
                        ("ack", 32), ("window", 16), ("tcp_flags", 8)):
            r[f] = rng.integers(0, 1 << bits, size=k)
        return r, ptr

    n_tx = n // 2
    tx, tx_ptr = side(n_tx, 0)
    rx, rx_ptr = side(n - n_tx, n_tx)
    payload = torch.randint(0, 256, (n * plen,), dtype=torch.uint8, device=dev)
    d = dict(tx=t(tx.view(np.uint8), np.uint8), rx=t(rx.view(np.uint8), np.uint8), tx_ptr=t(tx_ptr, np.int32),
             rx_ptr=t(rx_ptr, np.int32), ho=torch.zeros(hosts + 1, dtype=torch.int64, device=dev))

    def timed(fn, s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        plan.sync()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def torch_pcap(capture_len):
        """the same stream with torch ops -> (host_off int64 [hosts + 1], out uint8)"""
        recs = torch.cat([d["rx"].view(-1, 48), d["tx"].view(-1, 48)])  # received first at equal times
        cnt = torch.cat([d["rx_ptr"][1:] - d["rx_ptr"][:-1], d["tx_ptr"][1:] - d["tx_ptr"][:-1]]).to(torch.int64)
        host = torch.repeat_interleave(torch.arange(hosts, device=dev).repeat(2), cnt, output_size=n)
        w = recs.view(torch.int64).view(-1, 6)
        o = torch.sort(w[:, 0], stable=True).indices
        o = o[torch.sort(host[o], stable=True).indices]
        recs, host = recs[o], host[o]
        w = recs.view(torch.int64).view(-1, 6)
        b = recs.to(torch.int64)  # [n, 48] the records' bytes
        proto, ws = b[:, 40], b[:, 43] != 0
        hs = torch.where(proto == 17, 28, torch.where(ws, 44, 40))
        pl = b[:, 38] | b[:, 39] << 8
        total = hs + pl
        incl = total.clamp(max=capture_len)
        size = 16 + incl
        off = torch.cumsum(size, 0) - size
        per_host = torch.zeros(hosts, dtype=torch.int64, device=dev).index_add_(0, host, size)
        host_off = torch.zeros(hosts + 1, dtype=torch.int64, device=dev)
        host_off[1:] = torch.cumsum(per_host, 0)
        hdr = torch.zeros((n, 60), dtype=torch.uint8, device=dev)

        def put(col, v, nbytes, big):
            for i in range(nbytes):
                hdr[:, col + i] = (v >> 8 * (nbytes - 1 - i if big else i)) & 255

        tns = w[:, 0]
        put(0, tns // 1_000_000_000, 4, False)
        put(4, tns % 1_000_000_000 // 1000, 4, False)
        put(8, incl, 4, False)
        put(12, total, 4, False)
        hdr[:, 16], hdr[:, 22], hdr[:, 24], hdr[:, 25] = 0x45, 0x40, 0x40, proto
        put(18, total, 2, True)
        hdr[:, 28:40] = recs[:, 16:28]  # addresses and ports, already in network order
        tcp, flags = proto == 6, b[:, 41]
        seq = b[:, 28] | b[:, 29] << 8 | b[:, 30] << 16 | b[:, 31] << 24
        ack = b[:, 32] | b[:, 33] << 8 | b[:, 34] << 16 | b[:, 35] << 24
        zero = torch.zeros_like(seq)
        put(40, torch.where(tcp, seq, (pl + 8) << 16), 4, True)
        put(44, torch.where(tcp & ((flags & 0x10) != 0), ack, zero), 4, True)
        put(48, torch.where(tcp, (hs - 20) // 4 << 4, zero), 1, True)
        put(49, torch.where(tcp, flags & 0x17, zero), 1, True)
        put(50, torch.where(tcp, b[:, 36] | b[:, 37] << 8, zero), 2, True)
        opt = tcp & ws
        hdr[:, 56], hdr[:, 57], hdr[:, 58] = opt * 3, opt * 3, torch.where(opt, b[:, 42], zero)
        out = torch.zeros(int(host_off[-1]), dtype=torch.uint8, device=dev)
        col = torch.arange(60, device=dev)
        keep = col[None, :] < (16 + torch.minimum(incl, hs))[:, None]
        out[(off[:, None] + col[None, :])[keep]] = hdr[keep]
        nb = (incl - hs).clamp(min=0)
        if int(nb.sum()):
            first = torch.cumsum(nb, 0) - nb
            rec_of = torch.repeat_interleave(torch.arange(n, device=dev), nb)
            within = torch.arange(rec_of.numel(), device=dev) - first[rec_of]
            out[(off + 16 + hs)[rec_of] + within] = payload[w[:, 1][rec_of] + within]
        return host_off, out

    runs, same = {}, True
    for name, capture_len in (("header_only", 64), ("full", 65535)):
        per = 16 + min(capture_len, 44 + plen)
        out = torch.zeros(n * per, dtype=torch.uint8, device=dev)
        pc = PcapCapture(plan, hosts, capture_len, n)
        call = lambda: pc.run(d["tx"], d["tx_ptr"], d["rx"], d["rx_ptr"], payload, out, d["ho"])  # noqa: E731
        samples = {"pcap_ms": [], "torch_ms": [], "copy_ms": []}
        for k in range(args.warmup + args.reps):
            ms = timed(call, stream)
            if k >= args.warmup:
                samples["pcap_ms"].append(ms)
        # the same span is replayed on one instance, so every call after the first starts before the hosts' last
        # times: TIME_ORDER is expected (the records are written all the same) and no other flag is
        flags, n_recs, n_bytes = pc.status(check=False)
        same = same and flags in (0, _lib.PCAP_TIME_ORDER)
        total = int(d["ho"][-1])
        res = {}
        if not args.no_refs:
            for k in range(1 + args.ref_reps):
                ms = timed(lambda: res.__setitem__("t", torch_pcap(capture_len)), cur)
                if k:
                    samples["torch_ms"].append(ms)
            same = same and torch.equal(res["t"][0], d["ho"]) and torch.equal(res["t"][1], out[:total])
            res.clear()
            dst_buf = torch.empty(total, dtype=torch.uint8, device=dev)
            for k in range(args.warmup + args.reps):
                ms = timed(lambda: dst_buf.copy_(out[:total]), cur)
                if k >= args.warmup:
                    samples["copy_ms"].append(ms)
            del dst_buf
        pc.close()
        med = {f: statistics.median(v) for f, v in samples.items() if v}
        runs[name] = {"capture_len": capture_len, "flags": flags, "records_per_call": n_recs // (args.warmup + args.reps),
                      "bytes_per_call": total, "payload_bytes_read_per_call": int(max(0, per - 16 - 44) * n),
                      "median_ms": med, "stream_GBps": total / med["pcap_ms"] / 1e6, "samples": samples}
        if not args.no_refs:
            runs[name]["torch_over_pcap"] = med["torch_ms"] / med["pcap_ms"]
            runs[name]["pcap_over_copy"] = med["pcap_ms"] / med["copy_ms"]
            runs[name]["copy_GBps"] = total / med["copy_ms"] / 1e6
        del out
    plan.close()
    out = {"what": "srt_pcap_run at the C5 size, device ms per call (HIP events on the plan's stream around one call on a "
                   "warmed instance: four launches), a header-only and a full capture; beside each the torch formulation "
                   "of the same stream (stable sorts, cumsum, byte scatters; HIP events on torch's stream) and a plain "
                   "device-to-device copy of the call's bytes (the floor)",
           "measured_on": "MI355X", "records": n, "sent": n_tx, "received": n - n_tx, "hosts": hosts,
           "payload_len": plen, "tile_bytes": PcapCapture.tile_bytes(), "warmup": args.warmup, "reps": args.reps,
           "ref_reps": args.ref_reps, "outputs_equal": bool(same) and not args.no_refs, "runs": runs}
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
