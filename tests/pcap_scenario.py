"""Scenarios and hand-made cases of the pcap capture stage (srt_pcap), shared by
the CPU tests (the host-only instance) and the GPU tests (an instance on a
plan): generated multi-call scenarios with their self-check, a Runner that
feeds either form and returns what it wrote, the flag cases, the write pass's
tile edges and the error paths on raw ctypes.  The expected bytes always come
from pcap_model.PcapModel."""
import ctypes as C
import functools
import json
import os

import numpy as np

import pcap_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE, SPARSE = "dense", "sparse"
N_CALLS = 3
POISON = 0xAB
WINDOW_NS = 1_000_000
PAYLOAD_LENS = (0, 1, 3, 15, 16, 17, 1460)
CAPTURE_LENS = (0, 1, 19, 20, 21, 27, 28, 29, 39, 40, 43, 44, 45, 100, 65535)
POOL = 4096 + 1460 + 16  # bytes of a scenario's payload buffer


def golden():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "pcap_reference_vectors.json")))
    unhex = lambda s: bytes.fromhex(s.replace(" ", ""))  # noqa: E731
    for v in g["reference"].values():
        v["bytes"] = unhex(v["bytes"])
        if "data" in v:
            v["data"] = unhex(v["data"])
    for p in g["packets"]:
        p["bytes"], p["payload"] = unhex(p["bytes"]), unhex(p["payload"])
    return g


def rec(time_ns, protocol=PM.UDP, payload_off=0, payload_len=0, src="11.0.0.1", sport=1, dst="11.0.0.2", dport=2,
        seq=0, ack=0, window=0, tcp_flags=0, wscale=0, wscale_set=0):
    r = np.zeros(1, PM.REC)
    r["time_ns"], r["payload_off"], r["payload_len"], r["protocol"] = time_ns, payload_off, payload_len, protocol
    r["src_ip_be"], r["dst_ip_be"] = PM.ip_be(src), PM.ip_be(dst)
    r["src_port_be"], r["dst_port_be"] = PM.port_be(sport), PM.port_be(dport)
    r["seq"], r["ack"], r["window"], r["tcp_flags"] = seq, ack, window, tcp_flags
    r["wscale"], r["wscale_set"] = wscale, wscale_set
    return r


def fixture_rec(p, payload_off=0):
    return rec(p["time_ns"], p["protocol"], payload_off, len(p["payload"]), p["src"], p["sport"], p["dst"], p["dport"],
               p["seq"], p["ack"], p["window"], p["tcp_flags"], p["wscale"], p["wscale_set"])


def cat(*recs):
    return np.concatenate(recs) if recs else np.zeros(0, PM.REC)


def sized(time_ns, size, payload_off=0):
    """a UDP record whose bytes in the stream are `size` (at least 44) under a capture_len that does not cut it"""
    assert size >= 44
    return rec(time_ns, PM.UDP, payload_off, size - 44, sport=size & 0xffff)


def rand_recs(rng, times):
    n = len(times)
    r = np.zeros(n, PM.REC)
    r["time_ns"] = times
    kind = rng.integers(0, 3, n)  # UDP, TCP, TCP with window scale
    r["protocol"] = np.where(kind == 0, PM.UDP, PM.TCP)
    r["wscale_set"] = kind == 2
    r["wscale"] = rng.integers(0, 15, n)
    plen = np.where(rng.random(n) < 0.6, rng.choice(PAYLOAD_LENS, n), rng.integers(0, 1461, n))
    r["payload_len"] = plen
    r["payload_off"] = rng.integers(0, 4096 + 16, n)
    r["src_ip_be"], r["dst_ip_be"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n)
    r["src_port_be"], r["dst_port_be"] = rng.integers(0, 1 << 16, n), rng.integers(0, 1 << 16, n)
    r["seq"], r["ack"] = rng.integers(0, 1 << 32, n), rng.integers(1, 1 << 32, n)
    r["window"] = rng.integers(0, 1 << 16, n)
    r["tcp_flags"] = rng.integers(0, 256, n)
    return r


@functools.lru_cache(maxsize=None)
def scenario(n_hosts, shape):
    """N_CALLS calls in consecutive windows; times on a coarse grid, so a host's sent and received packets
    often share an instant; every call uses the index indirection on one of its lists"""
    rng = np.random.default_rng(1000 * n_hosts + (shape == DENSE))
    enabled = np.array([not (n_hosts > 3 and h % 7 == 3) for h in range(n_hosts)])
    payload = rng.integers(0, 256, POOL).astype(np.uint8)
    calls = []
    for c in range(N_CALLS):
        call = {}
        for side in ("tx", "rx"):
            if shape == DENSE:
                p = rng.random(n_hosts)
                cnt = np.where(p < 0.2, 0, np.where(p < 0.8, rng.integers(1, 21, n_hosts), rng.integers(65, 151, n_hosts)))
                if n_hosts == 1:
                    cnt[:] = 70 + c
            else:
                cnt = rng.integers(0, 3, n_hosts)
            ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
            times = np.concatenate([np.sort(c * WINDOW_NS + 1000 * rng.integers(0, 40 if shape == DENSE else 3, k)) for k in cnt] + [[]])
            recs = rand_recs(rng, times.astype(np.uint64))
            idx = None
            if (c + (side == "rx")) % 2 == 1:  # the list is recs[idx], recs holds strangers too
                n = len(recs)
                store = rand_recs(rng, rng.integers(0, 1 << 40, n + 5).astype(np.uint64))
                idx = rng.permutation(n + 5)[:n].astype(np.uint32)
                store[idx] = recs
                recs = store
            call[side], call[side + "_ptr"], call[side + "_idx"] = recs, ptr, idx
        calls.append(call)
    return {"n_hosts": n_hosts, "enabled": enabled, "payload": payload, "calls": calls,
            "rec_cap": max(1, max(int(c["tx_ptr"][-1]) + int(c["rx_ptr"][-1]) for c in calls))}


def listed(call, side):
    return call[side] if call[side + "_idx"] is None else call[side][call[side + "_idx"]]


def assert_scenario_is_not_empty(n_hosts, shape):
    """on the generator alone: every class the stage distinguishes is there"""
    sc = scenario(n_hosts, shape)
    allr = cat(*[listed(c, s) for c in sc["calls"] for s in ("tx", "rx")])
    assert len(allr) > n_hosts // 2
    assert (allr["protocol"] == PM.UDP).any() and (allr["protocol"] == PM.TCP).any()
    sizes = {PM.header_size(int(p), int(w)) for p, w in zip(allr["protocol"], allr["wscale_set"])}
    assert sizes == {28, 40, 44}, sizes
    assert (~sc["enabled"]).any() and sc["enabled"].sum() > n_hosts // 2
    assert all((c["tx_idx"] is None) != (c["rx_idx"] is None) for c in sc["calls"])
    ties = 0
    for c in sc["calls"]:
        tx, rx = listed(c, "tx"), listed(c, "rx")
        for h in np.nonzero(sc["enabled"])[0]:
            a = tx["time_ns"][c["tx_ptr"][h]:c["tx_ptr"][h + 1]]
            b = rx["time_ns"][c["rx_ptr"][h]:c["rx_ptr"][h + 1]]
            ties += len(np.intersect1d(a, b))
    assert ties > 5, ties
    if shape == DENSE:
        per_host = np.diff(sc["calls"][0]["tx_ptr"].astype(np.int64))
        assert per_host.max() > 64 and (per_host == 0).any()
        assert set(PAYLOAD_LENS) <= set(allr["payload_len"].tolist())
        assert len(set((allr["payload_off"] % 16).tolist())) == 16
    return ties


class Runner:
    """one srt_pcap instance, host-only (plan None, numpy) or on a plan (torch tensors of its device)"""

    def __init__(self, plan, n_hosts, capture_len, rec_cap, enabled=None, tx_first=False):
        from shadow_amd import PcapCapture, _lib

        self.plan, self.n_hosts = plan, n_hosts
        self.pc = PcapCapture(plan, n_hosts, capture_len, rec_cap, enabled,
                              _lib.PCAP_TX_FIRST if tx_first else _lib.PCAP_RX_FIRST)

    def _dev(self, a, view):
        if a is None:
            return None
        a = np.ascontiguousarray(a).view(view)
        if self.plan is None:
            return a.copy()
        import torch

        signed = {np.uint8: np.uint8, np.uint32: np.int32, np.uint64: np.int64}[view]
        return torch.from_numpy(a.view(signed).copy()).to("cuda:0")

    def run(self, tx, tx_ptr, rx, rx_ptr, payload, out_cap, tx_idx=None, rx_idx=None, misalign=0):
        """-> (host_off uint64 [n_hosts+1], the whole out buffer uint8 [out_cap], poisoned before the call)"""
        out = self._dev(np.full(out_cap + misalign, POISON, np.uint8), np.uint8)
        ho = self._dev(np.full(self.n_hosts + 1, 0x5555555555555555, np.uint64), np.uint64)
        self.pc.run(self._dev(tx, np.uint8), self._dev(np.asarray(tx_ptr, np.uint32), np.uint32),
                    self._dev(rx, np.uint8), self._dev(np.asarray(rx_ptr, np.uint32), np.uint32),
                    self._dev(payload, np.uint8), out[misalign:], ho,
                    self._dev(None if tx_idx is None else np.asarray(tx_idx, np.uint32), np.uint32),
                    self._dev(None if rx_idx is None else np.asarray(rx_idx, np.uint32), np.uint32))
        if self.plan is not None:
            import torch

            torch.cuda.synchronize()
            out, ho = out.cpu().numpy(), ho.cpu().numpy()
        return ho.view(np.uint64), out[misalign:]

    def status(self, check=False):
        return self.pc.status(check)

    def close(self):
        self.pc.close()


def check_call(r, m, tx, tx_ptr, rx, rx_ptr, payload, slack=37, out_cap=None, what=None, **kw):
    """the call on runner r and model m: the same host_off, the same bytes, poison behind them"""
    idx = {k: kw[k] for k in ("tx_idx", "rx_idx") if k in kw}
    probe = PM.PcapModel(m.n_hosts, m.capture_len, m.enabled, m.tx_first)
    probe.last = list(m.last)
    total = int(probe.run(tx, tx_ptr, rx, rx_ptr, payload, 1 << 62, **idx)[0][-1])
    cap = total + slack if out_cap is None else out_cap
    want_off, want = m.run(tx, tx_ptr, rx, rx_ptr, payload, cap, **idx)
    got_off, out = r.run(tx, tx_ptr, rx, rx_ptr, payload, cap, **kw)
    assert np.array_equal(got_off, want_off), (what, got_off, want_off)
    if want is None:
        assert (out == POISON).all(), (what, "OVERFLOW must leave d_out untouched")
        return total
    want = np.frombuffer(want, np.uint8)
    bad = np.nonzero(out[:total] != want)[0]
    assert not len(bad), (what, "first differing byte", int(bad[0]), "of", total)
    assert (out[total:] == POISON).all(), (what, "wrote past the call's total")
    return total


def run_scenario(plan, n_hosts, shape, capture_len, tx_first=False, misalign=0):
    """-> ([(host_off, bytes)] a call, status)"""
    sc = scenario(n_hosts, shape)
    want = model_scenario(n_hosts, shape, capture_len, tx_first)[0]
    r = Runner(plan, n_hosts, capture_len, sc["rec_cap"], sc["enabled"], tx_first)
    outs = []
    try:
        for c, (w_off, w) in zip(sc["calls"], want):
            off, out = r.run(c["tx"], c["tx_ptr"], c["rx"], c["rx_ptr"], sc["payload"], len(w) + 53,
                             tx_idx=c["tx_idx"], rx_idx=c["rx_idx"], misalign=misalign)
            assert (out[int(off[-1]):] == POISON).all()
            outs.append((off, out[:int(off[-1])].tobytes()))
        st = r.status()
    finally:
        r.close()
    return outs, st


@functools.lru_cache(maxsize=None)
def model_scenario(n_hosts, shape, capture_len, tx_first=False):
    sc = scenario(n_hosts, shape)
    m = PM.PcapModel(n_hosts, capture_len, sc["enabled"], tx_first)
    outs = [m.run(c["tx"], c["tx_ptr"], c["rx"], c["rx_ptr"], sc["payload"], 1 << 62, c["tx_idx"], c["rx_idx"])
            for c in sc["calls"]]
    return outs, m.status()


def same_outputs(got, want, what=None):
    assert len(got) == len(want) == N_CALLS
    for k, ((g_off, g), (w_off, w)) in enumerate(zip(got, want)):
        assert np.array_equal(g_off, w_off), (what, k)
        assert g == w, (what, k, len(g), len(w))


def parse_stream(data, capture_len):
    """the records of a host's stream, as (ts_sec, ts_usec, orig_len, packet bytes)"""
    import struct

    out, at = [], 0
    while at < len(data):
        sec, usec, incl, orig = struct.unpack_from("=IIII", data, at)
        assert incl == min(capture_len, orig) and at + 16 + incl <= len(data)
        out.append((sec, usec, orig, data[at + 16:at + 16 + incl]))
        at += 16 + incl
    return out


# ---- hand-made cases; make(n_hosts, capture_len, rec_cap, enabled=None, tx_first=False) -> Runner
def _pair(make, n_hosts, capture_len, rec_cap, enabled=None, tx_first=False):
    return make(n_hosts, capture_len, rec_cap, enabled, tx_first), PM.PcapModel(n_hosts, capture_len, enabled, tx_first)


def case_fixtures(make):
    """every hand-worked packet, alone, as sent and as received, its payload at an odd offset"""
    for p in golden()["packets"]:
        payload = np.frombuffer(b"\xee" * 3 + p["payload"] + b"\xdd", np.uint8)
        for side in (0, 1):
            r, m = _pair(make, 1, p["capture_len"], 4)
            try:
                one, none = fixture_rec(p, 3), cat()
                args = (one, [0, 1], none, [0, 0]) if side == 0 else (none, [0, 0], one, [0, 1])
                off, out = r.run(*args, payload, 200)
                m.run(*args, payload, 200)
                assert out[:int(off[1])].tobytes() == p["bytes"], p["name"]
                check_call(r, m, *args, payload, what=p["name"])
                assert r.status() == m.status() == (0, 2, 2 * len(p["bytes"]))
            finally:
                r.close()


def case_tie_rules(make):
    """a sent and a received packet of one instant between two others; both rules; equal times inside a list"""
    tx = cat(rec(10, sport=1), rec(20, sport=2), rec(20, sport=3), rec(30, sport=4))
    rx = cat(rec(20, sport=5), rec(20, sport=6), rec(25, sport=7))
    for tx_first, order in ((False, [1, 5, 6, 2, 3, 7, 4]), (True, [1, 2, 3, 5, 6, 7, 4])):
        r, m = _pair(make, 1, 28, 7, None, tx_first)
        try:
            off, out = r.run(tx, [0, 4], rx, [0, 3], None, 7 * 44)
            ports = [int.from_bytes(p[3][20:22], "big") for p in parse_stream(out[:int(off[1])].tobytes(), 28)]
            assert ports == order, (tx_first, ports)
        finally:
            r.close()
        r, m = _pair(make, 1, 28, 7, None, tx_first)
        try:
            check_call(r, m, tx, [0, 4], rx, [0, 3], None)
            assert r.status() == m.status() == (0, 7, 7 * 44)
        finally:
            r.close()


def case_overflow(make):
    """one byte short: host_off in full, d_out untouched, counts and last times as before; the retry is clean"""
    tx, rx = cat(rec(100, payload_len=5), rec(200)), cat(rec(150, PM.TCP, wscale_set=1))
    payload = np.arange(5, dtype=np.uint8)
    r, m = _pair(make, 2, 65535, 3)
    try:
        total = check_call(r, m, tx, [0, 1, 2], rx, [0, 0, 1], payload, out_cap=49 + 44 + 60 - 1, what="short")
        assert total == 153 and r.status() == m.status() == (PM.OVERFLOW, 0, 0)
        check_call(r, m, tx, [0, 1, 2], rx, [0, 0, 1], payload, out_cap=0, what="no room at all")
        assert r.status() == m.status() == (PM.OVERFLOW, 0, 0)
        check_call(r, m, tx, [0, 1, 2], rx, [0, 0, 1], payload, slack=0, what="retry")
        assert r.status() == m.status() == (0, 3, 153)
    finally:
        r.close()


def _skipped(make, bad, flag, payload_bytes=8):
    payload = np.arange(payload_bytes, dtype=np.uint8)
    tx, rx = cat(rec(10, payload_len=2), rec(30, payload_off=6, payload_len=2), bad), cat(rec(20, PM.TCP), bad)
    r, m = _pair(make, 2, 65535, 5)
    try:
        check_call(r, m, tx, [0, 0, 3], rx, [0, 2, 2], payload, what=flag)
        st = r.status()
        assert st == m.status() == (flag, 3, 46 + 46 + 56), st
        # the skipped record's time is not the host's last time: the same span again raises nothing
        check_call(r, m, cat(rec(31)), [0, 0, 1], cat(rec(21)), [0, 1, 1], payload, what=flag)
        assert r.status() == m.status() == (0, 5, 46 + 46 + 56 + 88)
    finally:
        r.close()


def case_bad_protocol(make):
    _skipped(make, rec(40, protocol=1), PM.BAD_PROTOCOL)


def case_bad_length(make):
    _skipped(make, rec(40, PM.TCP, payload_len=65496, wscale_set=0), PM.BAD_LENGTH, 65496)  # 40 + 65496 = 65536


def case_length_at_the_limit(make):
    """header + payload == 65535 is written whole"""
    payload = (np.arange(65507) % 251).astype(np.uint8)
    r, m = _pair(make, 1, 65535, 3)
    try:
        tx = cat(rec(1, PM.UDP, 0, 65507), rec(2, PM.TCP, 12, 65495), rec(3, PM.TCP, 16, 65491, wscale_set=1))
        check_call(r, m, tx, [0, 3], cat(), [0, 0], payload)
        assert r.status() == m.status() == (0, 3, 3 * 65551)
    finally:
        r.close()


def case_bad_payload(make):
    _skipped(make, rec(40, payload_off=7, payload_len=2), PM.BAD_PAYLOAD)
    _skipped(make, rec(40, payload_off=(1 << 64) - 1, payload_len=2), PM.BAD_PAYLOAD)


def case_time_order_in_a_list(make):
    """a list that decreases is written in list order, merged by the largest time so far"""
    tx = cat(rec(10, sport=1), rec(50, sport=2), rec(20, sport=3), rec(60, sport=4))
    rx = cat(rec(15, sport=5), rec(40, sport=6), rec(50, sport=7), rec(55, sport=8))
    r, m = _pair(make, 2, 28, 8)
    try:
        off, out = r.run(tx, [0, 0, 4], rx, [0, 0, 4], None, 8 * 44)
        m.run(tx, [0, 0, 4], rx, [0, 0, 4], None, 8 * 44)
        ports = [int.from_bytes(p[3][20:22], "big") for p in parse_stream(out[:int(off[2])].tobytes(), 28)]
        assert ports == [1, 5, 6, 7, 2, 3, 8, 4] and off[1] == 0, ports
        check_call(r, m, tx, [0, 0, 4], rx, [0, 0, 4], None)
        st = r.status()
        assert st == m.status() and st[0] == PM.TIME_ORDER and st[1] == 16
    finally:
        r.close()


def case_time_order_against_the_last_call(make):
    """host 1's second call starts before its first call's last record; host 0's does not"""
    r, m = _pair(make, 2, 28, 4)
    try:
        check_call(r, m, cat(rec(100), rec(500)), [0, 1, 2], cat(rec(90)), [0, 1, 1], None)
        assert r.status() == m.status() == (0, 3, 132)
        check_call(r, m, cat(rec(100), rec(500)), [0, 1, 2], cat(), [0, 0, 0], None)
        assert r.status() == m.status() == (0, 5, 220)
        check_call(r, m, cat(rec(101)), [0, 1, 1], cat(rec(499)), [0, 0, 1], None)
        assert r.status() == m.status() == (PM.TIME_ORDER, 7, 308)
    finally:
        r.close()


def case_disabled_hosts(make):
    """a host that does not capture has an empty range, bad records of it raise nothing; only the last host on"""
    bad = rec(5, protocol=99)
    tx, rx = cat(bad, rec(9), rec(7, payload_len=3)), cat(rec(3), rec(8, PM.TCP), rec(8))
    r = make(3, 65535, 6, [0, 0, 1])
    try:
        off, _ = r.run(tx, [0, 1, 2, 3], rx, [0, 1, 1, 3], np.zeros(3, np.uint8), 200)
        assert list(off) == [0, 0, 0, 47 + 56 + 44]
    finally:
        r.close()
    r, m = _pair(make, 3, 65535, 6, [0, 0, 1])
    try:
        check_call(r, m, tx, [0, 1, 2, 3], rx, [0, 1, 1, 3], np.zeros(3, np.uint8))
        assert r.status() == m.status() == (0, 3, 147)
    finally:
        r.close()


def case_empty_lists(make):
    """n_tx == 0, n_rx == 0, both"""
    r, m = _pair(make, 3, 65535, 4)
    try:
        some, none = cat(rec(1), rec(2, PM.TCP)), cat()
        payload = np.zeros(1, np.uint8)
        check_call(r, m, none, [0, 0, 0, 0], some, [0, 1, 1, 2], payload, what="n_tx == 0")
        check_call(r, m, cat(rec(3), rec(4, PM.TCP)), [0, 0, 2, 2], none, [0, 0, 0, 0], payload, what="n_rx == 0")
        assert check_call(r, m, none, [0, 0, 0, 0], none, [0, 0, 0, 0], payload, what="both") == 0
        assert r.status() == m.status() == (0, 4, 200)
    finally:
        r.close()


def case_null_payload(make):
    """d_payload may be NULL only when capture_len <= 28"""
    from shadow_amd import _lib

    tx = cat(rec(1, PM.UDP), rec(2, PM.TCP, wscale_set=1))
    r, m = _pair(make, 1, 28, 2)
    try:
        check_call(r, m, tx, [0, 2], cat(), [0, 0], None)
        assert r.status() == m.status() == (0, 2, 88)
    finally:
        r.close()
    r = make(1, 29, 2)
    try:
        try:
            r.run(tx, [0, 2], cat(), [0, 0], None, 200)
        except _lib.SrtError as e:
            assert e.code == _lib.SRT_ERR_INVALID and "capture_len" in str(e)
        else:
            raise AssertionError("a NULL payload with capture_len 29 must be refused")
        assert r.status() == (0, 0, 0)
    finally:
        r.close()


def case_payload_lengths_and_alignments(make):
    """every payload length of the list at every residue of payload_off mod 16, whole and cut one byte short"""
    payload = (np.arange(1460 + 32) * 7 % 253).astype(np.uint8)
    recs = [rec(1000 * i + res, (PM.UDP, PM.TCP)[(i + res) % 2], res + (16 if i % 2 else 0), n, wscale_set=res % 3 == 0)
            for i, n in enumerate(PAYLOAD_LENS) for res in range(16)]
    tx, rx = cat(*recs[0::2]), cat(*recs[1::2])
    for capture_len in (65535, 28 + 1459):
        r, m = _pair(make, 1, capture_len, len(recs))
        try:
            check_call(r, m, tx, [0, len(tx)], rx, [0, len(rx)], payload, what=capture_len)
            assert r.status() == m.status()
        finally:
            r.close()


CASES = [case_fixtures, case_tie_rules, case_overflow, case_bad_protocol, case_bad_length, case_length_at_the_limit,
         case_bad_payload, case_time_order_in_a_list, case_time_order_against_the_last_call, case_disabled_hosts,
         case_empty_lists, case_null_payload, case_payload_lengths_and_alignments]


# ---- the write pass at its tile edges; T = srt_pcap_tile_bytes()
def _sizes_call(make, sizes, what, misalign=0, enabled=None, n_hosts=1, host=0):
    """records of the given stream sizes, alternately sent and received, all of host `host`"""
    payload = (np.arange(max(sizes) + 16) * 13 % 251).astype(np.uint8)
    recs = [sized(10 * i, s, i % 16) for i, s in enumerate(sizes)]
    tx, rx = cat(*recs[0::2]), cat(*recs[1::2])
    ptr = lambda n: [0] * (host + 1) + [n] * (n_hosts - host)  # noqa: E731
    r, m = _pair(make, n_hosts, 65535, len(recs), enabled)
    try:
        total = check_call(r, m, tx, ptr(len(tx)), rx, ptr(len(rx)), payload, what=what, misalign=misalign)
        assert total == sum(sizes) and r.status() == m.status() == (0, len(sizes), total)
    finally:
        r.close()


def edge_totals(make):
    from shadow_amd import PcapCapture

    T = PcapCapture.tile_bytes()
    for total in (T - 1, T, T + 1, 2 * T + 1):
        n = total // 1000
        _sizes_call(make, [1000] * (n - 1) + [total - 1000 * (n - 1)], ("total", total))
        _sizes_call(make, [total] if total - 44 <= 65535 - 28 else [total - 50, 50], ("one record", total))


def edge_starts_and_ends(make):
    from shadow_amd import PcapCapture

    T = PcapCapture.tile_bytes()
    _sizes_call(make, [T - 1, 300], "a record starts at T - 1")
    _sizes_call(make, [T - 1, 44, 44], "a 44-byte record starts at T - 1")
    _sizes_call(make, [3000, T + 1 - 3000, 60], "a record ends at T + 1")
    _sizes_call(make, [T, 44], "a record ends at T")
    _sizes_call(make, [T - 16, 45, 100], "the record header ends at T")
    _sizes_call(make, [3 * T + 5, 44], "a record over four tiles")


def edge_alignments(make):
    """a 1,516-byte record (a full TCP segment) across a tile boundary at each of the 16 alignments"""
    from shadow_amd import PcapCapture

    T = PcapCapture.tile_bytes()
    for a in range(16):
        payload = (np.arange(T + 64) * 11 % 241).astype(np.uint8)
        recs = cat(sized(1, T - 700 + a, 3), rec(2, PM.TCP, 5 + a, 1460), sized(3, 77, 1))
        r, m = _pair(make, 1, 65535, 3)
        try:
            assert check_call(r, m, recs, [0, 3], cat(), [0, 0], payload, what=("alignment", a)) == T - 700 + a + 1516 + 77
        finally:
            r.close()
    if T < 1516:
        _sizes_call(make, [60, T + 9, 50], "a record longer than a tile")


def edge_out_misaligned(make):
    """d_out at every byte alignment: the first tile is partial"""
    from shadow_amd import PcapCapture

    T = PcapCapture.tile_bytes()
    for mis in (1, 3, 8, 15):
        _sizes_call(make, [T - 20, 100, T + 1, 44], ("misaligned", mis), misalign=mis)
        _sizes_call(make, [44], ("misaligned, one record", mis), misalign=mis)


def edge_last_host_only(make):
    from shadow_amd import PcapCapture

    T = PcapCapture.tile_bytes()
    _sizes_call(make, [T // 2, T // 2 + 1, 44], "only the last host captures", enabled=[0] * 64 + [1], n_hosts=65,
                host=64)


EDGES = [edge_totals, edge_starts_and_ends, edge_alignments, edge_out_misaligned, edge_last_host_only]


def error_paths(plan_handle=None):
    """raw ctypes: every refusal, and that a refused call changes nothing"""
    from shadow_amd import _lib

    L = _lib.lib()
    err = _lib.SrtErr()
    h = C.c_void_p()
    mk = lambda *a: L.srt_pcap_create(plan_handle, *a, C.byref(h), C.byref(err))  # noqa: E731
    assert L.srt_pcap_create(plan_handle, 1, 64, None, 4, 0, None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert mk(1 << 31, 64, None, 4, 0) == _lib.SRT_ERR_INVALID and not h
    assert mk(1, 64, None, 1 << 31, 0) == _lib.SRT_ERR_INVALID and b"rec_cap" in err.msg
    assert mk(1, 64, None, 4, 2) == _lib.SRT_ERR_INVALID and b"flag" in err.msg
    assert L.srt_pcap_status(None, None, None, None, C.byref(err)) == _lib.SRT_ERR_INVALID
    assert L.srt_pcap_run(None, None, None, None, 0, None, None, None, 0, None, 0, None, 0, None,
                          C.byref(err)) == _lib.SRT_ERR_INVALID
    L.srt_pcap_destroy(None)
    assert mk(2, 64, None, 4, 0) == _lib.SRT_OK and h
    try:
        if plan_handle is None:
            ptr, ho = np.zeros(3, np.uint32), np.zeros(3, np.uint64)
            recs, out, pay = np.zeros(8, PM.REC), np.zeros(64, np.uint8), np.zeros(4, np.uint8)
            p = lambda a: a.ctypes.data  # noqa: E731
        else:
            import torch

            ptr, ho = torch.zeros(3, dtype=torch.int32, device="cuda:0"), torch.zeros(3, dtype=torch.int64, device="cuda:0")
            recs, out = torch.zeros(8 * 48, dtype=torch.uint8, device="cuda:0"), torch.zeros(64, dtype=torch.uint8, device="cuda:0")
            pay = torch.zeros(4, dtype=torch.uint8, device="cuda:0")
            p = lambda a: a.data_ptr()  # noqa: E731
        run = lambda *a: L.srt_pcap_run(h, *a, C.byref(err))  # noqa: E731
        ok = (p(recs), None, p(ptr), 0, p(recs), None, p(ptr), 0, p(pay), 4, p(out), 64, p(ho))
        assert run(*ok) == _lib.SRT_OK
        for k in (2, 6, 12):  # the pointer arrays and d_host_off
            assert run(*[None if i == k else a for i, a in enumerate(ok)]) == _lib.SRT_ERR_INVALID
        assert run(None, None, p(ptr), 1, p(recs), None, p(ptr), 0, p(pay), 4, p(out), 64, p(ho)) == _lib.SRT_ERR_INVALID
        assert run(p(recs), None, p(ptr), 0, None, None, p(ptr), 1, p(pay), 4, p(out), 64, p(ho)) == _lib.SRT_ERR_INVALID
        assert run(p(recs), None, p(ptr), 0, p(recs), None, p(ptr), 0, p(pay), 4, None, 64, p(ho)) == _lib.SRT_ERR_INVALID
        assert run(p(recs), None, p(ptr), 3, p(recs), None, p(ptr), 2, p(pay), 4, p(out), 64, p(ho)) == _lib.SRT_ERR_INVALID
        assert b"rec_cap" in err.msg
        assert run(p(recs), None, p(ptr), 0, p(recs), None, p(ptr), 0, None, 0, p(out), 64, p(ho)) == _lib.SRT_ERR_INVALID
        assert b"capture_len" in err.msg
        # d_out may be NULL when out_cap is 0
        assert run(p(recs), None, p(ptr), 0, p(recs), None, p(ptr), 0, p(pay), 4, None, 0, p(ho)) == _lib.SRT_OK
        flags, a, b = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7)
        assert L.srt_pcap_status(h, C.byref(flags), C.byref(a), C.byref(b), C.byref(err)) == _lib.SRT_OK
        assert (flags.value, a.value, b.value) == (0, 0, 0)
        assert L.srt_pcap_status(h, None, None, None, None) == _lib.SRT_OK
        # the file side's refusals
        assert L.srt_pcap_open_files(h, None, C.byref(err)) == _lib.SRT_ERR_INVALID
        assert L.srt_pcap_append_files(h, np.zeros(3, np.uint64).ctypes.data, None, C.byref(err)) == _lib.SRT_ERR_INVALID
        assert b"no files" in err.msg
    finally:
        L.srt_pcap_destroy(h)
