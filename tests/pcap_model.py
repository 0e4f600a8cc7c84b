"""Plain-Python restatement of the reference's pcap capture, written from
utility/pcap_writer.rs (file header, record header, the cut at capture_len),
host/network/network_interface.c:119-134 (the timestamps), routing/packet.c:378-403
(header sizes) and network/packet.rs:374-586 (the bytes of the IP, TCP and UDP
headers), and of srt_pcap's contract in include/srt.h (the per-host merge, the
flags).  Independent of shadow_amd/csrc/srt_pcap_step.h: bytes are built with
struct, one record at a time."""
import struct

import numpy as np

REC = np.dtype([("time_ns", "<u8"), ("payload_off", "<u8"), ("src_ip_be", "<u4"), ("dst_ip_be", "<u4"),
                ("src_port_be", "<u2"), ("dst_port_be", "<u2"), ("seq", "<u4"), ("ack", "<u4"), ("window", "<u2"),
                ("payload_len", "<u2"), ("protocol", "u1"), ("tcp_flags", "u1"), ("wscale", "u1"),
                ("wscale_set", "u1"), ("reserved", "<u4")])
FIELDS = ("time_ns", "payload_off", "src_ip_be", "dst_ip_be", "src_port_be", "dst_port_be", "seq", "ack", "window",
          "payload_len", "protocol", "tcp_flags", "wscale", "wscale_set")
OVERFLOW, BAD_PROTOCOL, BAD_LENGTH, BAD_PAYLOAD, TIME_ORDER = 1, 2, 4, 8, 16
TCP, UDP = 6, 17
FIN, SYN, RST, ACK = 0x01, 0x02, 0x04, 0x10


def file_header(capture_len):
    return struct.pack("=IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, capture_len, 101)


def write_packet(ts_sec, ts_usec, data, capture_len):
    """PcapWriter::write_packet: the record for raw packet bytes"""
    incl = min(capture_len, len(data))
    return struct.pack("=IIII", ts_sec, ts_usec, incl, len(data)) + bytes(data[:incl])


def ip_be(dotted):
    """the u32 a little-endian host holds for an address in network byte order"""
    return int.from_bytes(bytes(int(x) for x in dotted.split(".")), "little")


def port_be(port):
    return int.from_bytes(struct.pack(">H", port), "little")


def header_size(protocol, wscale_set):
    if protocol == UDP:
        return 28
    if protocol == TCP:
        return 44 if wscale_set else 40  # 20 + 3 option bytes, padded to a multiple of four
    return None


def packet_bytes(r, payload):
    """the whole packet as display_bytes writes it; r: a mapping with FIELDS"""
    hs = header_size(int(r["protocol"]), int(r["wscale_set"]))
    total = hs + len(payload)
    src = struct.pack("<I", int(r["src_ip_be"]))
    dst = struct.pack("<I", int(r["dst_ip_be"]))
    out = b"\x45\x00" + struct.pack(">H", total) + b"\x00\x00" + b"\x40\x00" + b"\x40" + bytes([int(r["protocol"])]) + \
        b"\x00\x00" + src + dst
    ports = struct.pack("<HH", int(r["src_port_be"]), int(r["dst_port_be"]))
    if int(r["protocol"]) == TCP:
        flags = int(r["tcp_flags"])
        opts = 4 if int(r["wscale_set"]) else 0
        out += ports + struct.pack(">II", int(r["seq"]), int(r["ack"]) if flags & ACK else 0)
        out += bytes([((20 + opts) // 4) << 4, flags & (FIN | SYN | RST | ACK)])
        out += struct.pack(">HHH", int(r["window"]), 0, 0)
        if opts:
            out += bytes([3, 3, int(r["wscale"]), 0])
    else:
        out += ports + struct.pack(">HH", len(payload) + 8, 0)
    assert len(out) == hs
    return out + bytes(payload)


def record_bytes(r, payload, capture_len):
    now = int(r["time_ns"])
    return write_packet((now // 10**9) & 0xffffffff, (now % 10**9) // 1000, packet_bytes(r, payload), capture_len)


class PcapModel:
    def __init__(self, n_hosts, capture_len, enabled=None, tx_first=False):
        self.n_hosts, self.capture_len, self.tx_first = n_hosts, capture_len, tx_first
        self.enabled = [True] * n_hosts if enabled is None else [bool(x) for x in enabled]
        self.last = [0] * n_hosts
        self.flags = 0
        self.n_records = self.n_bytes = 0

    def run(self, tx, tx_ptr, rx, rx_ptr, payload, out_cap, tx_idx=None, rx_idx=None):
        """-> (host_off [n_hosts+1] uint64, the stream's bytes or None on OVERFLOW)"""
        payload = b"" if payload is None else bytes(payload)
        lists = []
        for recs, idx in ((tx, tx_idx), (rx, rx_idx)):
            recs = np.zeros(0, REC) if recs is None else recs
            lists.append(recs if idx is None else recs[np.asarray(idx, np.int64)])
        ptrs = (np.asarray(tx_ptr, np.int64), np.asarray(rx_ptr, np.int64))
        host_off, parts, n_recs, new_last = [0], [], 0, list(self.last)
        for h in range(self.n_hosts):
            chunk = []
            if self.enabled[h]:
                entries = []
                for side in (0, 1):
                    key = 0
                    prio = side if self.tx_first else 1 - side  # the side written first at equal times has 0
                    for k in range(int(ptrs[side][h]), int(ptrs[side][h + 1])):
                        t = int(lists[side][k]["time_ns"])
                        if t < key or t < self.last[h]:
                            self.flags |= TIME_ORDER
                        key = max(key, t)
                        entries.append((key, prio, k, side))
                for key, prio, k, side in sorted(entries):
                    r = lists[side][k]
                    hs = header_size(int(r["protocol"]), int(r["wscale_set"]))
                    off, n = int(r["payload_off"]), int(r["payload_len"])
                    if hs is None:
                        self.flags |= BAD_PROTOCOL
                    elif hs + n > 65535:
                        self.flags |= BAD_LENGTH
                    elif off + n > len(payload):
                        self.flags |= BAD_PAYLOAD
                    else:
                        chunk.append(record_bytes(r, payload[off:off + n], self.capture_len))
                        new_last[h] = max(new_last[h], int(r["time_ns"]))
            n_recs += len(chunk)
            parts.append(b"".join(chunk))
            host_off.append(host_off[-1] + len(parts[-1]))
        host_off = np.array(host_off, np.uint64)
        if host_off[-1] > out_cap:
            self.flags |= OVERFLOW
            return host_off, None
        self.last = new_last
        self.n_records += n_recs
        self.n_bytes += int(host_off[-1])
        return host_off, b"".join(parts)

    def status(self):
        f, self.flags = self.flags, 0
        return f, self.n_records, self.n_bytes
