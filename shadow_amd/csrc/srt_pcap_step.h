// srt_pcap_step.h -- the pcap capture of one interface class, batched over hosts:
// what _networkinterface_capturePacket (host/network/network_interface.c:119-134)
// hands to PcapWriter::write_packet_fmt (utility/pcap_writer.rs:86-142) and what
// PacketRc::display_bytes (network/packet.rs:374-586) writes through the Give
// writer (utility/give.rs), formatted as one byte stream a host.  Written once
// for the host and the device (srt_pcap.hip compiles it for both).
//
// A record is 16 + incl_len bytes: ts_sec, ts_usec, incl_len, orig_len (u32,
// native endian), then the first incl_len = min(capture_len, total) bytes of the
// packet, total = header_size + payload_len, header_size 28 (UDP), 40 (TCP) or 44
// (TCP with the window-scale option).  The cut is at exactly capture_len bytes,
// wherever it falls.
//
// A call, per host: the sent and the received list are merged stably by time
// (equal times: received first under SRT_PCAP_RX_FIRST, sent first under
// SRT_PCAP_TX_FIRST).  The key of a record is the largest time of its list up to
// and including it, so a list that decreases (flagged TIME_ORDER) still merges in
// list order; for a list in order the key is the record's time and the merged
// rank of a record is its place in its own list plus a binary search in the
// other one.  Merged position = tx_ptr[h] + rx_ptr[h] + rank: the call's records
// in merged order are one array, hosts in index order, and the byte offset of a
// record is the sum of the sizes before it.
//
// The passes:
//   hosts    a lane group a host: order check, ranks, sizes, the host's total
//   scan     the hosts' totals into d_host_off, OVERFLOW, the last times
//   offsets  a lane group a host: the byte offset of every merged position
//   write    a tile of TILE output bytes at a time: the records that overlap it
//            are found by a search in the offsets, a lane group a record puts
//            its headers and payload bytes into a tile buffer, the tile is
//            stored clipped to [0, total)
// Every write is preceded by its range check: merged positions are below
// te + re <= rec_cap, tile bytes inside the tile, output bytes below the call's
// total, which is at most out_cap; payload bytes are read only from a range
// checked against payload_bytes; a stale entry of the scratch arrays is
// re-validated before it is used.
#ifndef SRT_PCAP_STEP_H
#define SRT_PCAP_STEP_H

#include <stdint.h>
#include <string.h>

#include "../../include/srt.h"

#include "srt_relay_common.h"

namespace pcap {

using relay::raise;

constexpr uint32_t F_OVERFLOW = SRT_PCAP_OVERFLOW, F_BAD_PROTOCOL = SRT_PCAP_BAD_PROTOCOL,
                   F_BAD_LENGTH = SRT_PCAP_BAD_LENGTH, F_BAD_PAYLOAD = SRT_PCAP_BAD_PAYLOAD,
                   F_TIME_ORDER = SRT_PCAP_TIME_ORDER;
constexpr uint32_t TILE = 4096;     // output bytes a tile of the write pass
constexpr uint32_t REC_HDR = 16;    // the pcap record header
constexpr uint32_t HDR_WORDS = 15;  // record header + the longest packet header (44), in 32-bit words
constexpr uint32_t NO_ENT = 0xffffffffu, RX_BIT = 0x80000000u;
constexpr uint32_t DECREASES = 1, EARLY = 2;  // order_check's bits

// the words a call leaves behind, 32 bytes
struct State {
    uint32_t flags;  // SRT_PCAP_* bits since the last status call
    uint32_t pad;
    uint64_t n_recs, n_bytes;  // written since create
    uint64_t write_total;      // bytes the write pass of the current call stores (0 on OVERFLOW)
};

struct Ctx {
    State *st;
    uint64_t *last, *pend, *host_bytes;  // [n_hosts] last time written; this call's largest time; its bytes
    uint32_t *host_cnt;                  // [n_hosts] this call's records written
    const uint8_t *enabled;              // [n_hosts]
    uint32_t *ent, *size;                // [rec_cap] merged position -> list entry (RX_BIT | k, or NO_ENT), bytes
    uint64_t *off;                       // [rec_cap + 1] merged position -> byte offset in d_out
    uint32_t n_hosts, capture_len, rx_first, pad;
    // the call
    const srt_pcap_rec *rec[2];   // 0 tx, 1 rx
    const uint32_t *idx[2];       // nullptr: identity
    const uint32_t *ptr[2];       // [n_hosts + 1]
    uint32_t n[2];
    const uint8_t *payload;
    uint64_t payload_bytes;
    uint8_t *out;
    uint64_t out_cap;
    uint64_t *host_off;  // [n_hosts + 1]
};

struct Seg {
    uint32_t b[2], e[2];
};

struct HostAcc {
    uint64_t bytes, maxt;
    uint32_t cnt, flags;
};

SRT_HD uint32_t walked(const Ctx &c, uint32_t side) { return relay::walked(c.ptr[side], c.n_hosts, c.n[side]); }

// host h's segments of the two lists, held below the lists' lengths whatever ptr[] says
SRT_HD Seg segs(const Ctx &c, uint32_t h) {
    Seg s;
#pragma unroll
    for (uint32_t side = 0; side < 2; ++side) {
        const uint32_t lim = walked(c, side), b = c.ptr[side][h], e = c.ptr[side][h + 1];
        s.b[side] = b < lim ? b : lim;
        s.e[side] = e < lim ? e : lim;
        if (s.e[side] < s.b[side]) s.e[side] = s.b[side];
    }
    return s;
}

SRT_HD const srt_pcap_rec &rec_at(const Ctx &c, uint32_t side, uint32_t k) {
    return c.rec[side][c.idx[side] ? c.idx[side][k] : k];
}

SRT_HD uint64_t time_at(const Ctx &c, uint32_t side, uint32_t k) { return rec_at(c, side, k).time_ns; }

// packet_getHeaderSize (routing/packet.c:378-403) plus the IP header; 0: neither TCP nor UDP
SRT_HD uint32_t header_size(const srt_pcap_rec &r) {
    if (r.protocol == 17) return 28;
    if (r.protocol == 6) return r.wscale_set ? 44 : 40;
    return 0;
}

// the record's bytes in the stream, 16 + incl_len; 0: skipped, with its flag in `flags`
SRT_HD uint32_t rec_bytes(const Ctx &c, const srt_pcap_rec &r, uint32_t &flags) {
    const uint32_t hs = header_size(r);
    if (!hs) {
        flags |= F_BAD_PROTOCOL;
        return 0;
    }
    const uint32_t total = hs + r.payload_len;
    if (total > 65535u) {
        flags |= F_BAD_LENGTH;
        return 0;
    }
    if (r.payload_off > c.payload_bytes || r.payload_len > c.payload_bytes - r.payload_off) {
        flags |= F_BAD_PAYLOAD;
        return 0;
    }
    return REC_HDR + (total < c.capture_len ? total : c.capture_len);
}

// lane l of L: does a list of host h decrease, is a record earlier than the host's last time
SRT_HD uint32_t order_check(const Ctx &c, uint32_t h, const Seg &s, uint32_t l, uint32_t L) {
    const uint64_t last = c.last[h];
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t side = 0; side < 2; ++side)
        for (uint32_t k = s.b[side] + l; k < s.e[side]; k += L) {
            const uint64_t t = time_at(c, side, k);
            if (t < last) bits |= EARLY;
            if (k > s.b[side] && t < time_at(c, side, k - 1)) bits |= DECREASES;
        }
    return bits;
}

// list entry k of `side` takes merged position pos
SRT_HD void place(const Ctx &c, uint32_t pos, uint32_t side, uint32_t k, HostAcc &a) {
    const srt_pcap_rec &r = rec_at(c, side, k);
    const uint32_t sz = rec_bytes(c, r, a.flags);
    c.size[pos] = sz;
    c.ent[pos] = sz ? (side ? RX_BIT : 0u) | k : NO_ENT;
    if (sz) {
        a.bytes += sz;
        a.cnt += 1;
        if (r.time_ns > a.maxt) a.maxt = r.time_ns;
    }
}

// entries of [b, e) of `side` with time < t (upper: <= t); the list is in order
SRT_HD uint32_t bound(const Ctx &c, uint32_t side, uint32_t b, uint32_t e, uint64_t t, bool upper) {
    uint32_t lo = b, hi = e;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint64_t v = time_at(c, side, mid);
        if (upper ? v <= t : v < t) lo = mid + 1;
        else hi = mid;
    }
    return lo - b;
}

// both lists in order: a record's rank is its place in its list plus the other list's records before it
SRT_HD void merge_sorted(const Ctx &c, const Seg &s, uint32_t l, uint32_t L, HostAcc &a) {
    const uint32_t base = s.b[0] + s.b[1];
    for (uint32_t k = s.b[0] + l; k < s.e[0]; k += L)
        place(c, base + (k - s.b[0]) + bound(c, 1, s.b[1], s.e[1], time_at(c, 0, k), c.rx_first != 0), 0, k, a);
    for (uint32_t k = s.b[1] + l; k < s.e[1]; k += L)
        place(c, base + (k - s.b[1]) + bound(c, 0, s.b[0], s.e[0], time_at(c, 1, k), c.rx_first == 0), 1, k, a);
}

// a list decreases: one walker, the key of a record the largest time of its list so far
SRT_HD void merge_serial(const Ctx &c, const Seg &s, HostAcc &a) {
    uint32_t i = s.b[0], j = s.b[1], pos = s.b[0] + s.b[1];
    uint64_t kt = 0, kr = 0;
    while (i < s.e[0] || j < s.e[1]) {
        uint64_t nt = kt, nr = kr;
        if (i < s.e[0]) {
            const uint64_t t = time_at(c, 0, i);
            nt = t > kt ? t : kt;
        }
        if (j < s.e[1]) {
            const uint64_t t = time_at(c, 1, j);
            nr = t > kr ? t : kr;
        }
        const bool take_rx = j < s.e[1] && (i >= s.e[0] || nr < nt || (nr == nt && c.rx_first));
        if (take_rx) kr = nr, place(c, pos++, 1, j++, a);
        else kt = nt, place(c, pos++, 0, i++, a);
    }
}

// a host that does not capture: its positions hold nothing
SRT_HD void merge_disabled(const Ctx &c, const Seg &s, uint32_t l, uint32_t L) {
    const uint32_t base = s.b[0] + s.b[1], n = (s.e[0] - s.b[0]) + (s.e[1] - s.b[1]);
    for (uint32_t i = l; i < n; i += L) c.size[base + i] = 0, c.ent[base + i] = NO_ENT;
}

// the host's sums, once a host
SRT_HD void host_finish(const Ctx &c, uint32_t h, const HostAcc &a, uint32_t bits) {
    c.host_bytes[h] = a.bytes;
    c.host_cnt[h] = a.cnt;
    c.pend[h] = a.maxt;
    const uint32_t f = a.flags | (bits ? F_TIME_ORDER : 0u);
    if (f) raise(&c.st->flags, f);
}

// the end of the scan: the call's total, OVERFLOW, the counts
SRT_HD bool scan_finish(const Ctx &c, uint64_t total, uint64_t n_recs) {
    c.host_off[c.n_hosts] = total;
    c.off[walked(c, 0) + walked(c, 1)] = total;
    const bool ok = total <= c.out_cap;
    c.st->write_total = ok ? total : 0;
    if (ok) c.st->n_recs += n_recs, c.st->n_bytes += total;
    else raise(&c.st->flags, F_OVERFLOW);
    return ok;
}

SRT_HD void commit_last(const Ctx &c, uint32_t h) {
    if (c.pend[h] > c.last[h]) c.last[h] = c.pend[h];
}

// ---- the write pass
SRT_HD uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// the record header and the packet's headers as the 32-bit words the stream holds (little-endian host)
SRT_HD void header_words(const srt_pcap_rec &r, uint32_t incl, uint32_t hs, uint32_t (&w)[HDR_WORDS]) {
    const uint32_t total = hs + r.payload_len;
    w[0] = (uint32_t)(r.time_ns / 1000000000ull);
    w[1] = (uint32_t)(r.time_ns % 1000000000ull) / 1000u;
    w[2] = incl;
    w[3] = total;
    // network/packet.rs:374-456: version and IHL, DSCP, total length; id; flags and fragment; TTL, protocol, checksum
    w[4] = bswap32(0x45000000u | total);
    w[5] = bswap32(0x00004000u);
    w[6] = bswap32(0x40000000u | (uint32_t)r.protocol << 16);
    w[7] = r.src_ip_be;
    w[8] = r.dst_ip_be;
    w[9] = (uint32_t)r.src_port_be | (uint32_t)r.dst_port_be << 16;
    if (r.protocol == 6) {  // :460-555
        const uint32_t doff = ((hs - 20) / 4) << 4;
        w[10] = bswap32(r.seq);
        w[11] = (r.tcp_flags & 0x10) ? bswap32(r.ack) : 0u;
        w[12] = bswap32(doff << 24 | (uint32_t)(r.tcp_flags & 0x17) << 16 | r.window);
        w[13] = 0;
        w[14] = bswap32(0x03030000u | (uint32_t)r.wscale << 8);
    } else {  // :558-586
        w[10] = bswap32(((uint32_t)r.payload_len + 8u) << 16);
        w[11] = w[12] = w[13] = w[14] = 0;
    }
}

// the tile's bytes of the stream are [lo, hi) of tile k; false: none
SRT_HD bool tile_span(const Ctx &c, uint64_t total, uint64_t k, int64_t &ts, uint64_t &lo, uint64_t &hi) {
    const uint64_t mis = (uint64_t)(uintptr_t)c.out & 15u;  // tiles are aligned in memory, not in the stream
    ts = (int64_t)(k * TILE) - (int64_t)mis;
    lo = ts < 0 ? 0 : (uint64_t)ts;
    hi = (uint64_t)(ts + TILE) < total ? (uint64_t)(ts + TILE) : total;
    return lo < hi;
}

SRT_HD uint64_t tile_count(const Ctx &c, uint64_t total) {
    return total ? (total + ((uint64_t)(uintptr_t)c.out & 15u) + TILE - 1) / TILE : 0;
}

// the merged positions [p0, p1) whose records overlap [lo, hi)
SRT_HD void tile_range(const Ctx &c, uint64_t lo, uint64_t hi, uint32_t &p0, uint32_t &p1) {
    const uint32_t n = walked(c, 0) + walked(c, 1);
    uint32_t a = 0, b = n + 1;  // the first position with off > lo
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (c.off[mid] <= lo) a = mid + 1;
        else b = mid;
    }
    p0 = a ? a - 1 : 0;
    a = p0, b = n;  // the first position with off >= hi
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (c.off[mid] < hi) a = mid + 1;
        else b = mid;
    }
    p1 = a;
}

// what the write pass needs of merged position pos, every field re-validated; false: nothing to write
struct alignas(16) Chunk {
    uint32_t w[4];
};

struct Item {
    const srt_pcap_rec *r;
    int64_t at;  // the record's first byte relative to the tile
    uint32_t incl, hs;
};

SRT_HD bool item_at(const Ctx &c, uint32_t pos, int64_t ts, Item &it) {
    const uint32_t e = c.ent[pos];
    if (e == NO_ENT) return false;
    const uint32_t side = e >> 31, k = e & ~RX_BIT;
    if (k >= walked(c, side)) return false;
    it.r = &rec_at(c, side, k);
    uint32_t f = 0;
    const uint32_t sz = rec_bytes(c, *it.r, f);
    if (!sz) return false;
    it.incl = sz - REC_HDR;
    it.hs = header_size(*it.r);
    it.at = (int64_t)c.off[pos] - ts;
    return true;
}

// the record header and the packet's headers of one record, clipped to the tile
SRT_HD void put_headers(const Item &it, uint8_t *tile) {
    uint32_t w[HDR_WORDS];
    header_words(*it.r, it.incl, it.hs, w);
    const uint32_t nb = REC_HDR + (it.incl < it.hs ? it.incl : it.hs);
    if (it.at >= 0 && it.at + 4 * (int64_t)HDR_WORDS <= (int64_t)TILE && !(it.at & 3)) {
        // whole words inside the tile: the last word may be cut by capture_len
        uint32_t *t4 = reinterpret_cast<uint32_t *>(tile + it.at);
#pragma unroll
        for (uint32_t j = 0; j < HDR_WORDS; ++j) {
            if (4 * j + 4 <= nb) {
                t4[j] = w[j];
            } else {
#pragma unroll
                for (uint32_t x = 0; x < 4; ++x)
                    if (4 * j + x < nb) tile[it.at + 4 * j + x] = (uint8_t)(w[j] >> (8 * x));
            }
        }
        return;
    }
#pragma unroll
    for (uint32_t i = 0; i < 4 * HDR_WORDS; ++i) {
        const int64_t q = it.at + i;
        if (i < nb && q >= 0 && q < (int64_t)TILE) tile[q] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
    }
}

// lane l of nl: the payload bytes of one record, clipped to the tile
SRT_HD void put_payload(const Ctx &c, const Item &it, uint8_t *tile, uint32_t l, uint32_t nl) {
    if (it.incl <= it.hs) return;
    const int64_t o = it.at + REC_HDR + it.hs, nb = it.incl - it.hs;  // nb <= payload_len
    const int64_t b0 = o < 0 ? -o : 0, b1 = nb < (int64_t)TILE - o ? nb : (int64_t)TILE - o;
    if (b0 >= b1) return;
    // tile bytes [d0, d1) are payload bytes [d0 - o, d1 - o): 16 bytes at a time where the tile is aligned
    // (the source has any alignment), single bytes before and behind
    const uint8_t *src = c.payload + it.r->payload_off;  // src[q - o] belongs at tile[q]
    const int64_t d0 = o + b0, d1 = o + b1, q0 = (d0 + 15) & ~(int64_t)15, q1 = d1 & ~(int64_t)15;
    if (q0 >= q1) {
        for (int64_t q = d0 + l; q < d1; q += nl) tile[q] = src[q - o];
        return;
    }
    for (int64_t q = q0 + 16 * (int64_t)l; q < q1; q += 16 * (int64_t)nl) {
        Chunk v;
        memcpy(&v, src + (q - o), 16);
        *reinterpret_cast<Chunk *>(tile + q) = v;
    }
    for (int64_t q = d0 + l; q < q0; q += nl) tile[q] = src[q - o];
    for (int64_t q = q1 + l; q < d1; q += nl) tile[q] = src[q - o];
}

// lane l of group g (ng groups of nl lanes): every ng-th record of the tile; the group's first lane writes
// the headers, all its lanes copy the payload
SRT_HD void tile_records(const Ctx &c, int64_t ts, uint8_t *tile, uint32_t p0, uint32_t p1, uint32_t g, uint32_t ng,
                         uint32_t l, uint32_t nl) {
    for (uint32_t pos = p0 + g; pos < p1; pos += ng) {
        Item it;
        if (!item_at(c, pos, ts, it)) continue;
        if (l == 0) put_headers(it, tile);
        put_payload(c, it, tile, l, nl);
    }
}

// ---- the host-only form: the same step, one lane
inline void host_run(const Ctx &c) {
    uint64_t total = 0, n_recs = 0;
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        const Seg s = segs(c, h);
        HostAcc a = {0, 0, 0, 0};
        uint32_t bits = 0;
        if (!c.enabled[h]) {
            merge_disabled(c, s, 0, 1);
        } else {
            bits = order_check(c, h, s, 0, 1);
            if (bits & DECREASES) merge_serial(c, s, a);
            else merge_sorted(c, s, 0, 1, a);
        }
        host_finish(c, h, a, bits);
    }
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        c.host_off[h] = total;
        total += c.host_bytes[h];
        n_recs += c.host_cnt[h];
    }
    if (scan_finish(c, total, n_recs))
        for (uint32_t h = 0; h < c.n_hosts; ++h) commit_last(c, h);
    for (uint32_t h = 0; h < c.n_hosts; ++h) {
        const Seg s = segs(c, h);
        const uint32_t base = s.b[0] + s.b[1], n = (s.e[0] - s.b[0]) + (s.e[1] - s.b[1]);
        uint64_t run = c.host_off[h];
        for (uint32_t i = 0; i < n; ++i) c.off[base + i] = run, run += c.size[base + i];
    }
    const uint64_t wt = c.st->write_total, tiles = tile_count(c, wt);
    alignas(16) uint8_t tile[TILE];
    for (uint64_t k = 0; k < tiles; ++k) {
        int64_t ts;
        uint64_t lo, hi;
        if (!tile_span(c, wt, k, ts, lo, hi)) continue;
        uint32_t p0, p1;
        tile_range(c, lo, hi, p0, p1);
        tile_records(c, ts, tile, p0, p1, 0, 1, 0, 1);
        memcpy(c.out + lo, tile + ((int64_t)lo - ts), hi - lo);
    }
}

}  // namespace pcap
#endif
