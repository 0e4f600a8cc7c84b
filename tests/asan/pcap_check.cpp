// pcap_check.cpp -- the pcap capture stage's step (shadow_amd/csrc/srt_pcap_step.h) in its host-only
// form, tile assembly included, on host arrays allocated at exactly the sizes include/srt.h promises.
// A stand-alone program: built for the host with -fsanitize=address,undefined and run directly
// (tests/test_pcap_cpu.py), so a write one past the scratch arrays, d_host_off or d_out, or a read one
// past the payload, is a sanitizer report.  The stream is also checked against a plain re-statement,
// one byte after the other: the hand-made flag cases, every capture length around the header sizes,
// the payload lengths at every alignment, the totals around the tile, and random calls.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <tuple>
#include <vector>

#include "../../shadow_amd/csrc/srt_pcap_step.h"

namespace {

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            std::printf("pcap_check: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

template <class T>
std::unique_ptr<T[]> arr(size_t n) {
    return std::unique_ptr<T[]>(new T[n]());  // exactly n: one past it is a report
}

uint64_t rnd(uint64_t &s) {  // xorshift64*
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return s * 2685821657736338717ull;
}

constexpr uint8_t POISON = 0xAB;

struct Pcap {
    pcap::State st{};
    uint32_t n_hosts;
    uint64_t rec_cap;
    std::unique_ptr<uint64_t[]> last, pend, host_bytes, off;
    std::unique_ptr<uint32_t[]> host_cnt, ent, size;
    std::unique_ptr<uint8_t[]> enabled;
    pcap::Ctx base{};

    Pcap(uint32_t nh, uint32_t capture_len, uint64_t cap, bool tx_first, const std::vector<uint8_t> &en = {})
        : n_hosts(nh), rec_cap(cap), last(arr<uint64_t>(nh)), pend(arr<uint64_t>(nh)), host_bytes(arr<uint64_t>(nh)),
          off(arr<uint64_t>(cap + 1)), host_cnt(arr<uint32_t>(nh)), ent(arr<uint32_t>(cap)), size(arr<uint32_t>(cap)),
          enabled(arr<uint8_t>(nh)) {
        for (uint32_t h = 0; h < nh; ++h) enabled[h] = en.empty() ? 1 : en[h];
        base.st = &st;
        base.last = last.get(), base.pend = pend.get(), base.host_bytes = host_bytes.get(), base.off = off.get();
        base.host_cnt = host_cnt.get(), base.ent = ent.get(), base.size = size.get(), base.enabled = enabled.get();
        base.n_hosts = nh, base.capture_len = capture_len, base.rx_first = tx_first ? 0 : 1;
    }

    uint32_t flags() {
        const uint32_t f = st.flags;
        st.flags = 0;
        return f;
    }
};

struct Call {
    std::vector<srt_pcap_rec> rec[2];
    std::vector<uint32_t> idx[2];  // empty: identity
    std::vector<uint32_t> ptr[2];
    std::vector<uint8_t> payload;
};

// the plain re-statement: one byte after the other
void put(std::vector<uint8_t> &o, uint64_t v, int n, bool big) {
    for (int i = 0; i < n; ++i) o.push_back((uint8_t)(v >> 8 * (big ? n - 1 - i : i)));
}

bool plain_record(const srt_pcap_rec &r, const Call &c, uint32_t capture_len, std::vector<uint8_t> &o, uint32_t &flags) {
    uint32_t hs;
    if (r.protocol == 17) hs = 28;
    else if (r.protocol == 6) hs = r.wscale_set ? 44 : 40;
    else return flags |= SRT_PCAP_BAD_PROTOCOL, false;
    if (hs + r.payload_len > 65535u) return flags |= SRT_PCAP_BAD_LENGTH, false;
    if (r.payload_off > c.payload.size() || r.payload_len > c.payload.size() - r.payload_off)
        return flags |= SRT_PCAP_BAD_PAYLOAD, false;
    std::vector<uint8_t> p;
    const uint32_t total = hs + r.payload_len;
    put(p, 0x4500, 2, true), put(p, total, 2, true), put(p, 0, 2, true), put(p, 0x4000, 2, true);
    put(p, 0x40, 1, true), put(p, r.protocol, 1, true), put(p, 0, 2, true);
    put(p, r.src_ip_be, 4, false), put(p, r.dst_ip_be, 4, false);
    put(p, r.src_port_be, 2, false), put(p, r.dst_port_be, 2, false);
    if (r.protocol == 6) {
        put(p, r.seq, 4, true), put(p, (r.tcp_flags & 0x10) ? r.ack : 0, 4, true);
        put(p, (hs - 20) / 4 << 4, 1, true), put(p, r.tcp_flags & 0x17, 1, true), put(p, r.window, 2, true);
        put(p, 0, 4, true);
        if (r.wscale_set) put(p, 3, 1, true), put(p, 3, 1, true), put(p, r.wscale, 1, true), put(p, 0, 1, true);
    } else {
        put(p, r.payload_len + 8u, 2, true), put(p, 0, 2, true);
    }
    CHECK(p.size() == hs);
    for (uint32_t i = 0; i < r.payload_len; ++i) p.push_back(c.payload[r.payload_off + i]);
    const uint32_t incl = std::min<uint32_t>(capture_len, total);
    put(o, r.time_ns / 1000000000ull, 4, false), put(o, r.time_ns % 1000000000ull / 1000, 4, false);
    put(o, incl, 4, false), put(o, total, 4, false);
    o.insert(o.end(), p.begin(), p.begin() + incl);
    return true;
}

struct Want {
    std::vector<uint64_t> host_off;
    std::vector<uint8_t> bytes;
    uint32_t flags = 0;
    uint64_t n_recs = 0;
};

Want plain(const Pcap &pc, const Call &c, std::vector<uint64_t> &last) {
    Want w;
    w.host_off.push_back(0);
    std::vector<uint64_t> new_last = last;
    for (uint32_t h = 0; h < pc.n_hosts; ++h) {
        std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint32_t>> e;  // key, priority, k, side
        for (uint32_t side = 0; pc.enabled[h] && side < 2; ++side) {
            uint64_t key = 0;
            for (uint32_t k = c.ptr[side][h]; k < c.ptr[side][h + 1]; ++k) {
                const uint64_t t = c.rec[side][c.idx[side].empty() ? k : c.idx[side][k]].time_ns;
                if (t < key || t < last[h]) w.flags |= SRT_PCAP_TIME_ORDER;
                key = std::max(key, t);
                e.emplace_back(key, pc.base.rx_first ? 1 - side : side, k, side);
            }
        }
        std::sort(e.begin(), e.end());
        for (auto &x : e) {
            const uint32_t side = std::get<3>(x), k = std::get<2>(x);
            const srt_pcap_rec &r = c.rec[side][c.idx[side].empty() ? k : c.idx[side][k]];
            if (plain_record(r, c, pc.base.capture_len, w.bytes, w.flags))
                ++w.n_recs, new_last[h] = std::max(new_last[h], r.time_ns);
        }
        w.host_off.push_back(w.bytes.size());
    }
    last = new_last;
    return w;
}

// the call on exact arrays, d_out at byte alignment `mis`; slack < 0: out_cap one short (OVERFLOW)
void run(Pcap &pc, const Call &c, std::vector<uint64_t> &last, int slack = 3, uint32_t mis = 0) {
    std::vector<uint64_t> last_before = last;
    const Want w = plain(pc, c, last);
    const uint64_t total = w.bytes.size();
    const bool over = slack < 0 && total > 0;
    const uint64_t out_cap = over ? total - 1 : total + (slack < 0 ? 0 : slack);
    if (over) last = last_before;
    // d_out at byte alignment `mis`: behind `mis` bytes of an array that ends where d_out ends (an array the
    // allocator did not align to 16 is replaced by a longer one); the bytes around d_out are checked by value
    const size_t raw_n = out_cap + mis;
    auto raw = arr<uint8_t>(raw_n);
    size_t extra = 0;
    if ((uintptr_t)raw.get() & 15) extra = 16, raw = arr<uint8_t>(raw_n + extra);
    const size_t lead = mis + (extra ? (16 - ((uintptr_t)raw.get() & 15)) & 15 : 0);
    uint8_t *out = raw.get() + lead;
    CHECK(((uintptr_t)out & 15) == mis);
    for (size_t i = 0; i < raw_n + extra; ++i) raw[i] = 0xCD;
    for (uint64_t i = 0; i < out_cap; ++i) out[i] = POISON;
    auto host_off = arr<uint64_t>(pc.n_hosts + 1);
    auto pay = arr<uint8_t>(c.payload.size());
    std::copy(c.payload.begin(), c.payload.end(), pay.get());
    std::unique_ptr<srt_pcap_rec[]> recs[2] = {arr<srt_pcap_rec>(c.rec[0].size()), arr<srt_pcap_rec>(c.rec[1].size())};
    std::unique_ptr<uint32_t[]> idx[2] = {arr<uint32_t>(c.idx[0].size()), arr<uint32_t>(c.idx[1].size())};
    std::unique_ptr<uint32_t[]> ptr[2] = {arr<uint32_t>(pc.n_hosts + 1), arr<uint32_t>(pc.n_hosts + 1)};
    pcap::Ctx x = pc.base;
    for (uint32_t s = 0; s < 2; ++s) {
        std::copy(c.rec[s].begin(), c.rec[s].end(), recs[s].get());
        std::copy(c.idx[s].begin(), c.idx[s].end(), idx[s].get());
        std::copy(c.ptr[s].begin(), c.ptr[s].end(), ptr[s].get());
        x.rec[s] = recs[s].get(), x.idx[s] = c.idx[s].empty() ? nullptr : idx[s].get(), x.ptr[s] = ptr[s].get();
        x.n[s] = c.ptr[s][pc.n_hosts];
    }
    CHECK((uint64_t)x.n[0] + x.n[1] <= pc.rec_cap);
    x.payload = c.payload.empty() ? nullptr : pay.get(), x.payload_bytes = c.payload.size();
    x.out = out, x.out_cap = out_cap, x.host_off = host_off.get();
    const uint64_t recs_before = pc.st.n_recs, bytes_before = pc.st.n_bytes;
    pcap::host_run(x);
    for (size_t i = 0; i < raw_n + extra; ++i) CHECK((i >= lead && i < lead + out_cap) || raw[i] == 0xCD);
    for (uint32_t h = 0; h <= pc.n_hosts; ++h) CHECK(host_off[h] == w.host_off[h]);
    CHECK(pc.flags() == (w.flags | (over ? SRT_PCAP_OVERFLOW : 0u)));
    if (over) {
        for (uint64_t i = 0; i < out_cap; ++i) CHECK(out[i] == POISON);
        CHECK(pc.st.n_recs == recs_before && pc.st.n_bytes == bytes_before);
        return;
    }
    for (uint64_t i = 0; i < total; ++i) CHECK(out[i] == w.bytes[i]);
    for (uint64_t i = total; i < out_cap; ++i) CHECK(out[i] == POISON);
    CHECK(pc.st.n_recs == recs_before + w.n_recs && pc.st.n_bytes == bytes_before + total);
}

srt_pcap_rec rec(uint64_t t, uint8_t proto, uint64_t off, uint16_t len, uint8_t ws = 0, uint8_t flags = 0x10) {
    srt_pcap_rec r{};
    r.time_ns = t, r.payload_off = off, r.payload_len = len, r.protocol = proto;
    r.src_ip_be = 0x0100000bu, r.dst_ip_be = 0x0200000bu, r.src_port_be = 0x1027, r.dst_port_be = 0x5000;
    r.seq = 0x01020304u + (uint32_t)t, r.ack = 0xdeadbeefu, r.window = 0x1234, r.tcp_flags = flags;
    r.wscale = 7, r.wscale_set = ws;
    return r;
}

std::vector<uint8_t> bytes(size_t n) {
    std::vector<uint8_t> p(n);
    for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)(i * 7 % 251);
    return p;
}

// one host, records of the given kinds alternately sent and received
Call one_host(const std::vector<srt_pcap_rec> &rs, size_t payload_bytes) {
    Call c;
    for (size_t i = 0; i < rs.size(); ++i) c.rec[i % 2].push_back(rs[i]);
    for (uint32_t s = 0; s < 2; ++s) c.ptr[s] = {0, (uint32_t)c.rec[s].size()};
    c.payload = bytes(payload_bytes);
    return c;
}

void capture_lengths() {
    for (uint32_t cl : {0u, 1u, 19u, 20u, 21u, 27u, 28u, 29u, 39u, 40u, 43u, 44u, 45u, 100u, 65535u})
        for (bool tx_first : {false, true}) {
            Pcap pc(1, cl, 12, tx_first);
            std::vector<uint64_t> last(1, 0);
            std::vector<srt_pcap_rec> rs;
            for (uint32_t i = 0; i < 12; ++i)
                rs.push_back(rec(1000 * (i / 2) + 999999999ull * (i % 3), i % 3 == 0 ? 17 : 6, i, (uint16_t)(i * 9), i % 3 == 2,
                                 (uint8_t)(i * 37)));
            std::sort(rs.begin(), rs.end(), [](const srt_pcap_rec &a, const srt_pcap_rec &b) { return a.time_ns < b.time_ns; });
            run(pc, one_host(rs, 200), last, 3, cl % 16);
        }
}

void payload_alignments() {
    const uint16_t lens[] = {0, 1, 3, 15, 16, 17, 1460};
    for (uint32_t cl : {65535u, 1487u}) {
        Pcap pc(1, cl, 7 * 16, false);
        std::vector<uint64_t> last(1, 0);
        std::vector<srt_pcap_rec> rs;
        for (uint32_t i = 0; i < 7; ++i)
            for (uint32_t res = 0; res < 16; ++res) rs.push_back(rec(100 * i + res, (i + res) % 2 ? 6 : 17, res, lens[i], res % 3 == 0));
        run(pc, one_host(rs, 1460 + 15), last, 0);  // the last payload ends at the payload's last byte
    }
}

void tile_edges() {
    const uint32_t T = pcap::TILE;
    for (uint32_t mis : {0u, 1u, 15u})
        for (uint64_t total : {(uint64_t)T - 1, (uint64_t)T, (uint64_t)T + 1, (uint64_t)2 * T + 1}) {
            // records of 1000 bytes and a remainder; one record alone; a 1,516-byte record across the boundary
            std::vector<std::vector<uint32_t>> shapes = {{}, {(uint32_t)total}, {T - 700 + mis, 1516, (uint32_t)total}};
            for (uint64_t left = total; left;) {
                const uint32_t s = left >= 1044 ? 1000 : (uint32_t)left;
                shapes[0].push_back(s), left -= s;
            }
            for (auto &sizes : shapes) {
                Pcap pc(1, 65535, sizes.size(), false);
                std::vector<uint64_t> last(1, 0);
                std::vector<srt_pcap_rec> rs;
                uint32_t most = 0;
                for (size_t i = 0; i < sizes.size(); ++i) {
                    rs.push_back(rec(10 * i, 17, i % 16, (uint16_t)(sizes[i] - 44)));
                    most = std::max(most, sizes[i]);
                }
                run(pc, one_host(rs, most - 44 + 15), last, 0, mis);
                std::vector<uint64_t> again(1, 0);
                Pcap short_pc(1, 65535, sizes.size(), false);
                run(short_pc, one_host(rs, most - 44 + 15), again, -1, mis);
            }
        }
}

void flags_by_hand() {
    // each skip, and that the others of the call are written
    for (int bad = 0; bad < 3; ++bad) {
        Pcap pc(2, 65535, 5, false);
        std::vector<uint64_t> last(2, 0);
        Call c;
        srt_pcap_rec b = bad == 0 ? rec(40, 1, 0, 0) : bad == 1 ? rec(40, 6, 0, 65496) : rec(40, 17, 7, 2);
        c.payload = bytes(bad == 1 ? 65496 : 8);
        c.rec[0] = {rec(10, 17, 0, 2), rec(30, 17, 6, 2), b}, c.ptr[0] = {0, 0, 3};
        c.rec[1] = {rec(20, 6, 0, 0), b}, c.ptr[1] = {0, 2, 2};
        run(pc, c, last);
        CHECK(pc.st.n_recs == 3 && last[0] == 20 && last[1] == 30);
    }
    {  // a list that decreases; then a call before the last time; an overflow does not advance the last time
        Pcap pc(2, 28, 8, false);
        std::vector<uint64_t> last(2, 0);
        Call c;
        c.rec[0] = {rec(10, 17, 0, 0), rec(50, 6, 0, 0), rec(20, 17, 0, 0), rec(60, 6, 0, 0)}, c.ptr[0] = {0, 0, 4};
        c.rec[1] = {rec(15, 17, 0, 0), rec(40, 6, 0, 0), rec(50, 17, 0, 0), rec(55, 6, 0, 0)}, c.ptr[1] = {0, 0, 4};
        run(pc, c, last, -1);
        CHECK(last[1] == 0);
        run(pc, c, last);
        CHECK(last[1] == 60);
        Call d;
        d.rec[0] = {rec(59, 17, 0, 0)}, d.ptr[0] = {0, 0, 1}, d.ptr[1] = {0, 0, 0};
        run(pc, d, last);  // plain() expects TIME_ORDER
    }
    {  // disabled hosts, only the last host on; no hosts; no records
        Pcap pc(3, 65535, 6, false, {0, 0, 1});
        std::vector<uint64_t> last(3, 0);
        Call c;
        c.payload = bytes(3);
        c.rec[0] = {rec(5, 99, 0, 0), rec(9, 17, 0, 0), rec(7, 17, 0, 3)}, c.ptr[0] = {0, 1, 2, 3};
        c.rec[1] = {rec(3, 17, 0, 0), rec(8, 6, 0, 0), rec(8, 17, 0, 0)}, c.ptr[1] = {0, 1, 1, 3};
        run(pc, c, last);
        CHECK(pc.st.n_recs == 3 && pc.st.n_bytes == 147);
        Call e;
        e.ptr[0] = e.ptr[1] = {0, 0, 0, 0};
        run(pc, e, last);
        Pcap none(0, 64, 0, false);
        std::vector<uint64_t> l0;
        Call z;
        z.ptr[0] = z.ptr[1] = {0};
        run(none, z, l0);
    }
}

// random calls over several hosts with the index indirection, three in a row
void random_calls(uint32_t n_hosts, uint32_t per_max, uint32_t capture_len, bool tx_first, uint64_t seed) {
    uint64_t s = seed;
    std::vector<uint8_t> en(n_hosts);
    for (auto &e : en) e = rnd(s) % 5 != 0;
    const uint32_t cap = 2 * n_hosts * per_max;
    Pcap pc(n_hosts, capture_len, cap, tx_first, en);
    std::vector<uint64_t> last(n_hosts, 0);
    for (uint32_t call = 0; call < 3; ++call) {
        Call c;
        c.payload = bytes(3000);
        for (uint32_t side = 0; side < 2; ++side) {
            c.ptr[side].push_back(0);
            for (uint32_t h = 0; h < n_hosts; ++h) {
                const uint32_t n = (uint32_t)(rnd(s) % (per_max + 1));
                std::vector<uint64_t> ts(n);
                for (auto &t : ts) t = 1000000ull * call + 1000 * (rnd(s) % 30);
                std::sort(ts.begin(), ts.end());
                for (uint64_t t : ts) {
                    const uint32_t kind = (uint32_t)(rnd(s) % 3);
                    c.rec[side].push_back(rec(t, kind ? 6 : 17, rnd(s) % 1500, (uint16_t)(rnd(s) % 1461), kind == 2,
                                              (uint8_t)rnd(s)));
                }
                c.ptr[side].push_back((uint32_t)c.rec[side].size());
            }
            if ((call + side) % 2) {  // reversed storage behind an index array
                std::reverse(c.rec[side].begin(), c.rec[side].end());
                for (uint32_t k = 0; k < c.rec[side].size(); ++k) c.idx[side].push_back((uint32_t)c.rec[side].size() - 1 - k);
            }
        }
        run(pc, c, last, (int)(rnd(s) % 40), (uint32_t)(rnd(s) % 16));
    }
}

}  // namespace

int main() {
    capture_lengths();
    payload_alignments();
    tile_edges();
    flags_by_hand();
    for (uint32_t n_hosts : {1u, 7u, 65u}) {
        random_calls(n_hosts, 12, 65535, false, 11 + n_hosts);
        random_calls(n_hosts, 3, 100, true, 5 + n_hosts);
    }
    random_calls(2, 150, 64, false, 3);
    std::printf("pcap_check: clean\n");
    return 0;
}
