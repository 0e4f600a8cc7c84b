// udprecv_check.cpp -- the UDP receive stage's step (shadow_amd/csrc/srt_udprecv_step.h) and its host-only
// entry points (host_config, host_note, host_run, and config_at as the device's launch walks it) on host
// arrays allocated at exactly the sizes include/srt.h promises.  A stand-alone program: built for the host
// with -fsanitize=address,undefined and run directly (tests/test_udprecv_cpu.py), so a write one past the
// slots, a ring, the staged records, the results, the late list or the note ring is a sanitizer report.
// Generated windows (hosts with 0 to 70 slots, rings of 0, 1, 3 and 64 messages, note rings that overrun,
// late lists of 0 and 1 records) and truncated or broken inputs (pointer arrays that run past the lists,
// that decrease, slots nobody owns).  The sockets are also checked against a plain re-statement: a slot's
// len_bytes is the sum of its ring's messages, its counts add up, a blocked read waits on an empty buffer,
// and a record's status is deliver's plus exactly one of buffered and dropped when the slot is open.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../shadow_amd/csrc/srt_udprecv_step.h"

namespace {

#define CHECK(x)                                                               \
    do {                                                                       \
        if (!(x)) {                                                            \
            std::printf("udprecv_check: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

template <class T>
std::unique_ptr<T[]> arr(size_t n) {
    return std::unique_ptr<T[]>(new T[n]());  // exactly n: one past it is a report
}

uint64_t rnd(uint64_t &s) {  // xorshift64*
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return s * 2685821657736338717ull;
}

constexpr uint32_t HIT = SRT_PDS_RELAY_FORWARDED | SRT_PDS_RCV_INTERFACE_RECEIVED;
constexpr uint64_t NONE = udprecv::NONE;
constexpr uint64_t LIMITS[4] = {10, 300, 3000, 1u << 20}, OPTVALS[4] = {0, 1024, 1ull << 30, ~0ull};
constexpr uint32_t READ_FLAGS[4] = {0, SRT_UDP_PEEK, SRT_UDP_TRUNC, SRT_UDP_WAIT};

// the instance of srt_udprecv.hip's host-only form, on exact arrays
struct Inst {
    udprecv::State st{};
    uint32_t n_hosts, n_sockets, ring_cap;
    uint64_t note_cap, note_end = 0, read_base = 0, prev_until = 0;
    std::unique_ptr<uint32_t[]> socket_ptr;
    std::unique_ptr<udprecv::Sock[]> socks;
    std::unique_ptr<udprecv::Msg[]> ring;
    std::unique_ptr<srt_udp_meta[]> note_ring;
    udprecv::Ctx base{};

    Inst(const std::vector<uint32_t> &counts, uint32_t ring_cap_, uint64_t note_cap_)
        : n_hosts((uint32_t)counts.size()), ring_cap(ring_cap_), note_cap(note_cap_), socket_ptr(arr<uint32_t>(counts.size() + 1)) {
        for (uint32_t h = 0; h < n_hosts; ++h) socket_ptr[h + 1] = socket_ptr[h] + counts[h];
        n_sockets = socket_ptr[n_hosts];
        socks = arr<udprecv::Sock>(n_sockets);
        ring = arr<udprecv::Msg>((size_t)n_sockets * ring_cap);
        note_ring = arr<srt_udp_meta>(note_cap);
        for (uint32_t h = 0; h < n_hosts; ++h)
            for (uint32_t x = socket_ptr[h]; x < socket_ptr[h + 1]; ++x) {
                udprecv::sock_reset(socks[x], 0, 0);
                socks[x].host = h;
            }
        base.st = &st;
        base.socks = socks.get(), base.ring = ring.get(), base.note_ring = note_ring.get();
        base.n_hosts = n_hosts, base.n_sockets = n_sockets, base.ring_cap = ring_cap, base.note_cap = note_cap;
    }

    // as srt_udprecv_config: in list order, or sorted stably by slot and walked a step a thread
    void config(const std::vector<srt_udprecv_op> &ops, bool sorted) {
        udprecv::Ctx c = base;
        if (!sorted) {
            c.ops = ops.data(), c.n_ops = (uint32_t)ops.size();
            udprecv::host_config(c);
            return;
        }
        std::vector<srt_udprecv_op> s(ops);
        std::stable_sort(s.begin(), s.end(), [](const srt_udprecv_op &a, const srt_udprecv_op &b) { return a.slot < b.slot; });
        auto exact = arr<srt_udprecv_op>(s.size());
        std::copy(s.begin(), s.end(), exact.get());
        c.ops = exact.get(), c.n_ops = (uint32_t)s.size();
        for (uint32_t i = c.n_ops; i-- > 0;) udprecv::config_at(c, i);  // any order of the threads
    }

    void note(const srt_udp_meta *meta, uint32_t n, uint64_t tag_base) {
        CHECK(tag_base >= note_end);
        note_end = tag_base + n;
        if (!n || !note_cap) return;
        udprecv::Ctx c = base;
        c.note_in = meta, c.note_n = n;
        c.note_first = n > note_cap ? (uint32_t)(n - note_cap) : 0u;
        c.note_first_mod = (tag_base + c.note_first) % note_cap;
        udprecv::host_note(c);
    }

    uint64_t run(const uint32_t *hp, const uint32_t *sock, const uint64_t *fwd, const uint64_t *tag, const uint32_t *status,
                 uint32_t out_cap, const uint32_t *rp, const srt_udp_read *reads, uint32_t n_reads, uint64_t until,
                 uint32_t *rx, srt_udp_result *results, srt_udp_late *late, uint32_t late_cap, uint32_t *late_count,
                 uint64_t *first) {
        auto rec = arr<udprecv::Rec>(out_cap);
        udprecv::Ctx c = base;
        c.rec = rec.get();
        c.note_end = note_end, c.note_end_mod = note_cap ? note_end % note_cap : 0;
        c.out_host_ptr = hp, c.out_socket = sock, c.out_forward = fwd, c.out_tag = tag, c.out_status = status;
        c.out_cap = out_cap;
        c.read_host_ptr = n_reads ? rp : nullptr, c.reads = reads, c.n_reads = n_reads;
        c.read_seq_base = read_base, c.prev_until = prev_until, c.until = until;
        c.rx_status = rx, c.results = results, c.late = late, c.late_cap = late_cap, c.late_count = late_count;
        c.first_readable = first;
        udprecv::host_run(c);
        const uint64_t b = read_base;
        read_base += n_reads, prev_until = until;
        return b;
    }

    uint32_t flags() {
        const uint32_t f = st.flags;
        st.flags = 0;
        return f;
    }
};

// windows of random deliveries and reads; `broken`: pointer arrays that lie, slots nobody owns
void windows(uint32_t n_hosts, uint32_t ring_cap, uint64_t note_cap_or_0, uint32_t late_cap, bool broken, uint64_t seed) {
    constexpr uint32_t WINS = 5;
    constexpr uint64_t W = 1000000, GRID = 5000;
    uint64_t s = seed;
    std::vector<uint32_t> counts(n_hosts);
    for (uint32_t h = 0; h < n_hosts; ++h) counts[h] = h == 0 ? 70 : h == 1 ? 0 : (uint32_t)(rnd(s) % 9);
    const uint32_t per_max = 60;
    const uint64_t note_cap = note_cap_or_0 ? note_cap_or_0 : (uint64_t)n_hosts * per_max * WINS + 1;
    Inst in(counts, ring_cap, note_cap);
    const uint32_t ns = in.n_sockets;
    std::vector<srt_udprecv_op> ops;
    for (uint32_t x = 0; x < ns; ++x) {
        if (rnd(s) % 7 == 0) continue;  // foreign
        ops.push_back({SRT_UDPRECV_OPEN, x, LIMITS[rnd(s) % 4]});
        if (rnd(s) % 3 == 0) ops.push_back({SRT_UDPRECV_SET_PEER, x, 7ull | 9ull << 32});
        if (rnd(s) % 5 == 0) ops.push_back({SRT_UDPRECV_SET_RCVBUF, x, OPTVALS[rnd(s) % 4]});
    }
    in.config(ops, seed & 1);
    uint64_t tag_base = 0;
    for (uint32_t w = 0; w < WINS; ++w) {
        if (w == 2) {  // some sockets close and come back
            ops.clear();
            for (uint32_t x = 0; x < ns; x += 5) ops.push_back({SRT_UDPRECV_CLOSE, x, 0}), ops.push_back({SRT_UDPRECV_OPEN, x, 3000});
            in.config(ops, !(seed & 1));
        }
        auto hp = arr<uint32_t>(n_hosts + 1), rp = arr<uint32_t>(n_hosts + 1);
        for (uint32_t h = 0; h < n_hosts; ++h) {
            hp[h + 1] = hp[h] + (w + 1 < WINS ? (uint32_t)(rnd(s) % (per_max + 1)) : 0u);
            rp[h + 1] = rp[h] + (uint32_t)(rnd(s) % (per_max + 1));
        }
        const uint32_t n = hp[n_hosts], nr = rp[n_hosts];
        // broken: the lists are shorter than their pointer arrays say, and the arrays decrease somewhere
        const uint32_t out_cap = broken ? n / 2 : n, n_reads = broken ? nr / 2 : nr;
        if (broken && n_hosts > 3) std::swap(hp[1], hp[3]), std::swap(rp[1], rp[2]);
        auto meta = arr<srt_udp_meta>(n);
        auto sock = arr<uint32_t>(out_cap), status = arr<uint32_t>(out_cap), rx = arr<uint32_t>(out_cap);
        auto fwd = arr<uint64_t>(out_cap), tag = arr<uint64_t>(out_cap), first = arr<uint64_t>(ns);
        auto reads = arr<srt_udp_read>(n_reads);
        auto results = arr<srt_udp_result>(n_reads);
        auto late = arr<srt_udp_late>(late_cap);
        for (uint32_t i = 0; i < n; ++i) {
            meta[i].src_ip_be = rnd(s) % 4 ? 7 : 8, meta[i].src_port_be = 9;
            meta[i].payload_size = rnd(s) % 10 ? (uint32_t)(rnd(s) % 1400) : 0u, meta[i].user = i;
        }
        in.note(meta.get(), n, tag_base);
        for (uint32_t h = 0, k = 0, j = 0; h < n_hosts; ++h) {
            const uint32_t lo = in.socket_ptr[h], cnt = counts[h];
            uint64_t at = w * W, rt = w * W;
            for (; k < hp[h + 1] && !broken; ++k) {
                at += rnd(s) % 4 * GRID;
                fwd[k] = at < (w + 1) * W ? at : (w + 1) * W - 1, tag[k] = tag_base + k;
                const uint32_t r = (uint32_t)(rnd(s) % 20);
                sock[k] = !cnt || r == 0 ? 0xffffffffu : lo + (uint32_t)(rnd(s) % cnt);
                status[k] = r == 1 ? SRT_PDS_RELAY_FORWARDED : sock[k] == 0xffffffffu ? HIT | SRT_PDS_RCV_INTERFACE_DROPPED : HIT;
            }
            for (; j < rp[h + 1] && !broken; ++j) {
                rt += rnd(s) % 4 * GRID;
                reads[j].time_ns = rt < (w + 1) * W ? rt : (w + 1) * W - 1;
                reads[j].slot = cnt ? lo + (uint32_t)(rnd(s) % cnt) : 0;
                reads[j].len = rnd(s) % 2 ? 2000 : 16;
                reads[j].flags = READ_FLAGS[rnd(s) % 4];
                reads[j].user = j;
            }
        }
        for (uint32_t k = 0; broken && k < out_cap; ++k) {
            fwd[k] = w * W + rnd(s) % W, tag[k] = rnd(s) % 3 ? tag_base + k : rnd(s);
            sock[k] = rnd(s) % 4 ? (uint32_t)(rnd(s) % (ns + 3)) : (uint32_t)rnd(s), status[k] = rnd(s) % 8 ? HIT : (uint32_t)rnd(s);
        }
        for (uint32_t j = 0; broken && j < n_reads; ++j) {
            reads[j].time_ns = rnd(s) % 8 ? w * W + rnd(s) % W : rnd(s), reads[j].slot = rnd(s) % 4 ? (uint32_t)(rnd(s) % (ns + 3)) : (uint32_t)rnd(s);
            reads[j].len = (uint32_t)rnd(s), reads[j].flags = (uint32_t)rnd(s) & (SRT_UDP_PEEK | SRT_UDP_TRUNC | SRT_UDP_WAIT);
        }
        uint32_t late_count = 77;
        in.run(hp.get(), sock.get(), fwd.get(), tag.get(), status.get(), out_cap, rp.get(), reads.get(), n_reads, (w + 1) * W,
               rx.get(), results.get(), late.get(), late_cap, &late_count, first.get());
        tag_base += n;
        const uint32_t f = in.flags();
        if (broken || note_cap_or_0) continue;  // the arrays' bounds were the point
        CHECK(!(f & ~(udprecv::F_RING_OVERFLOW | udprecv::F_LATE_OVERFLOW | udprecv::F_BAD_SOCKET | udprecv::F_ARMED_TWICE)));
        CHECK(late_count <= late_cap || (f & udprecv::F_LATE_OVERFLOW));
        for (uint32_t k = 0; k < n; ++k) {
            const bool ours = (status[k] & SRT_PDS_RCV_INTERFACE_RECEIVED) && sock[k] < ns && in.socks[sock[k]].open;
            CHECK((rx[k] & ~(udprecv::PROCESSED | udprecv::DROPPED | udprecv::BUFFERED)) == status[k]);
            CHECK(ours ? (rx[k] & udprecv::PROCESSED) && !(rx[k] & udprecv::DROPPED) != !(rx[k] & udprecv::BUFFERED) : rx[k] == status[k]);
        }
        for (uint32_t j = 0; j < n_reads; ++j) {
            const srt_udp_result &r = results[j];
            CHECK(r.read_user == j || r.status == SRT_UDP_NOT_TAKEN);
            CHECK(r.status != SRT_UDP_DONE || r.return_val >= 0 || r.return_val == udprecv::E_WOULDBLOCK || r.return_val == udprecv::E_BADF);
        }
        // a late record is a read of an earlier call, done
        for (uint32_t k = 0; k < std::min(late_count, late_cap); ++k) CHECK(late[k].seq < in.read_base - n_reads && late[k].result.status == SRT_UDP_DONE);
    }
    if (broken || note_cap_or_0) return;
    // what the slots hold adds up
    for (uint32_t x = 0; x < ns; ++x) {
        const udprecv::Sock &k = in.socks[x];
        CHECK(k.n_proc == k.n_buf + k.n_drop && k.n_msgs <= ring_cap && k.ring_head < std::max(ring_cap, 1u));
        if (!k.open || k.overflow) continue;
        uint64_t bytes = 0;
        for (uint32_t i = 0; i < k.n_msgs; ++i) bytes += in.ring[(size_t)x * ring_cap + (k.ring_head + i) % ring_cap].size;
        CHECK(bytes == k.len_bytes);
        CHECK(k.armed_seq == NONE || k.n_msgs == 0);
    }
}

// the rules at their edges, by hand
void by_hand() {
    Inst in({2}, 2, 4);
    in.config({{SRT_UDPRECV_OPEN, 0, 10}, {SRT_UDPRECV_OPEN, 1, 10}, {SRT_UDPRECV_SET_RCVBUF, 1, 0}}, true);
    CHECK(in.socks[1].soft_limit == 2048 && udprecv::rcvbuf_limit(1024) == 2048 && udprecv::rcvbuf_limit(1ull << 30) == 1ull << 28 &&
          udprecv::rcvbuf_limit(~0ull) == 1ull << 28 && udprecv::rcvbuf_limit(5000) == 10000);
    srt_udp_meta ms[3] = {{1, 1, 0, 9, 100}, {1, 1, 0, 5, 101}, {1, 1, 0, 1, 102}};
    in.note(ms, 3, 0);
    const uint32_t hp[2] = {0, 3}, sock[3] = {0, 0, 0}, status[3] = {HIT, HIT, HIT}, rp[2] = {0, 2};
    const uint64_t fwd[3] = {10, 20, 30}, tag[3] = {0, 1, 2};
    const srt_udp_read reads[2] = {{5, 1, 8, SRT_UDP_WAIT, 0}, {25, 0, 4, SRT_UDP_TRUNC, 1}};
    uint32_t rx[3], late_count = 5;
    srt_udp_result res[2];
    uint64_t first[2];
    in.run(hp, sock, fwd, tag, status, 3, rp, reads, 2, 100, rx, res, nullptr, 0, &late_count, first);
    CHECK(rx[0] == (HIT | udprecv::PROCESSED | udprecv::BUFFERED) && rx[1] == rx[0] && rx[2] == rx[0]);  // 9, then 14 bytes, the read takes 9, 5 < 10
    CHECK(res[0].status == SRT_UDP_ARMED && res[1].return_val == 9 && res[1].msg_flags == SRT_UDP_MSG_TRUNC && res[1].user == 100);
    CHECK(first[0] == 10 && first[1] == NONE && late_count == 0 && in.socks[0].len_bytes == 6 && in.socks[0].n_msgs == 2);
    CHECK(in.socks[1].armed_seq == 0 && in.flags() == 0);
    // the armed read returns in the next call, to a late list that has no room
    const uint32_t hp2[2] = {0, 1}, sock2[1] = {1};
    const uint64_t fwd2[1] = {150}, tag2[1] = {2};
    in.run(hp2, sock2, fwd2, tag2, status, 1, nullptr, nullptr, 0, 200, rx, nullptr, nullptr, 0, &late_count, first);
    CHECK(late_count == 1 && in.flags() == udprecv::F_LATE_OVERFLOW && in.socks[1].armed_seq == NONE && in.socks[1].n_msgs == 0);
    CHECK(first[1] == 150 && in.socks[1].last_read_recv_ns == 150);
    // no hosts, no slots
    Inst none({}, 0, 0);
    const uint32_t hp0[1] = {0};
    none.run(hp0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, 5, nullptr, nullptr, nullptr, 0, &late_count, nullptr);
    CHECK(none.flags() == 0 && late_count == 0);
}

}  // namespace

int main() {
    by_hand();
    for (uint32_t n_hosts : {1u, 7u, 65u}) windows(n_hosts, 64, 0, 4096, false, 11 + n_hosts);
    for (uint32_t ring_cap : {0u, 1u, 3u}) windows(9, ring_cap, 0, 4096, false, 4 + ring_cap);
    for (uint32_t late_cap : {0u, 1u}) windows(9, 64, 0, late_cap, false, 8 + late_cap);
    for (uint64_t note_cap : {1ull, 63ull, 64ull, 65ull}) windows(9, 3, note_cap, 1, false, 3 + note_cap);
    for (uint64_t seed : {1ull, 2ull, 3ull, 4ull}) windows(12, seed % 2 ? 2 : 0, seed > 2 ? 5 : 0, (uint32_t)seed % 3, true, seed);
    std::printf("udprecv_check: clean\n");
    return 0;
}
