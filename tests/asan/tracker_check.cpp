// tracker_check.cpp -- the tracker stage's step (shadow_amd/csrc/srt_tracker_step.h) in its host-only
// form, fed by the outbound relay's step (srt_outbound_step.h) and its cached-seq accessor, on host
// arrays allocated at exactly the sizes include/srt.h promises.  A stand-alone program: built for the
// host with -fsanitize=address,undefined and run directly (tests/test_tracker_cpu.py), so a write one
// past a record array, the ring, the log or a count is a sanitizer report.  The counters are also
// checked against a plain re-statement: every packet the interface popped -- seen with
// SND_INTERFACE_SENT in its batch, in a late list, or as a host's cached packet -- is counted exactly
// once, in its class.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include "../../shadow_amd/csrc/srt_outbound_step.h"
#include "../../shadow_amd/csrc/srt_tracker_step.h"

namespace {

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            std::printf("tracker_check: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

template <class T>
std::unique_ptr<T[]> arr(size_t n) {
    return std::unique_ptr<T[]>(new T[n]());  // exactly n: one past it is a report
}

uint64_t rnd(uint64_t &s) {  // xorshift64*
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return s * 2685821657736338717ull;
}

constexpr uint32_t SENT = SRT_PDS_SND_INTERFACE_SENT;
constexpr uint32_t HIT = SRT_PDS_RELAY_FORWARDED | SRT_PDS_RCV_INTERFACE_RECEIVED;
constexpr uint64_t NONE = tracker::NONE;

struct Trk {
    tracker::State st{};
    uint32_t n_hosts, n_sockets;
    uint64_t note_cap, log_cap, note_end = 0;
    std::unique_ptr<srt_trk_counters[]> node_in, node_out, sock_in, sock_out;
    std::unique_ptr<uint64_t[]> cnt_tx, cnt_rx, remembered;
    std::unique_ptr<srt_trk_meta[]> ring, log;
    tracker::Ctx base{};

    Trk(uint32_t nh, uint32_t ns, uint64_t note_cap_, uint64_t log_cap_)
        : n_hosts(nh), n_sockets(ns), note_cap(note_cap_), log_cap(log_cap_), node_in(arr<srt_trk_counters>(nh)),
          node_out(arr<srt_trk_counters>(nh)), sock_in(arr<srt_trk_counters>(ns)), sock_out(arr<srt_trk_counters>(ns)),
          cnt_tx(arr<uint64_t>(nh)), cnt_rx(arr<uint64_t>(nh)), remembered(arr<uint64_t>(nh)),
          ring(arr<srt_trk_meta>(note_cap_)), log(arr<srt_trk_meta>(log_cap_)) {
        base.st = &st;
        base.node_in = node_in.get(), base.node_out = node_out.get();
        base.sock_in = sock_in.get(), base.sock_out = sock_out.get();
        base.cnt_tx = cnt_tx.get(), base.cnt_rx = cnt_rx.get(), base.remembered = remembered.get();
        base.ring = ring.get(), base.log = log.get();
        base.n_hosts = nh, base.n_sockets = ns, base.note_cap = note_cap, base.log_cap = log_cap;
        for (uint32_t h = 0; h < nh; ++h) remembered[h] = NONE;
    }

    void tx(const uint64_t *cached, const uint32_t *host_ptr, uint32_t n, const srt_trk_meta *meta, const uint32_t *status,
            uint64_t seq_base, const srt_outbound_late *late, uint32_t late_cap, const uint32_t *late_count) {
        tracker::Ctx c = base;
        c.base_mod = log_cap ? seq_base % log_cap : 0;
        c.end_mod = log_cap ? (seq_base + n) % log_cap : 0;
        c.cached_seq = cached, c.host_ptr = host_ptr, c.status = status, c.meta = meta;
        c.late = late, c.late_count = late_cap ? late_count : nullptr, c.late_cap = late_cap;
        c.seq_base = seq_base, c.n_pkts = n;
        tracker::host_tx(c);
    }

    void note(const srt_trk_meta *meta, uint32_t n, uint64_t tag_base) {
        CHECK(tag_base >= note_end);
        note_end = tag_base + n;
        if (!n || !note_cap) return;
        tracker::Ctx c = base;
        c.note_in = meta, c.note_n = n;
        c.note_first = n > note_cap ? (uint32_t)(n - note_cap) : 0u;
        c.note_first_mod = (tag_base + c.note_first) % note_cap;
        tracker::host_note(c);
    }

    void rx(const uint32_t *hp, const uint32_t *sock, const uint64_t *tag, const uint32_t *status, uint64_t out_cap) {
        tracker::Ctx c = base;
        c.note_end = note_end, c.note_end_mod = note_cap ? note_end % note_cap : 0;
        c.out_host_ptr = hp, c.out_socket = sock, c.out_tag = tag, c.out_status = status, c.out_cap = out_cap;
        tracker::host_rx(c);
    }

    void flat(const uint32_t *host, const uint32_t *sock, const srt_trk_meta *meta, uint32_t n) {
        tracker::Ctx c = base;
        c.f_host = host, c.f_socket = sock, c.f_meta = meta, c.f_n = n;
        tracker::host_rx_flat(c);
    }

    uint32_t flags() {
        const uint32_t f = st.flags;
        st.flags = 0;
        return f;
    }
};

uint64_t word(const srt_trk_counters &r, uint32_t j) { return reinterpret_cast<const uint64_t *>(&r)[j]; }

// the relay of srt_outbound.hip's host-only instance, on exact arrays
struct Relay {
    uint32_t n, cap, max_sockets;
    std::unique_ptr<outb::Host[]> hosts;
    std::unique_ptr<outb::RingEl[]> ring;
    std::unique_ptr<outb::Cur[]> cur;
    std::unique_ptr<uint32_t[]> sockq;
    alignas(8) uint32_t flags[4] = {0, 0, 0, 0};
    uint64_t base = 0, prev_until = 0;

    Relay(uint32_t n_, uint32_t cap_, uint32_t max_sockets_, const uint64_t *bw)
        : n(n_), cap(cap_), max_sockets(max_sockets_), hosts(arr<outb::Host>(n_)),
          ring(arr<outb::RingEl>((size_t)n_ * cap_)), cur(arr<outb::Cur>((size_t)n_ * max_sockets_)),
          sockq(arr<uint32_t>((size_t)n_ * max_sockets_)) {
        for (uint32_t h = 0; h < n; ++h) {
            hosts[h].refill = relay::bucket_refill(bw[h]);
            hosts[h].capacity = relay::sat_add(hosts[h].refill, relay::MTU);
            hosts[h].balance = hosts[h].capacity;
            hosts[h].task_ns = outb::NONE;
        }
        for (size_t i = 0; i < (size_t)n * max_sockets; ++i) cur[i] = outb::Cur{outb::NIL, outb::NIL};
    }

    uint64_t run(const srt_out_pkt *pkts, const uint32_t *host_ptr, uint32_t n_pkts, uint64_t until, uint32_t *status,
                 uint64_t *send_ns, uint64_t *send_rank, srt_outbound_late *late, uint32_t late_cap, uint32_t *late_count) {
        auto link = arr<uint32_t>(n_pkts);
        outb::Ctx c{};
        c.hosts = hosts.get(), c.ring = ring.get(), c.cur = cur.get(), c.sockq = sockq.get();
        c.pkts = pkts, c.link = link.get(), c.host_ptr = host_ptr;
        c.status = status, c.send_ns = send_ns, c.send_rank = send_rank;
        c.late = late, c.late_count = late_count, c.flags = flags;
        c.pending = reinterpret_cast<unsigned long long *>(flags + 2);
        c.base = base, c.until = until, c.boot_end = 0, c.prev_until = prev_until;
        c.n_hosts = n, c.ring_cap = cap, c.late_cap = late_cap, c.n_pkts = n_pkts;
        c.max_sockets = max_sockets, c.qdisc = SRT_QDISC_FIFO;
        *late_count = 0, *c.pending = 0;
        for (uint32_t i = 0; i < n_pkts; ++i) status[i] = 0, send_ns[i] = outb::NONE, send_rank[i] = outb::NONE;
        for (uint32_t h = 0; h < n; ++h) {
            outb::Run<false> r(c, h);
            r.run();
        }
        const uint64_t b = base;
        base += n_pkts, prev_until = until;
        return b;
    }

    // srt_outbound_cached_seq, host-only
    void cached_seq(uint64_t *seq) const {
        for (uint32_t h = 0; h < n; ++h) seq[h] = outb::cached_seq_of(hosts[h]);
    }
};

// windows of random packets through the relay and the tracker; afterwards every popped packet has
// been counted once
void relay_to_tracker(uint32_t n_hosts, uint32_t per_max, uint64_t log_cap_or_0, uint64_t seed) {
    constexpr uint32_t SOCKS = 3, WINS = 7;
    constexpr uint64_t MS = 1000000, W = 20 * MS;
    uint64_t s = seed;
    auto bw = arr<uint64_t>(n_hosts);
    for (uint32_t h = 0; h < n_hosts; ++h) bw[h] = (h % 3 == 0) ? 30000 : (h % 3 == 1) ? 2000000 : 1250000000;
    const uint32_t total_cap = n_hosts * per_max * WINS + 1;
    Relay rl(n_hosts, per_max * WINS + 1, SOCKS, bw.get());
    const uint64_t log_cap = log_cap_or_0 ? log_cap_or_0 : total_cap;
    Trk t(n_hosts, n_hosts * SOCKS, 0, log_cap);
    std::map<uint64_t, srt_trk_meta> metas;  // seq -> meta, every packet fed
    std::map<uint64_t, uint32_t> host_of;
    std::set<uint64_t> popped;
    std::vector<uint64_t> prio(n_hosts, 0);
    uint32_t rule2 = 0, rule2_known = 0, rule3 = 0;
    std::vector<uint64_t> remembered(n_hosts, NONE);
    for (uint32_t w = 0; w < WINS; ++w) {
        auto hp = arr<uint32_t>(n_hosts + 1);
        for (uint32_t h = 0; h < n_hosts; ++h)
            hp[h + 1] = hp[h] + (w + 1 < WINS ? (uint32_t)(rnd(s) % (per_max + 1)) : 0u);
        const uint32_t n = hp[n_hosts];
        auto pk = arr<srt_out_pkt>(n);
        auto meta = arr<srt_trk_meta>(n);
        for (uint32_t h = 0; h < n_hosts; ++h) {
            uint64_t at = w * W;
            for (uint32_t i = hp[h]; i < hp[h + 1]; ++i) {
                at += rnd(s) % (W / (per_max + 1));
                srt_trk_meta m{};
                m.header_size = 20 + (uint32_t)(rnd(s) % 3) * 12;
                m.payload_size = rnd(s) % 5 < 2 ? 0u : 1u + (uint32_t)(rnd(s) % 1400);
                m.flags = rnd(s) % 4 == 0 ? SRT_TRK_RETRANS : 0u;
                m.socket_slot = h * SOCKS + (uint32_t)(rnd(s) % SOCKS);
                meta[i] = m;
                pk[i].ready_ns = at, pk[i].priority = ++prio[h], pk[i].total_size = m.header_size + m.payload_size;
                pk[i].socket = m.socket_slot - h * SOCKS, pk[i].flags = rnd(s) % 20 == 0 ? SRT_OUT_LOCAL : 0u;
            }
        }
        auto status = arr<uint32_t>(n);
        auto send_ns = arr<uint64_t>(n), send_rank = arr<uint64_t>(n), cached = arr<uint64_t>(n_hosts);
        auto late = arr<srt_outbound_late>(total_cap);
        uint32_t late_count = 0;
        const uint64_t until = w + 1 < WINS ? (w + 1) * W : 400 * W;
        const uint64_t base = rl.run(pk.get(), hp.get(), n, until, status.get(), send_ns.get(), send_rank.get(),
                                     late.get(), total_cap, &late_count);
        CHECK(!(rl.flags[0] & ~outb::F_OVERSIZE));
        rl.cached_seq(cached.get());
        for (uint32_t h = 0; h < n_hosts; ++h)
            for (uint32_t i = hp[h]; i < hp[h + 1]; ++i) {
                metas[base + i] = meta[i], host_of[base + i] = h;
                if (status[i] & SENT) CHECK(popped.insert(base + i).second);
            }
        for (uint32_t k = 0; k < late_count; ++k) {
            const bool known = remembered[late[k].src_host] == late[k].seq;
            CHECK(popped.insert(late[k].seq).second != known);
            known ? ++rule2_known : ++rule2;
        }
        for (uint32_t h = 0; h < n_hosts; ++h) {
            if (cached[h] != NONE && cached[h] < base && cached[h] != remembered[h]) {
                CHECK(popped.insert(cached[h]).second);
                ++rule3;
            }
            remembered[h] = cached[h];
        }
        t.tx(cached.get(), hp.get(), n, meta.get(), status.get(), base, late.get(), total_cap, &late_count);
    }
    const uint32_t f = t.flags();
    CHECK(log_cap_or_0 ? !(f & ~tracker::F_LOG_OVERRUN) : f == 0);
    if (log_cap_or_0) return;  // the arrays' bounds were the point
    CHECK(rule2 && rule2_known && rule3 && !popped.empty());
    std::vector<srt_trk_counters> want(n_hosts), want_s(n_hosts * SOCKS);
    for (uint64_t seq : popped) {
        const srt_trk_meta &m = metas.at(seq);
        tracker::Acc a;
        tracker::acc_zero(a);
        tracker::acc_add(a, m);
        tracker::rec_merge(&want[host_of.at(seq)], a);
        tracker::rec_merge(&want_s[m.socket_slot], a);
    }
    uint64_t n_tx = 0;
    for (uint32_t h = 0; h < n_hosts; ++h) {
        n_tx += t.cnt_tx[h];
        for (uint32_t j = 0; j < tracker::N_CTR; ++j) CHECK(word(t.node_out[h], j) == word(want[h], j));
    }
    CHECK(n_tx == popped.size());
    for (uint32_t x = 0; x < n_hosts * SOCKS; ++x)
        for (uint32_t j = 0; j < tracker::N_CTR; ++j) CHECK(word(t.sock_out[x], j) == word(want_s[x], j));
}

// the input side at the note ring's edges, the flat form, the flags
void input_side() {
    Trk t(3, 2, 4, 0);
    srt_trk_meta ms[6] = {{20, 0, 0, 0}, {20, 5, 0, 0}, {32, 0, 1, 0}, {32, 6, 1, 0}, {40, 7, 0, 0}, {40, 8, 0, 0}};
    t.note(ms, 6, 10);  // more than the ring holds: tags 12..15 stay
    const uint32_t hp[4] = {0, 2, 2, 7}, sock[5] = {0, 1, 2, 0xffffffffu, 1};
    const uint64_t tag[5] = {12, 13, 14, 15, 11};
    const uint32_t status[5] = {HIT, HIT, HIT, HIT | SRT_PDS_RCV_INTERFACE_DROPPED, HIT};
    t.rx(hp, sock, tag, status, 5);  // hp[3] past out_cap: the walk ends at 5
    CHECK(t.flags() == (tracker::F_BAD_SOCKET | tracker::F_NOTE_OVERRUN));
    CHECK(t.cnt_rx[0] == 2 && t.cnt_rx[1] == 0 && t.cnt_rx[2] == 1);
    CHECK(t.node_in[0].packets_control_retrans == 1 && t.node_in[0].packets_data_retrans == 1);
    CHECK(t.node_in[2].packets_data == 1 && t.node_in[2].bytes_data_payload == 7);
    CHECK(t.sock_in[0].packets_control_retrans == 1 && t.sock_in[1].bytes_data_payload_retrans == 6);
    const uint32_t placeholder[1] = {SRT_PDS_RELAY_FORWARDED}, none[1] = {0xffffffffu}, hp1[4] = {0, 1, 1, 1};
    const uint64_t lost[1] = {~0ull};
    t.rx(hp1, none, lost, placeholder, 1);
    CHECK(t.flags() == tracker::F_NOTE_OVERRUN && t.cnt_rx[0] == 2);
    t.rx(hp1, nullptr, nullptr, nullptr, 0);
    const uint32_t fh[4] = {2, 3, 0xffffffffu, 2}, fs[4] = {1, 0, 0, 0xffffffffu};
    t.flat(fh, fs, ms, 4);
    CHECK(t.flags() == tracker::F_BAD_HOST && t.cnt_rx[2] == 2 && t.sock_in[1].packets_control == 1);
    // no slots, no hosts
    Trk none_s(1, 0, 1, 1);
    none_s.note(ms + 1, 1, 0);
    const uint32_t hp2[2] = {0, 1}, s7[1] = {7}, st1[1] = {HIT};
    const uint64_t t0[1] = {0};
    none_s.rx(hp2, s7, t0, st1, 1);
    CHECK(none_s.flags() == 0 && none_s.node_in[0].bytes_data_payload == 5);
    Trk none_h(0, 0, 0, 0);
    const uint32_t hp0[1] = {0};
    none_h.rx(hp0, nullptr, nullptr, nullptr, 0);
    none_h.tx(nullptr, hp0, 0, nullptr, nullptr, 0, nullptr, 0, nullptr);
    CHECK(none_h.flags() == 0);
}

}  // namespace

int main() {
    for (uint32_t n_hosts : {1u, 7u, 65u}) relay_to_tracker(n_hosts, 40, 0, 11 + n_hosts);
    relay_to_tracker(9, 3, 0, 5);
    for (uint64_t log_cap : {1ull, 2ull, 63ull, 64ull, 65ull}) relay_to_tracker(9, 30, log_cap, 3);
    input_side();
    std::printf("tracker_check: clean\n");
    return 0;
}
