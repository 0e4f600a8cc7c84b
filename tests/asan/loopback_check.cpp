// loopback_check.cpp -- the loopback stage's step (shadow_amd/csrc/srt_loopback_step.h) in its
// host-only form with the deliver step's table (table_build, lookup), on host arrays allocated at
// exactly the sizes include/srt.h promises.  A stand-alone program: built for the host with
// -fsanitize=address,undefined and run directly (tests/test_loopback_cpu.py), so a read or write one
// past the packets, the per-packet scratch, an output array, a record array or the table is a
// sanitizer report.  The order is also checked against a literal run of the queues (a deque a socket,
// the qdisc over the sockets' heads), the counters against a plain re-statement.  Cases: empty hosts,
// one long instant, a host_ptr that runs past n_pkts, flagged hosts (time order, bad socket), slots
// out of range, n_slots == 0, no trk_meta.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <vector>

#include "../../shadow_amd/csrc/srt_loopback_step.h"

namespace {

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::printf("loopback_check: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

template <class T>
std::unique_ptr<T[]> arr(size_t n) {
    return std::unique_ptr<T[]>(new T[n]());  // exactly n: one past it is a report
}

uint64_t rnd(uint64_t &s) {  // xorshift64*
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return s * 2685821657736338717ull;
}

constexpr uint32_t NO = loopb::NO_SOCKET;

struct Stage {
    loopb::State st{};
    uint32_t n_hosts, n_slots, slots_tab;
    std::unique_ptr<loopb::HostSt[]> hs;
    std::unique_ptr<uint32_t[]> cnt_recv, cnt_miss;
    std::unique_ptr<srt_trk_counters[]> node_in, node_out, slot_in, slot_out;
    std::unique_ptr<deliver::Slot[]> table;
    loopb::Ctx base{};

    Stage(uint32_t nh, uint32_t ns, uint32_t qdisc, uint32_t max_sockets, const std::vector<srt_assoc> &assoc)
        : n_hosts(nh), n_slots(ns), hs(arr<loopb::HostSt>(nh)), cnt_recv(arr<uint32_t>(nh)), cnt_miss(arr<uint32_t>(nh)),
          node_in(arr<srt_trk_counters>(nh)), node_out(arr<srt_trk_counters>(nh)), slot_in(arr<srt_trk_counters>(ns)),
          slot_out(arr<srt_trk_counters>(ns)) {
        slots_tab = 2;
        while (slots_tab < 2 * assoc.size()) slots_tab *= 2;
        table = arr<deliver::Slot>(slots_tab);
        uint32_t max_probe, wrapped;
        deliver::table_build(table.get(), slots_tab, assoc.data(), assoc.size(), &max_probe, &wrapped);
        for (uint32_t h = 0; h < nh; ++h) hs[h].last_ns = loopb::NONE;
        base.st = &st, base.hs = hs.get(), base.cnt_recv = cnt_recv.get(), base.cnt_miss = cnt_miss.get();
        base.node_in = node_in.get(), base.node_out = node_out.get();
        base.slot_in = slot_in.get(), base.slot_out = slot_out.get();
        base.table = table.get(), base.mask = slots_tab - 1;
        base.n_hosts = nh, base.n_slots = ns, base.max_sockets = max_sockets, base.qdisc = qdisc;
    }
};

struct Batch {
    uint32_t n;
    std::unique_ptr<srt_out_pkt[]> pkts;
    std::unique_ptr<uint32_t[]> host_ptr;
    std::unique_ptr<srt_rx_meta[]> rx;
    std::unique_ptr<srt_trk_meta[]> trk;
    std::unique_ptr<uint64_t[]> key, recv;
    std::unique_ptr<uint32_t[]> grp, gend, idx, sock, user, status;
};

void classify(srt_trk_counters &r, const srt_trk_meta &m) {
    const bool rt = m.flags & SRT_TRK_RETRANS;
    if (m.payload_size > 0) {
        if (rt) r.packets_data_retrans++, r.bytes_data_header_retrans += m.header_size, r.bytes_data_payload_retrans += m.payload_size;
        else r.packets_data++, r.bytes_data_header += m.header_size, r.bytes_data_payload += m.payload_size;
    } else if (rt) {
        r.packets_control_retrans++, r.bytes_control_header_retrans += m.header_size;
    } else {
        r.packets_control++, r.bytes_control_header += m.header_size;
    }
}

// one scenario: `calls` calls on one instance, every one checked against the literal queues
void scenario(uint64_t seed, uint32_t n_hosts, uint32_t max_sockets, uint32_t n_slots, uint32_t qdisc, uint32_t calls,
              uint32_t per_host_max, bool long_instant, bool with_trk, bool overrun_ptr) {
    uint64_t s = seed;
    std::vector<srt_assoc> assoc;
    for (uint32_t h = 0; h < n_hosts; ++h)
        for (uint32_t d = 0; d < max_sockets; ++d) {
            if (d % 3 == 0) assoc.push_back(srt_assoc{h, SRT_PROTO_TCP, 0x0100007Fu, (uint16_t)(1000 + d), (uint16_t)(2000 + d), h * max_sockets + d});
            if (d % 3 == 1) assoc.push_back(srt_assoc{h, SRT_PROTO_UDP, 0, (uint16_t)(1000 + d), 0, h * max_sockets + d});
        }
    Stage sg(n_hosts, n_slots, qdisc, max_sockets, assoc);
    std::vector<uint64_t> now(n_hosts, 1000), last(n_hosts, loopb::NONE), tasks(n_hosts, 0);
    std::vector<srt_trk_counters> w_node_in(n_hosts), w_node_out(n_hosts), w_slot_in(n_slots), w_slot_out(n_slots);
    uint64_t serial = 0;
    for (uint32_t call = 0; call < calls; ++call) {
        // the batch
        std::vector<uint32_t> cnt(n_hosts);
        uint32_t n = 0;
        for (uint32_t h = 0; h < n_hosts; ++h) n += cnt[h] = rnd(s) % 4 == 0 ? 0 : (uint32_t)(rnd(s) % (per_host_max + 1));
        Batch b;
        b.n = n;
        b.pkts = arr<srt_out_pkt>(n), b.host_ptr = arr<uint32_t>(n_hosts + 1), b.rx = arr<srt_rx_meta>(n);
        b.trk = arr<srt_trk_meta>(n), b.key = arr<uint64_t>(n), b.recv = arr<uint64_t>(n);
        b.grp = arr<uint32_t>(n), b.gend = arr<uint32_t>(n), b.idx = arr<uint32_t>(n), b.sock = arr<uint32_t>(n);
        b.user = arr<uint32_t>(n), b.status = arr<uint32_t>(n);
        // a host to flag in this call, and how
        const uint32_t bad_host = call % 2 ? (uint32_t)(rnd(s) % n_hosts) : NO, bad_kind = (uint32_t)(rnd(s) % 3);
        std::vector<uint32_t> want_flag(n_hosts, 0);
        uint32_t i = 0;
        for (uint32_t h = 0; h < n_hosts; ++h) {
            uint32_t left = cnt[h];
            const uint32_t hb = i;
            while (left) {
                const uint32_t g = long_instant ? left : 1 + (uint32_t)(rnd(s) % (left < 7 ? left : 7));
                if (!(left == cnt[h] && rnd(s) % 3 == 0 && last[h] != loopb::NONE)) now[h] += 1 + rnd(s) % 1000;  // else: continues
                for (uint32_t k = 0; k < g; ++k, ++i) {
                    const uint32_t src = (uint32_t)(rnd(s) % max_sockets), d = (uint32_t)(rnd(s) % max_sockets);
                    b.pkts[i] = srt_out_pkt{now[h], (rnd(s) >> 24 << 20) | ++serial, 0, src, 0, 0};
                    const uint32_t proto = rnd(s) % 16 == 0 ? 9u : d % 3 == 1 ? SRT_PROTO_UDP : SRT_PROTO_TCP;
                    b.rx[i] = srt_rx_meta{d % 3 == 0 ? 0x0100007Fu : (uint32_t)rnd(s) | 1u, (uint16_t)(d % 3 == 0 ? 2000 + d : 77),
                                          (uint16_t)(1000 + d), proto, (uint32_t)serial};
                    // a slot past n_slots now and then
                    b.trk[i] = srt_trk_meta{20 + (uint32_t)(rnd(s) % 40), rnd(s) % 3 ? (uint32_t)(rnd(s) % 1400) : 0u,
                                            (uint32_t)(rnd(s) % 5 == 0), rnd(s) % 32 == 0 ? n_slots + 3 : h * max_sockets + src};
                }
                left -= g;
            }
            if (h == bad_host && i - hb >= 2) {
                if (bad_kind == 0) b.pkts[i - 1].ready_ns = b.pkts[i - 2].ready_ns - 1, want_flag[h] = loopb::F_TIME_ORDER;
                else if (bad_kind == 1 && last[h] != loopb::NONE && b.pkts[hb].ready_ns > last[h])
                    b.pkts[hb].ready_ns = last[h] - 1, want_flag[h] = loopb::F_TIME_ORDER;
                else b.pkts[hb + 1].socket = max_sockets, want_flag[h] = loopb::F_BAD_SOCKET;
            }
            b.host_ptr[h + 1] = i;
        }
        CHECK(i == n);
        // a grouping that claims more packets than the call has: the walk is held below n_pkts
        uint32_t n_arg = n;
        if (overrun_ptr && n > 3) {
            n_arg = n - 3;
            b.host_ptr[n_hosts] = n + 1000;
        }
        loopb::Ctx c = sg.base;
        c.key = b.key.get(), c.grp = b.grp.get(), c.gend = b.gend.get();
        c.n_pkts = n_arg, c.pkts = b.pkts.get(), c.host_ptr = b.host_ptr.get(), c.rx_meta = b.rx.get();
        c.trk_meta = with_trk ? b.trk.get() : nullptr;
        c.out_index = b.idx.get(), c.out_socket = b.sock.get(), c.out_recv_ns = b.recv.get(), c.out_user = b.user.get();
        c.out_status = b.status.get();
        for (uint32_t k = 0; k < n; ++k) b.idx[k] = 0xdeadbeefu;
        loopb::host_run(c);
        // the literal queues
        uint32_t w_flags = 0, w_bad_slot = 0;
        uint64_t w_recv = 0, w_miss = 0;
        for (uint32_t h = 0; h < n_hosts; ++h) {
            const uint32_t hb = b.host_ptr[h] < n_arg ? b.host_ptr[h] : n_arg;
            uint32_t he = b.host_ptr[h + 1] < n_arg ? b.host_ptr[h + 1] : n_arg;
            if (he < hb) he = hb;
            uint32_t bad = 0;
            uint64_t prev = last[h];
            for (uint32_t k = hb; k < he; ++k) {
                if (prev != loopb::NONE && b.pkts[k].ready_ns < prev) bad |= loopb::F_TIME_ORDER;
                if (b.pkts[k].socket >= max_sockets) bad |= loopb::F_BAD_SOCKET;
                prev = b.pkts[k].ready_ns;
            }
            if (he == b.host_ptr[h + 1] && hb == b.host_ptr[h]) CHECK((bad != 0) == (want_flag[h] != 0));
            w_flags |= bad;
            if (bad) {
                for (uint32_t k = hb; k < he; ++k)
                    CHECK(b.idx[k] == k && b.sock[k] == NO && b.recv[k] == loopb::NONE && b.status[k] == 0 && b.user[k] == b.rx[k].user);
                continue;
            }
            uint32_t k = hb, pos = hb;
            while (k < he) {
                const uint64_t t = b.pkts[k].ready_ns;
                if (last[h] != t) ++tasks[h];
                last[h] = t;
                std::map<uint32_t, std::deque<uint32_t>> socks;
                std::deque<uint32_t> q;  // sockets in the qdisc, in joining order
                for (; k < he && b.pkts[k].ready_ns == t; ++k) {
                    auto &dq = socks[b.pkts[k].socket];
                    if (dq.empty()) q.push_back(b.pkts[k].socket);
                    dq.push_back(k);
                }
                while (!q.empty()) {
                    size_t at = 0;
                    if (qdisc == SRT_QDISC_FIFO)
                        for (size_t j = 1; j < q.size(); ++j)
                            if (b.pkts[socks[q[j]].front()].priority < b.pkts[socks[q[at]].front()].priority) at = j;
                    const uint32_t sk = q[at];
                    q.erase(q.begin() + at);
                    const uint32_t p = socks[sk].front();
                    socks[sk].pop_front();
                    if (!socks[sk].empty()) q.push_back(sk);
                    const uint32_t so = deliver::lookup(sg.table.get(), sg.slots_tab - 1, h, b.rx[p]);
                    CHECK(pos < he && b.idx[pos] == p && b.sock[pos] == so && b.recv[pos] == t && b.user[pos] == b.rx[p].user);
                    CHECK(b.status[pos] == (loopb::RECEIVED | (so == NO ? SRT_PDS_RCV_INTERFACE_DROPPED : 0u)));
                    ++w_recv, w_miss += so == NO;
                    if (with_trk) {
                        const srt_trk_meta &m = b.trk[p];
                        classify(w_node_out[h], m);
                        if (n_slots && m.socket_slot < n_slots) classify(w_slot_out[m.socket_slot], m);
                        else if (n_slots) w_bad_slot = loopb::F_BAD_SLOT;
                        if (so != NO) {
                            classify(w_node_in[h], m);
                            if (n_slots && so < n_slots) classify(w_slot_in[so], m);
                            else if (n_slots) w_bad_slot = loopb::F_BAD_SLOT;
                        }
                    }
                    ++pos;
                }
            }
            CHECK(pos == he);
        }
        for (uint32_t k = n_arg; k < n; ++k) CHECK(b.idx[k] == 0xdeadbeefu);  // nothing past the walk
        CHECK(sg.st.flags == (w_flags | w_bad_slot));
        sg.st.flags = 0;
        CHECK(sg.st.n_received == w_recv && sg.st.n_no_socket == w_miss);
        for (uint32_t h = 0; h < n_hosts; ++h) {
            CHECK(sg.hs[h].tasks == tasks[h] && sg.hs[h].last_ns == last[h]);
            CHECK(!std::memcmp(&sg.node_in[h], &w_node_in[h], 80) && !std::memcmp(&sg.node_out[h], &w_node_out[h], 80));
        }
        for (uint32_t x = 0; x < n_slots; ++x)
            CHECK(!std::memcmp(&sg.slot_in[x], &w_slot_in[x], 80) && !std::memcmp(&sg.slot_out[x], &w_slot_out[x], 80));
    }
}

}  // namespace

int main() {
    uint32_t runs = 0;
    for (uint32_t qdisc = SRT_QDISC_FIFO; qdisc <= SRT_QDISC_RR; ++qdisc) {
        for (uint64_t seed = 1; seed <= 6; ++seed) {
            scenario(seed * 77, 9, 5, 45, qdisc, 4, 20, false, true, false), ++runs;
            scenario(seed * 91, 1, 1, 1, qdisc, 3, 9, false, true, false), ++runs;
            scenario(seed * 13, 4, 3, 0, qdisc, 3, 30, false, true, seed % 2 == 0), ++runs;  // no slot counters
            scenario(seed * 29, 6, 4, 5, qdisc, 3, 12, false, true, true), ++runs;           // most slots out of range
            scenario(seed * 31, 5, 6, 30, qdisc, 2, 25, false, false, false), ++runs;        // nothing counted
        }
        scenario(5, 3, 4, 12, qdisc, 2, 400, true, true, false), ++runs;  // one long instant a host
        scenario(6, 70, 2, 140, qdisc, 2, 3, false, true, true), ++runs;
    }
    std::printf("loopback_check: clean (%u scenarios)\n", runs);
    return 0;
}
