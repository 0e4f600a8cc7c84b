// udpsend_check.cpp -- the UDP send side's step (shadow_amd/csrc/srt_udpsend_step.h) and its host-only entry
// points (host_config, host_run, and config_at as the device's launch walks it) on host arrays allocated at
// exactly the sizes include/srt.h promises.  A stand-alone program: built for the host with
// -fsanitize=address,undefined and run directly (tests/test_udpsend_cpu.py), so a write one past the hosts,
// the slots, a ring, the qdisc arrays, the staged records, the results, or either late list is a sanitizer
// report.  Generated windows (hosts with 0 to 5 slots, rings of 0, 1, 3 and 64 messages, late lists of 0 and
// 2 records, both qdiscs, hosts that forward everything and hosts that forward next to nothing) and truncated
// or broken inputs (pointer arrays that run past the list, that decrease, slots nobody owns, times that go
// back).  The state is also checked against a plain re-statement: a host's queue_len is the sum of its
// slots' n_msgs, a UDP slot's len_bytes is the sum of its ring's payloads unless it overflowed, only an open
// slot is armed, and an idle relay has nothing queued.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../shadow_amd/csrc/srt_udpsend_step.h"

namespace {

#define CHECK(x)                                                               \
    do {                                                                       \
        if (!(x)) {                                                            \
            std::printf("udpsend_check: %s:%d: %s\n", __FILE__, __LINE__, #x); \
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

constexpr uint64_t NONE = udps::NONE;
constexpr uint32_t IP0 = 0x0100000bu;  // 11.0.0.1 and up

// the instance of srt_udpsend.hip's host-only form, on exact arrays
struct Inst {
    udps::State st{};
    uint32_t n_hosts, n_sockets, ring_cap, call_no = 0;
    uint64_t seq = 0, prev_until = 0;
    std::unique_ptr<uint32_t[]> socket_ptr, sockq;
    std::unique_ptr<udps::Host[]> hosts;
    std::unique_ptr<udps::Sock[]> socks;
    std::unique_ptr<udps::RingEl[]> ring;
    udps::Ctx base{};

    Inst(const std::vector<uint32_t> &counts, uint32_t ring_cap_, uint32_t qdisc, uint64_t bw)
        : n_hosts((uint32_t)counts.size()), ring_cap(ring_cap_), socket_ptr(arr<uint32_t>(counts.size() + 1)) {
        for (uint32_t h = 0; h < n_hosts; ++h) socket_ptr[h + 1] = socket_ptr[h] + counts[h];
        n_sockets = socket_ptr[n_hosts];
        hosts = arr<udps::Host>(n_hosts);
        socks = arr<udps::Sock>(n_sockets);
        sockq = arr<uint32_t>(n_sockets);
        ring = arr<udps::RingEl>((size_t)n_sockets * (ring_cap + 1));
        for (uint32_t x = 0; x < n_sockets; ++x) udps::sock_init(socks[x]);
        for (uint32_t h = 0; h < n_hosts; ++h) {
            udps::Host &s = hosts[h];
            s.refill = relay::bucket_refill(h % 3 ? bw : 1000000000ull);
            s.capacity = relay::sat_add(s.refill, relay::MTU);
            s.balance = s.capacity;
            s.task_ns = NONE;
            s.next_priority = 1;
            s.ip = IP0 + (h << 24);
        }
        base.st = &st;
        base.hosts = hosts.get(), base.socks = socks.get(), base.ring = ring.get(), base.sockq = sockq.get();
        base.socket_ptr = socket_ptr.get();
        base.n_hosts = n_hosts, base.n_sockets = n_sockets, base.ring_cap = ring_cap, base.qdisc = qdisc;
    }

    // as srt_udpsend_config validates and applies them; `sorted`: the device's way, through config_at
    void config(std::vector<srt_udpsend_op> ops, bool sorted) {
        udps::Ctx c = base;
        if (sorted)
            std::stable_sort(ops.begin(), ops.end(), [](const srt_udpsend_op &a, const srt_udpsend_op &b) {
                const uint64_t ka = (uint64_t)(a.op == SRT_UDPSEND_SET_NEXT_PRIORITY) << 32 | a.slot;
                const uint64_t kb = (uint64_t)(b.op == SRT_UDPSEND_SET_NEXT_PRIORITY) << 32 | b.slot;
                return ka < kb;
            });
        const auto exact = arr<srt_udpsend_op>(ops.size());
        std::copy(ops.begin(), ops.end(), exact.get());
        c.ops = exact.get();
        c.n_ops = (uint32_t)ops.size();
        if (sorted)
            for (uint32_t i = 0; i < c.n_ops; ++i) udps::config_at(c, i);
        else
            udps::host_config(c);
    }
};

struct Out {
    std::unique_ptr<srt_udpsend_result[]> results;
    std::unique_ptr<uint32_t[]> status;
    std::unique_ptr<uint64_t[]> send_ns, send_rank, first;
    std::unique_ptr<srt_outbound_late[]> late;
    std::unique_ptr<srt_udpsend_late[]> late_res;
    uint32_t late_count = 0, late_res_count = 0;
};

// one srt_udpsend_run on exact arrays; host_ptr as given (it may lie)
Out run(Inst &in, const std::vector<srt_udp_send> &calls, const std::vector<uint32_t> &host_ptr, uint64_t until,
        uint32_t late_cap) {
    const uint32_t n = (uint32_t)calls.size();
    Out o;
    o.results = arr<srt_udpsend_result>(n);
    o.status = arr<uint32_t>(n);
    o.send_ns = arr<uint64_t>(n);
    o.send_rank = arr<uint64_t>(n);
    o.first = arr<uint64_t>(in.n_sockets);
    o.late = arr<srt_outbound_late>(late_cap);
    o.late_res = arr<srt_udpsend_late>(late_cap);
    const auto d_calls = arr<srt_udp_send>(n);
    std::copy(calls.begin(), calls.end(), d_calls.get());
    const auto hp = arr<uint32_t>(in.n_hosts + 1);
    std::copy(host_ptr.begin(), host_ptr.end(), hp.get());
    const auto rec = arr<udps::Rec>(n);
    udps::Ctx c = in.base;
    c.rec = rec.get();
    c.calls = d_calls.get();
    c.host_ptr = hp.get();
    c.results = o.results.get(), c.status = o.status.get(), c.send_ns = o.send_ns.get(), c.send_rank = o.send_rank.get();
    c.late = o.late.get(), c.late_cap = late_cap, c.late_count = &o.late_count;
    c.late_res = o.late_res.get(), c.late_res_cap = late_cap, c.late_res_count = &o.late_res_count;
    c.first_writable = o.first.get();
    c.base = in.seq, c.until = until, c.boot_end = 0, c.prev_until = in.prev_until;
    c.n_calls = n;
    c.call_no = ++in.call_no;
    udps::host_run(c);
    in.seq += n;
    in.prev_until = until;
    return o;
}

void check_state(const Inst &in) {
    for (uint32_t h = 0; h < in.n_hosts; ++h) {
        const udps::Host &s = in.hosts[h];
        const uint32_t b = in.socket_ptr[h], e = in.socket_ptr[h + 1];
        uint64_t queued = 0;
        uint32_t with_data = 0;
        for (uint32_t x = b; x < e; ++x) {
            const udps::Sock &k = in.socks[x];
            queued += k.n_msgs;
            with_data += k.n_msgs != 0;
            CHECK(k.n_msgs <= in.ring_cap && k.carry == k.n_msgs && k.ring_head == 0);
            CHECK(k.head == udps::NIL && k.tail == udps::NIL);
            uint64_t bytes = 0;
            bool raw = false;
            for (uint32_t p = 0; p < k.n_msgs; ++p) {
                const udps::RingEl &m = in.ring[(size_t)x * (in.ring_cap + 1) + p];
                raw = raw || (m.flags & udps::EL_RAW);
                bytes += m.size;
                CHECK(m.seq < in.seq);
            }
            if (!raw && !s.overflow) CHECK(k.len_bytes == bytes);
            if (k.armed_seq != NONE) CHECK((k.bits & udps::B_OPEN) && k.armed_seq < in.seq);
        }
        CHECK(s.n_queued == queued && s.q_len == with_data && s.q_len <= e - b);
        CHECK(s.cached <= 1);
        if (!queued && !s.cached && !s.overflow) CHECK(s.task_ns == NONE);
    }
}

void generated(uint32_t ring_cap, uint32_t qdisc, uint64_t bw, uint32_t late_cap, bool sorted, uint64_t seed) {
    uint64_t r = seed;
    std::vector<uint32_t> counts;
    for (uint32_t h = 0; h < 70; ++h) counts.push_back((uint32_t)(rnd(r) % 6));
    Inst in(counts, ring_cap, qdisc, bw);
    unsigned long long answered = 0;
    for (uint32_t w = 0; w < 6; ++w) {
        std::vector<srt_udpsend_op> ops;
        for (uint32_t x = 0; x < in.n_sockets; ++x) {
            const uint32_t roll = (uint32_t)(rnd(r) % 100);
            if (x % 6 == 5) continue;  // never opened: raw arrivals
            if (w == 0 || roll < 8) {
                ops.push_back({SRT_UDPSEND_OPEN, x, roll % 2 ? 4096u : 1u << 20});
                if (roll % 10) ops.push_back({SRT_UDPSEND_BIND, x, (uint64_t)(roll % 3 ? 0u : IP0) | 5000ull << 32});
                if (roll % 2) ops.push_back({SRT_UDPSEND_SET_PEER, x, (uint64_t)(IP0 + (1u << 24)) | 6000ull << 32});
            } else if (roll < 12) {
                ops.push_back({SRT_UDPSEND_CLOSE, x, 0});
            } else if (roll < 18) {
                ops.push_back({SRT_UDPSEND_SET_SNDBUF, x, roll % 2 ? 1u : 1ull << 40});
            } else if (roll < 21) {
                ops.push_back({SRT_UDPSEND_SHUT_WR, x, 0});
            }
        }
        ops.push_back({SRT_UDPSEND_SET_NEXT_PRIORITY, w % in.n_hosts, 1000 * (uint64_t)w + 1});
        in.config(ops, sorted);
        const uint64_t t0 = w * 100000000ull, until = t0 + 100000000ull;
        std::vector<srt_udp_send> calls;
        std::vector<uint32_t> hp(in.n_hosts + 1, 0);
        for (uint32_t h = 0; h < in.n_hosts; ++h) {
            const uint32_t lo = in.socket_ptr[h], hi = in.socket_ptr[h + 1];
            const uint32_t k = hi > lo && w < 5 ? (uint32_t)(rnd(r) % 30) : 0;
            std::vector<uint64_t> ts;
            for (uint32_t i = 0; i < k; ++i) ts.push_back(t0 + rnd(r) % 400 * 250000);
            std::sort(ts.begin(), ts.end());
            for (uint32_t i = 0; i < k; ++i) {
                srt_udp_send c{};
                c.time_ns = ts[i];
                c.slot = lo + (uint32_t)(rnd(r) % (hi - lo));
                c.user = (uint32_t)rnd(r);
                if (c.slot % 6 == 5) {
                    c.flags = SRT_UDPSEND_RAW | (rnd(r) % 8 ? 0u : SRT_UDPSEND_LOCAL);
                    c.len = 40 + (uint32_t)(rnd(r) % 1461);
                    c.priority = rnd(r) % 100000;
                } else {
                    c.len = rnd(r) % 50 ? (uint32_t)(rnd(r) % 1473) : 70000u;
                    c.flags = (rnd(r) % 2 ? SRT_UDPSEND_WAIT : 0u) | (rnd(r) % 2 ? SRT_UDPSEND_HAS_ADDR : 0u);
                    c.dst_ip_be = rnd(r) % 9 ? IP0 + ((uint32_t)(rnd(r) % 70) << 24) : udps::LOCALHOST_BE;
                }
                calls.push_back(c);
            }
            hp[h + 1] = (uint32_t)calls.size();
        }
        const Out o = run(in, calls, hp, until, late_cap);
        for (size_t i = 0; i < calls.size(); ++i) {
            const srt_udpsend_result &res = o.results[i];
            CHECK(res.user == calls[i].user && res.status <= SRT_UDPSEND_ARMED);
            answered += res.status == SRT_UDPSEND_DONE;
            if (o.status[i] & SRT_PDS_RELAY_FORWARDED) CHECK(o.send_ns[i] < until && o.send_ns[i] >= calls[i].time_ns);
            else CHECK(o.send_ns[i] == NONE && o.send_rank[i] == NONE);
        }
        for (uint32_t x = 0; x < in.n_sockets; ++x) CHECK(o.first[x] == NONE || (o.first[x] >= t0 && o.first[x] < until));
        check_state(in);
    }
    CHECK(answered > 1000);
    CHECK(in.st.n_acc > 500 && (bw > 20000 || in.st.n_wb > 10));
}

// pointer arrays that lie, slots nobody owns, times that go back: flagged or ignored, never out of bounds
void broken() {
    for (uint32_t variant = 0; variant < 4; ++variant) {
        Inst in({2, 0, 3}, 2, variant & 1, 1000);
        in.config({{SRT_UDPSEND_OPEN, 0, 4096}, {SRT_UDPSEND_BIND, 0, 5000ull << 32}, {SRT_UDPSEND_OPEN, 2, 4096},
                   {SRT_UDPSEND_BIND, 2, 5000ull << 32}, {SRT_UDPSEND_OPEN, 4, 100}, {SRT_UDPSEND_BIND, 4, 5000ull << 32}},
                  variant & 2);
        std::vector<srt_udp_send> calls;
        for (uint32_t i = 0; i < 12; ++i) {
            srt_udp_send c{};
            c.time_ns = i == 7 ? 1 : 1000 * i;  // one goes back
            c.slot = i % 6 == 5 ? 0xfffffff0u : i % 5;  // slots of other hosts, and of none
            c.len = 1000;
            c.flags = SRT_UDPSEND_HAS_ADDR | (i % 2 ? SRT_UDPSEND_WAIT : 0u) | (i % 4 == 3 ? SRT_UDPSEND_RAW : 0u);
            c.dst_ip_be = IP0 + (1u << 24);
            calls.push_back(c);
        }
        const std::vector<uint32_t> ptrs[4] = {{0, 4, 8, 12}, {0, 50, 60, 70}, {0, 9, 3, 12}, {5, 5, 5, 0xffffffffu}};
        Out o = run(in, calls, ptrs[variant], 6000, variant & 1);
        check_state(in);
        o = run(in, {}, {0, 0, 0, 0}, 1000000000000ull, variant & 1);  // everything drains, late lists of 0 or 1
        check_state(in);
        CHECK(in.st.flags != 0);
    }
    // no hosts, no slots, no calls
    Inst empty({}, 0, 0, 1000);
    run(empty, {}, {0}, 5, 0);
    Inst bare({0, 0}, 0, 1, 1000);
    srt_udp_send c{};
    run(bare, {c}, {0, 1, 1}, 5, 0);
    CHECK(bare.st.flags & udps::F_BAD_SOCKET);
}

}  // namespace

int main() {
    uint64_t seed = 0x9e3779b97f4a7c15ull;
    for (uint32_t ring_cap : {0u, 1u, 3u, 64u})
        for (uint32_t qdisc : {0u, 1u})
            for (uint64_t bw : {20000ull, 1000000ull})
                generated(ring_cap, qdisc, bw, ring_cap == 3 ? 0 : 2 + 4000 * (ring_cap == 64), qdisc != 0, seed += 77);
    broken();
    std::printf("udpsend_check: clean\n");
    return 0;
}
