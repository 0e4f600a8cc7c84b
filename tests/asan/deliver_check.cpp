// deliver_check.cpp -- the interface receive stage's step (shadow_amd/csrc/srt_deliver_step.h) alone,
// on host arrays allocated at exactly the sizes include/srt.h promises, at the sizes where the step
// takes another path.  A stand-alone program: built for the host with -fsanitize=address,undefined and
// run directly (tests/test_deliver_cpu.py), so a write one past the ring, the log, the table, a count or
// an output array is a sanitizer report.  Every delivery list is also checked against a plain
// re-statement: a linear search of the associations, the late records sorted by seq.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <vector>

#include "../../shadow_amd/csrc/srt_deliver_step.h"

namespace {

constexpr uint32_t FWD = SRT_PDS_ROUTER_ENQUEUED | SRT_PDS_ROUTER_DEQUEUED | SRT_PDS_RELAY_FORWARDED;
constexpr uint32_t QUEUED = SRT_PDS_ROUTER_ENQUEUED;
constexpr uint32_t G = deliver::SORT_CAP;
constexpr uint32_t NONE = deliver::NO_SOCKET;

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            std::printf("deliver_check: %s:%d: %s\n", __FILE__, __LINE__, #x); \
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

struct Out {
    std::vector<uint32_t> host_ptr, socket, user, status;
    std::vector<uint64_t> forward, tag;
};

struct Stage {
    deliver::State st{};
    uint32_t n_hosts, slots;
    uint64_t note_cap, log_cap, note_end = 0;
    std::vector<srt_assoc> assoc;
    std::unique_ptr<deliver::Slot[]> table;
    std::unique_ptr<srt_rx_meta[]> ring;
    std::unique_ptr<deliver::LogRec[]> log;
    std::unique_ptr<uint32_t[]> cnt, nlate, lfill;
    std::map<uint64_t, srt_rx_meta> noted;                      // tag -> meta, everything ever noted
    std::map<uint64_t, std::pair<uint64_t, bool>> logged;       // seq -> (tag, meta known)
    deliver::Ctx base{};

    Stage(uint32_t n_hosts_, uint32_t slots_, uint64_t note_cap_, uint64_t log_cap_)
        : n_hosts(n_hosts_), slots(slots_), note_cap(note_cap_), log_cap(log_cap_), table(arr<deliver::Slot>(slots_)),
          ring(arr<srt_rx_meta>(note_cap_)), log(arr<deliver::LogRec>(log_cap_)), cnt(arr<uint32_t>(n_hosts_)),
          nlate(arr<uint32_t>(n_hosts_)), lfill(arr<uint32_t>(n_hosts_)) {
        base.st = &st, base.n_hosts = n_hosts, base.ring = ring.get(), base.log = log.get();
        base.note_cap = note_cap, base.log_cap = log_cap;
        base.cnt = cnt.get(), base.nlate = nlate.get(), base.lfill = lfill.get();
        build();
    }

    void build() {
        uint32_t max_probe, wrapped;
        CHECK(2 * assoc.size() <= slots);
        deliver::table_build(table.get(), slots, assoc.data(), assoc.size(), &max_probe, &wrapped);
        base.table = table.get(), base.mask = slots - 1;
    }

    uint32_t plain_lookup(uint32_t h, const srt_rx_meta &m) const {
        for (int wild = 0; wild < 2; ++wild)
            for (const srt_assoc &a : assoc)
                if (a.host == h && a.protocol == m.protocol && a.local_port_be == m.local_port_be &&
                    a.peer_ip_be == (wild ? 0u : m.peer_ip_be) && a.peer_port_be == (wild ? 0 : m.peer_port_be))
                    return a.socket;
        return NONE;
    }

    void note(const std::vector<srt_rx_meta> &metas, uint64_t tag_base) {
        auto in = arr<srt_rx_meta>(metas.size());
        std::copy(metas.begin(), metas.end(), in.get());
        for (size_t i = 0; i < metas.size(); ++i) noted[tag_base + i] = metas[i];
        note_end = tag_base + metas.size();
        if (!note_cap || metas.empty()) return;
        deliver::Ctx c = base;
        c.note_in = in.get(), c.note_n = (uint32_t)metas.size();
        c.note_first = metas.size() > note_cap ? (uint32_t)(metas.size() - note_cap) : 0u;
        c.note_first_mod = (tag_base + c.note_first) % note_cap;
        deliver::host_note(c);
    }

    bool readable(uint64_t tag) const { return tag < note_end && note_end - tag <= note_cap; }

    // one run on arrays of exactly n_pkts / n_late / out_cap entries; the result is checked here
    Out run(const std::vector<uint32_t> &dst_ptr, uint64_t n_pkts, const std::vector<uint64_t> &tag,
            const std::vector<uint32_t> &status, const std::vector<uint64_t> &forward, uint64_t seq_base,
            const std::vector<srt_inbound_late> &late, uint64_t out_cap) {
        CHECK(dst_ptr.size() == (size_t)n_hosts + 1 && tag.size() == n_pkts && status.size() == n_pkts);
        auto dp = arr<uint32_t>(dst_ptr.size()), stt = arr<uint32_t>(n_pkts), lc = arr<uint32_t>(1);
        auto tg = arr<uint64_t>(n_pkts), fw = arr<uint64_t>(n_pkts);
        auto lt = arr<srt_inbound_late>(late.size());
        std::copy(dst_ptr.begin(), dst_ptr.end(), dp.get());
        std::copy(tag.begin(), tag.end(), tg.get());
        std::copy(status.begin(), status.end(), stt.get());
        std::copy(forward.begin(), forward.end(), fw.get());
        std::copy(late.begin(), late.end(), lt.get());
        lc[0] = (uint32_t)late.size() + 3;  // the count runs past the cap on overflow: only late_cap exist
        auto ohp = arr<uint32_t>((size_t)n_hosts + 1), osock = arr<uint32_t>(out_cap), ouser = arr<uint32_t>(out_cap),
             ost = arr<uint32_t>(out_cap);
        auto ofw = arr<uint64_t>(out_cap), otag = arr<uint64_t>(out_cap);
        deliver::Ctx c = base;
        c.note_end = note_end, c.note_end_mod = note_cap ? note_end % note_cap : 0;
        c.base_mod = log_cap ? seq_base % log_cap : 0, c.end_mod = log_cap ? (seq_base + n_pkts) % log_cap : 0;
        c.dst_ptr = dp.get(), c.status = stt.get(), c.tag = tg.get(), c.forward_ns = fw.get();
        c.late = lt.get(), c.late_count = late.empty() ? nullptr : lc.get(), c.late_cap = (uint32_t)late.size();
        c.seq_base = seq_base, c.n_pkts = (uint32_t)n_pkts, c.out_cap = out_cap;
        c.out_host_ptr = ohp.get(), c.out_socket = osock.get(), c.out_user = ouser.get(), c.out_status = ost.get();
        c.out_forward_ns = ofw.get(), c.out_tag = otag.get();
        deliver::host_run(c);

        // ---- the plain re-statement
        const uint64_t lim = std::min<uint64_t>(dst_ptr[n_hosts], n_pkts);
        for (uint64_t i = 0; i < lim; ++i)
            if (status[i] == QUEUED && lim - i <= log_cap) {
                for (auto it = logged.begin(); it != logged.end();)  // the slot's former owner is gone
                    it = (it->first % log_cap == (seq_base + i) % log_cap) ? logged.erase(it) : std::next(it);
                logged[seq_base + i] = {tag[i], readable(tag[i])};
            }
        Out want;
        uint32_t flags = 0;
        auto push = [&](uint32_t h, uint64_t t, uint64_t f, uint32_t s, bool known) {
            uint32_t sock = NONE, user = 0xffffffffu;
            if (known) {
                const srt_rx_meta &m = noted.at(t);
                sock = plain_lookup(h, m), user = m.user;
                s |= sock == NONE ? deliver::RECEIVED | deliver::DROPPED : deliver::RECEIVED;
            }
            want.socket.push_back(sock), want.user.push_back(user), want.status.push_back(s);
            want.forward.push_back(f), want.tag.push_back(t);
        };
        for (uint32_t h = 0; h < n_hosts; ++h) {
            want.host_ptr.push_back((uint32_t)want.tag.size());
            std::vector<srt_inbound_late> mine;
            for (const srt_inbound_late &r : late)
                if ((r.status & SRT_PDS_RELAY_FORWARDED) && r.dst_host == h) mine.push_back(r);
            std::sort(mine.begin(), mine.end(),
                      [](const srt_inbound_late &a, const srt_inbound_late &b) { return a.seq < b.seq; });
            for (const srt_inbound_late &r : mine) {
                const uint64_t end = seq_base + n_pkts;
                if (r.seq >= end || end - r.seq > log_cap) {
                    flags |= deliver::F_LOG_OVERRUN;
                    push(h, ~0ull, r.forward_ns, r.status, false);
                } else {
                    const auto g = logged.count(r.seq) ? logged.at(r.seq) : std::pair<uint64_t, bool>{0, false};
                    if (!g.second) flags |= deliver::F_NOTE_OVERRUN;
                    push(h, g.first, r.forward_ns, r.status, g.second);
                }
            }
            const uint64_t b = std::min<uint64_t>(dst_ptr[h], lim), e = std::max(b, std::min<uint64_t>(dst_ptr[h + 1], lim));
            for (uint64_t i = b; i < e; ++i)
                if (status[i] & SRT_PDS_RELAY_FORWARDED) {
                    if (!readable(tag[i])) flags |= deliver::F_NOTE_OVERRUN;
                    push(h, tag[i], forward[i], status[i], readable(tag[i]));
                }
        }
        want.host_ptr.push_back((uint32_t)want.tag.size());
        for (const srt_inbound_late &r : late)
            if ((r.status & SRT_PDS_RELAY_FORWARDED) && r.dst_host >= n_hosts) flags |= deliver::F_BAD_HOST;
        for (uint64_t i = 0; i < lim; ++i)
            if (status[i] == QUEUED && lim - i <= log_cap && !readable(tag[i])) flags |= deliver::F_NOTE_OVERRUN;
        const uint64_t total = want.tag.size();
        CHECK(st.n_delivered == total);
        for (uint32_t h = 0; h <= n_hosts; ++h) CHECK(ohp[h] == std::min<uint64_t>(want.host_ptr[h], out_cap));
        if (total > out_cap) {
            CHECK(st.flags & deliver::F_OUT_OVERFLOW);
            st.flags = 0;
            return want;
        }
        CHECK(st.flags == flags);
        st.flags = 0;
        uint64_t miss = 0;
        for (uint64_t k = 0; k < total; ++k) {
            CHECK(osock[k] == want.socket[k] && ouser[k] == want.user[k] && ost[k] == want.status[k]);
            CHECK(ofw[k] == want.forward[k] && otag[k] == want.tag[k]);
            miss += (want.status[k] & deliver::DROPPED) != 0;
        }
        CHECK(st.n_no_socket == miss);
        return want;
    }
};

srt_rx_meta rand_meta(uint64_t &seed, uint32_t user) {
    srt_rx_meta m;
    m.peer_ip_be = (uint32_t)(rnd(seed) % 3), m.peer_port_be = (uint16_t)(rnd(seed) % 2);
    m.local_port_be = (uint16_t)(80 + rnd(seed) % 2), m.protocol = 1 + (uint32_t)(rnd(seed) % 3), m.user = user;
    return m;
}

}  // namespace

int main() {
    uint64_t seed = 88172645463325252ull;
    {  // late runs of G - 1, G, G + 1 and 3G + 5 records, hosts with none and one; the late list shuffled
        const std::vector<uint32_t> sizes = {G - 1, 0, G, 1, G + 1, 3 * G + 5};
        uint32_t n = 0;
        for (uint32_t s : sizes) n += s;
        Stage s((uint32_t)sizes.size(), 64, n + 6, n + 6);
        for (uint32_t h = 0; h < sizes.size(); ++h) {
            s.assoc.push_back(srt_assoc{h, SRT_PROTO_TCP, 0, 80, 0, 100 + h});
            s.assoc.push_back(srt_assoc{h, SRT_PROTO_UDP, 1, 81, 1, 200 + h});
        }
        s.build();
        std::vector<srt_rx_meta> metas;
        for (uint32_t i = 0; i < n; ++i) metas.push_back(rand_meta(seed, i));
        s.note(metas, 0);
        std::vector<uint32_t> dp = {0};
        for (uint32_t k : sizes) dp.push_back(dp.back() + k);
        std::vector<uint64_t> tag(n), fw(n, ~0ull);
        for (uint32_t i = 0; i < n; ++i) tag[i] = n - 1 - i;
        Out o = s.run(dp, n, tag, std::vector<uint32_t>(n, QUEUED), fw, 0, {}, 0);
        CHECK(o.tag.empty());
        std::vector<srt_inbound_late> late;
        for (uint32_t h = 0; h < sizes.size(); ++h)
            for (uint32_t i = dp[h]; i < dp[h + 1]; ++i) late.push_back(srt_inbound_late{i, 1000 + i, FWD, h});
        for (size_t i = late.size(); i > 1; --i) std::swap(late[i - 1], late[rnd(seed) % i]);
        std::vector<srt_rx_meta> m2;
        for (uint32_t i = 0; i < 6; ++i) m2.push_back(rand_meta(seed, n + i));
        s.note(m2, n);
        std::vector<uint32_t> dp2 = {0, 1, 2, 3, 4, 5, 6};
        o = s.run(dp2, 6, {n, n + 1, n + 2, n + 3, n + 4, n + 5}, std::vector<uint32_t>(6, FWD),
                  std::vector<uint64_t>(6, 1u << 30), n, late, n + 6);  // the outputs exactly full
        CHECK(o.tag.size() == n + 6);
        // one short: nothing past out_cap, the bases held at it
        s.run(dp2, 6, {n, n + 1, n + 2, n + 3, n + 4, n + 5}, std::vector<uint32_t>(6, FWD),
              std::vector<uint64_t>(6, 1u << 30), n, late, n + 5);
        s.run(dp2, 6, {n, n + 1, n + 2, n + 3, n + 4, n + 5}, std::vector<uint32_t>(6, FWD),
              std::vector<uint64_t>(6, 1u << 30), n, late, 0);
    }
    {  // rings smaller than the traffic: NOTE_OVERRUN and LOG_OVERRUN placeholders, rings wrapping
        Stage s(3, 8, 5, 4);
        s.assoc = {srt_assoc{0, SRT_PROTO_TCP, 0, 80, 0, 1}, srt_assoc{1, SRT_PROTO_TCP, 1, 80, 1, 2},
                   srt_assoc{2, SRT_PROTO_UDP, 0, 81, 0, 3}, srt_assoc{2, SRT_PROTO_UDP, 2, 81, 1, 4}};
        s.build();
        uint64_t tags = 0, seq = 0;
        std::vector<srt_inbound_late> late;
        for (int round = 0; round < 12; ++round) {
            const uint32_t n = 3 + (uint32_t)(rnd(seed) % 6);  // 3 .. 8: above and below both caps
            std::vector<srt_rx_meta> metas;
            for (uint32_t i = 0; i < n; ++i) metas.push_back(rand_meta(seed, (uint32_t)tags + i));
            s.note(metas, tags);
            std::vector<uint32_t> dp = {0, n / 3, n / 2, n}, st(n);
            std::vector<uint64_t> tag(n), fw(n);
            std::vector<srt_inbound_late> next;
            for (uint32_t i = 0; i < n; ++i) {
                tag[i] = tags + (i * 5 + 1) % n;  // 5 and n coprime for n in 3 .. 8 but 5: then a repeat, harmless
                const uint64_t r = rnd(seed) % 4;
                st[i] = r == 0 ? QUEUED : r == 1 ? (QUEUED | SRT_PDS_ROUTER_DROPPED) : FWD;
                fw[i] = 100 * round + i;
                const uint32_t h = i < dp[1] ? 0 : i < dp[2] ? 1 : 2;
                if (st[i] == QUEUED) next.push_back(srt_inbound_late{seq + i, (uint64_t)100 * round + 50, FWD, h});
            }
            if (round == 5) late.push_back(srt_inbound_late{seq + n + 9, 1, FWD, 1});  // a seq from the future
            if (round == 7) late.push_back(srt_inbound_late{3, 1, FWD, 7});            // a host that does not exist
            s.run(dp, n, tag, st, fw, seq, late, n + late.size());
            late = next;
            tags += n, seq += n;
        }
    }
    {  // no hosts, no rings, the smallest table; n_pkts past the window and dst_ptr past n_pkts
        Stage s0(0, 2, 0, 0);
        s0.run({0}, 0, {}, {}, {}, 0, {srt_inbound_late{0, 1, FWD, 0}}, 0);
        Stage s(2, 2, 4, 4);
        s.assoc = {srt_assoc{1, SRT_PROTO_TCP, 0, 80, 0, 9}};
        s.build();
        s.note({rand_meta(seed, 0), rand_meta(seed, 1), rand_meta(seed, 2), rand_meta(seed, 3)}, 0);
        Out o = s.run({0, 1, 2}, 4, {0, 1, 2, 3}, {FWD, FWD, FWD, FWD}, {1, 2, 3, 4}, 0, {}, 2);
        CHECK(o.tag.size() == 2);
        o = s.run({0, 3, 9}, 4, {0, 1, 2, 3}, {FWD, QUEUED, FWD, FWD}, {1, 2, 3, 4}, 4, {}, 3);
        CHECK(o.tag.size() == 3 && o.host_ptr[1] == 2);
    }
    std::printf("deliver_check: clean\n");
    return 0;
}
