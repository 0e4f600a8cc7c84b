// flight_check.cpp -- the in-flight store's step (shadow_amd/csrc/srt_flight_step.h) alone, on host
// arrays allocated at exactly the sizes include/srt.h promises, at the sizes where the step takes
// another path.  A stand-alone program: built for the host with -fsanitize=address,undefined and run
// directly (tests/test_flight_cpu.py), so a write one past the pool, the stage or a window array is a
// sanitizer report.  Every window is also checked against a sort of plain tuples.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <tuple>
#include <vector>

#include "../../shadow_amd/csrc/srt_flight_step.h"

namespace {

constexpr uint32_t SENT = SRT_PDS_INET_SENT;
constexpr uint32_t G = 256;  // FL_CAP of srt_flight.hip

#define CHECK(x)                                                          \
    do {                                                                  \
        if (!(x)) {                                                       \
            std::printf("flight_check: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

template <class T>
std::unique_ptr<T[]> arr(size_t n) {
    return std::unique_ptr<T[]>(new T[n]());  // exactly n: one past it is a report
}

struct Rec {
    uint64_t deliver, event_id, tag;
    uint32_t src, dst, size;
};

struct Store {
    flight::State st{};
    std::unique_ptr<uint64_t[]> deliver, event_id, tag;
    std::unique_ptr<uint32_t[]> src, dst, size, cnt, slot;
    std::unique_ptr<flight::Rec[]> stage;
    flight::Ctx base{};
    uint64_t last_until = 0, tag_next = 0;
    std::vector<Rec> model;  // what the store must hold

    Store(uint32_t n_dst, uint64_t cap)
        : deliver(arr<uint64_t>(2 * cap)), event_id(arr<uint64_t>(2 * cap)), tag(arr<uint64_t>(2 * cap)),
          src(arr<uint32_t>(2 * cap)), dst(arr<uint32_t>(2 * cap)), size(arr<uint32_t>(2 * cap)),
          cnt(arr<uint32_t>(n_dst)), slot(arr<uint32_t>(cap)), stage(arr<flight::Rec>(cap)) {
        base.st = &st;
        base.pool = flight::Pool{deliver.get(), event_id.get(), tag.get(), src.get(), dst.get(), size.get()};
        base.cnt = cnt.get(), base.slot = slot.get(), base.stage = stage.get();
        base.pool_cap = cap, base.n_dst = n_dst;
    }

    // one push: host_ptr has n_src + 1 entries, the packet arrays exactly n
    void push(const std::vector<uint32_t> &host_ptr, const std::vector<uint32_t> &flags,
              const std::vector<uint64_t> &dl, const std::vector<uint32_t> &ds, const std::vector<uint64_t> &ei,
              const std::vector<uint32_t> &sz) {
        const size_t n = flags.size();
        auto hp = arr<uint32_t>(host_ptr.size());
        auto f = arr<uint32_t>(n), d = arr<uint32_t>(n), s = arr<uint32_t>(n);
        auto t = arr<uint64_t>(n), e = arr<uint64_t>(n);
        std::copy(host_ptr.begin(), host_ptr.end(), hp.get());
        std::copy(flags.begin(), flags.end(), f.get());
        std::copy(dl.begin(), dl.end(), t.get());
        std::copy(ds.begin(), ds.end(), d.get());
        std::copy(ei.begin(), ei.end(), e.get());
        std::copy(sz.begin(), sz.end(), s.get());
        flight::Ctx c = base;
        c.host_ptr = hp.get(), c.flags_in = f.get(), c.deliver_in = t.get(), c.dst_in = d.get();
        c.event_id_in = e.get(), c.size_in = s.get(), c.tag_in = nullptr;
        c.tag_base = tag_next, c.last_until = last_until;
        c.n_src = (uint32_t)host_ptr.size() - 1, c.n_pkts = (uint32_t)n;
        flight::host_push(c);
        for (uint32_t h = 0; h + 1 < host_ptr.size(); ++h)
            for (uint32_t i = host_ptr[h]; i < host_ptr[h + 1] && i < n; ++i)
                if (flags[i] == SENT && ds[i] < base.n_dst && model.size() < base.pool_cap)
                    model.push_back(Rec{dl[i], ei[i], tag_next + i, h, ds[i], sz[i]});
        tag_next += n;
    }

    // one pop into window arrays of exactly out_cap entries; returns the number popped
    uint64_t pop(uint64_t until, uint64_t out_cap) {
        auto order = arr<uint32_t>(out_cap), wsz = arr<uint32_t>(out_cap), wsrc = arr<uint32_t>(out_cap);
        auto wdl = arr<uint64_t>(out_cap), wei = arr<uint64_t>(out_cap), wtag = arr<uint64_t>(out_cap);
        auto dp = arr<uint32_t>((size_t)base.n_dst + 1);
        flight::Ctx c = base;
        c.until = until, c.out_cap = out_cap;
        c.pre_flags = until < last_until ? flight::F_TIME_REGRESSION : 0u;
        c.w_order = order.get(), c.w_dst_ptr = dp.get();
        c.w = flight::Pool{wdl.get(), wei.get(), wtag.get(), wsrc.get(), nullptr, wsz.get()};
        last_until = std::max(last_until, until);
        flight::host_pop(c);
        // the model: the due records as tuples in (dst, deliver, src, event id) order
        std::vector<std::tuple<uint32_t, uint64_t, uint32_t, uint64_t, uint64_t, uint32_t>> due;
        std::vector<Rec> rest;
        for (const Rec &r : model)
            if (r.deliver < until) due.emplace_back(r.dst, r.deliver, r.src, r.event_id, r.tag, r.size);
            else rest.push_back(r);
        CHECK(st.n_popped == due.size());
        if (due.size() > out_cap) {
            CHECK(st.is_void == 1 && (st.flags & flight::F_OUT_OVERFLOW));
            for (uint32_t d = 0; d <= base.n_dst; ++d) CHECK(dp[d] == 0);
            CHECK(flight::stored(base, st.len) == model.size());
            return 0;
        }
        std::sort(due.begin(), due.end());
        model = rest;
        CHECK(dp[base.n_dst] == due.size() && flight::stored(base, st.len) == model.size());
        for (size_t k = 0; k < due.size(); ++k) {
            const auto &[d, t, s, e, g, z] = due[k];
            CHECK(dp[d] <= k && k < dp[d + 1]);
            CHECK(order[k] == k && wdl[k] == t && wsrc[k] == s && wei[k] == e && wtag[k] == g && wsz[k] == z);
        }
        return due.size();
    }
};

uint64_t rnd(uint64_t &s) {  // xorshift64*
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return s * 2685821657736338717ull;
}

// n sent packets over n_src hosts, destinations drawn so that group d gets sizes[d] packets
void fill(Store &st, uint32_t n_src, const std::vector<uint32_t> &sizes, uint64_t t0, uint64_t span, uint64_t &seed,
          uint32_t unsent_every = 0) {
    std::vector<uint32_t> ds;
    for (uint32_t d = 0; d < sizes.size(); ++d) ds.insert(ds.end(), sizes[d], d);
    for (size_t i = ds.size(); i > 1; --i) std::swap(ds[i - 1], ds[rnd(seed) % i]);
    const size_t n = ds.size();
    std::vector<uint32_t> hp(n_src + 1), fl(n, SENT), sz(n);
    std::vector<uint64_t> dl(n), ei(n);
    for (uint32_t h = 0; h <= n_src; ++h) hp[h] = (uint32_t)(n * h / n_src);
    for (size_t i = 0; i < n; ++i) {
        dl[i] = t0 + rnd(seed) % span;
        ei[i] = (1ull << 40) + st.tag_next + i;
        sz[i] = 40 + (uint32_t)(rnd(seed) % 1500);
        if (unsent_every && i % unsent_every == 0) fl[i] = SRT_PDS_INET_DROPPED, ei[i] = ~0ull;
    }
    st.push(hp, fl, dl, ds, ei, sz);
}

}  // namespace

int main() {
    uint64_t seed = 88172645463325252ull;
    {  // destination groups of G - 1, G, G + 1 and 3G + 5 packets, an empty one, tied deliver times
        const std::vector<uint32_t> sizes = {G - 1, 0, G, G + 1, 3 * G + 5};
        const uint32_t n = 6 * G + 5;
        Store s(5, n);
        fill(s, 7, sizes, 1000, 40, seed);
        CHECK(s.pop(500, n) == 0);   // nothing due
        CHECK(s.pop(2000, n) == n);  // everything due, the window arrays exactly full
        CHECK(s.st.flags == 0 && s.st.len == 0);
    }
    {  // three pushes over four windows, survivors compacted from half to half; unsent packets skipped
        Store s(9, 3000);
        fill(s, 13, std::vector<uint32_t>(9, 100), 1000, 400, seed, 7);
        fill(s, 13, std::vector<uint32_t>(9, 110), 1000, 400, seed, 5);
        uint64_t got = s.pop(1100, 3000);
        fill(s, 13, std::vector<uint32_t>(9, 90), 1100, 300, seed, 3);
        for (uint64_t u = 1200; u <= 1400; u += 100) got += s.pop(u, 3000);
        CHECK(got > 2000 && s.model.empty() && s.st.len == 0 && s.st.flags == 0);
    }
    {  // the pool filled to exactly pool_cap, then one more
        Store s(2, 64);
        fill(s, 1, {32, 32}, 10, 5, seed);
        CHECK(s.st.len == 64 && s.st.flags == 0);
        fill(s, 1, {1, 0}, 10, 5, seed);
        CHECK(s.st.flags == flight::F_POOL_OVERFLOW && s.st.n_lost == 1 && flight::stored(s.base, s.st.len) == 64);
        s.st.flags = 0;
        // out_cap equal to the due count, then one short: the void pop leaves the store as it was
        CHECK(s.pop(100, 63) == 0 && s.st.flags == flight::F_OUT_OVERFLOW && s.st.n_popped == 64);
        s.st.flags = 0;
        CHECK(s.pop(100, 64) == 64 && s.st.flags == 0);
        CHECK(s.pop(100, 0) == 0 && s.st.flags == 0);  // nothing stored, no room: not void
    }
    {  // a destination out of range, a late push, a step back in time; host_ptr past the batch
        Store s(2, 8);
        s.push({0, 2, 9}, {SENT, SENT, SENT}, {10, 11, 12}, {0, 2, 0xffffffffu}, {0, 0, 1}, {1, 1, 1});
        CHECK(s.st.flags == flight::F_BAD_HOST && s.st.len == 1);
        s.st.flags = 0;
        CHECK(s.pop(20, 8) == 1);
        s.push({0, 1}, {SENT}, {19}, {1}, {5}, {1});
        CHECK(s.st.flags == flight::F_LATE_PUSH);
        s.st.flags = 0;
        CHECK(s.pop(15, 8) == 0 && s.st.flags == flight::F_TIME_REGRESSION);
        s.st.flags = 0;
        CHECK(s.pop(20, 8) == 1 && s.st.flags == 0);
    }
    {  // no destinations, no pool: every array empty
        Store s(0, 0);
        s.push({0, 1}, {SENT}, {5}, {0}, {0}, {1});
        CHECK(s.st.flags == flight::F_BAD_HOST);
        CHECK(s.pop(9, 0) == 0);
    }
    {  // full-width keys: deliver times above 2^63, event ids above 2^32
        Store s(1, 8);
        const uint64_t hi = 1ull << 63, big = 1ull << 32;
        s.push({0, 5}, std::vector<uint32_t>(5, SENT), {hi + 5, 5, hi + 5, hi + 4, hi + 5}, {0, 0, 0, 0, 0},
               {2 * big + 1, 7, big + 1, 3, big + 2}, {1, 2, 3, 4, 5});
        CHECK(s.pop(hi, 8) == 1 && s.pop(~0ull, 8) == 4);
    }
    std::printf("flight_check: clean\n");
    return 0;
}
