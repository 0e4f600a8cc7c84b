// srt_deliver.hip -- the interface's receive stage behind the inbound router:
// from one srt_inbound_run call's results (status and forward_ns per window
// packet, the late list) to the per-host delivery list, every packet with the
// socket its host's associations give it (networkinterface_push).  The step --
// which packets, their order, the lookup, the ring and log rules, the range
// checks -- is srt_deliver_step.h, compiled here for the device and for the
// host-only instance alike.  No global sort: only a host's late run is ordered.
//
// Device form, on the plan's stream, never waiting for the device.
// Note, one launch: a copy of the round's metas into the ring.
// Run, five launches (three without a late list):
//   (1) count: a group of L lanes owns one destination host and walks its
//       segment of d_status with coalesced loads; the forwarded packets are
//       counted across the group's lanes and the count stored, every host's,
//       with its two late counters zeroed, so the scratch needs no reset.  L is
//       64 (a wave a host) when the batch averages more than 16 packets a host,
//       else 8 (eight hosts a wave).  A packet that stays queued has its tag
//       and meta written to the seq log here;
//   (2) late: one thread a late record (grid-stride), an atomic on the host's
//       late count;
//   (3) scan: one workgroup; each thread sums a contiguous chunk of the hosts'
//       counts (late + batch), the sums are scanned across the workgroup, the
//       chunk's bases stored clamped to out_cap;
//   (4) scatter: the groups of (1) walk again; a forwarded packet's place is
//       base + late count + its rank among the forwarded packets before it, a
//       ballot prefix carried along the walk.  The meta comes from the note
//       ring by tag, the lookup is one or two probes of 16 bytes, the record
//       is five stores.  In further workgroups one thread a late record takes
//       a place in its host's late run with a returning atomic and leaves its
//       index there;
//   (5) late order: one single-wave workgroup a host with late records ranks
//       the run's seqs against LDS chunks of SORT_CAP keys (one chunk for a
//       run that fits: quadratic in the run's length, exact, no host), writes
//       the indices at their ranks, then emits each record in place: the log
//       read, the lookup, the five stores.
// No kernel of a run adds to one address from every wave: a host's packets that
// no socket took are counted into its own scratch word (the batch count's, free
// after the scan), and srt_deliver_status, which synchronises anyway, sums the
// words with one more launch.  (One atomic a wave on a call-wide counter
// measured 144 us for the scatter of 1M packets and 136 us for the late order
// of 500k: 10k dependent atomics on one address.)
// Lookup alone (srt_deliver_lookup_flat), one launch: one thread a (host, meta)
// record over the same probe, for the SRT_OUT_LOCAL packets of an outbound
// call, which never reach the inbound stage.  The loopback interface's stage
// (srt_loopback.hip) takes an instance's table through srt::deliver_table,
// the upload path of the run.
// Every value is written with ordinary stores from plain C++.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <tuple>
#include <vector>

#include "srt_internal.h"
#include "srt_deliver_step.h"
#include "srt_stage.h"

namespace {

static_assert(sizeof(srt_rx_meta) == 16 && sizeof(srt_assoc) == 20 && sizeof(deliver::Slot) == 16 &&
                  sizeof(deliver::LogRec) == 32 && sizeof(deliver::State) == 24 && sizeof(srt_inbound_late) == 24,
              "record layouts");

using stage::BT;
using stage::ST;
using stage::set_err;
constexpr uint32_t DL_CAP = deliver::SORT_CAP;
constexpr uint32_t ORDER_BLOCKS = 1u << 20;  // at most, each striding over the hosts

__global__ __launch_bounds__(BT) void deliver_note_kernel(const deliver::Ctx c) {
    for (uint64_t i = (uint64_t)c.note_first + (uint64_t)blockIdx.x * BT + threadIdx.x; i < c.note_n;
         i += (uint64_t)gridDim.x * BT)
        deliver::note_store(c, (uint32_t)i);
}

template <uint32_t L>
__global__ __launch_bounds__(BT) void deliver_count_kernel(const deliver::Ctx c) {
    const stage::Group<L> G(c.n_hosts);
    uint32_t n = 0;
    if (G.own()) {
        const uint32_t lim = deliver::walked(c);
        uint32_t b, e;
        deliver::segment(c, lim, (uint32_t)G.g, b, e);
        for (uint32_t i = b + G.l; i < e; i += L) {
            const uint32_t st = c.status[i];
            if (deliver::forwarded(st)) ++n;
            else deliver::log_keep(c, lim, i, st);
        }
    }
    // every lane is here: the group's lanes hold its partial counts (written out: through stage::group_add
    // the three stores below are scheduled in another order)
    for (uint32_t off = L / 2; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (G.own() && G.l == 0) {
        c.cnt[G.g] = n;
        c.nlate[G.g] = 0;
        c.lfill[G.g] = 0;
    }
}

__global__ __launch_bounds__(BT) void deliver_late_kernel(const deliver::Ctx c) {
    for (uint64_t k : stage::grid_stride(deliver::late_n(c))) deliver::count_late(c, (uint32_t)k);
}

__global__ __launch_bounds__(ST) void deliver_scan_kernel(const deliver::Ctx c) {
    stage::scan_hosts<ST>(
        c.n_hosts, [&](uint32_t h) { return (uint64_t)c.cnt[h] + c.nlate[h]; },
        [&](uint32_t h, uint64_t run) {
            c.out_host_ptr[h] = deliver::host_base(c, run);
            return (uint64_t)c.cnt[h] + c.nlate[h];
        },
        [&](uint64_t total) { deliver::scan_end(c, total); });
}

template <uint32_t L>
__global__ __launch_bounds__(BT) void deliver_scatter_kernel(const deliver::Ctx c, uint32_t host_blocks) {
    if (blockIdx.x < host_blocks) {
        const stage::Group<L> G(c.n_hosts);
        const uint32_t l = G.l, lane = threadIdx.x & 63;
        const uint32_t shift = lane & ~(L - 1);  // the group's first lane in the wave's ballot
        uint64_t gmask = ~0ull;
        if constexpr (L < 64) gmask = ((1ull << L) - 1ull) << shift;
        uint32_t b = 0, e = 0, h = 0;
        uint64_t pos = 0;
        if (G.own()) {
            h = (uint32_t)G.g;
            deliver::segment(c, deliver::walked(c), h, b, e);
            pos = (uint64_t)c.out_host_ptr[h] + c.nlate[h];
        }
        uint32_t miss = 0;
        // every lane of the wave takes every step: the ballots are over the whole wave
        for (uint32_t i = b + l; __any(i < e); i += L) {
            const bool fw = i < e && deliver::forwarded(c.status[i]);
            const uint64_t m = __ballot(fw) & gmask;
            if (fw) miss += deliver::emit_batch(c, h, i, pos + (uint64_t)__popcll(m & ((1ull << lane) - 1ull)));
            pos += (uint64_t)__popcll(m);
        }
        for (uint32_t off = L / 2; off > 0; off >>= 1) miss += __shfl_xor(miss, off);  // written out, as in the count
        if (G.own() && l == 0) c.cnt[h] = miss;  // the batch count has been scanned: the word is free
    } else {
        const uint32_t n = deliver::late_n(c);
        const uint64_t stride = (uint64_t)(gridDim.x - host_blocks) * BT;
        for (uint64_t k = (uint64_t)(blockIdx.x - host_blocks) * BT + threadIdx.x; k < n; k += stride)
            deliver::place_late(c, (uint32_t)k);
    }
}

__global__ __launch_bounds__(64) void deliver_order_kernel(const deliver::Ctx c) {
    __shared__ uint64_t ks[DL_CAP];
    const uint32_t t = threadIdx.x;
    const uint32_t n_late = deliver::late_n(c);
    for (uint64_t h64 = blockIdx.x; h64 < c.n_hosts; h64 += gridDim.x) {
        const uint32_t h = (uint32_t)h64;
        uint64_t b;
        const uint32_t m = deliver::late_run(c, h, b);  // the same in every lane
        if (!m) continue;
        // the run's indices 64 at a time against every chunk of DL_CAP seqs; the index goes to its rank
        // in out_socket (out_user still holds the run in placing order for the lanes that rank later)
        for (uint32_t i0 = 0; i0 < m; i0 += 64) {
            const uint32_t i = i0 + t;
            const bool has = i < m;
            const uint32_t mine = has ? c.out_user[b + i] : 0u;
            const uint64_t key = has ? deliver::late_seq(c, mine, n_late) : 0ull;
            uint32_t r = 0;
            for (uint32_t j0 = 0; j0 < m; j0 += DL_CAP) {
                const uint32_t mj = m - j0 < DL_CAP ? m - j0 : DL_CAP;
                __syncthreads();  // the previous chunk has been read
                for (uint32_t j = t; j < mj; j += 64) ks[j] = deliver::late_seq(c, c.out_user[b + j0 + j], n_late);
                __syncthreads();
                if (has)
                    for (uint32_t j = 0; j < mj; ++j) r += (ks[j] < key) | ((ks[j] == key) & (j0 + j < i));
            }
            if (has) c.out_socket[b + r] = mine;  // r < m: inside the run
        }
        __threadfence_block();
        __syncthreads();  // every rank of the run is written
        uint32_t miss = 0;
        for (uint32_t j = t; j < m; j += 64) miss += deliver::emit_late(c, h, b + j, c.out_socket[b + j], n_late);
        miss = stage::group_add<64>(miss);
        if (t == 0) c.cnt[h] += miss;  // this workgroup alone has host h now
        __syncthreads();  // LDS reused by the next host
    }
}

// srt_deliver_status: the hosts' counts of packets no socket took, summed by one workgroup
__global__ __launch_bounds__(ST) void deliver_sum_kernel(const deliver::Ctx c) {
    __shared__ uint64_t wsum[ST / 64];
    const uint32_t t = threadIdx.x;
    uint64_t sum = 0;
    for (uint32_t h = t; h < c.n_hosts; h += ST) sum += c.cnt[h];
    for (uint32_t off = 32; off > 0; off >>= 1) sum += __shfl_xor((unsigned long long)sum, off);
    if ((t & 63) == 0) wsum[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        uint64_t all = 0;
        for (uint32_t w = 0; w < ST / 64; ++w) all += wsum[w];
        c.st->n_no_socket = all;
    }
}

// srt_deliver_lookup_flat: one thread a record over the stage's own lookup
__global__ __launch_bounds__(BT) void deliver_lookup_kernel(const deliver::Slot *__restrict__ table, uint32_t mask,
                                                            uint32_t n_hosts, const uint32_t *__restrict__ hosts,
                                                            const srt_rx_meta *__restrict__ meta, uint32_t n,
                                                            uint32_t *__restrict__ sockets) {
    const uint64_t k = (uint64_t)blockIdx.x * BT + threadIdx.x;
    if (k >= n) return;
    const uint32_t h = hosts[k];
    sockets[k] = h < n_hosts ? deliver::lookup(table, mask, h, meta[k]) : deliver::NO_SOCKET;
}

// (host, protocol, local port, peer ip, peer port)
using Key = std::tuple<uint32_t, uint32_t, uint16_t, uint32_t, uint16_t>;
Key key_of(const srt_assoc &a) { return Key(a.host, a.protocol, a.local_port_be, a.peer_ip_be, a.peer_port_be); }

}  // namespace

struct srt_deliver {
    srt_plan *plan = nullptr;  // nullptr: host-only
    uint32_t n_hosts = 0;
    uint64_t note_cap = 0, log_cap = 0;
    uint64_t note_end = 0;
    bool ran = false;  // a run has been enqueued: the hosts' counts hold its packets that no socket took
    std::map<Key, uint32_t> assoc;  // the authoritative table
    std::vector<deliver::Slot> h_table;  // the flat table as the next run sees it
    uint32_t slots = 0, max_probe = 0, wrapped = 0;
    bool stale = true;      // h_table is older than assoc
    bool uploaded = false;  // the device copy equals h_table
    uint32_t d_slots = 0;   // slots the device copy and the pinned copy have room for
    deliver::Slot *d_table = nullptr, *pin = nullptr;
    hipEvent_t up_done = nullptr;
    void *mem = nullptr;  // device form: state, counts, ring, log in one allocation; host-only: h_mem
    std::vector<uint64_t> h_mem;
    deliver::Ctx base;
};

namespace {

// h_table from assoc: slots doubles while the load is above 1/2
bool rebuild(srt_deliver *dl) {
    if (!dl->stale) return true;
    while ((uint64_t)dl->slots < 2 * (uint64_t)dl->assoc.size()) dl->slots *= 2;
    try {
        std::vector<srt_assoc> flat;
        flat.reserve(dl->assoc.size());
        for (const auto &kv : dl->assoc)
            flat.push_back(srt_assoc{std::get<0>(kv.first), std::get<1>(kv.first), std::get<3>(kv.first),
                                     std::get<2>(kv.first), std::get<4>(kv.first), kv.second});
        dl->h_table.resize(dl->slots);
        deliver::table_build(dl->h_table.data(), dl->slots, flat.data(), flat.size(), &dl->max_probe, &dl->wrapped);
    } catch (const std::bad_alloc &) {
        return false;
    }
    dl->stale = false;
    dl->uploaded = false;
    return true;
}

// the device copy follows h_table, on the stream
srt_status upload(srt_deliver *dl, srt_err *err) {
    if (!rebuild(dl)) {
        set_err(err, SRT_ERR_OOM, "deliver: host allocation failed");
        return SRT_ERR_OOM;
    }
    if (!dl->plan || dl->uploaded) return SRT_OK;
    hipStream_t s = dl->plan->stream;
    bool ok = true;
    if (dl->d_slots < dl->slots) {  // the table has doubled: the one place a run waits for the stream
        ok = hipStreamSynchronize(s) == hipSuccess;
        (void)hipFree(dl->d_table);
        (void)hipHostFree(dl->pin);
        dl->d_table = dl->pin = nullptr;
        dl->d_slots = 0;
        ok = ok && hipMalloc(&dl->d_table, (size_t)dl->slots * 16) == hipSuccess &&
             hipHostMalloc(&dl->pin, (size_t)dl->slots * 16) == hipSuccess;
        if (ok) dl->d_slots = dl->slots;
    } else {
        ok = hipEventSynchronize(dl->up_done) == hipSuccess;  // the previous upload has left the pinned copy
    }
    if (ok) {
        std::memcpy(dl->pin, dl->h_table.data(), (size_t)dl->slots * 16);
        ok = hipMemcpyAsync(dl->d_table, dl->pin, (size_t)dl->slots * 16, hipMemcpyHostToDevice, s) == hipSuccess &&
             hipEventRecord(dl->up_done, s) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        set_err(err, SRT_ERR_HIP, "deliver: table upload failed");
        return SRT_ERR_HIP;
    }
    dl->uploaded = true;
    return SRT_OK;
}

}  // namespace

namespace srt {
// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_deliver() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&deliver_scan_kernel));
}

// the table for a launch of another stage on the same stream (srt_loopback_run)
srt_status deliver_table(srt_deliver *dl, srt_plan **plan, uint32_t *n_hosts, const deliver::Slot **table,
                         uint32_t *mask, srt_err *err) {
    *plan = dl->plan;
    *n_hosts = dl->n_hosts;
    if (dl->plan && !stage::use_device(dl->plan)) return SRT_ERR_HIP;
    const srt_status up = upload(dl, err);
    if (up != SRT_OK) return up;
    *table = dl->plan ? dl->d_table : dl->h_table.data();
    *mask = dl->slots - 1;
    return SRT_OK;
}
}  // namespace srt

extern "C" void srt_deliver_destroy(srt_deliver *dl) {
    if (!dl) return;
    if (dl->plan) {
        (void)stage::use_device(dl->plan);
        (void)hipStreamSynchronize(dl->plan->stream);
        (void)hipFree(dl->mem);
        (void)hipFree(dl->d_table);
        (void)hipHostFree(dl->pin);
        if (dl->up_done) (void)hipEventDestroy(dl->up_done);
    }
    delete dl;
}

extern "C" srt_status srt_deliver_create(srt_plan *plan, uint32_t n_hosts, uint32_t table_slots_min, uint64_t note_cap,
                                         uint64_t log_cap, srt_deliver **out, srt_err *err) {
    stage::begin(err);
    if (!out) return stage::null_argument(err);
    *out = nullptr;
    if (n_hosts == 0xffffffffu || table_slots_min > (1u << 30) || note_cap > (1ull << 31) || log_cap > (1ull << 31)) {
        set_err(err, SRT_ERR_INVALID,
                "deliver: n_hosts, table_slots_min (at most 2^30), note_cap or log_cap (at most 2^31) out of range");
        return SRT_ERR_INVALID;
    }
    srt_deliver *dl = new (std::nothrow) srt_deliver;
    if (!dl) return SRT_ERR_OOM;
    dl->plan = plan;
    dl->n_hosts = n_hosts;
    dl->note_cap = note_cap;
    dl->log_cap = log_cap;
    dl->slots = 2;
    while (dl->slots < table_slots_min) dl->slots *= 2;
    // state, the ring, the log, then the hosts' three counts
    const size_t head = 32, bytes = head + 16 * (size_t)note_cap + 32 * (size_t)log_cap + 12 * (size_t)n_hosts;
    bool ok = rebuild(dl);
    if (ok && !plan) {
        try {
            dl->h_mem.assign(bytes / 8 + 1, 0);
        } catch (const std::bad_alloc &) {
            ok = false;
        }
        dl->mem = dl->h_mem.data();
    } else if (ok) {
        srt::init_wait();
        ok = stage::use_device(plan);
        ok = ok && hipMalloc(&dl->mem, bytes + 8) == hipSuccess;
        ok = ok && hipMemset(dl->mem, 0, bytes + 8) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&dl->up_done, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            (void)hipFree(dl->mem);
            if (dl->up_done) (void)hipEventDestroy(dl->up_done);
        }
    }
    if (!ok) {
        delete dl;
        set_err(err, SRT_ERR_OOM, "deliver: allocation failed");
        return SRT_ERR_OOM;
    }
    deliver::Ctx &c = dl->base;
    std::memset(&c, 0, sizeof c);
    char *p = static_cast<char *>(dl->mem);
    c.st = reinterpret_cast<deliver::State *>(p);
    c.ring = reinterpret_cast<srt_rx_meta *>(p + head);
    c.log = reinterpret_cast<deliver::LogRec *>(p + head + 16 * (size_t)note_cap);
    c.cnt = reinterpret_cast<uint32_t *>(p + head + 16 * (size_t)note_cap + 32 * (size_t)log_cap);
    c.nlate = c.cnt + n_hosts;
    c.lfill = c.nlate + n_hosts;
    c.n_hosts = n_hosts;
    c.note_cap = note_cap;
    c.log_cap = log_cap;
    *out = dl;
    return SRT_OK;
}

extern "C" srt_status srt_deliver_associate(srt_deliver *dl, const srt_assoc *assoc, uint64_t n, srt_err *err) {
    stage::begin(err);
    if (!dl || (n && !assoc)) return stage::null_argument(err);
    try {
        // nothing changes unless the whole batch can go in
        std::vector<Key> keys;
        keys.reserve(n);
        for (uint64_t k = 0; k < n; ++k) {
            const srt_assoc &a = assoc[k];
            if (a.host >= dl->n_hosts || a.socket >= 0x80000000u ||
                (a.protocol != SRT_PROTO_TCP && a.protocol != SRT_PROTO_UDP)) {
                set_err(err, SRT_ERR_INVALID, "deliver: an association's host, socket (below 2^31) or protocol is out of range");
                return SRT_ERR_INVALID;
            }
            keys.push_back(key_of(a));
        }
        std::vector<Key> sorted = keys;
        std::sort(sorted.begin(), sorted.end());
        bool dup = std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
        for (uint64_t k = 0; k < n && !dup; ++k) dup = dl->assoc.count(keys[k]) != 0;
        if (dup) {
            set_err(err, SRT_ERR_INVALID, "deliver: an association's key exists already (nothing was added)");
            return SRT_ERR_INVALID;
        }
        for (uint64_t k = 0; k < n; ++k) dl->assoc.emplace(keys[k], assoc[k].socket);
    } catch (const std::bad_alloc &) {
        set_err(err, SRT_ERR_OOM, "deliver: host allocation failed");
        return SRT_ERR_OOM;
    }
    if (n) dl->stale = true;
    return SRT_OK;
}

extern "C" srt_status srt_deliver_disassociate(srt_deliver *dl, const srt_assoc *assoc, uint64_t n, srt_err *err) {
    stage::begin(err);
    if (!dl || (n && !assoc)) return stage::null_argument(err);
    for (uint64_t k = 0; k < n; ++k)
        if (dl->assoc.erase(key_of(assoc[k]))) dl->stale = true;
    return SRT_OK;
}

extern "C" srt_status srt_deliver_lookup(srt_deliver *dl, const uint32_t *hosts, const srt_rx_meta *meta, uint64_t n,
                                         uint32_t *sockets, srt_err *err) {
    stage::begin(err);
    if (!dl || (n && (!hosts || !meta || !sockets))) return stage::null_argument(err);
    if (!rebuild(dl)) {
        set_err(err, SRT_ERR_OOM, "deliver: host allocation failed");
        return SRT_ERR_OOM;
    }
    for (uint64_t k = 0; k < n; ++k) sockets[k] = deliver::lookup(dl->h_table.data(), dl->slots - 1, hosts[k], meta[k]);
    return SRT_OK;
}

extern "C" srt_status srt_deliver_lookup_flat(srt_deliver *dl, const uint32_t *d_hosts, const srt_rx_meta *d_meta,
                                              uint64_t n, uint32_t *d_sockets, srt_err *err) {
    if (!dl || !dl->plan) return srt_deliver_lookup(dl, d_hosts, d_meta, n, d_sockets, err);
    stage::begin(err);
    if (n && (!d_hosts || !d_meta || !d_sockets)) return stage::null_argument(err);
    if (n >= 0x80000000ull) {
        set_err(err, SRT_ERR_INVALID, "more than 2^31-1 records in one call");
        return SRT_ERR_INVALID;
    }
    if (!stage::use_device(dl->plan)) return SRT_ERR_HIP;
    const srt_status up = upload(dl, err);
    if (up != SRT_OK || !n) return up;
    hipLaunchKernelGGL(deliver_lookup_kernel, dim3((uint32_t)((n + BT - 1) / BT)), dim3(BT), 0, dl->plan->stream,
                       dl->d_table, dl->slots - 1, dl->n_hosts, d_hosts, d_meta, (uint32_t)n, d_sockets);
    return stage::launched(err, "deliver");
}

extern "C" srt_status srt_deliver_table_stats(srt_deliver *dl, uint64_t *n_assoc, uint32_t *n_slots,
                                              uint32_t *max_probe, uint32_t *wrapped, srt_err *err) {
    stage::begin(err);
    if (!dl) return stage::null_argument(err);
    if (!rebuild(dl)) {
        set_err(err, SRT_ERR_OOM, "deliver: host allocation failed");
        return SRT_ERR_OOM;
    }
    if (n_assoc) *n_assoc = dl->assoc.size();
    if (n_slots) *n_slots = dl->slots;
    if (max_probe) *max_probe = dl->max_probe;
    if (wrapped) *wrapped = dl->wrapped;
    return SRT_OK;
}

extern "C" srt_status srt_deliver_note(srt_deliver *dl, const srt_rx_meta *d_meta, uint64_t n_pkts, uint64_t tag_base,
                                       srt_err *err) {
    stage::begin(err);
    if (!dl || (n_pkts && !d_meta)) return stage::null_argument(err);
    if (n_pkts >= 0x80000000ull || tag_base < dl->note_end || tag_base + n_pkts < tag_base) {
        set_err(err, SRT_ERR_INVALID, "deliver: more than 2^31-1 packets in one note, or tag_base below the previous note's end");
        return SRT_ERR_INVALID;
    }
    dl->note_end = tag_base + n_pkts;
    if (!n_pkts || !dl->note_cap) return SRT_OK;
    deliver::Ctx c = dl->base;
    c.note_in = d_meta;
    c.note_n = (uint32_t)n_pkts;
    c.note_first = n_pkts > dl->note_cap ? (uint32_t)(n_pkts - dl->note_cap) : 0u;
    c.note_first_mod = (tag_base + c.note_first) % dl->note_cap;
    if (!dl->plan) {
        deliver::host_note(c);
        return SRT_OK;
    }
    if (!stage::use_device(dl->plan)) return SRT_ERR_HIP;
    hipLaunchKernelGGL(deliver_note_kernel, dim3(stage::strided_blocks(n_pkts - c.note_first, stage::NOTE_BLOCKS)),
                       dim3(BT), 0, dl->plan->stream, c);
    return stage::launched(err, "deliver");
}

extern "C" srt_status srt_deliver_run(srt_deliver *dl, const uint32_t *d_dst_ptr, uint64_t n_pkts,
                                      const uint64_t *d_tag, const uint32_t *d_status, const uint64_t *d_forward_ns,
                                      uint64_t seq_base, const srt_inbound_late *d_late, uint32_t late_cap,
                                      const uint32_t *d_late_count, uint32_t *d_out_host_ptr, uint32_t *d_out_socket,
                                      uint64_t *d_out_forward_ns, uint64_t *d_out_tag, uint32_t *d_out_user,
                                      uint32_t *d_out_status, uint64_t out_cap, srt_err *err) {
    stage::begin(err);
    if (!dl || !d_dst_ptr || !d_out_host_ptr || (n_pkts && (!d_tag || !d_status || !d_forward_ns)) ||
        (late_cap && (!d_late || !d_late_count)) ||
        (out_cap && (!d_out_socket || !d_out_forward_ns || !d_out_tag || !d_out_user || !d_out_status)))
        return stage::null_argument(err);
    if (n_pkts >= 0x80000000ull || late_cap >= 0x80000000u) {
        set_err(err, SRT_ERR_INVALID, "more than 2^31-1 packets in one batch or late list");
        return SRT_ERR_INVALID;
    }
    if (dl->plan && !stage::use_device(dl->plan)) return SRT_ERR_HIP;
    const srt_status up = upload(dl, err);
    if (up != SRT_OK) return up;
    deliver::Ctx c = dl->base;
    c.table = dl->plan ? dl->d_table : dl->h_table.data();
    c.mask = dl->slots - 1;
    c.note_end = dl->note_end;
    c.note_end_mod = dl->note_cap ? dl->note_end % dl->note_cap : 0;
    c.base_mod = dl->log_cap ? seq_base % dl->log_cap : 0;
    c.end_mod = dl->log_cap ? (seq_base + n_pkts) % dl->log_cap : 0;
    c.dst_ptr = d_dst_ptr;
    c.status = d_status;
    c.tag = d_tag;
    c.forward_ns = d_forward_ns;
    c.late = d_late;
    c.late_count = late_cap ? d_late_count : nullptr;
    c.late_cap = late_cap;
    c.seq_base = seq_base;
    c.n_pkts = (uint32_t)n_pkts;
    c.out_cap = out_cap < 0xffffffffull ? out_cap : 0xffffffffull;  // positions are u32
    c.out_host_ptr = d_out_host_ptr;
    c.out_socket = d_out_socket;
    c.out_forward_ns = d_out_forward_ns;
    c.out_tag = d_out_tag;
    c.out_user = d_out_user;
    c.out_status = d_out_status;
    if (!dl->plan) {
        try {
            deliver::host_run(c);
        } catch (const std::bad_alloc &) {
            set_err(err, SRT_ERR_OOM, "deliver: host allocation failed");
            return SRT_ERR_OOM;
        }
        return SRT_OK;
    }
    hipStream_t s = dl->plan->stream;
    dl->ran = true;
    const bool wide = stage::wide(n_pkts, c.n_hosts);
    const uint32_t host_blocks = stage::host_blocks(c.n_hosts, wide);
    const uint32_t late_blocks = stage::strided_blocks(late_cap, stage::LATE_BLOCKS);
    if (host_blocks)
        stage::launch_grouped(deliver_count_kernel<64>, deliver_count_kernel<8>, wide, host_blocks, BT, s, c);
    if (late_blocks) hipLaunchKernelGGL(deliver_late_kernel, dim3(late_blocks), dim3(BT), 0, s, c);
    hipLaunchKernelGGL(deliver_scan_kernel, dim3(1), dim3(ST), 0, s, c);
    if (host_blocks) {
        stage::launch_grouped(deliver_scatter_kernel<64>, deliver_scatter_kernel<8>, wide,
                              host_blocks + late_blocks, BT, s, c, host_blocks);
        if (late_blocks)
            hipLaunchKernelGGL(deliver_order_kernel, dim3(std::min(c.n_hosts, ORDER_BLOCKS)), dim3(64), 0, s, c);
    }
    return stage::launched(err, "deliver");
}

extern "C" srt_status srt_deliver_status(srt_deliver *dl, uint32_t *flags, uint64_t *n_delivered,
                                         uint64_t *n_no_socket, srt_err *err) {
    stage::begin(err);
    if (!dl) return stage::null_argument(err);
    deliver::State w;
    if (!dl->plan) {
        w = *dl->base.st;
        dl->base.st->flags = 0;
    } else {
        if (!stage::use_device(dl->plan)) return SRT_ERR_HIP;
        if (dl->ran && dl->n_hosts)
            hipLaunchKernelGGL(deliver_sum_kernel, dim3(1), dim3(ST), 0, dl->plan->stream, dl->base);
        const srt_status st = stage::read_status(dl->plan, &w, dl->base.st, sizeof w, err, "deliver");
        if (st != SRT_OK) return st;
    }
    const uint32_t f = w.flags & 15u;
    if (flags) *flags = f;
    if (n_delivered) *n_delivered = w.n_delivered;
    if (n_no_socket) *n_no_socket = w.n_no_socket;
    if (!f) return SRT_OK;
    if (err) {
        err->code = SRT_ERR_INVALID;
        std::snprintf(err->msg, sizeof err->msg, "deliver:%s%s%s%s",
                      f & deliver::F_OUT_OVERFLOW ? " more delivered packets than out_cap (nothing past it written);" : "",
                      f & deliver::F_LOG_OVERRUN ? " a late packet's seq is older than the log holds;" : "",
                      f & deliver::F_NOTE_OVERRUN ? " a tag the note ring does not hold;" : "",
                      f & deliver::F_BAD_HOST ? " a late record's dst_host is not below n_hosts (skipped);" : "");
    }
    return SRT_ERR_INVALID;
}
