// srt_flight.hip -- the in-flight store: the packets a round's send decision
// marked SENT stay on the device until the window their deliver time falls in
// (srt_flight_push), and each window's set comes out grouped by destination
// host, each group in the event queue's pop order, as the arrays
// srt_inbound_run takes (srt_flight_pop).  The step -- which packets are
// taken, the range checks, the pop order, the words a call leaves -- is
// srt_flight_step.h, compiled here for the device and for the host-only
// instance alike.
//
// Device form, on the plan's stream, never waiting for the device.
// Push, one launch: a group of L lanes owns one source host and walks its
// segment of the batch with coalesced loads, twice: the workgroup first counts
// the packets it will take, reserves their places with ONE atomic on the pool
// length, then stores them (a ballot gives every lane its place).  L is 64 (a
// wave a host) when the batch averages more than 16 packets a host, else 8
// (eight hosts a wave).  (One atomic a wave and step measured 248 us for 1M
// packets: 20k dependent atomics on one address at 12 ns each.)
// Pop, four launches:
//   (1) count: grid-stride over the stored deliver times (8 bytes a packet);
//       a due packet's destination is read and counted with a global atomic,
//       and the count it found is kept as its slot within the destination's
//       run, so that no second pass of atomics is needed;
//   (2) scan: one workgroup; the counts become w_dst_ptr and are zeroed for
//       the next call; the pop is void when the total is over out_cap (every
//       w_dst_ptr entry 0, nothing moves), else the halves swap roles;
//   (3) move: a due packet goes as one 32-byte record to stage[w_dst_ptr[dst]
//       + slot]; the survivors are copied to the other half, one atomic a
//       workgroup and 1,024 records on the new length;
//   (4) sort: one single-wave workgroup a destination loads its run of the
//       stage (contiguous) into LDS -- FL_CAP records, 8 KB -- ranks it by
//       (deliver, source host, event id) and writes each record's fields at
//       its rank.  A longer run is ranked by the same workgroup against LDS
//       chunks of FL_CAP keys: quadratic in the run's length, exact, no host.
//       (Staging pool indices and gathering the records from the pool's
//       arrays in this kernel measured 183 us against the move's 81: six
//       random lines a packet.)
// Every value is written with ordinary stores from plain C++.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "srt_internal.h"
#include "srt_flight_step.h"
#include "srt_stage.h"

namespace {

static_assert(sizeof(flight::State) == 48 && sizeof(flight::Rec) == 32, "state and record layouts");

using stage::BT;  // threads a workgroup of (1) and (3)
using stage::ST;
using stage::set_err;
constexpr uint32_t PT = 1024;        // threads a workgroup of the push: one atomic for 16 or 128 hosts
constexpr uint32_t ITEMS = 4;        // records a thread of (3) moves a step: 1,024 a workgroup
constexpr uint32_t MAX_BLOCKS = 2048;  // of the grid-stride launches
constexpr uint32_t FL_CAP = 256;     // G: the records a destination's run may hold for the one-pass LDS sort
constexpr uint32_t SORT_BLOCKS = 1u << 20;  // at most, each striding over the destinations

template <uint32_t L>
__global__ __launch_bounds__(PT) void flight_push_kernel(const flight::Ctx c) {
    __shared__ uint32_t wtot[PT / 64];
    __shared__ unsigned long long bbase;
    const stage::Group<L, PT> G(c.n_src);
    const uint32_t l = G.l, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t b = 0, e = 0;
    if (G.own()) flight::segment(c, (uint32_t)G.g, b, e);
    const flight::Pool to = flight::half(c, c.st->cur);
    // every lane of the wave takes every step: the ballots are over the whole wave
    uint32_t wcount = 0;
    for (uint32_t i = b + l; __any(i < e); i += L) wcount += (uint32_t)__popcll(__ballot(i < e && flight::push_wants(c, i)));
    if (lane == 0) wtot[wave] = wcount;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < PT / 64; ++w) all += wtot[w];
        bbase = all ? atomicAdd(reinterpret_cast<unsigned long long *>(&c.st->len), (unsigned long long)all) : 0ull;
    }
    __syncthreads();
    uint64_t place = bbase;
    for (uint32_t w = 0; w < wave; ++w) place += wtot[w];
    for (uint32_t i = b + l; __any(i < e); i += L) {
        const bool take = i < e && flight::push_takes(c, i);
        const uint64_t m = __ballot(take);
        const bool lost = take && !flight::push_store(c, to, place + (uint64_t)__popcll(m & ((1ull << lane) - 1ull)),
                                                      (uint32_t)G.g, i);
        place += (uint64_t)__popcll(m);
        const uint64_t lm = __ballot(lost);
        if (lane == 0) flight::push_lost(c, (uint64_t)__popcll(lm));
    }
}

__global__ __launch_bounds__(BT) void flight_count_kernel(const flight::Ctx c) {
    const flight::Pool from = flight::half(c, c.st->cur);
    const uint64_t n = flight::stored(c, c.st->len);
    for (uint64_t i : stage::grid_stride(n))
        if (flight::due(c, from, i)) flight::count_due(c, from, i);
}

__global__ __launch_bounds__(ST) void flight_scan_kernel(const flight::Ctx c) {
    __shared__ uint64_t wsum[ST / 64];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (uint32_t)(((uint64_t)c.n_dst + ST - 1) / ST);  // below 2^22: t * per fits
    const uint64_t b64 = (uint64_t)t * per;
    const uint32_t b = b64 < c.n_dst ? (uint32_t)b64 : c.n_dst;
    const uint32_t e = b64 + per < c.n_dst ? (uint32_t)(b64 + per) : c.n_dst;
    uint64_t sum = 0;
    for (uint32_t d = b; d < e; ++d) sum += c.cnt[d];
    // inclusive scan of the threads' sums: within the wave, then over the waves' totals
    uint64_t inc = sum;
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up((unsigned long long)inc, off);
        if ((t & 63) >= off) inc += o;
    }
    if ((t & 63) == 63) wsum[t >> 6] = inc;
    __syncthreads();
    uint64_t before = 0, total = 0;
    for (uint32_t w = 0; w < ST / 64; ++w) {
        if (w < (t >> 6)) before += wsum[w];
        total += wsum[w];
    }
    const bool is_void = total > c.out_cap;
    uint64_t run = before + inc - sum;
    for (uint32_t d = b; d < e; ++d) {
        const uint32_t n = c.cnt[d];
        c.cnt[d] = 0;
        c.w_dst_ptr[d] = is_void ? 0u : (uint32_t)run;
        run += n;
    }
    if (t == 0) {
        c.w_dst_ptr[c.n_dst] = is_void ? 0u : (uint32_t)total;
        flight::scan_end(c, total);
    }
}

__global__ __launch_bounds__(BT) void flight_move_kernel(const flight::Ctx c) {
    __shared__ uint32_t wtot[BT / 64];
    __shared__ unsigned long long bbase;
    if (c.st->is_void) return;
    const flight::Pool from = flight::half(c, c.st->prev), to = flight::half(c, c.st->cur);
    const uint64_t n = c.st->prev_n;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr uint64_t TILE = (uint64_t)BT * ITEMS;
    // n and the stride are the same in every thread: the barriers are taken by all
    for (uint64_t t0 = (uint64_t)blockIdx.x * TILE; t0 < n; t0 += (uint64_t)gridDim.x * TILE) {
        uint64_t m[ITEMS];
        uint32_t stay = 0, wcount = 0;
#pragma unroll
        for (uint32_t k = 0; k < ITEMS; ++k) {
            const uint64_t i = t0 + (uint64_t)k * BT + threadIdx.x;
            bool s = false;
            if (i < n) {
                if (flight::due(c, from, i)) flight::stage_due(c, from, i);
                else s = true;
            }
            m[k] = __ballot(s);
            stay |= (uint32_t)s << k;
            wcount += (uint32_t)__popcll(m[k]);
        }
        if (lane == 0) wtot[wave] = wcount;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t all = 0;
            for (uint32_t w = 0; w < BT / 64; ++w) all += wtot[w];
            bbase = all ? atomicAdd(reinterpret_cast<unsigned long long *>(&c.st->len), (unsigned long long)all) : 0ull;
        }
        __syncthreads();
        uint64_t place = bbase;
        for (uint32_t w = 0; w < wave; ++w) place += wtot[w];
#pragma unroll
        for (uint32_t k = 0; k < ITEMS; ++k) {
            if (stay >> k & 1u)
                flight::keep(c, from, to, t0 + (uint64_t)k * BT + threadIdx.x,
                             place + (uint64_t)__popcll(m[k] & ((1ull << lane) - 1ull)));
            place += (uint64_t)__popcll(m[k]);
        }
        __syncthreads();  // wtot and bbase are written again by the next step
    }
}

// a run of m <= 64 K records in LDS: lane t ranks elements t, t + 64, ... and writes them out
template <uint32_t K>
__device__ __forceinline__ void rank_small(const flight::Ctx &c, uint64_t b, uint32_t m, const uint64_t *kd,
                                           const uint64_t *ke, const uint64_t *kt, const uint32_t *ks,
                                           const uint32_t *kz) {
    static_assert(K * 64 <= FL_CAP, "the run fits the LDS arrays");
    const uint32_t t = threadIdx.x;
    flight::Key mk[K];
    uint32_t r[K];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t i = t + 64 * k < m ? t + 64 * k : m - 1;  // an idle slot ranks the last element again
        mk[k].deliver = kd[i], mk[k].event_id = ke[i], mk[k].src = ks[i];
        r[k] = 0;
    }
    for (uint32_t j = 0; j < m; ++j) {
        flight::Key o;
        o.deliver = kd[j], o.event_id = ke[j], o.src = ks[j];
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) r[k] += flight::before_at(o, j, mk[k], t + 64 * k);
    }
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t i = t + 64 * k;
        if (i < m) {
            flight::Rec mine;
            mine.deliver = kd[i], mine.event_id = ke[i], mine.tag = kt[i], mine.src = ks[i], mine.size = kz[i];
            flight::emit(c, mine, b + r[k]);
        }
    }
}

__global__ __launch_bounds__(64) void flight_sort_kernel(const flight::Ctx c) {
    __shared__ uint64_t kd[FL_CAP], ke[FL_CAP], kt[FL_CAP];
    __shared__ uint32_t ks[FL_CAP], kz[FL_CAP];
    if (c.st->is_void) return;
    const uint32_t t = threadIdx.x;
    for (uint64_t d64 = blockIdx.x; d64 < c.n_dst; d64 += gridDim.x) {
        const uint32_t d = (uint32_t)d64;
        const uint64_t b = c.w_dst_ptr[d], e = c.w_dst_ptr[d + 1];
        if (e <= b || e > c.pool_cap) continue;  // the same in every lane
        const uint32_t m = (uint32_t)(e - b);
        if (m <= FL_CAP) {
            for (uint32_t j = t; j < m; j += 64) {
                const flight::Rec r = c.stage[b + j];
                kd[j] = r.deliver, ke[j] = r.event_id, kt[j] = r.tag, ks[j] = r.src, kz[j] = r.size;
            }
            __syncthreads();
            // K elements a lane, ranked in one walk over the keys (each key is read from LDS once)
            switch ((m + 63) / 64) {
                case 1: rank_small<1>(c, b, m, kd, ke, kt, ks, kz); break;
                case 2: rank_small<2>(c, b, m, kd, ke, kt, ks, kz); break;
                case 3: rank_small<3>(c, b, m, kd, ke, kt, ks, kz); break;
                default: rank_small<4>(c, b, m, kd, ke, kt, ks, kz); break;
            }
        } else {
            // the run's elements 64 at a time against every chunk of FL_CAP keys
            for (uint32_t i0 = 0; i0 < m; i0 += 64) {
                const uint32_t i = i0 + t;
                const bool has = i < m;
                flight::Rec mine = {0, 0, 0, 0, 0};
                if (has) mine = c.stage[b + i];
                const flight::Key mk = flight::key_of(mine);
                uint32_t r = 0;
                for (uint32_t j0 = 0; j0 < m; j0 += FL_CAP) {
                    const uint32_t mj = m - j0 < FL_CAP ? m - j0 : FL_CAP;
                    __syncthreads();  // the previous chunk has been read
                    for (uint32_t j = t; j < mj; j += 64) {
                        const flight::Rec x = c.stage[b + j0 + j];
                        kd[j] = x.deliver, ke[j] = x.event_id, ks[j] = x.src;
                    }
                    __syncthreads();
                    if (has)
                        for (uint32_t j = 0; j < mj; ++j) {
                            flight::Key o;
                            o.deliver = kd[j], o.event_id = ke[j], o.src = ks[j];
                            r += flight::before_at(o, j0 + j, mk, i);
                        }
                }
                if (has) flight::emit(c, mine, b + r);
            }
        }
        __syncthreads();  // LDS reused by the next destination
    }
}

}  // namespace

struct srt_flight {
    srt_plan *plan = nullptr;  // nullptr: host-only
    uint32_t n_dst = 0;
    uint64_t pool_cap = 0;
    uint64_t bound = 0;       // no more than this many records are stored (sizes the grids)
    uint64_t last_until = 0;  // the largest until_ns of a pop so far
    uint64_t tag_next = 0;    // the running count of all earlier pushes' n_pkts
    void *mem = nullptr;      // device form: the one device allocation; host-only: h_mem
    std::vector<uint64_t> h_mem;
    flight::Ctx base;         // the instance's own pointers
};

namespace srt {
// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_flight() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&flight_scan_kernel));
}
}  // namespace srt

extern "C" void srt_flight_destroy(srt_flight *fl) {
    if (!fl) return;
    if (fl->plan) {
        (void)stage::use_device(fl->plan);
        (void)hipStreamSynchronize(fl->plan->stream);
        (void)hipFree(fl->mem);
    }
    delete fl;
}

extern "C" srt_status srt_flight_create(srt_plan *plan, uint32_t n_dst_hosts, uint64_t pool_cap, srt_flight **out,
                                        srt_err *err) {
    stage::begin(err);
    if (!out) return stage::null_argument(err);
    *out = nullptr;
    if (n_dst_hosts == 0xffffffffu || pool_cap > (1ull << 31)) {
        set_err(err, SRT_ERR_INVALID, "flight: n_dst_hosts or pool_cap (at most 2^31) out of range");
        return SRT_ERR_INVALID;
    }
    srt_flight *fl = new (std::nothrow) srt_flight;
    if (!fl) return SRT_ERR_OOM;
    fl->plan = plan;
    fl->n_dst = n_dst_hosts;
    fl->pool_cap = pool_cap;
    // state, the per-destination counts, then the stage, the pool's u64 and u32 arrays and the slots
    const size_t head = sizeof(flight::State) + 8ull * ((n_dst_hosts + 1ull) / 2);
    const size_t bytes = head + 108ull * pool_cap;
    if (!plan) {
        try {
            fl->h_mem.assign(bytes / 8 + 1, 0);
        } catch (const std::bad_alloc &) {
            delete fl;
            set_err(err, SRT_ERR_OOM, "flight: host allocation failed");
            return SRT_ERR_OOM;
        }
        fl->mem = fl->h_mem.data();
    } else {
        srt::init_wait();
        bool ok = stage::use_device(plan);
        ok = ok && hipMalloc(&fl->mem, bytes + 8) == hipSuccess;
        ok = ok && hipMemset(fl->mem, 0, head) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            (void)hipFree(fl->mem);
            delete fl;
            set_err(err, SRT_ERR_OOM, "flight: device allocation failed");
            return SRT_ERR_OOM;
        }
    }
    flight::Ctx &c = fl->base;
    std::memset(&c, 0, sizeof c);
    char *p = static_cast<char *>(fl->mem);
    c.st = reinterpret_cast<flight::State *>(p);
    c.cnt = reinterpret_cast<uint32_t *>(p + sizeof(flight::State));
    c.stage = reinterpret_cast<flight::Rec *>(p + head);
    uint64_t *q = reinterpret_cast<uint64_t *>(c.stage + pool_cap);
    c.pool.deliver = q;
    c.pool.event_id = q + 2 * pool_cap;
    c.pool.tag = q + 4 * pool_cap;
    uint32_t *r = reinterpret_cast<uint32_t *>(q + 6 * pool_cap);
    c.pool.src = r;
    c.pool.dst = r + 2 * pool_cap;
    c.pool.size = r + 4 * pool_cap;
    c.slot = r + 6 * pool_cap;
    c.pool_cap = pool_cap;
    c.n_dst = n_dst_hosts;
    *out = fl;
    return SRT_OK;
}

extern "C" srt_status srt_flight_push(srt_flight *fl, const uint32_t *d_host_pkt_ptr, uint32_t n_src_hosts,
                                      uint64_t n_pkts, const uint32_t *d_flags, const uint64_t *d_deliver,
                                      const uint32_t *d_dst_host, const uint64_t *d_event_id,
                                      const uint32_t *d_total_size, const uint64_t *d_tag, uint64_t *tag_base,
                                      srt_err *err) {
    stage::begin(err);
    if (!fl || !d_host_pkt_ptr ||
        (n_pkts && (!d_flags || !d_deliver || !d_dst_host || !d_event_id || !d_total_size)))
        return stage::null_argument(err);
    if (n_pkts >= 0x80000000ull || n_src_hosts == 0xffffffffu) {
        set_err(err, SRT_ERR_INVALID, "more than 2^31-1 packets in one batch, or n_src_hosts out of range");
        return SRT_ERR_INVALID;
    }
    flight::Ctx c = fl->base;
    c.host_ptr = d_host_pkt_ptr;
    c.flags_in = d_flags;
    c.deliver_in = d_deliver;
    c.dst_in = d_dst_host;
    c.event_id_in = d_event_id;
    c.size_in = d_total_size;
    c.tag_in = d_tag;
    c.tag_base = fl->tag_next;
    c.last_until = fl->last_until;
    c.n_src = n_src_hosts;
    c.n_pkts = (uint32_t)n_pkts;
    if (tag_base) *tag_base = fl->tag_next;
    fl->tag_next += n_pkts;
    fl->bound = std::min(fl->pool_cap, fl->bound + n_pkts);
    if (!fl->plan) {
        flight::host_push(c);
        return SRT_OK;
    }
    if (!n_pkts || !n_src_hosts) return SRT_OK;
    if (!stage::use_device(fl->plan)) return SRT_ERR_HIP;
    const bool wide = stage::wide(n_pkts, c.n_src);
    stage::launch_grouped(flight_push_kernel<64>, flight_push_kernel<8>, wide,
                          stage::host_blocks(c.n_src, wide, PT), PT, fl->plan->stream, c);
    return stage::launched(err, "flight");
}

extern "C" srt_status srt_flight_pop(srt_flight *fl, uint64_t until_ns, uint32_t *d_w_order, uint32_t *d_w_dst_ptr,
                                     uint64_t *d_w_deliver, uint32_t *d_w_total_size, uint32_t *d_w_src_host,
                                     uint64_t *d_w_event_id, uint64_t *d_w_tag, uint64_t out_cap, srt_err *err) {
    stage::begin(err);
    if (!fl || !d_w_dst_ptr ||
        (out_cap && (!d_w_order || !d_w_deliver || !d_w_total_size || !d_w_src_host || !d_w_event_id || !d_w_tag)))
        return stage::null_argument(err);
    flight::Ctx c = fl->base;
    c.until = until_ns;
    c.out_cap = out_cap < 0xffffffffull ? out_cap : 0xffffffffull;  // positions are u32
    c.pre_flags = until_ns < fl->last_until ? flight::F_TIME_REGRESSION : 0u;
    c.w_order = d_w_order;
    c.w_dst_ptr = d_w_dst_ptr;
    c.w.deliver = d_w_deliver;
    c.w.size = d_w_total_size;
    c.w.src = d_w_src_host;
    c.w.event_id = d_w_event_id;
    c.w.tag = d_w_tag;
    c.w.dst = nullptr;
    fl->last_until = std::max(fl->last_until, until_ns);
    if (!fl->plan) {
        flight::host_pop(c);
        return SRT_OK;
    }
    if (!stage::use_device(fl->plan)) return SRT_ERR_HIP;
    hipStream_t s = fl->plan->stream;
    const uint32_t count_blocks = stage::strided_blocks(fl->bound, MAX_BLOCKS);
    const uint32_t move_blocks = (uint32_t)std::min<uint64_t>((fl->bound + BT * ITEMS - 1) / (BT * ITEMS), MAX_BLOCKS);
    if (count_blocks) hipLaunchKernelGGL(flight_count_kernel, dim3(count_blocks), dim3(BT), 0, s, c);
    hipLaunchKernelGGL(flight_scan_kernel, dim3(1), dim3(ST), 0, s, c);
    if (move_blocks) hipLaunchKernelGGL(flight_move_kernel, dim3(move_blocks), dim3(BT), 0, s, c);
    if (move_blocks && c.n_dst)
        hipLaunchKernelGGL(flight_sort_kernel, dim3(std::min(c.n_dst, SORT_BLOCKS)), dim3(64), 0, s, c);
    return stage::launched(err, "flight");
}

extern "C" srt_status srt_flight_status(srt_flight *fl, uint32_t *flags, uint64_t *n_popped, uint64_t *n_stored,
                                        uint64_t *n_lost, srt_err *err) {
    stage::begin(err);
    if (!fl) return stage::null_argument(err);
    flight::State w;
    if (!fl->plan) {
        w = *fl->base.st;
        fl->base.st->flags = 0;
    } else {
        if (!stage::use_device(fl->plan)) return SRT_ERR_HIP;
        const srt_status st = stage::read_status(fl->plan, &w, fl->base.st, sizeof w, err, "flight");
        if (st != SRT_OK) return st;
    }
    const uint64_t stored = flight::stored(fl->base, w.len);
    fl->bound = stored;
    const uint32_t f = w.flags & 31u;
    if (flags) *flags = f;
    if (n_popped) *n_popped = w.n_popped;
    if (n_stored) *n_stored = stored;
    if (n_lost) *n_lost = w.n_lost;
    if (!f) return SRT_OK;
    if (err) {
        err->code = SRT_ERR_INVALID;
        std::snprintf(err->msg, sizeof err->msg, "flight:%s%s%s%s%s",
                      f & flight::F_POOL_OVERFLOW ? " more packets than pool_cap (the excess is lost);" : "",
                      f & flight::F_OUT_OVERFLOW ? " more due than out_cap (the pop took nothing);" : "",
                      f & flight::F_BAD_HOST ? " a dst_host not below n_dst_hosts (not stored);" : "",
                      f & flight::F_LATE_PUSH ? " a deliver time pushed before the last pop's until_ns;" : "",
                      f & flight::F_TIME_REGRESSION ? " a pop's until_ns went backwards;" : "");
    }
    return SRT_ERR_INVALID;
}
