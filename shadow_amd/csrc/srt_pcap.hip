// srt_pcap.hip -- per-host pcap capture streams of one interface class, built on
// the device: the records networkinterface_pop and networkinterface_push hand to
// the PcapWriter (host/network/network_interface.c:119-134, 140-202, 310-340;
// utility/pcap_writer.rs), one byte stream a host.  The step -- sizes, validity,
// the merge rule, the header words, the tile assembly, the range checks -- is
// srt_pcap_step.h, compiled here for the device and for the host-only instance.
//
// Device form, four launches a call on the plan's stream, no wait between them:
//   (1) hosts: a group of L lanes owns a host (L 64 when the call averages more
//       than 16 records a host, else 8): order check, each record's merged rank
//       by a binary search in the host's other list, its size and validity, the
//       host's byte total, reduced across the group's lanes;
//   (2) scan: one workgroup scans the hosts' totals into d_host_off, decides
//       OVERFLOW, advances the hosts' last times and the counts;
//   (3) offsets: the geometry of (1): a segmented scan of the sizes in merged
//       order, from the host's offset;
//   (4) write: a workgroup owns one 16-byte-aligned tile of TILE bytes of d_out;
//       it finds the records that overlap the tile by a 256-way search in the
//       offsets (three rounds), 8 to 64 lanes a record put the record and packet
//       headers and the payload bytes (16 at a time) into LDS, and the tile
//       leaves with one 16-byte store a thread, byte stores only at the ends of
//       the call's range.
// Every value is written with ordinary vector stores from plain C++; flags with
// vector atomics.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "srt_internal.h"
#include "srt_pcap_step.h"
#include "srt_stage.h"

namespace {

static_assert(sizeof(srt_pcap_rec) == 48 && offsetof(srt_pcap_rec, payload_off) == 8 &&
                  offsetof(srt_pcap_rec, src_ip_be) == 16 && offsetof(srt_pcap_rec, src_port_be) == 24 &&
                  offsetof(srt_pcap_rec, seq) == 28 && offsetof(srt_pcap_rec, ack) == 32 &&
                  offsetof(srt_pcap_rec, window) == 36 && offsetof(srt_pcap_rec, payload_len) == 38 &&
                  offsetof(srt_pcap_rec, protocol) == 40 && offsetof(srt_pcap_rec, wscale_set) == 43 &&
                  sizeof(pcap::State) == 32,
              "record layouts");

using stage::BT;
using stage::ST;
using stage::set_err;
constexpr uint32_t WRITE_BLOCKS = 1u << 20;  // at most, each striding over the tiles
static_assert(pcap::TILE == BT * 16, "a thread stores 16 bytes of the tile");

template <uint32_t L>
__global__ __launch_bounds__(BT) void pcap_hosts_kernel(const pcap::Ctx c) {
    const stage::Group<L> G(c.n_hosts);
    const uint64_t g = G.g;
    const uint32_t l = G.l;
    pcap::Seg s = {{0, 0}, {0, 0}};
    pcap::HostAcc a = {0, 0, 0, 0};
    uint32_t bits = 0;
    bool on = false;
    if (G.own()) {
        s = pcap::segs(c, (uint32_t)g);
        on = c.enabled[g] != 0;
        if (on) bits = pcap::order_check(c, (uint32_t)g, s, l, L);
    }
    bits = stage::group_or<L>(bits);  // every lane is here
    if (G.own()) {
        if (!on) pcap::merge_disabled(c, s, l, L);
        else if (!(bits & pcap::DECREASES)) pcap::merge_sorted(c, s, l, L, a);
        else if (l == 0) pcap::merge_serial(c, s, a);
    }
    a.bytes = stage::group_add<L>(a.bytes);
    a.cnt = (uint32_t)stage::group_add<L>((unsigned long long)a.cnt);  // summed in 64 bits like the bytes
    a.maxt = stage::group_max<L>(a.maxt);
    a.flags = stage::group_or<L>(a.flags);
    if (G.own() && l == 0) pcap::host_finish(c, (uint32_t)g, a, bits);
}

__global__ __launch_bounds__(ST) void pcap_scan_kernel(const pcap::Ctx c) {
    __shared__ uint64_t wsum[ST / 64], csum[ST / 64];
    __shared__ uint32_t ok_s;
    const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63;
    uint64_t carry = 0;
    unsigned long long cnt = 0;
    for (uint64_t base = 0; base < c.n_hosts; base += ST) {  // uniform
        const uint64_t h = base + t;
        const unsigned long long v = h < c.n_hosts ? c.host_bytes[h] : 0;
        if (h < c.n_hosts) cnt += c.host_cnt[h];
        unsigned long long inc = v;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        uint64_t before = 0, all = 0;
        for (uint32_t x = 0; x < ST / 64; ++x) {
            if (x < w) before += wsum[x];
            all += wsum[x];
        }
        if (h < c.n_hosts) c.host_off[h] = carry + before + inc - v;
        carry += all;
        __syncthreads();
    }
    cnt = stage::group_add<64>(cnt);
    if (lane == 0) csum[w] = cnt;
    __syncthreads();
    if (t == 0) {
        uint64_t n = 0;
        for (uint32_t x = 0; x < ST / 64; ++x) n += csum[x];
        ok_s = pcap::scan_finish(c, carry, n) ? 1u : 0u;
    }
    __syncthreads();
    if (ok_s)
        for (uint64_t h = t; h < c.n_hosts; h += ST) pcap::commit_last(c, (uint32_t)h);
}

template <uint32_t L>
__global__ __launch_bounds__(BT) void pcap_offsets_kernel(const pcap::Ctx c) {
    const stage::Group<L> G(c.n_hosts);
    const uint64_t g = G.g;
    const uint32_t l = G.l;
    uint32_t base = 0, n = 0;
    unsigned long long run = 0;
    if (G.own()) {
        const pcap::Seg s = pcap::segs(c, (uint32_t)g);
        base = s.b[0] + s.b[1];
        n = (s.e[0] - s.b[0]) + (s.e[1] - s.b[1]);
        run = c.host_off[g];
    }
    for (uint32_t i0 = 0; i0 < n; i0 += L) {  // uniform in the group
        const uint32_t i = i0 + l;
        const unsigned long long v = i < n ? c.size[base + i] : 0;
        unsigned long long inc = v;
#pragma unroll
        for (uint32_t d = 1; d < L; d <<= 1) {
            const unsigned long long o = __shfl_up(inc, d, L);
            if (l >= d) inc += o;
        }
        if (i < n) c.off[base + i] = run + inc - v;
        run += __shfl(inc, L - 1, L);
    }
}

// entries of a[0 .. n) that are <= key (le) or < key, a nondecreasing: the workgroup probes BT places a round
// and keeps the piece the boundary is in (three rounds for 2^24 entries); every thread calls it
__device__ __forceinline__ uint32_t block_count(const uint64_t *a, uint32_t n, uint64_t key, bool le) {
    uint32_t lo = 0, len = n;
    while (len) {  // uniform
        const uint32_t step = (len + BT - 1) / BT;
        const uint64_t first = (uint64_t)threadIdx.x * step;  // this thread's piece of [lo, lo + len)
        bool in = false;
        if (first < len) {
            const uint64_t v = a[lo + (uint32_t)std::min<uint64_t>(first + step, len) - 1];  // the piece's last entry
            in = le ? v <= key : v < key;
        }
        const uint32_t full = (uint32_t)__syncthreads_count(in);  // pieces wholly counted
        const uint64_t skip = (uint64_t)full * step;
        if (skip >= len) return lo + len;
        lo += (uint32_t)skip;
        len = std::min<uint32_t>(step - 1, len - (uint32_t)skip);  // the piece's last entry is not counted
    }
    return lo;
}

__global__ __launch_bounds__(BT) void pcap_write_kernel(const pcap::Ctx c) {
    __shared__ uint4 tile4[pcap::TILE / 16];
    uint8_t *tile = reinterpret_cast<uint8_t *>(tile4);
    const uint32_t t = threadIdx.x;
    const uint64_t total = c.st->write_total, tiles = pcap::tile_count(c, total);
    const uint32_t n = pcap::walked(c, 0) + pcap::walked(c, 1);
    for (uint64_t k = blockIdx.x; k < tiles; k += gridDim.x) {  // uniform
        int64_t ts;
        uint64_t lo, hi;
        if (!pcap::tile_span(c, total, k, ts, lo, hi)) continue;
        // pcap::tile_range's two positions, searched by the whole workgroup
        const uint32_t le = block_count(c.off, n + 1, lo, true), p0 = le ? le - 1 : 0;
        const uint32_t p1 = std::max(p0, block_count(c.off, n, hi, false));
        // lanes a record: 8 (128 payload bytes a step) when the tile holds many records, up to a wave when few
        const uint32_t recs = p1 - p0, gl = recs <= 4 ? 64u : recs <= 8 ? 32u : recs <= 16 ? 16u : 8u;
        pcap::tile_records(c, ts, tile, p0, p1, t / gl, BT / gl, t % gl, gl);
        __syncthreads();
        const int64_t a = ts + 16 * (int64_t)t;  // this thread's 16 bytes of the stream
        if (a >= (int64_t)lo && (uint64_t)(a + 16) <= hi) {
            *reinterpret_cast<uint4 *>(c.out + a) = tile4[t];
        } else {
            for (uint32_t x = 0; x < 16; ++x)
                if (a + x >= (int64_t)lo && (uint64_t)(a + x) < hi) c.out[a + x] = tile[16 * t + x];
        }
        __syncthreads();  // the next tile reuses the buffer
    }
}

}  // namespace

struct srt_pcap {
    srt_plan *plan = nullptr;  // nullptr: host-only
    uint32_t n_hosts = 0, capture_len = 0;
    uint64_t rec_cap = 0;
    void *mem = nullptr;  // device form: everything in one allocation; host-only: h_mem
    std::vector<uint64_t> h_mem;
    std::vector<FILE *> files;  // [n_hosts] after srt_pcap_open_files
    pcap::Ctx base;
};

namespace srt {
// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_pcap() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&pcap_scan_kernel));
}
}  // namespace srt

namespace {
void close_files(srt_pcap *pc) {
    for (FILE *f : pc->files)
        if (f) std::fclose(f);
    pc->files.clear();
}
}  // namespace

extern "C" uint32_t srt_pcap_tile_bytes(void) { return pcap::TILE; }

extern "C" void srt_pcap_file_header(uint32_t capture_len, uint8_t out[24]) {
    if (!out) return;
    // utility/pcap_writer.rs:25-54, native endian
    const uint32_t magic = 0xA1B2C3D4u, zero = 0, linktype = 101;
    const uint16_t major = 2, minor = 4;
    std::memcpy(out, &magic, 4);
    std::memcpy(out + 4, &major, 2);
    std::memcpy(out + 6, &minor, 2);
    std::memcpy(out + 8, &zero, 4);
    std::memcpy(out + 12, &zero, 4);
    std::memcpy(out + 16, &capture_len, 4);
    std::memcpy(out + 20, &linktype, 4);
}

extern "C" void srt_pcap_destroy(srt_pcap *pc) {
    if (!pc) return;
    if (pc->plan) {
        (void)stage::use_device(pc->plan);
        (void)hipStreamSynchronize(pc->plan->stream);
        (void)hipFree(pc->mem);
    }
    close_files(pc);
    delete pc;
}

extern "C" srt_status srt_pcap_create(srt_plan *plan, uint32_t n_hosts, uint32_t capture_len, const uint8_t *enabled,
                                      uint64_t rec_cap, uint32_t flags, srt_pcap **out, srt_err *err) {
    stage::begin(err);
    if (!out) return stage::null_argument(err);
    *out = nullptr;
    if (n_hosts >= 0x80000000u || rec_cap >= 0x80000000ull || (flags & ~SRT_PCAP_TX_FIRST)) {
        set_err(err, SRT_ERR_INVALID, "pcap: n_hosts or rec_cap not below 2^31, or an unknown flag");
        return SRT_ERR_INVALID;
    }
    srt_pcap *pc = new (std::nothrow) srt_pcap;
    if (!pc) return SRT_ERR_OOM;
    pc->plan = plan;
    pc->n_hosts = n_hosts;
    pc->capture_len = capture_len;
    pc->rec_cap = rec_cap;
    // state; per host last, pend, bytes (u64), count (u32), enabled (u8, padded to 4); per record off (u64, one
    // more), ent, size (u32)
    const size_t head = sizeof(pcap::State), nh = n_hosts, nr = (size_t)rec_cap;
    const size_t bytes = head + 32 * nh + 8 * (nr + 1) + 8 * nr;
    std::vector<uint8_t> en;
    bool ok = true;
    try {
        en.assign(nh, 1);
        if (!plan) pc->h_mem.assign(bytes / 8 + 1, 0);
    } catch (const std::bad_alloc &) {
        ok = false;
    }
    for (size_t h = 0; ok && enabled && h < nh; ++h) en[h] = enabled[h] ? 1 : 0;
    if (ok && !plan) pc->mem = pc->h_mem.data();
    if (ok && plan) {
        srt::init_wait();
        ok = stage::use_device(plan);
        ok = ok && hipMalloc(&pc->mem, bytes + 8) == hipSuccess;
        ok = ok && hipMemset(pc->mem, 0, bytes + 8) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            (void)hipFree(pc->mem);
        }
    }
    if (!ok) {
        delete pc;
        set_err(err, SRT_ERR_OOM, "pcap: allocation failed");
        return SRT_ERR_OOM;
    }
    pcap::Ctx &c = pc->base;
    std::memset(&c, 0, sizeof c);
    char *p = static_cast<char *>(pc->mem);
    c.st = reinterpret_cast<pcap::State *>(p);
    c.last = reinterpret_cast<uint64_t *>(p + head);
    c.pend = c.last + nh;
    c.host_bytes = c.pend + nh;
    c.off = c.host_bytes + nh;
    c.host_cnt = reinterpret_cast<uint32_t *>(c.off + nr + 1);
    c.ent = c.host_cnt + nh;
    c.size = c.ent + nr;
    uint8_t *d_en = reinterpret_cast<uint8_t *>(c.size + nr);  // nh bytes of the 4 * nh left
    c.enabled = d_en;
    c.n_hosts = n_hosts;
    c.capture_len = capture_len;
    c.rx_first = (flags & SRT_PCAP_TX_FIRST) ? 0u : 1u;
    if (!plan) {
        if (nh) std::memcpy(d_en, en.data(), nh);
    } else if (nh && hipMemcpy(d_en, en.data(), nh, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(pc->mem);
        delete pc;
        set_err(err, SRT_ERR_HIP, "pcap: device initialisation failed");
        return SRT_ERR_HIP;
    }
    *out = pc;
    return SRT_OK;
}

extern "C" srt_status srt_pcap_run(srt_pcap *pc, const srt_pcap_rec *d_tx, const uint32_t *d_tx_idx,
                                   const uint32_t *d_tx_host_ptr, uint64_t n_tx, const srt_pcap_rec *d_rx,
                                   const uint32_t *d_rx_idx, const uint32_t *d_rx_host_ptr, uint64_t n_rx,
                                   const uint8_t *d_payload, uint64_t payload_bytes, uint8_t *d_out, uint64_t out_cap,
                                   uint64_t *d_host_off, srt_err *err) {
    stage::begin(err);
    if (!pc || !d_tx_host_ptr || !d_rx_host_ptr || !d_host_off || (n_tx && !d_tx) || (n_rx && !d_rx) ||
        (out_cap && !d_out))
        return stage::null_argument(err);
    if (n_tx > pc->rec_cap || n_rx > pc->rec_cap || n_tx + n_rx > pc->rec_cap) {
        set_err(err, SRT_ERR_INVALID, "pcap: n_tx + n_rx exceeds rec_cap");
        return SRT_ERR_INVALID;
    }
    if (!d_payload && pc->capture_len > 28) {
        set_err(err, SRT_ERR_INVALID, "pcap: d_payload may be NULL only when capture_len is at most 28");
        return SRT_ERR_INVALID;
    }
    pcap::Ctx c = pc->base;
    c.rec[0] = d_tx, c.rec[1] = d_rx;
    c.idx[0] = d_tx_idx, c.idx[1] = d_rx_idx;
    c.ptr[0] = d_tx_host_ptr, c.ptr[1] = d_rx_host_ptr;
    c.n[0] = (uint32_t)n_tx, c.n[1] = (uint32_t)n_rx;
    c.payload = d_payload;
    c.payload_bytes = payload_bytes;
    c.out = d_out;
    c.out_cap = out_cap;
    c.host_off = d_host_off;
    if (!pc->plan) {
        pcap::host_run(c);
        return SRT_OK;
    }
    if (!stage::use_device(pc->plan)) return SRT_ERR_HIP;
    hipStream_t s = pc->plan->stream;
    const bool wide = stage::wide(n_tx + n_rx, c.n_hosts);
    const uint32_t hb = stage::host_blocks(c.n_hosts, wide);
    if (hb) stage::launch_grouped(pcap_hosts_kernel<64>, pcap_hosts_kernel<8>, wide, hb, BT, s, c);
    hipLaunchKernelGGL(pcap_scan_kernel, dim3(1), dim3(ST), 0, s, c);
    if (hb) stage::launch_grouped(pcap_offsets_kernel<64>, pcap_offsets_kernel<8>, wide, hb, BT, s, c);
    // the call's bytes are at most out_cap (else nothing is written) and at most 16 + min(capture_len, 65535) a record
    const uint64_t per_rec = pcap::REC_HDR + std::min<uint64_t>(pc->capture_len, 65535);
    const uint64_t most = std::min<uint64_t>(out_cap, (n_tx + n_rx) * per_rec);
    if (most) {
        const uint64_t tiles = (most + 15 + pcap::TILE - 1) / pcap::TILE;
        hipLaunchKernelGGL(pcap_write_kernel, dim3((uint32_t)std::min<uint64_t>(tiles, WRITE_BLOCKS)), dim3(BT), 0, s,
                           c);
    }
    return stage::launched(err, "pcap");
}

extern "C" srt_status srt_pcap_status(srt_pcap *pc, uint32_t *flags, uint64_t *n_records, uint64_t *n_bytes,
                                      srt_err *err) {
    stage::begin(err);
    if (!pc) return stage::null_argument(err);
    pcap::State w;
    if (!pc->plan) {
        w = *pc->base.st;
        pc->base.st->flags = 0;
    } else {
        if (!stage::use_device(pc->plan)) return SRT_ERR_HIP;
        const srt_status st = stage::read_status(pc->plan, &w, pc->base.st, sizeof w, err, "pcap");
        if (st != SRT_OK) return st;
    }
    const uint32_t f = w.flags & 31u;
    if (flags) *flags = f;
    if (n_records) *n_records = w.n_recs;
    if (n_bytes) *n_bytes = w.n_bytes;
    if (!f) return SRT_OK;
    if (err) {
        err->code = SRT_ERR_INVALID;
        std::snprintf(err->msg, sizeof err->msg, "pcap:%s%s%s%s%s",
                      f & pcap::F_OVERFLOW ? " a call's bytes exceed out_cap (nothing written);" : "",
                      f & pcap::F_BAD_PROTOCOL ? " a protocol is neither 6 nor 17 (skipped);" : "",
                      f & pcap::F_BAD_LENGTH ? " a packet is longer than 65535 bytes (skipped);" : "",
                      f & pcap::F_BAD_PAYLOAD ? " a payload range ends past payload_bytes (skipped);" : "",
                      f & pcap::F_TIME_ORDER ? " a list decreases in time or starts before the host's last record;" : "");
    }
    return SRT_ERR_INVALID;
}

extern "C" srt_status srt_pcap_open_files(srt_pcap *pc, const char *const *paths, srt_err *err) {
    stage::begin(err);
    if (!pc || (pc->n_hosts && !paths)) return stage::null_argument(err);
    close_files(pc);
    try {
        pc->files.assign(pc->n_hosts, nullptr);
    } catch (const std::bad_alloc &) {
        return SRT_ERR_OOM;
    }
    uint8_t head[24];
    srt_pcap_file_header(pc->capture_len, head);
    for (uint32_t h = 0; h < pc->n_hosts; ++h) {
        if (!paths[h]) continue;
        FILE *f = std::fopen(paths[h], "wb");  // File::create: create or truncate
        if (!f || std::fwrite(head, 1, 24, f) != 24) {
            if (f) std::fclose(f);
            close_files(pc);
            char msg[200];
            std::snprintf(msg, sizeof msg, "pcap: cannot create %.150s", paths[h]);
            set_err(err, SRT_ERR_INVALID, msg);
            if (err) err->a_id = h;
            return SRT_ERR_INVALID;
        }
        pc->files[h] = f;
    }
    return SRT_OK;
}

extern "C" srt_status srt_pcap_append_files(srt_pcap *pc, const uint64_t *host_off, const uint8_t *bytes,
                                            srt_err *err) {
    stage::begin(err);
    if (!pc || !host_off) return stage::null_argument(err);
    if (pc->files.size() != pc->n_hosts) {
        set_err(err, SRT_ERR_INVALID, "pcap: no files are open");
        return SRT_ERR_INVALID;
    }
    for (uint32_t h = 0; h < pc->n_hosts; ++h)
        if (host_off[h + 1] < host_off[h] || (host_off[h + 1] > host_off[h] && !bytes)) {
            set_err(err, SRT_ERR_INVALID, "pcap: host_off decreases, or bytes is NULL");
            return SRT_ERR_INVALID;
        }
    for (uint32_t h = 0; h < pc->n_hosts; ++h) {
        const uint64_t n = host_off[h + 1] - host_off[h];
        if (!pc->files[h] || !n) continue;
        if (std::fwrite(bytes + host_off[h], 1, n, pc->files[h]) != n || std::fflush(pc->files[h]) != 0) {
            set_err(err, SRT_ERR_INVALID, "pcap: write failed");
            if (err) err->a_id = h;
            return SRT_ERR_INVALID;
        }
    }
    return SRT_OK;
}
