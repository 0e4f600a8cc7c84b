// srt_stage.h -- what the packet stages' .hip files share (srt_inbound,
// srt_outbound, srt_sendbatch, srt_flight, srt_deliver, srt_tracker,
// srt_loopback, srt_pcap; srt_events for the error record): the launch
// constants, the lane-group geometry and its reductions, the single-workgroup
// scan over the hosts, the grid-stride loop, and the host glue around a launch.
// HIP only: what the host-only programs of tests/asan compile as well lives in
// the step headers and srt_relay_common.h.
//
// A device helper here is used by a kernel only where the kernel compiles to
// the same instructions with it as with the lines written out.  Where it does
// not, the kernel keeps its own lines and says so: the status sums
// (deliver_sum_kernel, tracker_sum_kernel, loopback_sum_kernel: no shared form
// reproduces them), the note kernels' loops, the reductions of deliver's count
// and scatter, the fused count-and-minimum of sendbatch's count.
#ifndef SRT_STAGE_H
#define SRT_STAGE_H

#include <cstdio>
#include <cstring>

#include "srt_internal.h"

namespace stage {

constexpr uint32_t BT = 256;            // threads a workgroup of the hosts' walks and the grid-stride kernels
constexpr uint32_t ST = 1024;           // threads of a scan's or a sum's one workgroup
constexpr uint32_t WIDE_AVG = 16;       // more packets a host on average: a wave a host
constexpr uint32_t LATE_BLOCKS = 1024;  // at most, each striding over a late list or flat records
constexpr uint32_t NOTE_BLOCKS = 4096;  // at most, each striding over a note

// ---- device: a group of L lanes owns one host; workgroups of T threads hold T / L hosts
template <uint32_t L, uint32_t T = BT>
struct Group {
    uint64_t g;  // the group's host, when own()
    uint32_t l;  // the lane's place in the group
    uint32_t n_hosts;
    __device__ __forceinline__ explicit Group(uint32_t n)
        : g(((uint64_t)blockIdx.x * T + threadIdx.x) / L), l(threadIdx.x % L), n_hosts(n) {}
    // false: the tail of the last workgroup
    __device__ __forceinline__ bool own() const { return g < n_hosts; }
};

// the reductions over a group's L lanes, the result in every one of them; every lane of the wave calls them
template <uint32_t L, class V>
__device__ __forceinline__ V group_add(V v) {
#pragma unroll
    for (uint32_t off = L / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <uint32_t L, class V>
__device__ __forceinline__ V group_max(V v) {
#pragma unroll
    for (uint32_t off = L / 2; off > 0; off >>= 1) {
        const V o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

template <uint32_t L, class V>
__device__ __forceinline__ V group_or(V v) {
#pragma unroll
    for (uint32_t off = L / 2; off > 0; off >>= 1) v |= __shfl_xor(v, off);
    return v;
}

// N sums at once (a lane's counters)
template <uint32_t L, uint32_t N>
__device__ __forceinline__ void group_sum(uint64_t (&a)[N]) {
#pragma unroll
    for (uint32_t j = 0; j < N; ++j) {
        unsigned long long v = a[j];
#pragma unroll
        for (uint32_t off = L / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
        a[j] = v;
    }
}

// for (uint64_t k : grid_stride(n)): a thread an item, striding by the grid of BT-thread workgroups, below
// n; only the workgroups from `block0` on take part
struct grid_stride {
    uint64_t n;
    uint32_t block0;
    __device__ __forceinline__ explicit grid_stride(uint64_t n_, uint32_t block0_ = 0) : n(n_), block0(block0_) {}
    struct It {
        uint64_t k;
        uint32_t block0;
        __device__ __forceinline__ uint64_t operator*() const { return k; }
        __device__ __forceinline__ void operator++() { k += (uint64_t)(gridDim.x - block0) * BT; }
        __device__ __forceinline__ bool operator!=(const It &end) const { return k < end.k; }
    };
    __device__ __forceinline__ It begin() const { return It{(uint64_t)(blockIdx.x - block0) * BT + threadIdx.x, block0}; }
    __device__ __forceinline__ It end() const { return It{n, block0}; }
};

// The exclusive scan of the hosts' counts by one workgroup of T threads: each thread sums a contiguous
// chunk of count(h), the sums are scanned across the workgroup, then place(h, run) stores host h's base
// and returns its count again (so a stage orders that load and store as it needs); end(total) runs in
// thread T - 1.
template <uint32_t T, class Count, class Place, class End>
__device__ __forceinline__ void scan_hosts(uint32_t n_hosts, Count count, Place place, End end) {
    __shared__ uint64_t wsum[T / 64];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (uint32_t)(((uint64_t)n_hosts + T - 1) / T);  // below 2^22: t * per fits
    const uint64_t b64 = (uint64_t)t * per;
    const uint32_t b = b64 < n_hosts ? (uint32_t)b64 : n_hosts;
    const uint32_t e = b64 + per < n_hosts ? (uint32_t)(b64 + per) : n_hosts;
    uint64_t sum = 0;
    for (uint32_t h = b; h < e; ++h) sum += count(h);
    // inclusive scan of the threads' sums: within the wave, then over the waves' totals
    uint64_t inc = sum;
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up((unsigned long long)inc, off);
        if ((t & 63) >= off) inc += o;
    }
    if ((t & 63) == 63) wsum[t >> 6] = inc;
    __syncthreads();
    uint64_t before = 0;
    for (uint32_t w = 0; w < (t >> 6); ++w) before += wsum[w];
    uint64_t run = before + inc - sum;
    for (uint32_t h = b; h < e; ++h) run += place(h, run);
    if (t == T - 1) end(before + inc);
}

// ---- host: the launch geometry
constexpr bool wide(uint64_t n, uint32_t n_hosts) { return n > (uint64_t)WIDE_AVG * n_hosts; }

// workgroups of the hosts' walk: threads / L hosts each
constexpr uint32_t host_blocks(uint32_t n_hosts, bool wide, uint32_t threads = BT) {
    const uint32_t per = threads / (wide ? 64 : 8);
    return (uint32_t)(((uint64_t)n_hosts + per - 1) / per);
}

// workgroups of a grid-stride kernel over n items: a thread an item, at most `cap`
constexpr uint32_t strided_blocks(uint64_t n, uint32_t cap) {
    const uint64_t blocks = n / BT + (n % BT != 0);  // n + BT - 1 could wrap
    return (uint32_t)(blocks < cap ? blocks : cap);
}

static_assert(!wide(0, 0) && !wide(0, 1) && wide(1, 0) && !wide(WIDE_AVG, 1) && wide(WIDE_AVG + 1, 1) &&
                  !wide(16ull * 0xfffffffeu, 0xfffffffeu) && wide(16ull * 0xfffffffeu + 1, 0xfffffffeu),
              "wide: strictly more than WIDE_AVG a host, in 64 bits");
static_assert(host_blocks(0, false) == 0 && host_blocks(0, true) == 0 && host_blocks(1, false) == 1 &&
                  host_blocks(1, true) == 1 && host_blocks(BT / 8, false) == 1 && host_blocks(BT / 8 + 1, false) == 2 &&
                  host_blocks(BT / 8, true) == 8 && host_blocks(BT / 8 + 1, true) == 9 &&
                  host_blocks(0xfffffffeu, false) == 0x08000000u && host_blocks(0xfffffffeu, true) == 0x40000000u &&
                  host_blocks(ST / 8 + 1, false, ST) == 2 && host_blocks(ST / 64 + 1, true, ST) == 2,
              "host_blocks: BT / 8 or BT / 64 hosts a workgroup, rounded up in 64 bits");
static_assert(strided_blocks(0, LATE_BLOCKS) == 0 && strided_blocks(1, LATE_BLOCKS) == 1 &&
                  strided_blocks(BT, LATE_BLOCKS) == 1 && strided_blocks(BT + 1, LATE_BLOCKS) == 2 &&
                  strided_blocks((uint64_t)LATE_BLOCKS * BT, LATE_BLOCKS) == LATE_BLOCKS &&
                  strided_blocks((uint64_t)LATE_BLOCKS * BT + 1, LATE_BLOCKS) == LATE_BLOCKS &&
                  strided_blocks(~0ull, NOTE_BLOCKS) == NOTE_BLOCKS && strided_blocks(5, 0) == 0,
              "strided_blocks: rounded up, clamped to cap, no overflow");

// ---- host: the glue around a launch
inline void set_err(srt_err *err, srt_status code, const char *msg) {
    if (!err) return;
    err->code = code;
    std::snprintf(err->msg, sizeof err->msg, "%s", msg);
}

// every entry point starts from a clean error record
inline void begin(srt_err *err) {
    if (err) std::memset(err, 0, sizeof *err);
}

inline srt_status null_argument(srt_err *err) {
    set_err(err, SRT_ERR_INVALID, "null argument");
    return SRT_ERR_INVALID;
}

inline bool use_device(const srt_plan *plan) { return hipSetDevice(plan->device) == hipSuccess; }

// after a call's launches
inline srt_status launched(srt_err *err, const char *who) {
    if (hipGetLastError() == hipSuccess) return SRT_OK;
    char msg[64];
    std::snprintf(msg, sizeof msg, "%s: launch failed", who);
    set_err(err, SRT_ERR_HIP, msg);
    return SRT_ERR_HIP;
}

// the <64> instantiation of a kernel template (a wave a host) when `wide`, else the <8> one
template <class... P, class... A>
inline void launch_grouped(void (*k64)(P...), void (*k8)(P...), bool wide, uint32_t blocks, uint32_t threads,
                           hipStream_t s, const A &...args) {
    if (wide) hipLaunchKernelGGL(k64, dim3(blocks), dim3(threads), 0, s, args...);
    else hipLaunchKernelGGL(k8, dim3(blocks), dim3(threads), 0, s, args...);
}

// a status call's words: `bytes` from src (device) to dst on the plan's stream, which is waited for; their
// first word is the stage's flag word, cleared on the device if it was set
inline srt_status read_status(const srt_plan *plan, void *dst, void *src, size_t bytes, srt_err *err, const char *who) {
    hipStream_t s = plan->stream;
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        (void)hipGetLastError();
        char msg[64];
        std::snprintf(msg, sizeof msg, "%s: stream failed", who);
        set_err(err, SRT_ERR_HIP, msg);
        return SRT_ERR_HIP;
    }
    uint32_t flags;
    std::memcpy(&flags, dst, 4);
    if (flags) (void)hipMemsetAsync(src, 0, 4, s);
    return SRT_OK;
}

}  // namespace stage
#endif
