// srt_rowfold.h -- what the two row-per-workgroup passes share: the exact-loss
// fold after Floyd-Warshall (srt_loss.hip) and the level solve
// (srt_level.hip).  Included by those two units and nothing else: every
// definition here is internal to the including unit.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <rocprim/device/device_scan.hpp>

#include "srt_internal.h"

namespace srt {

// sharded tails (srt_loss.hip): staged slots [s0, s0 + slots) into the table
// on the main stream, and every chunk behind its all-gather
void expand_slots(srt_plan *p, size_t s0, uint32_t slots);
void expand_chunks_behind(srt_plan *p, uint32_t W);
// Measurement only (rank emulation, no comm): a modelled all-gather on stream
// s, bytes_per_rank from each of W - 1 peers -- a wait of SRT_FW_EMU_AG_US
// (default 25) + received bytes / SRT_FW_EMU_AG_GBPS (default 300)
void emu_allgather(int device, uint32_t W, double bytes_per_rank, hipStream_t s);

namespace {

constexpr int NBK = 2048;        // latency buckets per row
constexpr int LOSS_NT = 1024;    // threads of the fold workgroup (16 waves)
constexpr size_t LDS_BUDGET = 160 * 1024 - 1024;
constexpr uint32_t TR_CH = 256;  // chunks (64 entries) a wave keeps in LDS: rows up to 16,384 entries
constexpr uint32_t HIST_BYTES = ((NBK + 1) * 4 + 15) & ~15u;
constexpr uint32_t WC = 31;   // weight classes at most (exact weights, or quantized: floor(w / q))
constexpr size_t SOLVE_HIST = 256;  // level ends, levels <= LWC
constexpr uint32_t LWC = 63;        // the level solve's classes / levels at most (CLSN 64)

// The LDS row of a workgroup, said once for the kernels that carve it and the
// hosts that size it: `hist` bytes of level ends, then for V vertices the
// levels u16 (at `hist`, rounded up to 16 B), the loss f32 bits (at
// lds_prow_off) and the members u16 (at lds_mem_off; rounded up too when
// mem16).  The kernels add these offsets to their dynamic LDS base themselves:
// a helper that takes the base as an argument changes the register
// allocation of the pipelined solve.  The quantized solve keeps one u64 key a
// vertex at SOLVE_HIST.
__host__ __device__ constexpr size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t lds_prow_off(size_t hist, size_t V) { return hist + up16(V * 2); }
__host__ __device__ constexpr size_t lds_mem_off(size_t hist, size_t V) { return lds_prow_off(hist, V) + V * 4; }
__host__ __device__ constexpr size_t fold_lds_bytes(size_t V) { return lds_mem_off(HIST_BYTES, V) + V * 2; }
// The packed row of the integer level solve (levels <= PACK_LMAX): `hist`,
// then one u32 key a vertex at SOLVE_HIST -- the loss's f32 bits in the low 30
// (a loss in [0, 1]: bits <= 0x3f800000), the state in the top 2 (3 unreached:
// the initial key is all ones; 1 entered the level being built; 0 settled, the
// loss final) -- then one 4-bit level a vertex (0xF until settled), the four
// vertices 4 k .. 4 k + 3 in the u16 word k at pack_lev_off.  4.5 B a vertex;
// the members live in a per-workgroup global scratch (level_scratch_bytes).
constexpr uint32_t PACK_LMAX = 14;      // the largest level a 4-bit field holds beside 0xF
constexpr uint32_t PACK_LOSS = 0x3fffffffu;  // a key's loss bits
constexpr uint32_t PACK_NT = 512;       // threads of a packed-row workgroup (two a CU: 4 waves a SIMD)
__host__ __device__ constexpr size_t pack_lev_off(size_t V) { return SOLVE_HIST + up16(V * 4); }
__host__ __device__ constexpr size_t solve_lds_bytes(size_t V, bool quant, bool packed = false) {
    return quant    ? SOLVE_HIST + V * 8
           : packed ? pack_lev_off(V) + up16((V + 3) / 4 * 2)
                    : lds_mem_off(SOLVE_HIST, V) + up16(V * 2);
}

template <typename K>
struct KeyLat;
template <>
struct KeyLat<uint16_t> {
    static __device__ __forceinline__ bool inf(uint16_t k) { return k >= KEY16_INF; }
    static __device__ __forceinline__ uint64_t lat(uint16_t k) { return k; }
};
template <>
struct KeyLat<uint32_t> {
    static __device__ __forceinline__ bool inf(uint32_t k) { return k >= KEY32_INF; }
    static __device__ __forceinline__ uint64_t lat(uint32_t k) { return k; }
};
template <>
struct KeyLat<double> {
    static __device__ __forceinline__ bool inf(double k) { return !(k < 9007199254740992.0); }
    static __device__ __forceinline__ uint64_t lat(double k) { return (uint64_t)k; }
};
template <>
struct KeyLat<uint64_t> {
    static __device__ __forceinline__ bool inf(uint64_t k) { return k >= KEY_INF; }
    static __device__ __forceinline__ uint64_t lat(uint64_t k) { return k; }
};

// latency (units of g) of closure entry idx; kt = srt_plan::key_type (uniform)
__device__ __forceinline__ uint64_t closure_lat(const void *D, uint64_t idx, int kt, bool &inf) {
    if (kt == KEY_U16) {
        const uint16_t k = reinterpret_cast<const uint16_t *>(D)[idx];
        inf = KeyLat<uint16_t>::inf(k);
        return k;
    }
    if (kt == KEY_U32) {
        const uint32_t k = reinterpret_cast<const uint32_t *>(D)[idx];
        inf = KeyLat<uint32_t>::inf(k);
        return k;
    }
    if (kt == KEY_F64) {
        const double k = reinterpret_cast<const double *>(D)[idx];
        inf = KeyLat<double>::inf(k);
        return inf ? 0 : KeyLat<double>::lat(k);
    }
    const uint64_t k = reinterpret_cast<const uint64_t *>(D)[idx];
    inf = KeyLat<uint64_t>::inf(k);
    return k;
}

// A non-pipelined class walk's step: UNR entries (VW = 1) or entry pairs (VW =
// 2: 16-B loads from the even entry at or below e0) a lane from ce + b, lane
// `sub` of LPT; ei: the entries' indices, ok: inside [e0, e1) (the arrays are
// padded past their end, so the loads are unconditional).
template <int UNR, int LPT, int VW>
__device__ __forceinline__ void load_entries(const uint64_t *__restrict__ ce, uint32_t b, uint32_t sub, uint32_t e0,
                                             uint32_t e1, uint64_t (&wd)[UNR * VW], uint32_t (&ei)[UNR * VW],
                                             bool (&ok)[UNR * VW]) {
#pragma unroll
    for (int q = 0; q < UNR; ++q) {
        const uint32_t at = b + (sub + q * LPT) * VW;
        if constexpr (VW == 2) {
            const uint4 r2 = *reinterpret_cast<const uint4 *>(ce + at);
            wd[2 * q] = ((uint64_t)r2.y << 32) | r2.x;
            wd[2 * q + 1] = ((uint64_t)r2.w << 32) | r2.z;
            ei[2 * q] = at;
            ei[2 * q + 1] = at + 1;
        } else {
            wd[q] = ce[at];
            ei[q] = at;
        }
    }
#pragma unroll
    for (int q = 0; q < UNR * VW; ++q) ok[q] = ei[q] < e1 && (VW == 1 || ei[q] >= e0);
}

#ifndef LOSS_COUNT
#define LOSS_COUNT 0
#endif
// diagnostic builds (-DLOSS_COUNT=1): a row's phase ticks (tk0: the phase's
// start) added to slot `slot` of the including unit's counter array `cnt`
#if LOSS_COUNT
#define LOSS_TICK_TO(cnt, slot)                                                  \
    if (tid == 0) {                                                              \
        const unsigned long long tk1 = wall_clock64();                           \
        atomicAdd(&cnt[slot], tk1 - tk0);                                        \
        tk0 = tk1;                                                               \
    }
#else
#define LOSS_TICK_TO(cnt, slot)
#endif

inline srt_status fail(srt_err *err, hipError_t e, const char *what) {
    const srt_status st = e == hipErrorOutOfMemory ? SRT_ERR_OOM : SRT_ERR_HIP;
    if (err) {
        err->code = st;
        std::snprintf(err->msg, sizeof err->msg, "%s: %s", what, hipGetErrorString(e));
    }
    return st;
}

template <typename T>
srt_status grow(T **p, uint64_t *cap, uint64_t need, srt_err *err, const char *what) {
    if (need <= *cap && *p) return SRT_OK;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max<uint64_t>(need, 1) * sizeof(T));
    if (e != hipSuccess) return fail(err, e, what);
    *p = (T *)q;
    *cap = need;
    return SRT_OK;
}

inline int cu_count(int dev) {
    static int cached[64] = {0};
    if (dev >= 0 && dev < 64 && cached[dev]) return cached[dev];
    int c = 256;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    if (dev >= 0 && dev < 64) cached[dev] = c;
    return c;
}

inline int bits_of(uint64_t x) {
    int b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

// rows: [row0, row1) of the table, or the sharded tail's row list (RowJob)
struct RowJob {
    const uint32_t *list = nullptr;  // device, count entries
    uint32_t count = 0;
    bool range = false;              // no list: table rows [r0, r1) instead of [row0, row1)
    uint32_t r0 = 0, r1 = 0;
    void *out32 = nullptr;           // staging row 0 (u16 or u32 latency units, see srt_plan::stage16)
    float *out32_loss = nullptr;
};

// the class offset and count arrays (p->tcls_cap entries each) for 2 * vc1
inline srt_status ensure_class_arrays(srt_plan *p, uint64_t vc1, srt_err *err) {
    uint64_t c1 = p->tcls_cap, c2 = p->tcls_cap;
    srt_status st = grow(&p->d_tcls, &c1, 2 * vc1, err, "hipMalloc(class offsets)");
    if (st == SRT_OK) st = grow(&p->d_tccnt, &c2, 2 * vc1, err, "hipMalloc(class counts)");
    p->tcls_cap = std::min(c1, c2);
    return st;
}

// rocPRIM's scan scratch (p->d_tscan_tmp) for `count` u32, and the scan itself
// on the plan's stream (scratch sized beforehand is not allocated again)
inline srt_status scan_scratch(srt_plan *p, size_t count, srt_err *err) {
    size_t need = 0;
    const hipError_t e = rocprim::exclusive_scan(nullptr, need, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, count,
                                                 rocprim::plus<uint32_t>(), p->stream);
    if (e != hipSuccess) return fail(err, e, "class scan (size)");
    uint64_t tcap = p->tscan_tmp_cap;
    const srt_status st =
        grow(reinterpret_cast<uint8_t **>(&p->d_tscan_tmp), &tcap, need + 256, err, "hipMalloc(scan scratch)");
    p->tscan_tmp_cap = tcap;
    return st;
}
inline srt_status exclusive_scan_u32(srt_plan *p, uint32_t *in, uint32_t *out, size_t count, srt_err *err) {
    const srt_status st = scan_scratch(p, count, err);
    if (st != SRT_OK) return st;
    size_t have = p->tscan_tmp_cap;
    const hipError_t e =
        rocprim::exclusive_scan(p->d_tscan_tmp, have, in, out, 0u, count, rocprim::plus<uint32_t>(), p->stream);
    return e == hipSuccess ? SRT_OK : fail(err, e, "class scan");
}

// an event pool grown to `count` events
inline srt_status ensure_events(std::vector<hipEvent_t> &ev, size_t count, unsigned flags, srt_err *err) {
    while (ev.size() < count) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, flags) != hipSuccess) return fail(err, hipErrorUnknown, "event");
        ev.push_back(e);
    }
    return SRT_OK;
}

// the sharded tails' row staging (d_slat / d_sloss: lrow_max rows of n pairs a rank, 4 B each)
inline srt_status ensure_row_staging(srt_plan *p, uint32_t W, srt_err *err) {
    if (p->d_slat) return SRT_OK;
    const size_t bytes = std::max<size_t>((size_t)p->lrow_max * p->n * W, 1) * 4;
    void *a = nullptr, *b = nullptr;
    hipError_t e = hipMalloc(&a, bytes);
    if (e == hipSuccess) e = hipMalloc(&b, bytes);
    if (e != hipSuccess) {
        (void)hipFree(a);
        return fail(err, e, "hipMalloc(row staging)");
    }
    p->d_slat = (uint32_t *)a;
    p->d_sloss = (float *)b;
    return SRT_OK;
}

}  // namespace

}  // namespace srt
