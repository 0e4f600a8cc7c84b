// srt_loss.hip -- exact packet_loss of the dense routing build ("K5"), gfx950.
//
// The blocked Floyd-Warshall (srt_fw.hip) closes LATENCIES only.  The
// reference's path cost is lexicographic (latency, loss) with loss folded from
// the source, one f32 rounding per op (graph/mod.rs:305-331):
//     l_0 = 0,  l_{k+1} = 1f32 - (1f32 - l_k) * (1f32 - e_k).
// petgraph's Dijkstra (strict `<`, visited set) returns for every target the
// lexicographic minimum over all paths; with latencies > 0 and the fold
// monotone in the prefix loss that is
//     loss[s][v] = min over tight in-edges (u -> v, e) of fold(loss[s][u], e),
//     tight: lat[s][u] + lat_e == lat[s][v],
// evaluated in increasing lat[s][.], loss[s][s] = 0.  Every tight predecessor
// has a strictly smaller latency, so it is final before v is read -- exactly
// what Dijkstra's settle order guarantees -- and the result is bit-identical.
//
// Two steps per build, after the closure:
//  1. tight-edge CSR.  An edge u -> v can be tight for some source only if its
//     own latency equals the closure's D[u][v] (else D[s][u] + D[u][v] would
//     beat it).  One pass over the adjacency flags those entries and counts
//     them per target, a scan and a fill build their pull CSR.  On the 16k
//     complete graph ~155 of the 16k in-edges per vertex survive.  When the
//     vertex index and the largest tight latency fit 32 bits together, an
//     entry is ONE u64, (1f32 - e) bits << 32 | (w << ubits) | u, and every
//     target's row is sorted by w (rocPRIM segmented radix sort on the w bits)
//     so a scan stops at the first w > lat[s][v].
//  2. fold.  One workgroup per table row (source s) keeps lat[s][.] and
//     loss[s][.] in LDS (8 B per vertex: 16k vertices = 128 KiB), buckets the
//     vertices by latency (counting sort: bucket = lat >> shift, shift chosen so
//     the row's range fits NBK buckets; wave-aggregated LDS atomics when the
//     row has few buckets; the sorted order holds 16-B records {v, first and
//     end in-edge, lat[s][v]}) and processes the buckets in increasing order,
//     LPT lanes per target scanning its tight in-edges, candidates min-ed into
//     loss[s][v] by LDS atomics on the f32 bits.  Bucket width 1 (shift 0)
//     needs one pass per bucket: a tight predecessor is always in an earlier
//     bucket.  Wider buckets repeat the bucket until a pass changes nothing
//     (monotone fixpoint of the same fold, so the same bits).  The row is then
//     written out: latency = lat * g, loss, the raw self-loop on the diagonal
//     (mod.rs:210-217), min latency and unreachable count reduced into stats
//     (mod.rs:219, 474-476).
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "srt_rowfold.h"

namespace srt {

namespace {

// push scan: edges a lane loads per step (C3: 2 / 4 / 8 / 16 -> 24.8 / 20.7 /
// 21.7 / 25.7 ms for the pass: a member's edges below its bound are few, so
// wider steps fetch past the bound and narrower ones expose the latency)
constexpr int PUNR = 4;

// ---------------------------------------------------------- tight-edge CSR
// Pass 1 (one wave per adjacency row u): flag entry k (u -> v = col[k], not a
// self-loop) when lat[k] == D[u][v] * g, count it for v, track the largest
// tight latency.
template <typename K>
__global__ void tight_flag_kernel(const K *__restrict__ D, uint32_t Vp, uint32_t u0, uint32_t u1,
                                  const uint64_t *__restrict__ row_ptr, const uint32_t *__restrict__ col,
                                  const uint64_t *__restrict__ lat, uint64_t g, uint8_t *__restrict__ flag,
                                  uint32_t *__restrict__ cnt, unsigned long long *maxw,
                                  unsigned long long *total) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    uint64_t mw = 0, tot = 0;
    for (uint32_t u = u0 + wave; u < u1; u += nwaves) {
        const K *Du = D + (uint64_t)u * Vp;
        const uint64_t b = row_ptr[u], e = row_ptr[u + 1];
        for (uint64_t k = b + lane; k < e; k += 64) {
            const uint32_t v = col[k];
            uint8_t f = 0;
            if (v != u) {
                const K d = Du[v];
                const uint64_t w = KeyLat<K>::lat(d);
                if (!KeyLat<K>::inf(d) && w * g == lat[k]) {
                    f = 1;
                    if (cnt) atomicAdd(&cnt[v], 1u);
                    mw = w > mw ? w : mw;
                    ++tot;
                }
            }
            flag[k] = f;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(mw, off);
        mw = o > mw ? o : mw;
        tot += __shfl_xor(tot, off);
    }
    if (lane == 0 && mw) atomicMax(maxw, (unsigned long long)mw);
    if (lane == 0 && total && tot) atomicAdd(total, (unsigned long long)tot);
}

// Sharded tail: the flagged entries of the rank's own adjacency rows [u0, u1)
// as records {v, u, w, 1f32 - e bits} at list[cursor..): a wave counts its
// row's flags, takes the row's range with one atomic (one per chunk would
// serialise ~10^6 atomics on the cursor), then writes them in order.
__global__ void tight_list_kernel(uint32_t u0, uint32_t u1, const uint64_t *__restrict__ row_ptr,
                                  const uint32_t *__restrict__ col, const uint64_t *__restrict__ lat,
                                  const float *__restrict__ loss, uint64_t g, const uint8_t *__restrict__ flag,
                                  uint4 *__restrict__ list, unsigned long long *cursor) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t u = u0 + wave; u < u1; u += nwaves) {
        const uint64_t b = row_ptr[u], e = row_ptr[u + 1];
        uint32_t cnt = 0;
        for (uint64_t k = b + lane; k < e; k += 64) cnt += flag[k];
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
        if (!cnt) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(cursor, (unsigned long long)cnt);
        base = __shfl(base, 0);
        for (uint64_t k0 = b; k0 < e; k0 += 64) {
            const uint64_t k = k0 + lane;
            const bool f = k < e && flag[k];
            const uint64_t m = __ballot(f);
            if (f) {
                const uint64_t pos = base + __popcll(m & ((1ull << lane) - 1ull));
                const float eb = 1.0f - loss[k];  // the reference's (1f32 - other.packet_loss), mod.rs:328
                list[pos] = make_uint4(col[k], u, (uint32_t)(lat[k] / g), __float_as_uint(eb));
            }
            base += __popcll(m);
        }
    }
}

// One GPU, packed forms: the tight edges of adjacency rows [0, V) straight
// into the list, one wave per row in two passes -- pass 1 tests each 64-entry
// chunk (w * g == lat and w == D[u][v]) and keeps its ballot in LDS (chunks
// past TR_CH are tested again in pass 2), one atomic takes the row's range,
// pass 2 writes the records of the set lanes.  No flag array: against the
// flag + list kernels (1.16 + 0.74 ms on C3) the adjacency is read once and
// the second pass touches only the tight entries.  Writes only when the whole
// row fits below cap (list slots); total and max w are always counted, so a
// run with cap 0 (or too small a list) counts and the caller runs it again.
template <typename K>
__global__ __launch_bounds__(256) void tight_rows_kernel(const K *__restrict__ D, uint32_t Vp, uint32_t V,
                                                         const uint64_t *__restrict__ row_ptr,
                                                         const uint32_t *__restrict__ col,
                                                         const uint64_t *__restrict__ lat,
                                                         const float *__restrict__ loss, uint64_t g,
                                                         uint4 *__restrict__ list, uint64_t cap,
                                                         unsigned long long *cursor, unsigned long long *maxw,
                                                         unsigned long long *total) {
    __shared__ uint64_t bal[4][TR_CH];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    uint64_t mw = 0, tot = 0, mnw = ~0ull;
    auto test = [&](uint32_t u, const K *Du, uint64_t k, uint64_t e) -> bool {
        if (k >= e) return false;
        const uint32_t v = col[k];
        if (v == u) return false;
        const K d = Du[v];
        const uint64_t w = KeyLat<K>::lat(d);
        return !KeyLat<K>::inf(d) && w * g == lat[k];
    };
    for (uint32_t u = wave; u < V; u += nwaves) {
        const K *Du = D + (uint64_t)u * Vp;
        const uint64_t b = row_ptr[u], e = row_ptr[u + 1];
        const uint32_t nch = (uint32_t)((e - b + 63) / 64);
        uint32_t cnt = 0;
        // 4 chunks per step: their col / lat loads, then their D loads, in flight together
        for (uint32_t c0 = 0; c0 < nch; c0 += 4) {
            uint32_t v[4];
            uint64_t l[4];
            K d[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t k = b + 64ull * (c0 + q) + lane;
                v[q] = k < e ? col[k] : u;
                l[q] = k < e ? lat[k] : 0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) d[q] = Du[v[q]];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t w = KeyLat<K>::lat(d[q]);
                const bool f = v[q] != u && !KeyLat<K>::inf(d[q]) && w * g == l[q];
                const uint64_t m = __ballot(f);
                if (f) {
                    mw = w > mw ? w : mw;
                    mnw = w < mnw ? w : mnw;
                }
                if (c0 + q < TR_CH && lane == 0) bal[wv][c0 + q] = m;
                cnt += (uint32_t)__popcll(m);
            }
        }
        if (!cnt) continue;
        tot += cnt;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(cursor, (unsigned long long)cnt);
        base = __shfl(base, 0);
        if (base + cnt > cap) continue;  // uniform: the caller grows the list and runs again
        for (uint32_t c = 0; c < nch; ++c) {
            const uint64_t k = b + 64ull * c + lane;
            const uint64_t m = c < TR_CH ? bal[wv][c] : __ballot(test(u, Du, k, e));
            if (!m) continue;  // uniform
            if ((m >> lane) & 1ull) {
                const uint64_t pos = base + __popcll(m & ((1ull << lane) - 1ull));
                const float eb = 1.0f - loss[k];  // the reference's (1f32 - other.packet_loss), mod.rs:328
                list[pos] = make_uint4(col[k], u, (uint32_t)(lat[k] / g), __float_as_uint(eb));
            }
            base += __popcll(m);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(mw, off);
        mw = o > mw ? o : mw;
        const uint64_t o2 = __shfl_xor(mnw, off);
        mnw = o2 < mnw ? o2 : mnw;
    }
    // tot is uniform per wave (ballot counts); total[1]: max of ~min w (zeroed by the caller)
    if (lane == 0 && mw) atomicMax(maxw, (unsigned long long)mw);
    if (lane == 0 && tot) {
        atomicAdd(total, (unsigned long long)tot);
        atomicMax(total + 1, (unsigned long long)~mnw);
    }
}

// Per-row counts of a tight-edge list (v = ~0: padding): rows by target v
// (pull CSR) or, BY_SRC, by source u (push CSR)
template <bool BY_SRC>
__global__ void tight_list_count_kernel(const uint4 *__restrict__ list, uint64_t slots, uint32_t *__restrict__ cnt,
                                        uint32_t nv) {
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < slots; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 r = list[e];
        if (r.x != ~0u && r.x < nv && r.y < nv) atomicAdd(&cnt[BY_SRC ? r.y : r.x], 1u);
    }
}

// ... and the packed CSR entries of the list: (1-e) bits << 32 | w << ubits |
// the other endpoint (u for pull rows, v for push rows)
template <bool BY_SRC>
__global__ void tight_list_fill_kernel(const uint4 *__restrict__ list, uint64_t slots,
                                       const uint64_t *__restrict__ ptr, uint32_t *__restrict__ cur,
                                       uint64_t *__restrict__ tpk, uint32_t ubits, uint32_t nv) {
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < slots; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 r = list[e];
        if (r.x == ~0u || r.x >= nv || r.y >= nv) continue;  // padding (or a record the transport damaged)
        const uint32_t row = BY_SRC ? r.y : r.x, other = BY_SRC ? r.x : r.y;
        const uint64_t pos = ptr[row] + atomicAdd(&cur[row], 1u);
        tpk[pos] = ((uint64_t)r.w << 32) | ((r.z << ubits) | other);
    }
}

// Sharded tail: every rank's staged rows into the table.  slot s = r * lrow_max
// + k holds table row lrows[s] (~0: padding) as latency units (~0:
// unreachable) and loss.
// Dfull (u16 keys, the symmetric sharded closure on every rank): the staging
// holds only the loss; latencies come from D (the diagonal: the self-loop).
__global__ void expand_rows_kernel(const uint32_t *__restrict__ lrows, uint32_t slots, uint32_t n,
                                   const void *__restrict__ slat, bool lat16, const float *__restrict__ sloss,
                                   uint64_t g, uint64_t *__restrict__ out_lat, float *__restrict__ out_loss,
                                   const uint16_t *__restrict__ Dfull, uint32_t Vp, const uint32_t *__restrict__ nodes,
                                   const uint64_t *__restrict__ sl_lat) {
    for (uint32_t sl = blockIdx.x; sl < slots; sl += gridDim.x) {
        const uint32_t i = lrows[sl];
        if (i == ~0u) continue;
        const uint16_t *s16 = reinterpret_cast<const uint16_t *>(slat) + (uint64_t)sl * n;
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(slat) + (uint64_t)sl * n;
        const float *sp = sloss + (uint64_t)sl * n;
        uint64_t *ol = out_lat + (uint64_t)i * n;
        float *op = out_loss + (uint64_t)i * n;
        const uint16_t *Drow = Dfull ? Dfull + (uint64_t)nodes[i] * Vp : nullptr;
        for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
            uint64_t l;
            if (j == i) {
                l = sl_lat[i];  // the raw self-loop: need not fit the staged latency field
            } else if (Drow) {
                const uint32_t x = Drow[nodes[j]];
                l = x >= KEY16_INF ? ~0ull : (uint64_t)x * g;
            } else if (lat16) {
                const uint32_t x = s16[j];
                l = x == 0xffffu ? ~0ull : (uint64_t)x * g;
            } else {
                const uint32_t x = s32[j];
                l = x == ~0u ? ~0ull : (uint64_t)x * g;
            }
            ol[j] = l;
            op[j] = sp[j];
        }
    }
}

// Single workgroup: ptr = exclusive scan of cnt (ptr[V] = total), cnt reset
// to 0 (the fill cursor).
__global__ __launch_bounds__(1024) void tight_scan_kernel(uint32_t *__restrict__ cnt, uint64_t *__restrict__ ptr,
                                                          uint32_t V) {
    __shared__ uint64_t wsum[16];
    const uint32_t t = threadIdx.x, per = (V + 1023) / 1024;
    const uint32_t b = std::min<uint32_t>(V, t * per), e = std::min<uint32_t>(V, b + per);
    uint64_t s = 0;
    for (uint32_t i = b; i < e; ++i) s += cnt[i];
    // inclusive scan of s over the block
    const int lane = t & 63, w = t >> 6;
    uint64_t x = s;
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (int k = 0; k < 16; ++k) {
        if (k < w) before += wsum[k];
        all += wsum[k];
    }
    uint64_t run = before + x - s;
    for (uint32_t i = b; i < e; ++i) {
        ptr[i] = run;
        run += cnt[i];
        cnt[i] = 0;
    }
    if (t == 0) ptr[V] = all;
}

// Pass 2: place every flagged entry into its target's pull row; PACKED: one
// u64 per entry, (1f32 - e) bits << 32 | (w << ubits) | u, else separate
// u / w / 1-e arrays.
template <typename LatT, bool PACKED>
__global__ void tight_fill_kernel(uint32_t V, const uint64_t *__restrict__ row_ptr, const uint32_t *__restrict__ col,
                                  const uint64_t *__restrict__ lat, const float *__restrict__ loss, uint64_t g,
                                  const uint8_t *__restrict__ flag, const uint64_t *__restrict__ ptr,
                                  uint32_t *__restrict__ cur, uint32_t *__restrict__ tu, LatT *__restrict__ tw,
                                  float *__restrict__ teb, uint64_t *__restrict__ tpk, uint32_t ubits) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t u = wave; u < V; u += nwaves) {
        const uint64_t b = row_ptr[u], e = row_ptr[u + 1];
        for (uint64_t k = b + lane; k < e; k += 64) {
            if (!flag[k]) continue;
            const uint32_t v = col[k];
            const uint64_t pos = ptr[v] + atomicAdd(&cur[v], 1u);
            const uint64_t w = lat[k] / g;
            const float eb = 1.0f - loss[k];  // the reference's (1f32 - other.packet_loss), mod.rs:328
            if constexpr (PACKED) {
                tpk[pos] = ((uint64_t)__float_as_uint(eb) << 32) | (((uint32_t)w << ubits) | u);
            } else {
                tu[pos] = u;
                tw[pos] = (LatT)w;
                teb[pos] = eb;
            }
        }
    }
}

// ------------------------------------------------------------------- fold
// The whole wave calls this (uniform trip counts): for every active lane,
// the old value of hist[b] + its rank among the wave's lanes with the same b,
// and hist[b] incremented by their count -- one LDS atomic per distinct b.
__device__ __forceinline__ uint32_t agg_inc(uint32_t *hist, uint32_t b, bool active) {
    const uint32_t lane = threadIdx.x & 63;
    uint64_t todo = __ballot(active);
    uint32_t res = 0;
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t lb = __builtin_amdgcn_readlane(b, leader);
        const uint64_t m = __ballot(active && b == lb) & todo;
        uint32_t base = 0;
        if (lane == (uint32_t)leader) base = atomicAdd(&hist[lb], (uint32_t)__popcll(m));
        base = __builtin_amdgcn_readlane(base, leader);
        if ((m >> lane) & 1ull) res = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        todo &= ~m;
    }
    return res;
}

// One pass over the members ord[m0, m1) of a bucket, packed form: LPT lanes
// per target, UNR in-edges per lane per step (loads in flight: the scan is
// latency bound).  The edge array is padded past its end, so the UNR loads of
// a step are unconditional (one 8-B load each:
// {word, 1-e}); a slot counts only if it is inside the row and its w <= lv
// (rows are sorted by w).  Tight
// candidates go into prow[v] by LDS atomic min on the f32 bits (non-negative
// floats order like their bits); a tight edge with w == lv can only start at
// s (every other vertex has latency >= 1), and those were pushed from s's
// adjacency row beforehand, so a lane stops at w >= lv.  ITER (buckets wider
// than one latency) also
// reports whether any value dropped.  The next target's record is loaded
// while the current one is scanned.
template <typename LatT, int LPT, int UNR, bool ITER>
__device__ __forceinline__ int scan_bucket_packed(const uint4 *__restrict__ ord, uint32_t m0, uint32_t m1,
                                                  uint32_t grp, uint32_t sub, uint32_t ngrp,
                                                  const uint64_t *__restrict__ tpk, const LatT *lrow, float *prow,
                                                  uint32_t ubits, uint32_t umask) {
    int changed = 0;
    uint32_t m = m0 + grp;
    uint4 rec = m < m1 ? ord[m] : make_uint4(0, 0, 0, 0);
    for (; m < m1; m += ngrp) {
        const uint4 cur = rec;
        if (m + ngrp < m1) rec = ord[m + ngrp];
        const uint32_t v = cur.x, e1 = cur.z;
        const LatT lv = (LatT)cur.w;
        const uint64_t *wp = tpk + cur.y + sub;
        uint32_t *dst = reinterpret_cast<uint32_t *>(prow) + v;
        for (uint32_t e = cur.y + sub; e < e1; e += UNR * LPT, wp += UNR * LPT) {
            uint64_t wd[UNR];
#pragma unroll
            for (int q = 0; q < UNR; ++q) wd[q] = wp[q * LPT];
            bool ok[UNR];
            uint32_t u[UNR];
            LatT need[UNR], lu[UNR];
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                const uint32_t lo = (uint32_t)wd[q], w = lo >> ubits;
                ok[q] = e + q * LPT < e1 && (LatT)w < lv;  // w == lv: only from s (pushed)
                u[q] = ok[q] ? lo & umask : 0u;
                need[q] = lv - (LatT)w;
            }
#pragma unroll
            for (int q = 0; q < UNR; ++q) lu[q] = lrow[u[q]];
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                if (ok[q] && lu[q] == need[q]) {
                    const float c = 1.0f - __fmul_rn(1.0f - prow[u[q]], __uint_as_float((uint32_t)(wd[q] >> 32)));
                    if constexpr (ITER) changed |= __float_as_uint(c) < atomicMin(dst, __float_as_uint(c));
                    else atomicMin(dst, __float_as_uint(c));
                }
            }
            if (!ok[UNR - 1]) break;
        }
    }
    return changed;
}

// Push form (the default when the tight out-edge CSR is built): ord's members
// are the sources u of the bucket, record {u, first tight out-edge, end, lim}
// with lim = max latency of the row + 1 - lat(u); u's final loss goes along
// each out-edge u -> v with w < lim (no target of the row is further away)
// where lat(v) == lat(u) + w, by LDS atomic min on prow[v].  Against the pull
// form's per-target bound (w < lat(v)) the row-wide bound scans far fewer
// edges on the dense configs (C3: a vertex two units away pushes only its
// one-unit edges).
template <typename LatT, int LPT, int UNR, bool ITER>
__device__ __forceinline__ int scan_bucket_push(const uint4 *__restrict__ ord, uint32_t m0, uint32_t m1,
                                                uint32_t grp, uint32_t sub, uint32_t ngrp,
                                                const uint64_t *__restrict__ tpk, const LatT *lrow, float *prow,
                                                uint32_t ubits, uint32_t umask, LatT maxp1) {
    int changed = 0;
    uint32_t m = m0 + grp;
    uint4 rec = m < m1 ? ord[m] : make_uint4(0, 0, 0, 0);
    for (; m < m1; m += ngrp) {
        const uint4 cur = rec;
        if (m + ngrp < m1) rec = ord[m + ngrp];
        const uint32_t e1 = cur.z;
        const LatT lim = (LatT)cur.w, lu = maxp1 - lim;
        const float onem = 1.0f - prow[cur.x];
        const uint64_t *wp = tpk + cur.y + sub;
        for (uint32_t e = cur.y + sub; e < e1; e += UNR * LPT, wp += UNR * LPT) {
            uint64_t wd[UNR];
#pragma unroll
            for (int q = 0; q < UNR; ++q) wd[q] = wp[q * LPT];
            bool ok[UNR];
            uint32_t v[UNR];
            LatT want[UNR], lv[UNR];
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                const uint32_t lo = (uint32_t)wd[q], w = lo >> ubits;
                ok[q] = e + q * LPT < e1 && (LatT)w < lim;
                v[q] = ok[q] ? lo & umask : 0u;
                want[q] = lu + (LatT)w;
            }
#pragma unroll
            for (int q = 0; q < UNR; ++q) lv[q] = lrow[v[q]];
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                if (ok[q] && lv[q] == want[q]) {
                    const float c = 1.0f - __fmul_rn(onem, __uint_as_float((uint32_t)(wd[q] >> 32)));
                    uint32_t *dst = reinterpret_cast<uint32_t *>(prow) + v[q];
                    if constexpr (ITER) changed |= __float_as_uint(c) < atomicMin(dst, __float_as_uint(c));
                    else atomicMin(dst, __float_as_uint(c));
                }
            }
            if (!ok[UNR - 1]) break;
        }
    }
    return changed;
}

template <typename LatT, bool LROWS, int LPT, bool PACKED, bool PUSH>
__global__ __launch_bounds__(LOSS_NT) void tight_loss_kernel(
    const void *__restrict__ D, int key_type, uint32_t Vp, uint32_t V, const uint32_t *__restrict__ nodes,
    uint32_t n, uint32_t row0, uint32_t row1, const uint64_t *__restrict__ tptr, const uint32_t *__restrict__ tu,
    const LatT *__restrict__ tw, const float *__restrict__ teb, const uint64_t *__restrict__ tpk, uint32_t ubits,
    uint64_t g, const uint64_t *__restrict__ sl_lat, const float *__restrict__ sl_loss,
    uint64_t *__restrict__ out_lat, float *__restrict__ out_loss, unsigned long long *stats,
    uint4 *__restrict__ ord_all, LatT *lat_all, float *loss_all, const uint64_t *__restrict__ row_ptr,
    const uint32_t *__restrict__ col, const uint64_t *__restrict__ elat, const float *__restrict__ eloss,
    const uint32_t *__restrict__ row_list, void *__restrict__ out32, float *__restrict__ out32_loss, bool stage16) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint64_t red[16];
    __shared__ unsigned long long red_min[16], red_cnt[16];
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem);
    LatT *lrow;
    float *prow;
    if constexpr (LROWS) {
        lrow = reinterpret_cast<LatT *>(smem + HIST_BYTES);
        prow = reinterpret_cast<float *>(smem + HIST_BYTES + (((size_t)V * sizeof(LatT) + 15) & ~(size_t)15));
    } else {
        lrow = lat_all + (size_t)blockIdx.x * V;
        prow = loss_all + (size_t)blockIdx.x * V;
    }
    // ord[pos] = {v, first tight in-edge, end, lat[s][v]} in bucket order: the
    // member loop needs one 16-B load per target, no tptr / lrow lookups
    uint4 *ord = ord_all + (size_t)blockIdx.x * V;
    const LatT LINF = (LatT)~(LatT)0;
    const uint32_t umask = (1u << ubits) - 1u;
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
    const uint32_t grp = tid / LPT, sub = tid % LPT, ngrp = nt / LPT;
    uint64_t mn = ~0ull;
    unsigned long long unreach = 0;

    // rows: [row0, row1) of the table, or (sharded tail) row_list[0, row1) --
    // then the row goes to slot k of the u32 staging (latency units, ~0 =
    // unreachable) instead of the table
    const uint32_t nrows = row_list ? row1 : row1 - row0;
    for (uint32_t k = blockIdx.x; k < nrows; k += gridDim.x) {
        const uint32_t i = row_list ? row_list[k] : row0 + k;
        const uint32_t s = nodes[i];
        // 1. the row's latencies (units of g) and its largest finite one
        uint64_t mx = 0;
        for (uint32_t v = tid; v < V; v += nt) {
            bool inf;
            const uint64_t l64 = closure_lat(D, (uint64_t)s * Vp + v, key_type, inf);
            const LatT l = inf ? LINF : (LatT)l64;
            lrow[v] = l;
            prow[v] = __builtin_inff();
            if (!inf && l64 > mx) mx = l64;
        }
        for (uint32_t b = tid; b <= (uint32_t)NBK; b += nt) hist[b] = 0;
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
        }
        if (lane == 0) red[wv] = mx;
        __syncthreads();
        mx = 0;
        for (int k = 0; k < nw; ++k) mx = red[k] > mx ? red[k] : mx;
        int shift = 0;
        while ((mx >> shift) >= (uint64_t)NBK) ++shift;
        const uint32_t nb = (uint32_t)(mx >> shift) + 1;
        const bool few = nb <= 64;  // uniform: aggregate the LDS atomics per wave
        // 2. counting sort of the reachable vertices (s excluded) by bucket
        for (uint32_t base = 0; base < V; base += nt) {
            const uint32_t v = base + tid;
            const LatT l = v < V ? lrow[v] : LINF;
            const bool ok = v < V && v != s && l != LINF;
            const uint32_t b = ok ? (uint32_t)((uint64_t)l >> shift) : 0u;
            if (few) agg_inc(hist, b, ok);
            else if (ok) atomicAdd(&hist[b], 1u);
        }
        if (tid == 0) prow[s] = 0.0f;  // petgraph's zero score (0 ns, 0.0)
        __syncthreads();
        // the one-hop tight paths: s's own edges s -> v with lat == lat[s][v]
        // (fold(0, e) = 1 - (1 - 0) (1 - e)); the pull scans then skip every
        // in-edge with w == lat[s][v], whose tail can only be s.  Push: s's
        // tight out-edges (w <= the row's max latency), else its adjacency row.
        if constexpr (PUSH) {
            const uint64_t p0 = tptr[s], p1 = tptr[s + 1];
            for (uint64_t k = p0 + tid; k < p1; k += nt) {
                const uint64_t wd = tpk[k];
                const uint32_t lo = (uint32_t)wd, w = lo >> ubits, v = lo & umask;
                if ((uint64_t)w <= mx && lrow[v] == (LatT)w) {
                    const float c = 1.0f - __fmul_rn(1.0f - 0.0f, __uint_as_float((uint32_t)(wd >> 32)));
                    atomicMin(reinterpret_cast<uint32_t *>(prow) + v, __float_as_uint(c));
                }
            }
        } else {
            for (uint64_t k = row_ptr[s] + tid; k < row_ptr[s + 1]; k += nt) {
                const uint32_t v = col[k];
                const LatT l = lrow[v];
                if (v != s && l != LINF && (uint64_t)l * g == elat[k]) {
                    const float c = 1.0f - __fmul_rn(1.0f - 0.0f, 1.0f - eloss[k]);
                    atomicMin(reinterpret_cast<uint32_t *>(prow) + v, __float_as_uint(c));
                }
            }
        }
        {  // exclusive scan of hist[0, NBK): each thread a contiguous run
            const uint32_t per = (NBK + nt - 1) / nt, b0 = std::min<uint32_t>(NBK, tid * per),
                           b1 = std::min<uint32_t>(NBK, b0 + per);
            uint32_t sum = 0;
            for (uint32_t b = b0; b < b1; ++b) sum += hist[b];
            uint32_t x = sum;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t y = __shfl_up(x, off);
                if (lane >= off) x += y;
            }
            __syncthreads();  // everyone has read red (max) before it is rewritten
            if (lane == 63) red[wv] = x;
            __syncthreads();
            uint32_t run = x - sum;
            for (int k = 0; k < wv; ++k) run += (uint32_t)red[k];
            for (uint32_t b = b0; b < b1; ++b) {
                const uint32_t c = hist[b];
                hist[b] = run;
                run += c;
            }
        }
        __syncthreads();
        for (uint32_t base = 0; base < V; base += nt) {
            const uint32_t v = base + tid;
            const LatT l = v < V ? lrow[v] : LINF;
            const bool ok = v < V && v != s && l != LINF;
            const uint32_t b = ok ? (uint32_t)((uint64_t)l >> shift) : 0u;
            uint32_t pos = 0;
            if (few) pos = agg_inc(hist, b, ok);
            else if (ok) pos = atomicAdd(&hist[b], 1u);
            if (ok)
                ord[pos] = make_uint4(v, (uint32_t)tptr[v], (uint32_t)tptr[v + 1],
                                      PUSH ? (uint32_t)(mx + 1 - (uint64_t)l) : (uint32_t)l);
        }
        __syncthreads();
        // hist[b] is now the end of bucket b (its start: hist[b-1], or 0)
        // 3. buckets in increasing latency
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t m0 = b ? hist[b - 1] : 0u, m1 = hist[b];
            if (m0 == m1) continue;  // uniform
            for (;;) {
                int changed = 0;
                if constexpr (PUSH) {
                    if (shift)
                        changed = scan_bucket_push<LatT, LPT, PUNR, true>(ord, m0, m1, grp, sub, ngrp, tpk, lrow, prow,
                                                                    ubits, umask, (LatT)(mx + 1));
                    else
                        scan_bucket_push<LatT, LPT, PUNR, false>(ord, m0, m1, grp, sub, ngrp, tpk, lrow, prow, ubits,
                                                           umask, (LatT)(mx + 1));
                } else if constexpr (PACKED) {
                    if (shift)
                        changed = scan_bucket_packed<LatT, LPT, 8, true>(ord, m0, m1, grp, sub, ngrp, tpk, lrow, prow,
                                                                      ubits, umask);
                    else
                        scan_bucket_packed<LatT, LPT, 8, false>(ord, m0, m1, grp, sub, ngrp, tpk, lrow, prow, ubits,
                                                             umask);
                } else {
                    for (uint32_t base = m0; base < m1; base += ngrp) {
                        const uint32_t m = base + grp;
                        const bool act = m < m1;
                        uint32_t v = 0;
                        float best = __builtin_inff();
                        if (act) {
                            const uint4 rec = ord[m];
                            v = rec.x;
                            const LatT lv = lrow[v];
                            const uint64_t e1 = tptr[v + 1];
                            for (uint64_t e = tptr[v] + sub; e < e1; e += 2 * LPT) {
                                const uint64_t e2 = e + LPT;
                                const bool h2 = e2 < e1;
                                const LatT w1 = tw[e], w2 = h2 ? tw[e2] : LINF;
                                const uint32_t u1 = tu[e], u2 = h2 ? tu[e2] : 0u;
                                const float b1 = teb[e], b2 = h2 ? teb[e2] : 0.0f;
                                if (w1 <= lv && lrow[u1] == lv - w1)
                                    best = fminf(best, 1.0f - __fmul_rn(1.0f - prow[u1], b1));
                                if (w2 <= lv && lrow[u2] == lv - w2)
                                    best = fminf(best, 1.0f - __fmul_rn(1.0f - prow[u2], b2));
                            }
                        }
#pragma unroll
                        for (int off = LPT / 2; off > 0; off >>= 1) best = fminf(best, __shfl_xor(best, off));
                        if (act && sub == 0 && best < prow[v]) {
                            prow[v] = best;
                            changed = 1;
                        }
                    }
                }
                const int any = __syncthreads_or(changed);
                if (shift == 0 || !any) break;  // width-1 buckets: one pass is exact
            }
        }
        // 4. table row i (or staging slot k)
        uint64_t *ol = out_lat + (uint64_t)i * n;
        float *op = out_loss + (uint64_t)i * n;
        // staging slot k: latency units as u16 (stage16: u16 keys, < 0x7fff)
        // or u32, ~0 = unreachable
        uint32_t *o32 = out32 && !stage16 ? reinterpret_cast<uint32_t *>(out32) + (uint64_t)k * n : nullptr;
        uint16_t *o16 = out32 && stage16 ? reinterpret_cast<uint16_t *>(out32) + (uint64_t)k * n : nullptr;
        float *o32p = out32_loss ? out32_loss + (uint64_t)k * n : nullptr;  // staging (loss only if !out32)
        for (uint32_t j = tid; j < n; j += nt) {
            uint64_t latv;
            float lossv;
            if (j == i) {
                latv = sl_lat[j];
                lossv = sl_loss[j];
            } else {
                const uint32_t v = nodes[j];
                const LatT l = lrow[v];
                if (l == LINF) {
                    ++unreach;
                    latv = ~0ull;
                    lossv = 1.0f;
                } else {
                    latv = (uint64_t)l * g;
                    lossv = prow[v];
                }
            }
            if (o32p) {
                if (o16) o16[j] = latv == ~0ull ? (uint16_t)0xffffu : (uint16_t)(latv / g);
                else if (o32) o32[j] = latv == ~0ull ? ~0u : (uint32_t)(latv / g);
                o32p[j] = lossv;
            } else {
                ol[j] = latv;
                op[j] = lossv;
            }
            mn = latv < mn ? latv : mn;
        }
        __syncthreads();  // the next row rewrites the LDS rows
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(mn, off);
        mn = o < mn ? o : mn;
        unreach += __shfl_xor(unreach, off);
    }
    if (lane == 0) {
        red_min[wv] = mn;
        red_cnt[wv] = unreach;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = red_min[0], c = red_cnt[0];
        for (int k = 1; k < nw; ++k) {
            m = red_min[k] < m ? red_min[k] : m;
            c += red_cnt[k];
        }
        atomicMin(&stats[0], m);
        if (c) atomicAdd(&stats[1], c);
    }
}

// --------------------------------------------------------------- level fold
// The pull form scans, for every target v of a row, its tight in-edges with
// w < lat[s][v]; the push form scans, for every u, its tight out-edges up to
// the row's largest latency.  Both walk ~10x more edges than end up tight for
// the row (C3: ~1.9M edge tests a row for ~0.27M tight ones).  With the
// vertices grouped by latency level (N_l = {v : lat[s][v] = l}, N_0 = {s})
// the candidates of level l are exactly the edges u -> v, u in N_j, v in N_l,
// of weight w = l - j, and for each weight class w that set can be walked
// from either end: push from N_j along class-w out-edges, or pull into N_l
// along class-w in-edges -- whichever level is smaller (a class's out- and
// in-degrees are alike).  C3: ~0.26M edge tests a row.  Every candidate is
// the same fold(loss[s][u], e) either way, min-ed into loss[s][v] by LDS
// atomics, and level j < l is final before level l starts (one barrier per
// level), so the result is the same bits as the single-direction scans.
//
// Class CSRs (built from the tight-edge list, no sort): out-rows and in-rows
// grouped by exact weight w = 1..WC; tcls[x*cls + w-1] .. tcls[x*cls + w] is
// class w of vertex x.  Applies when every tight edge has w <= WC, every
// closure latency is < NBK units (proof bound lmax), V < 65536 (u16 member
// lists) and the row fits LDS: lat u16 + loss f32 + members u16 (8 B/vertex).
// offsets per vertex (p->t_cls: classes 1..cls-1, then the end): 16 when
// every class is <= 15 (C3: half the offset arrays of 32, 6.8 vs 7.0 ms), else 32

// class of a tight weight w: w itself (q = 1), else floor(w / q) (quantized
// levels, q = the smallest tight weight)
__device__ __forceinline__ uint32_t wclass(uint32_t w, uint32_t q) { return q == 1 ? w : w / q; }

__global__ void tcls_count_kernel(const uint4 *__restrict__ list, uint64_t slots, uint32_t *__restrict__ cnt,
                                  uint64_t vc1, uint32_t q, uint32_t cls) {
    const uint64_t nv = (vc1 - 1) / cls;
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < slots; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 r = list[e];
        if (r.x == ~0u) continue;
        const uint32_t c = wclass(r.z, q);
        if (r.x >= nv || r.y >= nv || c == 0 || c >= cls) continue;  // a record the transport damaged
        atomicAdd(&cnt[(uint64_t)r.y * cls + c - 1], 1u);        // out-row of u
        atomicAdd(&cnt[vc1 + (uint64_t)r.x * cls + c - 1], 1u);  // in-row of v
    }
}

__global__ void tcls_fill_kernel(const uint4 *__restrict__ list, uint64_t slots, const uint32_t *__restrict__ off,
                                 uint32_t *__restrict__ cur, uint64_t *__restrict__ ce_out,
                                 uint64_t *__restrict__ ce_in, uint64_t vc1, uint32_t q, uint32_t *__restrict__ cw,
                                 uint64_t cw_in, uint32_t cls) {
    const uint64_t nv = (vc1 - 1) / cls;
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < slots; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 r = list[e];
        if (r.x == ~0u) continue;
        const uint32_t c = wclass(r.z, q);
        if (r.x >= nv || r.y >= nv || c == 0 || c >= cls) continue;
        const uint64_t a = (uint64_t)r.y * cls + c - 1, b = vc1 + (uint64_t)r.x * cls + c - 1;
        const uint64_t ia = off[a] + atomicAdd(&cur[a], 1u), ib = off[b] + atomicAdd(&cur[b], 1u);
        ce_out[ia] = ((uint64_t)r.w << 32) | r.x;
        ce_in[ib] = ((uint64_t)r.w << 32) | r.y;
        if (cw) {  // quantized classes: the exact weight beside each entry
            cw[ia] = r.z;
            cw[cw_in + ib] = r.z;
        }
    }
}

// One workgroup per table row, 16 waves.  LDS: hist (level ends), lat u16
// (0xffff: unreachable), loss f32 bits, members u16 (the vertices in level
// order, counting sort).  Output as tight_loss_kernel.
// QUANT (level width qw > 1, see level_q): lrow holds floor(L / qw); a class-c
// edge's tail lies in level l - c or l - c - 1, and a candidate is taken only
// when L(s,u) + w == L(s,v) exactly (the closure row's exact values, read from
// D; the class entries' weights from cw).  The output latencies come from D.
#if LOSS_COUNT
__device__ unsigned long long loss_cnt[9];  // diagnostic builds: items, edge visits, hits, levels, phase ticks x4, push hits
#endif
#define LOSS_TICK(slot) LOSS_TICK_TO(loss_cnt, slot)
template <int LPT, int UNR, bool QUANT, uint32_t CLSN, int VW>
__global__ __launch_bounds__(LOSS_NT) void level_loss_kernel(
    const void *__restrict__ D, int key_type, uint32_t Vp, uint32_t V, const uint32_t *__restrict__ nodes, uint32_t n,
    uint32_t row0, uint32_t row1, const uint32_t *__restrict__ tcls, uint64_t vc1,
    const uint64_t *__restrict__ ce_out, const uint64_t *__restrict__ ce_in, uint64_t g,
    const uint64_t *__restrict__ sl_lat, const float *__restrict__ sl_loss, uint64_t *__restrict__ out_lat,
    float *__restrict__ out_loss, unsigned long long *stats, const uint32_t *__restrict__ row_list,
    void *__restrict__ out32, float *__restrict__ out32_loss, bool stage16, uint32_t qw,
    const uint32_t *__restrict__ cw, uint64_t cw_in) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint64_t red[16];
    __shared__ unsigned long long red_min[16], red_cnt[16];
    constexpr uint32_t WCN = CLSN - 1;
    __shared__ uint32_t plan_end[WCN + 1];  // inclusive prefix of the class item counts
    __shared__ uint32_t wcnt[16][32];      // few-level sort: per-wave level counts, then bases
    __shared__ uint32_t plan_push;         // bit w: class w pushes from N_{l-w}
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem);
    uint16_t *lrow = reinterpret_cast<uint16_t *>(smem + HIST_BYTES);
    uint32_t *prow = reinterpret_cast<uint32_t *>(smem + lds_prow_off(HIST_BYTES, V));
    uint16_t *mem = reinterpret_cast<uint16_t *>(smem + lds_mem_off(HIST_BYTES, V));
    const uint16_t LINF = 0xffffu;
    const uint32_t FINF = 0x7f800000u;  // +inf bits
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
    const uint32_t grp = tid / LPT, sub = tid % LPT, ngrp = nt / LPT;
    const uint32_t *cls_out = tcls, *cls_in = tcls + vc1;
    uint64_t mn = ~0ull;
    unsigned long long unreach = 0;
#if LOSS_COUNT
    uint32_t c_vis = 0, c_hit = 0, c_phit = 0;
#endif
    const uint32_t nrows = row_list ? row1 : row1 - row0;
    for (uint32_t k = blockIdx.x; k < nrows; k += gridDim.x) {
        const uint32_t i = row_list ? row_list[k] : row0 + k;
        const uint32_t s = nodes[i];
#if LOSS_COUNT
        unsigned long long tk0 = wall_clock64();
#endif
        // 1. the row's latencies (units of g, < NBK by the host's proof bound)
        uint32_t mx = 0;
        auto put = [&](uint32_t v, bool inf, uint64_t l64) {
            const uint16_t l = inf ? LINF : v == s ? (uint16_t)0 : (uint16_t)(QUANT ? l64 / qw : l64);
            lrow[v] = l;
            prow[v] = v == s ? 0u : FINF;  // petgraph's zero score (0 ns, 0.0) at s
            if (l != LINF && l > mx) mx = l;
        };
        if (key_type == KEY_U16 && (Vp & 7u) == 0) {
            // 2-byte keys: 8 a thread in one 16-byte load (C3: 2 loads a
            // thread instead of 16 dependent round trips; the row is padded to Vp)
            const uint16_t *Dr = reinterpret_cast<const uint16_t *>(D) + (uint64_t)s * Vp;
            for (uint32_t v8 = tid * 8; v8 < V; v8 += nt * 8) {
                const uint4 raw = *reinterpret_cast<const uint4 *>(Dr + v8);
                auto put2 = [&](uint32_t v, uint32_t wd) {
                    const uint16_t k0 = (uint16_t)wd, k1 = (uint16_t)(wd >> 16);
                    if (v < V) put(v, k0 >= KEY16_INF, k0);
                    if (v + 1 < V) put(v + 1, k1 >= KEY16_INF, k1);
                };
                put2(v8, raw.x);
                put2(v8 + 2, raw.y);
                put2(v8 + 4, raw.z);
                put2(v8 + 6, raw.w);
            }
        } else {
            for (uint32_t v = tid; v < V; v += nt) {
                bool inf;
                const uint64_t l64 = closure_lat(D, (uint64_t)s * Vp + v, key_type, inf);
                put(v, inf, l64);
            }
        }
        for (uint32_t b = tid; b <= (uint32_t)NBK; b += nt) hist[b] = 0;
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
        }
        if (lane == 0) red[wv] = mx;
        __syncthreads();
        mx = 0;
        for (int q = 0; q < nw; ++q) mx = red[q] > mx ? (uint32_t)red[q] : mx;
        LOSS_TICK(4)
        // 2. counting sort of the reachable vertices (s at level 0) by level.
        // Few levels (mx < 32, C3: ~6): one ballot per level and 64-vertex
        // chunk, a wave's count of level l in lane l; the per-wave counts are
        // scanned level-major, so every wave places its chunks' vertices at
        // its own bases without atomics.  Else LDS atomics per distinct level.
        if (mx < 32) {
            uint32_t mine = 0;  // lane l: this wave's vertices at level l
            for (uint32_t base = 0; base < V; base += nt) {
                const uint32_t v = base + tid;
                const uint16_t l = v < V ? lrow[v] : LINF;
                for (uint32_t q = 0; q <= mx; ++q) {
                    const uint64_t m = __ballot(l == q);
                    if (lane == (int)q) mine += (uint32_t)__popcll(m);
                }
            }
            if (lane < 32) wcnt[wv][lane] = lane <= (int)mx ? mine : 0u;
            __syncthreads();
            if (wv == 0 && lane < 32) {
                uint32_t tot = 0;
                for (int q = 0; q < nw; ++q) tot += wcnt[q][lane];
                uint32_t x = tot;  // inclusive scan over the levels (lanes 0..31)
                for (int off = 1; off < 32; off <<= 1) {
                    const uint32_t y = __shfl_up(x, off, 32);
                    if (lane >= off) x += y;
                }
                uint32_t run = x - tot;  // start of level `lane`
                for (int q = 0; q < nw; ++q) {
                    const uint32_t c = wcnt[q][lane];
                    wcnt[q][lane] = run;
                    run += c;
                }
                if (lane <= (int)mx) hist[lane] = x;  // end of level `lane`
            }
            __syncthreads();
            uint32_t at = wcnt[wv][lane & 31];  // lane l: where this wave's next level-l vertex goes
            for (uint32_t base = 0; base < V; base += nt) {
                const uint32_t v = base + tid;
                const uint16_t l = v < V ? lrow[v] : LINF;
                for (uint32_t q = 0; q <= mx; ++q) {
                    const uint64_t m = __ballot(l == q);
                    if (!m) continue;  // uniform
                    const uint32_t b = __builtin_amdgcn_readlane(at, q);
                    if (l == q) mem[b + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)v;
                    if (lane == (int)q) at += (uint32_t)__popcll(m);
                }
            }
            __syncthreads();
        } else {
        for (uint32_t base = 0; base < V; base += nt) {
            const uint32_t v = base + tid;
            const uint16_t l = v < V ? lrow[v] : LINF;
            const bool ok = l != LINF;
            if (ok) atomicAdd(&hist[l], 1u);
        }
        __syncthreads();
        {  // exclusive scan of hist[0, NBK): each thread a contiguous run
            const uint32_t per = (NBK + nt - 1) / nt, b0 = std::min<uint32_t>(NBK, tid * per),
                           b1 = std::min<uint32_t>(NBK, b0 + per);
            uint32_t sum = 0;
            for (uint32_t b = b0; b < b1; ++b) sum += hist[b];
            uint32_t x = sum;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t y = __shfl_up(x, off);
                if (lane >= off) x += y;
            }
            __syncthreads();  // everyone has read red (max) before it is rewritten
            if (lane == 63) red[wv] = x;
            __syncthreads();
            uint32_t run = x - sum;
            for (int q = 0; q < wv; ++q) run += (uint32_t)red[q];
            for (uint32_t b = b0; b < b1; ++b) {
                const uint32_t c = hist[b];
                hist[b] = run;
                run += c;
            }
        }
        __syncthreads();
        for (uint32_t base = 0; base < V; base += nt) {
            const uint32_t v = base + tid;
            const uint16_t l = v < V ? lrow[v] : LINF;
            const bool ok = l != LINF;
            if (ok) mem[atomicAdd(&hist[l], 1u)] = (uint16_t)v;
        }
        __syncthreads();
        }
        // hist[l] is now the end of level l (its start: hist[l-1], or 0)
        LOSS_TICK(5)
        // 3. levels in increasing latency, every weight class from its smaller end
        for (uint32_t l = 1; l <= mx; ++l) {
            const uint32_t lo = hist[l - 1], cnt_l = hist[l] - lo;
            if (!cnt_l) continue;  // uniform
            if (tid == 0) {
                uint32_t run = 0, pm = 0;
                for (uint32_t w = 1; w <= WCN; ++w) {
                    uint32_t items = 0;
                    if (w <= l) {
                        // the tails' levels: l - w (and, quantized, l - w - 1)
                        const uint32_t j = l - w, jl = QUANT && j ? j - 1 : j;
                        const uint32_t nj = hist[j] - (jl ? hist[jl - 1] : 0u);
                        if (nj <= cnt_l) pm |= 1u << w;
                        items = nj < cnt_l ? nj : cnt_l;
                    }
                    run += items;
                    plan_end[w] = run;
                }
                plan_push = pm;
            }
            __syncthreads();
            const uint32_t T = plan_end[WCN], pm = plan_push;
            // item t -> (class w, member x, its edge range); the next item's
            // range is loaded while the current one is walked
            auto item = [&](uint32_t t, uint32_t &w, uint32_t &x, uint32_t &e0, uint32_t &e1) {
                w = 1;
                while (t >= plan_end[w]) ++w;
                const uint32_t m = t - (w > 1 ? plan_end[w - 1] : 0u), j = l - w, jl = QUANT && j ? j - 1 : j;
                const bool push = (pm >> w) & 1u;
                x = mem[(push ? (jl ? hist[jl - 1] : 0u) : lo) + m];
                const uint32_t *cl = push ? cls_out : cls_in;
                e0 = cl[(uint64_t)x * CLSN + w - 1];
                e1 = cl[(uint64_t)x * CLSN + w];
            };
            uint32_t nw_ = 1, nx = 0, ne0 = 0, ne1 = 0;
#if LOSS_COUNT
            if (tid == 0) { atomicAdd(&loss_cnt[0], (unsigned long long)T); atomicAdd(&loss_cnt[3], 1ull); }
#endif
            if (grp < T) item(grp, nw_, nx, ne0, ne1);
            for (uint32_t t = grp; t < T; t += ngrp) {
                const uint32_t w = nw_, x = nx, e0 = ne0, e1 = ne1, j = l - w;
                if (t + ngrp < T) item(t + ngrp, nw_, nx, ne0, ne1);
                const bool push = (pm >> w) & 1u;
                const uint64_t *ce = push ? ce_out : ce_in;
                // push: x in N_j, its class-w out-edges x -> v, v in N_l;
                // pull: x in N_l, its class-w in-edges u -> x, u in N_j
                const uint16_t want = (uint16_t)(push ? l : j);
                const float onem = push ? 1.0f - __uint_as_float(prow[x]) : 0.0f;
                // exact closure values of the quantized fold (2- or 4-byte keys, level_q)
                auto exact = [&](uint32_t y) -> uint32_t {
                    const uint64_t idx = (uint64_t)s * Vp + y;
                    return key_type == KEY_U16 ? (uint32_t)reinterpret_cast<const uint16_t *>(D)[idx]
                                               : reinterpret_cast<const uint32_t *>(D)[idx];
                };
                const uint32_t Lx = QUANT ? exact(x) : 0u;
                const uint32_t *cwp = QUANT ? cw + (push ? 0 : cw_in) : nullptr;
                // VW = 2: a lane loads 2 adjacent entries (16 B) at a time from
                // the even entry at or below e0, masking the entries outside [e0, e1)
                constexpr int NE = UNR * VW;  // entries a lane an iteration
                for (uint32_t b = VW == 2 ? e0 & ~1u : e0; b < e1; b += UNR * LPT * VW) {
                    uint64_t wd[NE];
                    uint32_t ei[NE], o[NE];
                    bool ok[NE];
                    load_entries<UNR, LPT, VW>(ce, b, sub, e0, e1, wd, ei, ok);
#pragma unroll
                    for (int q = 0; q < NE; ++q) o[q] = ok[q] ? (uint32_t)wd[q] : 0u;
                    uint16_t lo_[NE];
#pragma unroll
                    for (int q = 0; q < NE; ++q) lo_[q] = lrow[o[q]];
                    bool hit[NE];
#pragma unroll
                    for (int q = 0; q < NE; ++q) {
                        if (!QUANT) {
                            hit[q] = ok[q] && lo_[q] == want;
                        } else {
                            // the tail's level (j or j - 1) or the head's (l), then exact
                            hit[q] = ok[q] && (push ? lo_[q] == want : lo_[q] == want || lo_[q] + 1 == want);
                            if (hit[q]) {
                                const uint32_t Lo = exact(o[q]), wq = cwp[ei[q]];
                                hit[q] = push ? Lx + wq == Lo : Lo + wq == Lx;  // finite: no wrap below 2^31
                            }
                        }
                    }
#if LOSS_COUNT
                    for (int q = 0; q < NE; ++q) {
                        c_vis += ok[q];
                        c_hit += hit[q];
                        c_phit += push && hit[q];
                    }
#endif
#pragma unroll
                    for (int q = 0; q < NE; ++q) {
                        if (hit[q]) {
                            const float r = __uint_as_float((uint32_t)(wd[q] >> 32));
                            if (push) {
                                const float c = 1.0f - __fmul_rn(onem, r);
                                atomicMin(&prow[o[q]], __float_as_uint(c));
                            } else {
                                const float c = 1.0f - __fmul_rn(1.0f - __uint_as_float(prow[o[q]]), r);
                                atomicMin(&prow[x], __float_as_uint(c));
                            }
                        }
                    }
                }
            }
            __syncthreads();  // level l final; plan_end rewritten by the next level
        }
        LOSS_TICK(6)
        // 4. table row i (or staging slot k)
        uint64_t *ol = out_lat + (uint64_t)i * n;
        float *op = out_loss + (uint64_t)i * n;
        uint32_t *o32 = out32 && !stage16 ? reinterpret_cast<uint32_t *>(out32) + (uint64_t)k * n : nullptr;
        uint16_t *o16 = out32 && stage16 ? reinterpret_cast<uint16_t *>(out32) + (uint64_t)k * n : nullptr;
        float *o32p = out32_loss ? out32_loss + (uint64_t)k * n : nullptr;  // staging (loss only if !out32)
        // (4 node ids loaded ahead a thread; the staged latency is the
        // closure's unit count, no division by g)
        for (uint32_t j0 = tid; j0 < n; j0 += 4 * nt) {
            uint32_t vv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) vv[q] = j0 + q * nt < n ? nodes[j0 + q * nt] : 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t j = j0 + q * nt;
                if (j >= n) break;
                uint64_t latv, lu;
                float lossv;
                if (j == i) {
                    latv = sl_lat[j];
                    lossv = sl_loss[j];
                    lu = latv == ~0ull ? ~0ull : latv / g;
                } else {
                    const uint32_t v = vv[q];
                    const uint16_t l = lrow[v];
                    if (l == LINF) {
                        ++unreach;
                        latv = lu = ~0ull;
                        lossv = 1.0f;
                    } else {
                        bool vinf;
                        lu = QUANT ? closure_lat(D, (uint64_t)s * Vp + v, key_type, vinf) : (uint64_t)l;
                        latv = lu * g;
                        lossv = __uint_as_float(prow[v]);
                    }
                }
                if (o32p) {
                    if (o16) o16[j] = latv == ~0ull ? (uint16_t)0xffffu : (uint16_t)lu;
                    else if (o32) o32[j] = latv == ~0ull ? ~0u : (uint32_t)lu;
                    o32p[j] = lossv;
                } else {
                    ol[j] = latv;
                    op[j] = lossv;
                }
                mn = latv < mn ? latv : mn;
            }
        }
        __syncthreads();  // the next row rewrites the LDS rows
        LOSS_TICK(7)
    }
#if LOSS_COUNT
    atomicAdd(&loss_cnt[1], (unsigned long long)c_vis);
    atomicAdd(&loss_cnt[2], (unsigned long long)c_hit);
    atomicAdd(&loss_cnt[8], (unsigned long long)c_phit);
#endif
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(mn, off);
        mn = o < mn ? o : mn;
        unreach += __shfl_xor(unreach, off);
    }
    if (lane == 0) {
        red_min[wv] = mn;
        red_cnt[wv] = unreach;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = red_min[0], c = red_cnt[0];
        for (int q = 1; q < nw; ++q) {
            m = red_min[q] < m ? red_min[q] : m;
            c += red_cnt[q];
        }
        atomicMin(&stats[0], m);
        if (c) atomicAdd(&stats[1], c);
    }
}

__global__ void loss_stats_init_kernel(unsigned long long *stats, unsigned long long *maxw) {
    stats[0] = ~0ull;
    stats[1] = 0ull;
    *maxw = 0ull;
}

template <typename LatT, bool LROWS, int LPT, bool PACKED, bool PUSH>
srt_status launch_fold(srt_plan *p, unsigned long long *d_stats, uint32_t ubits, const RowJob &job, srt_err *err) {
    const uint32_t V = p->V, rows = job.list ? job.count : job.range ? job.r1 - job.r0 : p->row1 - p->row0;
    const uint32_t nt = V >= 2048 ? LOSS_NT : 256;
    const size_t lds = LROWS ? HIST_BYTES + (((size_t)V * sizeof(LatT) + 15) & ~(size_t)15) + (size_t)V * 4
                             : HIST_BYTES;
    const int per_cu_threads = 2048 / (int)nt;
    const int per_cu_lds = (int)std::max<size_t>(1, (160 * 1024) / (lds + 2048));
    const int per_cu = std::max(1, std::min(per_cu_threads, per_cu_lds));
    const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(rows, (uint32_t)(cu_count(p->device) * per_cu)));
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t ord_b = up16((size_t)grid * V * 16), lat_b = LROWS ? 0 : up16((size_t)grid * V * sizeof(LatT)),
                 loss_b = LROWS ? 0 : up16((size_t)grid * V * 4);
    uint64_t cap = p->lscratch_cap;
    srt_status st = grow(reinterpret_cast<uint8_t **>(&p->d_lscratch), &cap, ord_b + lat_b + loss_b + 64, err,
                         "hipMalloc(loss scratch)");
    p->lscratch_cap = cap;
    if (st != SRT_OK) return st;
    uint8_t *base = reinterpret_cast<uint8_t *>(p->d_lscratch);
    uint4 *ord = reinterpret_cast<uint4 *>(base);
    LatT *lat_all = reinterpret_cast<LatT *>(base + ord_b);
    float *loss_all = reinterpret_cast<float *>(base + ord_b + lat_b);
    auto kern = tight_loss_kernel<LatT, LROWS, LPT, PACKED, PUSH>;
    // set on every launch (cheap): a once-per-process flag would miss a
    // second device and race between plans built concurrently
    if (LROWS)
        (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(LDS_BUDGET - 4096));
    if (rows)
        hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), lds, p->stream, (const void *)p->d_D, p->key_type, p->Vp, V,
                           p->d_nodes, p->n, job.list ? 0u : job.range ? job.r0 : p->row0,
                           job.list ? job.count : job.range ? job.r1 : p->row1, p->d_tptr, p->d_tu,
                           reinterpret_cast<const LatT *>(p->d_tw), p->d_teb, p->d_tpk, ubits, p->kp.g, p->d_sl_lat,
                           p->d_sl_loss, p->d_out_lat, p->d_out_loss, d_stats, ord, lat_all, loss_all, p->d_row_ptr,
                           p->d_col, p->d_lat, p->d_loss, job.list, job.out32, job.out32_loss, p->stage16);
    return SRT_OK;
}

template <typename LatT, bool LROWS, bool PACKED>
srt_status launch_fold_lpt(srt_plan *p, unsigned long long *d_stats, uint32_t ubits, const RowJob &job,
                           srt_err *err) {
    // lanes per target ~ the average tight in-degree (a group walks a target's
    // in-edges 2-4 per lane per step)
    const double avg = p->V ? (double)p->t_edges / p->V : 0.0;
    if constexpr (PACKED) {
        if (p->t_push) {
            if (avg > 10.0) return launch_fold<LatT, LROWS, 4, true, true>(p, d_stats, ubits, job, err);
            return launch_fold<LatT, LROWS, 2, true, true>(p, d_stats, ubits, job, err);
        }
        // 4 lanes x 8 edges per target (C3, same box: 4 / 8 / 16 lanes ->
        // 31.9 / 33.0 / 36.5 ms for the pass)
        if (avg > 10.0) return launch_fold<LatT, LROWS, 4, PACKED, false>(p, d_stats, ubits, job, err);
        return launch_fold<LatT, LROWS, 2, PACKED, false>(p, d_stats, ubits, job, err);
    }
    if (avg > 48.0) return launch_fold<LatT, LROWS, 32, PACKED, false>(p, d_stats, ubits, job, err);
    if (avg > 10.0) return launch_fold<LatT, LROWS, 8, PACKED, false>(p, d_stats, ubits, job, err);
    return launch_fold<LatT, LROWS, 2, PACKED, false>(p, d_stats, ubits, job, err);
}

// tight edge arrays for p->t_edges entries (grown together, 25% headroom;
// +1024: the packed scan reads up to (UNR - 1) * LPT entries past a row's end)
srt_status ensure_edge_arrays(srt_plan *p, srt_err *err) {
    if (p->t_edges + 1024 <= p->t_cap && p->d_tu) return SRT_OK;
    const size_t wsz = p->kp.lat32 ? 4 : 8;
    const uint64_t cap = std::max<uint64_t>(p->t_edges + p->t_edges / 4 + 1024, 2048);
    for (void *q : {(void *)p->d_tu, p->d_tw, (void *)p->d_teb, (void *)p->d_tpk, (void *)p->d_tpk2}) (void)hipFree(q);
    p->d_tu = nullptr;
    p->d_tw = nullptr;
    p->d_teb = nullptr;
    p->d_tpk = p->d_tpk2 = nullptr;
    p->t_cap = 0;
    void *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr, *f = nullptr;
    hipError_t e = hipMalloc(&a, cap * 4);
    if (e == hipSuccess) e = hipMalloc(&b, cap * wsz);
    if (e == hipSuccess) e = hipMalloc(&c, cap * 4);
    if (e == hipSuccess) e = hipMalloc(&d, cap * 8);
    if (e == hipSuccess) e = hipMalloc(&f, cap * 8);
    if (e != hipSuccess) {
        for (void *q : {a, b, c, d, f}) (void)hipFree(q);
        return fail(err, e, "hipMalloc(tight edges)");
    }
    p->d_tu = (uint32_t *)a;
    p->d_tw = b;
    p->d_teb = (float *)c;
    p->d_tpk = (uint64_t *)d;
    p->d_tpk2 = (uint64_t *)f;
    p->t_cap = cap;
    return SRT_OK;
}

// packed entries d_tpk2 (rows by d_tptr) -> d_tpk, every target's row sorted
// by w (bits ubits .. of the low word)
srt_status sort_packed(srt_plan *p, uint32_t ubits, uint64_t maxw, srt_err *err) {
    const unsigned end_bit = ubits + (unsigned)std::max(1, bits_of(maxw));
    size_t need = 0;
    hipError_t e = rocprim::segmented_radix_sort_keys(nullptr, need, p->d_tpk2, p->d_tpk, (unsigned)p->t_edges, p->V,
                                                      p->d_tptr, p->d_tptr + 1, ubits, end_bit, p->stream);
    if (e != hipSuccess) return fail(err, e, "segmented sort (size)");
    uint64_t tcap = p->tsort_tmp_cap;
    srt_status st = grow(reinterpret_cast<uint8_t **>(&p->d_tsort_tmp), &tcap, need + 256, err, "hipMalloc(sort scratch)");
    p->tsort_tmp_cap = tcap;
    if (st != SRT_OK) return st;
    size_t have = p->tsort_tmp_cap;
    e = rocprim::segmented_radix_sort_keys(p->d_tsort_tmp, have, p->d_tpk2, p->d_tpk, (unsigned)p->t_edges, p->V,
                                           p->d_tptr, p->d_tptr + 1, ubits, end_bit, p->stream);
    if (e != hipSuccess) return fail(err, e, "segmented sort");
    return SRT_OK;
}

// The tight-edge list buffer holds p->tlist_cap uint4 slots in every path
// (one GPU: the whole list; sharded and emulated: W per-rank chunks of C
// slots).  Grow to `cap` slots when fewer than `need` are allocated.
static srt_status ensure_tlist(srt_plan *p, uint64_t cap, uint64_t need, srt_err *err) {
    if (p->d_tlist && need <= p->tlist_cap) return SRT_OK;
    (void)hipFree(p->d_tlist);
    p->d_tlist = nullptr;
    p->tlist_cap = 0;
    hipError_t e = hipMalloc(&p->d_tlist, cap * sizeof(uint4));
    if (e != hipSuccess) return fail(err, e, "hipMalloc(tight list)");
    p->tlist_cap = cap;
    return SRT_OK;
}

// The level fold applies (see level_loss_kernel): every tight weight <= WC,
// every closure latency < NBK units, u16 member lists, the row in LDS.
// Returns the fold's level width q in units of g: 1 (exact levels) when every
// tight weight is its own class (w <= WC) and every closure latency < NBK;
// else, when the smallest tight weight minw is known (one-GPU tight pass),
// quantized levels floor(L / q) with q = minw: a tight edge then climbs at
// least one level, its class floor(w / q) <= WC places its tail in one of two
// levels, and an exact test L(s,u) + w == L(s,v) on the closure row picks the
// candidates (C3 with ns latencies: g = 1 ns, tight weights 1.0-16 ms).  0: no.
uint32_t level_q(const srt_plan *p, uint64_t maxw, uint64_t minw) {
    if (const char *e = std::getenv("SRT_LOSS_LEVEL"))  // A/B and parity tests of the scan folds
        if (std::atoi(e) == 0) return 0;
    const size_t lds = fold_lds_bytes(p->V);
    if (!(p->kp.lat32 && p->V < 65536 && lds + 16 <= LDS_BUDGET - 4096 && maxw >= 1)) return 0;
    if (maxw <= WC && p->kp.lmax < (uint64_t)NBK) return 1;
    if (minw >= 2 && minw <= maxw && maxw / minw <= WC && p->kp.lmax / minw < (uint64_t)NBK - 1 &&
        minw < (1ull << 32) && (p->key_type == srt::KEY_U16 || p->key_type == srt::KEY_U32) &&
        !std::getenv("SRT_LOSS_NOQ"))
        return (uint32_t)minw;
    return 0;
}

// The class CSRs of the list's slots (records {v, u, w, 1-e bits}, v = ~0:
// padding) at level width p->t_q: out-rows in d_tpk, in-rows in d_tpk2,
// grouped by (vertex, class floor(w / q)) -- no sort.
srt_status build_class_csr(srt_plan *p, uint64_t slots, uint64_t maxw, srt_err *err) {
    hipStream_t M = p->stream;
    const uint32_t V = p->V;
    srt_status st;
    const uint32_t lblocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(8192, (slots + 255) / 256));
    const uint32_t q = p->t_q;
    if (q > 1 && p->tcw_cap < 2 * p->t_cap) {  // the exact weights beside the class entries
        (void)hipFree(p->d_tcw);
        p->d_tcw = nullptr;
        p->tcw_cap = 0;
        const hipError_t e = hipMalloc(&p->d_tcw, 2 * p->t_cap * sizeof(uint32_t));
        if (e != hipSuccess) return fail(err, e, "hipMalloc(class weights)");
        p->tcw_cap = 2 * p->t_cap;
    }
    const uint32_t mc = q == 1 ? (uint32_t)maxw : (uint32_t)(maxw / q);  // the largest class
    p->t_cls = mc < 16 ? 16 : 32;
    const uint32_t cls = p->t_cls;
    const uint64_t vc1 = (uint64_t)V * cls + 1;
    if ((st = ensure_class_arrays(p, vc1, err)) != SRT_OK) return st;
    (void)hipMemsetAsync(p->d_tccnt, 0, 2 * vc1 * 4, M);
    hipLaunchKernelGGL(tcls_count_kernel, dim3(lblocks), dim3(256), 0, M, p->d_tlist, slots, p->d_tccnt, vc1, q,
                       cls);
    for (int d = 0; d < 2; ++d)
        if ((st = exclusive_scan_u32(p, p->d_tccnt + d * vc1, p->d_tcls + d * vc1, (size_t)vc1, err)) != SRT_OK)
            return st;
    (void)hipMemsetAsync(p->d_tccnt, 0, 2 * vc1 * 4, M);
    hipLaunchKernelGGL(tcls_fill_kernel, dim3(lblocks), dim3(256), 0, M, p->d_tlist, slots, p->d_tcls,
                       p->d_tccnt, p->d_tpk, p->d_tpk2, vc1, q, q > 1 ? p->d_tcw : nullptr, p->t_cap, cls);
    p->t_push = false;
    return SRT_OK;
}

// Rows of the tight-edge list (slots records, v = ~0: padding, p->t_edges
// real ones): the class CSRs when the level fold applies (no sort), else the
// packed push (rows by source) or pull rows sorted by w.
srt_status build_tight_rows(srt_plan *p, uint64_t slots, uint32_t ubits, uint64_t maxw, srt_err *err,
                            uint64_t minw = 0) {
    hipStream_t M = p->stream;
    const uint32_t V = p->V;
    const uint32_t lblocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(8192, (slots + 255) / 256));
    p->t_q = level_q(p, maxw, minw);
    p->t_level = p->t_q != 0;
    if (p->t_level) return build_class_csr(p, slots, maxw, err);
    (void)hipMemsetAsync(p->d_tcnt, 0, (size_t)V * 4, M);
    // push form: CSR over tight OUT-edges (the pull form over in-edges
    // measured slower and was removed)
    hipLaunchKernelGGL(tight_list_count_kernel<true>, dim3(lblocks), dim3(256), 0, M, p->d_tlist, slots, p->d_tcnt, V);
    hipLaunchKernelGGL(tight_scan_kernel, dim3(1), dim3(1024), 0, M, p->d_tcnt, p->d_tptr, V);
    hipLaunchKernelGGL(tight_list_fill_kernel<true>, dim3(lblocks), dim3(256), 0, M, p->d_tlist, slots, p->d_tptr,
                       p->d_tcnt, p->d_tpk2, ubits, V);
    p->t_push = true;
    return sort_packed(p, ubits, maxw, err);
}

template <int LPT>
srt_status launch_level(srt_plan *p, unsigned long long *d_stats, const RowJob &job) {
    const uint32_t V = p->V, rows = job.list ? job.count : job.range ? job.r1 - job.r0 : p->row1 - p->row0;
    if (!rows) return SRT_OK;
    const size_t lds = fold_lds_bytes(V);
    const uint32_t nt = V >= 2048 ? LOSS_NT : 256;
    const int per_cu = std::max(1, std::min(2048 / (int)nt, (int)std::max<size_t>(1, (160 * 1024) / (lds + 2048))));
    const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(rows, (uint32_t)(cu_count(p->device) * per_cu)));
    // exact forms: loads of 2 entries (16 B), 4 in flight a lane with 16
    // classes (C3 loss pass 6.5 -> 6.2 ms vs 8 single entries; 6 pairs 6.8,
    // 2 lanes an item 7.2), 2 with 32 (C2 ~2% faster than 4 single entries);
    // quantized: 3 (16 classes) or 2 (32) single entries (the exact weights
    // beside them leave no registers for pairs)
    auto kern = p->t_cls == 16 ? (p->t_q > 1 ? level_loss_kernel<LPT, 3, true, 16, 1> : level_loss_kernel<LPT, 4, false, 16, 2>)
                               : (p->t_q > 1 ? level_loss_kernel<LPT, 2, true, 32, 1> : level_loss_kernel<LPT, 2, false, 32, 2>);
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_BUDGET - 4096));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), lds, p->stream, (const void *)p->d_D, p->key_type, p->Vp, V,
                       p->d_nodes, p->n, job.list ? 0u : job.range ? job.r0 : p->row0,
                       job.list ? job.count : job.range ? job.r1 : p->row1, p->d_tcls, (uint64_t)V * p->t_cls + 1,
                       p->d_tpk, p->d_tpk2, p->kp.g, p->d_sl_lat, p->d_sl_loss, p->d_out_lat, p->d_out_loss, d_stats,
                       job.list, job.out32, job.out32_loss, p->stage16, p->t_q, p->d_tcw, p->t_cap);
#if LOSS_COUNT
    {  // diagnostic builds (-DLOSS_COUNT=1): totals of every level fold so far
        unsigned long long c[9];
        (void)hipStreamSynchronize(p->stream);
        (void)hipMemcpyFromSymbol(c, HIP_SYMBOL(loss_cnt), sizeof c);
        std::fprintf(stderr,
                     "[srt] level fold: items %llu visits %llu hits %llu (push %llu) levels %llu rows %u; us per row: "
                     "load %.2f sort %.2f levels %.2f out %.2f\n",
                     c[0], c[1], c[2], c[8], c[3], rows, c[4] * 0.01 / rows, c[5] * 0.01 / rows, c[6] * 0.01 / rows,
                     c[7] * 0.01 / rows);
    }
#endif
    return SRT_OK;
}

// Push-form tight CSR on one GPU: the flagged adjacency entries compacted
// per source row (tight_list_kernel), then rows by source u, packed with v and
// sorted by w.  *done = false: not packable, the caller builds the pull form.
template <typename K>
srt_status tight_csr_push_t(srt_plan *p, unsigned long long *d_stats, bool *done, srt_err *err) {
    hipStream_t M = p->stream;
    const uint32_t V = p->V;
    *done = false;
    srt_status st;
    uint64_t cap_info = p->d_tinfo ? 2 : 0, cap_cur = p->d_tcursor ? 1 : 0;
    if ((st = grow(&p->d_tinfo, &cap_info, 2, err, "hipMalloc(tight info)")) != SRT_OK ||
        (st = grow(&p->d_tcursor, &cap_cur, 1, err, "hipMalloc(tight cursor)")) != SRT_OK)
        return st;
    hipLaunchKernelGGL(loss_stats_init_kernel, dim3(1), dim3(1), 0, M, d_stats, (unsigned long long *)p->d_tmaxw);
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(8192, (V + 3) / 4));
    // the list straight from the adjacency (tight_rows_kernel) into the list
    // the last run sized; a first run (or a larger count) counts, grows the
    // list and runs again
    auto rows = [&]() {
        (void)hipMemsetAsync(p->d_tinfo, 0, 2 * sizeof(unsigned long long), M);
        (void)hipMemsetAsync(p->d_tcursor, 0, sizeof(unsigned long long), M);
        hipLaunchKernelGGL(tight_rows_kernel<K>, dim3(blocks), dim3(256), 0, M, reinterpret_cast<const K *>(p->d_D),
                           p->Vp, V, p->d_row_ptr, p->d_col, p->d_lat, p->d_loss, p->kp.g, p->d_tlist,
                           p->d_tlist ? p->tlist_cap : 0ull, p->d_tcursor, (unsigned long long *)p->d_tmaxw,
                           p->d_tinfo);
        (void)hipMemcpyAsync(p->h_tcount, p->d_tinfo, sizeof(uint64_t), hipMemcpyDeviceToHost, M);
        (void)hipMemcpyAsync(p->h_tcount + 1, p->d_tmaxw, sizeof(uint64_t), hipMemcpyDeviceToHost, M);
        (void)hipMemcpyAsync(p->h_tcount + 2, p->d_tinfo + 1, sizeof(uint64_t), hipMemcpyDeviceToHost, M);
        return hipStreamSynchronize(M);
    };
    if (!p->d_tlist) {
        // a plan's first run (every end-to-end build): a list of n_adj / 32
        // records up front (C3: 8.4M slots for the 2.5M tight edges), so the
        // pass runs once; a larger count grows the list and runs again
        const uint64_t guess = std::max<uint64_t>(1ull << 16, p->n_adj / 32);
        if ((st = ensure_tlist(p, guess, guess, err)) != SRT_OK) return st;
    }
    hipError_t e = rows();
    if (e != hipSuccess) return fail(err, e, "tight-edge list");
    const uint64_t total = p->h_tcount[0], maxw = p->h_tcount[1];
    const uint64_t minw = total ? ~p->h_tcount[2] : 0;  // the kernel kept max(~w)
    const uint32_t ubits = (uint32_t)std::max(1, bits_of(V ? V - 1 : 0));
    // the level fold's class CSRs need no packed (u, w) word: wide weights
    // (ns units) still fold by levels when level_q allows
    const bool packable = p->kp.lat32 && ubits + bits_of(maxw) <= 32 && total < (1ull << 32);
    if (!packable && !(total && level_q(p, maxw, minw))) return SRT_OK;
    p->t_edges = total;
    if ((st = ensure_edge_arrays(p, err)) != SRT_OK) return st;
    const uint64_t C = std::max<uint64_t>(total, 1);
    if (!p->d_tlist || total > p->tlist_cap) {
        if ((st = ensure_tlist(p, C + C / 4 + 64, C, err)) != SRT_OK) return st;
        if ((e = rows()) != hipSuccess) return fail(err, e, "tight-edge list");
    }
    if ((st = build_tight_rows(p, total, ubits, maxw, err, minw)) != SRT_OK) return st;
    if (std::getenv("SRT_TRACE"))
        std::fprintf(stderr, "[srt] tight edges %llu, w in [%llu, %llu] units, lmax %llu: %s fold, level width %u\n",
                     (unsigned long long)total, (unsigned long long)minw, (unsigned long long)maxw,
                     (unsigned long long)p->kp.lmax, p->t_level ? "level" : "scan", p->t_q);
    p->t_packed = packable;
    *done = true;
    return SRT_OK;
}

template <typename K>
srt_status tight_csr_t(srt_plan *p, unsigned long long *d_stats, srt_err *err) {
    hipStream_t M = p->stream;
    const uint32_t V = p->V;
    srt_status st;
    uint64_t cap_flag = p->d_tflag ? p->n_adj : 0, cap_cnt = p->d_tcnt ? V : 0, cap_ptr = p->d_tptr ? V + 1ull : 0,
             cap_mw = p->d_tmaxw ? 1 : 0;
    if ((st = grow(&p->d_tflag, &cap_flag, p->n_adj, err, "hipMalloc(tight flags)")) != SRT_OK ||
        (st = grow(&p->d_tcnt, &cap_cnt, V, err, "hipMalloc(tight counts)")) != SRT_OK ||
        (st = grow(&p->d_tptr, &cap_ptr, V + 1ull, err, "hipMalloc(tight ptr)")) != SRT_OK ||
        (st = grow(&p->d_tmaxw, &cap_mw, 1, err, "hipMalloc(tight max)")) != SRT_OK)
        return st;
    if (!p->h_tcount) {
        const hipError_t e = hipHostMalloc((void **)&p->h_tcount, 4 * sizeof(uint64_t), 0);
        if (e != hipSuccess) return fail(err, e, "hipHostMalloc");
    }
    p->t_push = false;
    p->t_level = false;
    if (V && !std::getenv("SRT_LOSS_UNPACKED")) {
        bool done = false;
        if ((st = tight_csr_push_t<K>(p, d_stats, &done, err)) != SRT_OK || done) return st;
    }
    hipLaunchKernelGGL(loss_stats_init_kernel, dim3(1), dim3(1), 0, M, d_stats,
                       (unsigned long long *)p->d_tmaxw);
    (void)hipMemsetAsync(p->d_tcnt, 0, (size_t)V * 4, M);
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(8192, (V + 3) / 4));
    p->h_tcount[0] = p->h_tcount[1] = 0;
    if (V) {
        hipLaunchKernelGGL(tight_flag_kernel<K>, dim3(blocks), dim3(256), 0, M, reinterpret_cast<const K *>(p->d_D),
                           p->Vp, 0u, V, p->d_row_ptr, p->d_col, p->d_lat, p->kp.g, p->d_tflag, p->d_tcnt,
                           (unsigned long long *)p->d_tmaxw, (unsigned long long *)nullptr);
        hipLaunchKernelGGL(tight_scan_kernel, dim3(1), dim3(1024), 0, M, p->d_tcnt, p->d_tptr, V);
        (void)hipMemcpyAsync(p->h_tcount, p->d_tptr + V, sizeof(uint64_t), hipMemcpyDeviceToHost, M);
        (void)hipMemcpyAsync(p->h_tcount + 1, p->d_tmaxw, sizeof(uint64_t), hipMemcpyDeviceToHost, M);
    }
    hipError_t e = hipStreamSynchronize(M);
    if (e != hipSuccess) return fail(err, e, "tight-edge count");
    p->t_edges = p->h_tcount[0];
    const uint64_t maxw = p->h_tcount[1];
    const uint32_t ubits = (uint32_t)std::max(1, bits_of(V ? V - 1 : 0));
    // packed form: u and w share one word, rows sorted by w (knob
    // SRT_LOSS_UNPACKED=1 forces the 3-array form for A/B and parity tests)
    p->t_packed = p->kp.lat32 && ubits + bits_of(maxw) <= 32 && p->t_edges < (1ull << 32) &&
                  !std::getenv("SRT_LOSS_UNPACKED");
    if ((st = ensure_edge_arrays(p, err)) != SRT_OK) return st;
    if (!V) return SRT_OK;
    if (p->t_packed) {
        hipLaunchKernelGGL((tight_fill_kernel<uint32_t, true>), dim3(blocks), dim3(256), 0, M, V, p->d_row_ptr,
                           p->d_col, p->d_lat, p->d_loss, p->kp.g, p->d_tflag, p->d_tptr, p->d_tcnt,
                           (uint32_t *)nullptr, (uint32_t *)nullptr, (float *)nullptr, p->d_tpk2, ubits);
        if ((st = sort_packed(p, ubits, maxw, err)) != SRT_OK) return st;
    } else if (p->kp.lat32) {
        hipLaunchKernelGGL((tight_fill_kernel<uint32_t, false>), dim3(blocks), dim3(256), 0, M, V, p->d_row_ptr,
                           p->d_col, p->d_lat, p->d_loss, p->kp.g, p->d_tflag, p->d_tptr, p->d_tcnt, p->d_tu,
                           (uint32_t *)p->d_tw, p->d_teb, (uint64_t *)nullptr, 0u);
    } else {
        hipLaunchKernelGGL((tight_fill_kernel<uint64_t, false>), dim3(blocks), dim3(256), 0, M, V, p->d_row_ptr,
                           p->d_col, p->d_lat, p->d_loss, p->kp.g, p->d_tflag, p->d_tptr, p->d_tcnt, p->d_tu,
                           (uint64_t *)p->d_tw, p->d_teb, (uint64_t *)nullptr, 0u);
    }
    return SRT_OK;
}

srt_status fold(srt_plan *p, unsigned long long *d_stats, const RowJob &job, srt_err *err) {
    const uint32_t V = p->V;
    if (p->t_level) {
        return launch_level<4>(p, d_stats, job);  // 4 lanes per class walk (2 and 8 measured slower)
    }
    const uint32_t ubits = (uint32_t)std::max(1, bits_of(V ? V - 1 : 0));
    const bool lds_rows = HIST_BYTES + (size_t)V * 8 + 16 <= LDS_BUDGET - 4096;
    if (p->kp.lat32) {
        if (p->t_packed)
            return lds_rows ? launch_fold_lpt<uint32_t, true, true>(p, d_stats, ubits, job, err)
                            : launch_fold_lpt<uint32_t, false, true>(p, d_stats, ubits, job, err);
        return lds_rows ? launch_fold_lpt<uint32_t, true, false>(p, d_stats, 0, job, err)
                        : launch_fold_lpt<uint32_t, false, false>(p, d_stats, 0, job, err);
    }
    return launch_fold_lpt<uint64_t, false, false>(p, d_stats, 0, job, err);
}

// Sharded tail (comm bound): the tight edges of this rank's own adjacency
// rows (its closure block-rows, final locally), the (count, max latency) of
// every rank exchanged, then -- when the packed form applies -- the edge
// lists all-gathered and the full pull CSR built from them on every rank.
// *sharded = false: not packable, the caller falls back to the key
// all-gather and the replicated CSR.
template <typename K>
srt_status tight_csr_shard_t(srt_plan *p, unsigned long long *d_stats, bool *sharded, srt_err *err) {
    hipStream_t M = p->stream;
    const uint32_t V = p->V, W = (uint32_t)p->comm->nranks, r = (uint32_t)p->comm->rank;
    const uint32_t u0 = (uint32_t)std::min<uint64_t>((uint64_t)p->rb0 * FW_B, V);
    const uint32_t u1 = (uint32_t)std::min<uint64_t>((uint64_t)p->rb1 * FW_B, V);
    *sharded = false;
    srt_status st;
    uint64_t cap_flag = p->d_tflag ? p->n_adj : 0, cap_cnt = p->d_tcnt ? V : 0, cap_ptr = p->d_tptr ? V + 1ull : 0,
             cap_mw = p->d_tmaxw ? 1 : 0, cap_info = p->d_tinfo ? 2ull * W : 0, cap_cur = p->d_tcursor ? 1 : 0;
    if ((st = grow(&p->d_tflag, &cap_flag, std::max<uint64_t>(p->n_adj, 1), err, "hipMalloc(tight flags)")) != SRT_OK ||
        (st = grow(&p->d_tcnt, &cap_cnt, std::max<uint64_t>(V, 1), err, "hipMalloc(tight counts)")) != SRT_OK ||
        (st = grow(&p->d_tptr, &cap_ptr, V + 1ull, err, "hipMalloc(tight ptr)")) != SRT_OK ||
        (st = grow(&p->d_tmaxw, &cap_mw, 1, err, "hipMalloc(tight max)")) != SRT_OK ||
        (st = grow(&p->d_tinfo, &cap_info, 2ull * W, err, "hipMalloc(tight info)")) != SRT_OK ||
        (st = grow(&p->d_tcursor, &cap_cur, 1, err, "hipMalloc(tight cursor)")) != SRT_OK)
        return st;
    if (!p->h_tinfo) {
        const hipError_t e = hipHostMalloc((void **)&p->h_tinfo, 2 * sizeof(unsigned long long) * W, 0);
        if (e != hipSuccess) return fail(err, e, "hipHostMalloc");
    }
    hipLaunchKernelGGL(loss_stats_init_kernel, dim3(1), dim3(1), 0, M, d_stats, (unsigned long long *)p->d_tmaxw);
    (void)hipMemsetAsync(p->d_tinfo, 0, 2 * sizeof(unsigned long long) * W, M);
    (void)hipMemsetAsync(p->d_tcursor, 0, sizeof(unsigned long long), M);
    const uint32_t own_rows = u1 > u0 ? u1 - u0 : 0;
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(8192, (own_rows + 3) / 4));
    if (own_rows)
        hipLaunchKernelGGL(tight_flag_kernel<K>, dim3(blocks), dim3(256), 0, M, reinterpret_cast<const K *>(p->d_D),
                           p->Vp, u0, u1, p->d_row_ptr, p->d_col, p->d_lat, p->kp.g, p->d_tflag, (uint32_t *)nullptr,
                           p->d_tinfo + 2 * r + 1, p->d_tinfo + 2 * r);
    if ((st = comm_allgather_inplace(p->comm, p->d_tinfo, 2 * sizeof(unsigned long long), M, err)) != SRT_OK)
        return st;
    (void)hipMemcpyAsync(p->h_tinfo, p->d_tinfo, 2 * sizeof(unsigned long long) * W, hipMemcpyDeviceToHost, M);
    hipError_t e = hipStreamSynchronize(M);
    if (e != hipSuccess) return fail(err, e, "tight-edge count exchange");
    uint64_t total = 0, maxw = 0, C = 1;
    for (uint32_t q = 0; q < W; ++q) {
        total += p->h_tinfo[2 * q];
        maxw = std::max<uint64_t>(maxw, p->h_tinfo[2 * q + 1]);
        C = std::max<uint64_t>(C, p->h_tinfo[2 * q]);
    }
    const uint32_t ubits = (uint32_t)std::max(1, bits_of(V ? V - 1 : 0));
    if (!(p->kp.lat32 && ubits + bits_of(maxw) <= 32 && total < (1ull << 32) && !std::getenv("SRT_LOSS_UNPACKED")))
        return SRT_OK;
    if ((st = ensure_tlist(p, (C + C / 4 + 64) * W, C * W, err)) != SRT_OK) return st;
    // own chunk: the records, then v = ~0 padding up to C
    (void)hipMemsetAsync(p->d_tlist + (uint64_t)r * C, 0xff, C * sizeof(uint4), M);
    if (own_rows)
        hipLaunchKernelGGL(tight_list_kernel, dim3(blocks), dim3(256), 0, M, u0, u1, p->d_row_ptr, p->d_col, p->d_lat,
                           p->d_loss, p->kp.g, p->d_tflag, p->d_tlist + (uint64_t)r * C, p->d_tcursor);
    if ((st = comm_allgather_inplace(p->comm, p->d_tlist, C * sizeof(uint4), M, err)) != SRT_OK) return st;
    p->t_edges = total;
    p->t_packed = true;
    if ((st = ensure_edge_arrays(p, err)) != SRT_OK) return st;
    if ((st = build_tight_rows(p, C * W, ubits, maxw, err)) != SRT_OK) return st;
    *sharded = true;
    return SRT_OK;
}

// Measurement only (SRT_FW_EMULATE_RANKS = N, no comm): wait `ticks` of the
// constant wall clock on the stream -- stands in for a collective
__global__ void emu_wait_kernel(long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

}  // namespace

void emu_allgather(int device, uint32_t W, double bytes_per_rank, hipStream_t s) {
    int khz = 100000;
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device);
    const double lat_us = std::getenv("SRT_FW_EMU_AG_US") ? std::atof(std::getenv("SRT_FW_EMU_AG_US")) : 25.0;
    const double gbps = std::getenv("SRT_FW_EMU_AG_GBPS") ? std::atof(std::getenv("SRT_FW_EMU_AG_GBPS")) : 300.0;
    const double us = lat_us + bytes_per_rank * (W - 1) / (gbps * 1e3);
    hipLaunchKernelGGL(emu_wait_kernel, dim3(1), dim3(64), 0, s, (long long)(us * khz / 1000.0));
}

// staged slots [s0, s0 + slots) into the table, on the main stream
void expand_slots(srt_plan *p, size_t s0, uint32_t slots) {
    if (!slots || !p->n) return;
    const size_t lb = p->stage16 ? 2 : 4;
    hipLaunchKernelGGL(expand_rows_kernel, dim3(std::min<uint32_t>(slots, 4096)), dim3(256), 0, p->stream,
                       p->d_lrows + s0, slots, p->n,
                       (const void *)(reinterpret_cast<const uint8_t *>(p->d_slat) + s0 * p->n * lb), p->stage16,
                       p->d_sloss + s0 * p->n, p->kp.g, p->d_out_lat, p->d_out_loss,
                       p->stage_loss_only ? reinterpret_cast<const uint16_t *>(p->d_D) : nullptr, p->Vp, p->d_nodes,
                       p->d_sl_lat);
}

// chunk c of the staging into the table as soon as its all-gather is done
// (ev_tail[q + c]): the expansion of chunk c overlaps the all-gathers of the
// later chunks (emulated C3, 8 ranks: the 1.4 ms expansion was serial after
// the last all-gather)
void expand_chunks_behind(srt_plan *p, uint32_t W) {
    const uint32_t q = p->tail_q, cr = p->tail_cr;
    for (uint32_t c = 0; c < q; ++c) {
        (void)hipStreamWaitEvent(p->stream, p->ev_tail[q + c], 0);
        expand_slots(p, (size_t)c * W * cr, W * cr);
    }
    p->tail_expanded = true;
}

namespace {
template <typename K>
srt_status loss_sharded_t(srt_plan *p, unsigned long long *d_stats, srt_err *err) {
    bool sharded = false;
    srt_status st = tight_csr_shard_t<K>(p, d_stats, &sharded, err);
    if (st != SRT_OK) return st;
    if (!sharded) {
        // replicated fallback: every rank's closure rows, then the CSR of all rows
        if ((st = fw_gather_keys(p, err)) != SRT_OK) return st;
        if ((st = tight_csr_t<K>(p, d_stats, err)) != SRT_OK) return st;
        return fold(p, d_stats, RowJob{}, err);
    }
    const uint32_t W = (uint32_t)p->comm->nranks, r = (uint32_t)p->comm->rank;
    p->stage16 = p->key_type == KEY_U16;
    // every rank holds the whole closure: exchange the loss only (knob
    // SRT_TAIL_LAT=1 stages the latencies too, for A/B)
    p->stage_loss_only = p->fw_full_d && p->stage16;
    const size_t lb = p->stage16 ? 2 : 4;  // bytes per staged latency
    if (srt_status s2 = ensure_row_staging(p, W, err); s2 != SRT_OK) return s2;
    // the fold in tail_q chunks of tail_cr rows; chunk c's rows go to every
    // rank on the comm stream while chunk c + 1 folds (collectives stay in
    // one order on every rank: the chunks, then -- on M, after the last
    // chunk -- the rank stats)
    const uint32_t q = p->tail_q, cr = p->tail_cr;
    const size_t cbytes = (size_t)cr * p->n * 4, lbytes = (size_t)cr * p->n * lb;
    hipStream_t M = p->stream, C = p->comm_stream;
    for (uint32_t c = 0; c < q; ++c) {
        const size_t slot = ((size_t)c * W + r) * cr;
        RowJob job;
        job.list = p->d_lrows + slot;
        job.count = p->lrow_cnt[r] > c * cr ? std::min(cr, p->lrow_cnt[r] - c * cr) : 0u;
        job.out32 = p->stage_loss_only ? nullptr : reinterpret_cast<uint8_t *>(p->d_slat) + slot * p->n * lb;
        job.out32_loss = p->d_sloss + slot * p->n;
        if ((st = fold(p, d_stats, job, err)) != SRT_OK) return st;
        (void)hipEventRecord(p->ev_tail[c], M);
        (void)hipStreamWaitEvent(C, p->ev_tail[c], 0);
        const size_t base = (size_t)c * W * cr * p->n;
        if ((!p->stage_loss_only &&
             (st = comm_allgather_inplace(p->comm, reinterpret_cast<uint8_t *>(p->d_slat) + base * lb, lbytes, C,
                                          err)) != SRT_OK) ||
            (st = comm_allgather_inplace(p->comm, p->d_sloss + base, cbytes, C, err)) != SRT_OK)
            return st;
        (void)hipEventRecord(p->ev_tail[q + c], C);
    }
    expand_chunks_behind(p, W);
    p->shard_tail = true;
    return SRT_OK;
}

// Emulated rank 0 of an N-rank sharded tail, on the closure the first run
// left in D: the flags of its own adjacency rows, the list over every row
// (the other rows' flags are the closing run's, of the same D), the count /
// scan / fill / sort of the full list, the fold of its own rows into the
// staging.  The three all-gathers are waits of SRT_FW_EMU_AG_US (default 25)
// + received bytes / SRT_FW_EMU_AG_GBPS (default 300).
template <typename K>
srt_status loss_emulated_t(srt_plan *p, unsigned long long *d_stats, srt_err *err) {
    hipStream_t M = p->stream;
    const uint32_t V = p->V, W = p->emulate_ranks;
    const uint32_t u1 = (uint32_t)std::min<uint64_t>((uint64_t)std::max<uint32_t>(1, p->Vp / FW_B / W) * FW_B, V);
    srt_status st;
    uint64_t cap_info = p->d_tinfo ? 2 : 0, cap_cur = p->d_tcursor ? 1 : 0;
    if ((st = grow(&p->d_tinfo, &cap_info, 2, err, "hipMalloc(tight info)")) != SRT_OK ||
        (st = grow(&p->d_tcursor, &cap_cur, 1, err, "hipMalloc(tight cursor)")) != SRT_OK)
        return st;
    if (!p->h_tinfo) {
        const hipError_t e = hipHostMalloc((void **)&p->h_tinfo, 2 * sizeof(unsigned long long), 0);
        if (e != hipSuccess) return fail(err, e, "hipHostMalloc");
    }
    auto allgather_on = [&](double bytes_per_rank, hipStream_t s) { emu_allgather(p->device, W, bytes_per_rank, s); };
    auto allgather = [&](double bytes_per_rank) { allgather_on(bytes_per_rank, M); };
    hipLaunchKernelGGL(loss_stats_init_kernel, dim3(1), dim3(1), 0, M, d_stats, (unsigned long long *)p->d_tmaxw);
    (void)hipMemsetAsync(p->d_tinfo, 0, 2 * sizeof(unsigned long long), M);
    (void)hipMemsetAsync(p->d_tcursor, 0, sizeof(unsigned long long), M);
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(8192, (u1 + 3) / 4));
    hipLaunchKernelGGL(tight_flag_kernel<K>, dim3(blocks), dim3(256), 0, M, reinterpret_cast<const K *>(p->d_D), p->Vp,
                       0u, u1, p->d_row_ptr, p->d_col, p->d_lat, p->kp.g, p->d_tflag, (uint32_t *)nullptr,
                       p->d_tinfo + 1, p->d_tinfo);
    allgather(16.0);
    (void)hipMemcpyAsync(p->h_tinfo, p->d_tinfo, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, M);
    hipError_t e = hipStreamSynchronize(M);
    if (e != hipSuccess) return fail(err, e, "tight-edge count");
    const uint64_t total = p->emu_tight, maxw = p->emu_maxw;
    const uint64_t C = std::max<uint64_t>({1, p->h_tinfo[0], (total + W - 1) / W});
    const uint32_t ubits = (uint32_t)std::max(1, bits_of(V ? V - 1 : 0));
    if (!(p->kp.lat32 && ubits + bits_of(maxw) <= 32 && total < (1ull << 32)))
        return fail(err, hipErrorNotSupported, "rank emulation needs the packed tight-edge form");
    const uint64_t slots = C * W;
    if ((st = ensure_tlist(p, slots, slots, err)) != SRT_OK) return st;
    (void)hipMemsetAsync(p->d_tlist, 0xff, slots * sizeof(uint4), M);
    const uint32_t vblocks = std::max<uint32_t>(1, std::min<uint32_t>(8192, (V + 3) / 4));
    hipLaunchKernelGGL(tight_list_kernel, dim3(vblocks), dim3(256), 0, M, 0u, V, p->d_row_ptr, p->d_col, p->d_lat,
                       p->d_loss, p->kp.g, p->d_tflag, p->d_tlist, p->d_tcursor);
    allgather((double)C * sizeof(uint4));
    p->t_edges = total;
    p->t_packed = true;
    if ((st = ensure_edge_arrays(p, err)) != SRT_OK) return st;
    if ((st = build_tight_rows(p, slots, ubits, maxw, err)) != SRT_OK) return st;
    p->stage16 = p->key_type == KEY_U16;
    p->stage_loss_only = p->fw_full_d && p->stage16;
    const size_t lb = p->stage_loss_only ? 0 : p->stage16 ? 2 : 4;  // bytes per staged latency
    if (srt_status s2 = ensure_row_staging(p, W, err); s2 != SRT_OK) return s2;
    const uint32_t q = p->tail_q, cr = p->tail_cr;
    hipStream_t Cs = p->comm_stream;
    for (uint32_t c = 0; c < q; ++c) {
        const size_t slot = (size_t)c * W * cr;  // rank 0's slots of chunk c
        RowJob job;
        job.list = p->d_lrows + slot;
        job.count = p->lrow_cnt[0] > c * cr ? std::min(cr, p->lrow_cnt[0] - c * cr) : 0u;
        job.out32 = p->stage_loss_only ? nullptr : reinterpret_cast<uint8_t *>(p->d_slat) + slot * p->n * lb;
        job.out32_loss = p->d_sloss + slot * p->n;
        if ((st = fold(p, d_stats, job, err)) != SRT_OK) return st;
        (void)hipEventRecord(p->ev_tail[c], M);
        (void)hipStreamWaitEvent(Cs, p->ev_tail[c], 0);
        allgather_on((double)cr * p->n * (4.0 + lb), Cs);  // latency units + loss
        (void)hipEventRecord(p->ev_tail[q + c], Cs);
    }
    expand_chunks_behind(p, W);  // emulation: the others' slots are stale (same volume)
    allgather(16.0);  // rank stats
    p->shard_tail = true;
    return SRT_OK;
}

}  // namespace

void expand_shard_rows(srt_plan *p, int nranks) { expand_slots(p, 0, (uint32_t)nranks * p->lrow_max); }

// f(K{}) for the closure's key type K
template <typename F>
static srt_status by_key_type(int key_type, F f) {
    return key_type == KEY_U16   ? f(uint16_t{})
           : key_type == KEY_U32 ? f(uint32_t{})
           : key_type == KEY_F64 ? f(double{})
                                 : f(uint64_t{});
}

srt_status fw_loss(srt_plan *p, unsigned long long *d_stats, srt_err *err) {
    if (p->algo == SRT_ALGO_LEVEL) return level_run(p, d_stats, err);
    if (!p->ev_loss0) {
        (void)hipEventCreate(&p->ev_loss0);
        (void)hipEventCreate(&p->ev_loss1);
    }
    (void)hipEventRecord(p->ev_loss0, p->stream);
    srt_status st;
    p->shard_tail = false;
    p->tail_expanded = false;
    if (p->comm) {
        st = by_key_type(p->key_type, [&](auto k) { return loss_sharded_t<decltype(k)>(p, d_stats, err); });
        if (st != SRT_OK) return st;
        (void)hipEventRecord(p->ev_loss1, p->stream);
        return SRT_OK;
    }
    if (p->emulate_ranks > 1 && p->emu_closed) {
        st = by_key_type(p->key_type, [&](auto k) { return loss_emulated_t<decltype(k)>(p, d_stats, err); });
        if (st != SRT_OK) return st;
        (void)hipEventRecord(p->ev_loss1, p->stream);
        return SRT_OK;
    }
    st = by_key_type(p->key_type, [&](auto k) { return tight_csr_t<decltype(k)>(p, d_stats, err); });
    if (st != SRT_OK) return st;
    p->emu_tight = p->t_edges;
    p->emu_maxw = p->h_tcount[1];
    if (p->fold_chunk_rows) {
        // chunks of table rows, each followed by its event (the end-to-end
        // download of chunk c overlaps the fold of chunk c + 1)
        const uint32_t cr = p->fold_chunk_rows, nc = (p->row1 - p->row0 + cr - 1) / cr;
        if ((st = ensure_events(p->ev_fold, nc, hipEventDisableTiming, err)) != SRT_OK) return st;
        for (uint32_t c = 0; c < nc; ++c) {
            RowJob job;
            job.range = true;
            job.r0 = p->row0 + c * cr;
            job.r1 = std::min(p->row1, job.r0 + cr);
            if ((st = fold(p, d_stats, job, err)) != SRT_OK) return st;
            (void)hipEventRecord(p->ev_fold[c], p->stream);
        }
    } else if ((st = fold(p, d_stats, RowJob{}, err)) != SRT_OK) {
        return st;
    }
    (void)hipEventRecord(p->ev_loss1, p->stream);
    return SRT_OK;
}

// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_loss() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&loss_stats_init_kernel));
}

}  // namespace srt
