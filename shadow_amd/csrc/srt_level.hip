// srt_level.hip -- the level solve (SRT_ALGO_LEVEL), gfx950: the class CSRs
// of the short edges, the create-time probe and the per-row solve.
//
// Closure-free dense build (SRT_ALGO_LEVEL): petgraph's Dijkstra per source
// (mod.rs:195-198) as a bucket queue with unit-wide buckets -- Dial's
// algorithm -- over the graph's edges of latency <= B units, where B bounds
// every shortest path (the create-time probe: out- plus in-eccentricity of one
// in-use node, level_probe).  No edge longer than B can lie on a shortest
// path, so the pruned graph has the same distances and the same tight edges.
// Latencies are integers in units of g >= 1, so the bucket of level l holds
// exactly N_l = {v : L(s,v) = l}, final once every level j < l is: its members
// are the heads of the class-(l - j) edges out of N_j.  For each class w the
// candidates of level l are walked from the smaller end, as in the level fold
// above: push along class-w out-edges of N_{l-w}, or -- when the still
// unsettled set U_l is smaller -- pull along class-w in-edges of every u in
// U_l, testing the tail's level.  A hit sets the head's level to l (a plain
// store: every writer stores l) and min-folds the loss candidate
// 1 - (1 - loss[u]) (1 - e) into it by an LDS atomic on the f32 bits: the tails
// are final, so the result is the min over tight in-edges, the same bits as the
// reference's lexicographic (latency, loss) Dijkstra (the level fold's
// argument).  One workgroup per table row; LDS: level u16, loss f32, and
// the settled vertices in level order u16 (8 B a vertex, as the level fold).
// C3 (16k complete graph, latencies 1-300 ms): B = 8, levels of ~1 / 60 /
// 3,000 / 13,000 / few vertices, ~175k edge visits a row against 16,384^2 / 2
// relaxations a row for the triangle Floyd-Warshall.
#include "srt_rowfold.h"

namespace srt {

namespace {

// Level solve (the closure-free dense path, see level_solve_kernel): the
// class CSRs of the edges u -> v (v != u) of latency <= wmax units, straight
// from the adjacency.  Out-rows: one wave per adjacency row u (whose entries
// ARE u's out-edges), two passes -- pass 1 tests each 64-entry chunk (the
// latency first; the column is loaded only for the lanes that pass: C3 ~2% of
// the entries), counts the hits per class by LDS atomics and stages each hit
// (its place in the row, 16 bits, and its weight in units, 16 bits, or a mark
// that pass 2 reads the latency again) in LDS at its ballot rank; one
// global atomic takes the row's range, the row's class offsets are written
// (slot k: start of class k + 1; slot CLS - 1: the row's end), and pass 2
// deals the staged hits, OUT_PL a lane at once (their loss / column gathers in
// flight together), writing each (1f32 - e bits << 32 | v; 0 bits
// without losses) at its class's running position and counting it for the
// in-row of (v, class).  A row with more than OUT_SCAP hits, or of more than
// 65,536 entries, is tested again chunk by chunk in pass 2.  No global atomic per entry on the out side, where
// a row's ~50 entries of a class would all hit one counter.  Entries past
// `cap` are counted, not written (the caller sizes and runs again).
constexpr uint32_t OUT_SCAP = 1024;  // hits a wave stages in LDS (C3: ~330 a row at the bound, more in the probes)
#ifndef SRT_OUT_PL
#define SRT_OUT_PL 4
#endif
constexpr int OUT_PL = SRT_OUT_PL;  // staged hits a lane places at once (pass 2)
#ifndef SRT_OUT_UNR
#define SRT_OUT_UNR 8
#endif
constexpr int OUT_UNR = SRT_OUT_UNR;  // chunks of a row in flight a lane (pass 1)
#ifndef SRT_OUT_UNR16
#define SRT_OUT_UNR16 8
#endif
constexpr int OUT_UNR16 = SRT_OUT_UNR16;  // ... of the u16 copy: 256-entry chunks (8 B a lane)
// CE4 (identity rows of symmetric plans with losses, exact classes): the 4-byte
// entry v | (0x3f800000 - bits(1f32 - e)) << vb of the packed row's walk (vb:
// the bits of V - 1); a hit whose difference needs more than 32 - vb bits sets
// *ovf, and the run is repeated with 8-byte entries (level_run).
template <bool WITH_LOSS, bool IN = true, bool IDENT = false, bool L16 = false, bool CE4 = false>
__global__ __launch_bounds__(256) void lvl_out_kernel(uint32_t u0, uint32_t V, const uint64_t *__restrict__ row_ptr,
                                                      const uint32_t *__restrict__ col,
                                                      const uint64_t *__restrict__ lat, const float *__restrict__ loss,
                                                      uint64_t g, double inv_g, uint64_t wmax_ns, uint32_t cls,
                                                      uint32_t q, uint32_t vb,
                                                      uint32_t *__restrict__ off_out, uint32_t *__restrict__ in_cnt,
                                                      uint64_t *__restrict__ ce_out, uint64_t cap,
                                                      unsigned long long *cursor, unsigned long long *maxw,
                                                      const uint16_t *__restrict__ lat16 = nullptr,
                                                      unsigned long long *ovf = nullptr) {
    static_assert(!L16 || (IDENT && !IN), "the u16 copy: identity rows of symmetric plans");
    static_assert(!CE4 || (IDENT && !IN && WITH_LOSS), "4-byte entries: out-rows of symmetric plans, with losses");
    __shared__ uint32_t stage[4][OUT_SCAP];  // per wave: place in the row | units << 16 (0xffff: read again) of hit j
    __shared__ uint32_t ccnt[4][64];      // per wave: hits per class (pass 1), running positions (pass 2)
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t mw = 0;
    // l = w * g exactly; the class: w / q (q = 0: the exact weight)
    auto units_of = [&](uint64_t l) -> uint64_t { return (uint64_t)((double)l * inv_g + 0.5); };
    auto cls_of_units = [&](uint64_t wu) -> uint32_t { return (uint32_t)(q ? wu / q : wu); };
    for (uint32_t u = u0 + wave; u < V; u += nwaves) {  // rows [u0, V)
        const uint64_t b = row_ptr[u], e = row_ptr[u + 1];
        const uint32_t nch = (uint32_t)((e - b + 63) / 64);
        ccnt[wv][lane] = 0;
        uint32_t cnt = 0;
        const uint32_t wmax_u = (uint32_t)(wmax_ns / g);  // L16: the bound in units (wmax_ns = wmax_u g, < 0xffff)
        if (L16) {  // u16 units, 4 a lane a 256-entry chunk (identity rows of V % 4 == 0 entries)
            const uint2 *row = reinterpret_cast<const uint2 *>(lat16 + b);
            const uint32_t len = (uint32_t)(e - b), nq = (len + 255) / 256;
            for (uint32_t c0 = 0; c0 < nq; c0 += OUT_UNR16) {
                uint2 x[OUT_UNR16];
#pragma unroll
                for (int r = 0; r < OUT_UNR16; ++r) {
                    const uint32_t o = 256 * (c0 + r) + 4 * lane;
                    x[r] = o < len ? row[64 * (c0 + r) + lane] : make_uint2(~0u, ~0u);
                }
#pragma unroll
                for (int r = 0; r < OUT_UNR16; ++r) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint32_t w = ((i < 2 ? x[r].x : x[r].y) >> (16 * (i & 1))) & 0xffffu;
                        const uint32_t o = 256 * (c0 + r) + 4 * lane + i;
                        const bool f = w <= wmax_u && o != u;
                        const uint64_t m = __ballot(f);
                        if (f) {
                            const uint32_t c = cls_of_units(w);
                            atomicAdd(&ccnt[wv][c - 1], 1u);
                            mw = c > mw ? c : mw;
                            const uint32_t j = cnt + (uint32_t)__popcll(m & below);
                            if (j < OUT_SCAP) stage[wv][j] = o | w << 16;
                        }
                        cnt += (uint32_t)__popcll(m);
                    }
                }
            }
        }
        for (uint32_t c0 = 0; c0 < (L16 ? 0u : nch); c0 += OUT_UNR) {
            uint64_t l[OUT_UNR];
#pragma unroll
            for (int r = 0; r < OUT_UNR; ++r) {
                const uint64_t k = b + 64ull * (c0 + r) + lane;
                l[r] = k < e ? lat[k] : ~0ull;
            }
#pragma unroll
            for (int r = 0; r < OUT_UNR; ++r) {
                const uint64_t k = b + 64ull * (c0 + r) + lane;
                // col only where the latency passes; identity rows (IDENT): the
                // column is the entry's place in its row
                const bool f = l[r] <= wmax_ns && (IDENT ? (uint32_t)(k - b) != u : col[k] != u);
                const uint64_t m = __ballot(f);
                if (f) {
                    const uint64_t wu = units_of(l[r]);
                    const uint32_t c = cls_of_units(wu);
                    atomicAdd(&ccnt[wv][c - 1], 1u);
                    mw = c > mw ? c : mw;
                    const uint32_t j = cnt + (uint32_t)__popcll(m & below);
                    if (j < OUT_SCAP) stage[wv][j] = (uint32_t)(k - b) | (wu < 0xffffu ? (uint32_t)wu : 0xffffu) << 16;
                }
                cnt += (uint32_t)__popcll(m);
            }
        }
        // cnt is uniform (ballot counts); ccnt complete for this wave's lanes
        unsigned long long base = 0;
        if (cnt && lane == 0) base = atomicAdd(cursor, (unsigned long long)cnt);
        base = __shfl(base, 0);
        const bool fits = base + cnt <= cap;
        // class offsets of row u: exclusive prefix of the class counts (lanes < cls)
        uint32_t x = lane < cls ? ccnt[wv][lane] : 0u, incl = x;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        const uint32_t start = (uint32_t)base + incl - x;
        if (lane < cls) off_out[(uint64_t)u * cls + lane] = fits ? (lane == cls - 1 ? (uint32_t)(base + cnt) : start) : 0u;
        ccnt[wv][lane] = start;  // running positions
        if (!cnt || !fits) continue;  // uniform
        const bool staged = cnt <= OUT_SCAP && e - b <= 65536;
        auto put = [&](uint32_t v, uint64_t wu, float ls) {
            const uint32_t cl = cls_of_units(wu);
            const uint32_t pos = atomicAdd(&ccnt[wv][cl - 1], 1u);
            const float eb = WITH_LOSS ? 1.0f - ls : 0.0f;  // (1f32 - other.packet_loss), mod.rs:328
            // q > 0 (quantized classes): the weight's remainder w - c q rides
            // along, (1 - e) in bits 34.. (a loss in [0, 1]: its bits are < 2^30)
            if constexpr (CE4) {
                // (a loss outside [0, 1] or a NaN wraps the difference past every field: it overflows too)
                const uint32_t d = 0x3f800000u - __float_as_uint(eb);
                if (d >> (32u - vb)) atomicOr(ovf, 1ull);
                reinterpret_cast<uint32_t *>(ce_out)[pos] = v | d << vb;
            } else
            ce_out[pos] = q ? ((uint64_t)__float_as_uint(eb) << 34) | ((wu - (uint64_t)cl * q) << vb) | v
                            : ((uint64_t)__float_as_uint(eb) << 32) | v;
            if (IN) atomicAdd(&in_cnt[(uint64_t)v * cls + cl - 1], 1u);  // symmetric plans: no in-rows
        };
        if (staged) {  // uniform: the staged hits, OUT_PL a lane at once
            for (uint32_t j0 = 0; j0 < cnt; j0 += 64 * OUT_PL) {
                uint32_t o[OUT_PL], v[OUT_PL];
                uint64_t wu[OUT_PL];
                float ls[OUT_PL];
#pragma unroll
                for (int r = 0; r < OUT_PL; ++r) {
                    const uint32_t j = j0 + 64 * r + lane;
                    const uint32_t h = j < cnt ? stage[wv][j] : 0u;
                    o[r] = h & 0xffffu;
                    wu[r] = h >> 16;
                }
#pragma unroll
                for (int r = 0; r < OUT_PL; ++r) {
                    const bool ok = j0 + 64 * r + lane < cnt;
                    v[r] = IDENT ? o[r] : ok ? col[b + o[r]] : 0u;
                    ls[r] = WITH_LOSS && ok ? loss[b + o[r]] : 0.0f;
                    if (ok && wu[r] == 0xffffu) wu[r] = units_of(lat[b + o[r]]);  // wide weights
                }
#pragma unroll
                for (int r = 0; r < OUT_PL; ++r)
                    if (j0 + 64 * r + lane < cnt) put(v[r], wu[r], ls[r]);
            }
        } else if (L16) {  // rows of more hits: tested again
            for (uint64_t k = b + lane; k < e; k += 64) {
                const uint32_t w = lat16[k];
                if (w <= wmax_u && (uint32_t)(k - b) != u) put((uint32_t)(k - b), w, WITH_LOSS ? loss[k] : 0.0f);
            }
        } else {  // rows of more hits: tested again, chunk by chunk
            for (uint32_t c = 0; c < nch; ++c) {
                const uint64_t k = b + 64ull * c + lane;
                const uint64_t l = k < e ? lat[k] : ~0ull;
                if (l <= wmax_ns && (IDENT ? (uint32_t)(k - b) != u : col[k] != u))
                    put(IDENT ? (uint32_t)(k - b) : col[k], units_of(l), WITH_LOSS ? loss[k] : 0.0f);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(mw, off);
        mw = o > mw ? o : mw;
    }
    if (lane == 0 && mw) atomicMax(maxw, (unsigned long long)mw);
}

// In-rows of the level solve's class CSRs: every out-entry u -> v of class c
// (walked per out-row, one wave a row) placed at its (v, c) slot's cursor
// (in_off: the exclusive scan of lvl_out_kernel's counts), its head v (the
// bits of vmask) replaced by the tail u.
__global__ __launch_bounds__(256) void lvl_in_kernel(uint32_t V, uint32_t cls, uint64_t vmask,
                                                     const uint32_t *__restrict__ off_out,
                                                     const uint64_t *__restrict__ ce_out,
                                                     const uint32_t *__restrict__ in_off, uint32_t *__restrict__ in_cur,
                                                     uint64_t *__restrict__ ce_in) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t u = wave; u < V; u += nwaves) {
        const uint32_t *ou = off_out + (uint64_t)u * cls;
        const uint32_t e0 = ou[0], e1 = ou[cls - 1];
        for (uint32_t k = e0 + lane; k < e1; k += 64) {
            uint32_t c = 1;  // the class of entry k: the last class whose start is <= k
            while (c + 1 < cls && ou[c] <= k) ++c;
            const uint64_t w = ce_out[k];
            const uint32_t v = (uint32_t)(w & vmask);
            const uint64_t slot = (uint64_t)v * cls + c - 1;
            const uint32_t pos = in_off[slot] + atomicAdd(&in_cur[slot], 1u);
            ce_in[pos] = (w & ~vmask) | u;
        }
    }
}

// a latency in units of g for the u16 adjacency copy (exact: g divides every
// edge latency; 0xffff: longer than any class bound)
__device__ __forceinline__ uint16_t units16(uint64_t l, double inv_g) {
    const uint64_t u = (uint64_t)((double)l * inv_g + 0.5);
    return (uint16_t)(u < 0xffffu ? u : 0xffffu);
}

// Exact check that a level plan's class in-rows equal its out-rows, so the
// run builds only the out-rows (lvl_sym): the adjacency is V identity rows
// (proved by the host scan, CsrStats::ident: entry (u, v) at u * V + v) and
// every pair of latency <= wmax_ns has its mirror with the same latency (and,
// loss != nullptr, the same loss bits) -- then the class-c in-entries of x are
// the class-c out-entries of x, entry for entry.  Triangle tile pairs (bi <=
// bj) of 64 x 64: tile (bj, bi) staged in LDS, tile (bi, bj) compared with it
// transposed; a wave reads 64 consecutive latencies of a row a step (512 B),
// losses only where a latency is short enough to matter.  Any difference
// clears *ok.
__global__ __launch_bounds__(256) void lvl_sym_tile_kernel(uint32_t V, const uint64_t *__restrict__ lat,
                                                           const float *__restrict__ loss, uint64_t wmax_ns,
                                                           uint32_t *ok, uint16_t *__restrict__ lat16, double inv_g) {
    __shared__ uint64_t tl[64][65];
    __shared__ uint32_t tp[64][65];
    const uint32_t nb = (V + 63) / 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const uint64_t ntri = (uint64_t)nb * (nb + 1) / 2;
    bool bad = false;
    for (uint64_t t = blockIdx.x; t < ntri; t += gridDim.x) {
        // triangle index -> (bi, bj), bi <= bj: row bi starts at bi * nb - bi (bi - 1) / 2
        const double nn = 2.0 * nb + 1.0;
        uint32_t bi = (uint32_t)((nn - sqrt(nn * nn - 8.0 * (double)t)) * 0.5);
        auto row0 = [&](uint64_t r) { return r * nb - r * (r - 1) / 2; };
        while (bi > 0 && row0(bi) > t) --bi;
        while (row0(bi + 1) <= t) ++bi;
        const uint32_t bj = bi + (uint32_t)(t - row0(bi));
        // a wave's 16 rows of a tile in flight at once (latency and loss
        // together: 12 B a lane a row), then through LDS
        const uint32_t v_a = bi * 64 + tx;  // staged tile (bj, bi): column bi * 64 + tx
        uint64_t la[16];
        uint32_t pa[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t u = bj * 64 + ty + 4 * i;
            const bool in = u < V && v_a < V;
            const uint64_t k = (uint64_t)u * V + v_a;
            la[i] = in ? lat[k] : 0ull;
            pa[i] = in && loss ? __float_as_uint(loss[k]) : 0u;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            tl[ty + 4 * i][tx] = la[i];
            tp[ty + 4 * i][tx] = pa[i];
        }
        __syncthreads();
        // the u16-unit copy of the adjacency (V % 4 == 0): every tile, the
        // triangle's and its mirror's, out of the LDS tile 4 entries (8 B) a store
        auto put16 = [&](uint32_t r0, uint32_t c0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t gi = threadIdx.x + 256 * i, r = gi >> 4, c = (gi & 15) * 4;
                if (r0 + r < V && c0 + c < V) {
                    const uint32_t lo = units16(tl[r][c], inv_g) | (uint32_t)units16(tl[r][c + 1], inv_g) << 16;
                    const uint32_t hi = units16(tl[r][c + 2], inv_g) | (uint32_t)units16(tl[r][c + 3], inv_g) << 16;
                    *reinterpret_cast<uint2 *>(lat16 + (uint64_t)(r0 + r) * V + c0 + c) = make_uint2(lo, hi);
                }
            }
        };
        const uint32_t v_b = bj * 64 + tx;  // compared tile (bi, bj)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t u = bi * 64 + ty + 4 * i;
            const bool in = u < V && v_b < V;
            const uint64_t k = (uint64_t)u * V + v_b;
            la[i] = in ? lat[k] : 0ull;
            pa[i] = in && loss ? __float_as_uint(loss[k]) : 0u;
        }
        if (lat16) put16(bj * 64, bi * 64);  // the staged tile's, behind the compared tile's loads
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t r = ty + 4 * i, u = bi * 64 + r;
            if (u < V && v_b < V && u != v_b) {
                const uint64_t l = la[i], lm = tl[tx][r];
                if (l <= wmax_ns || lm <= wmax_ns) bad |= l != lm || pa[i] != tp[tx][r];
            }
        }
        __syncthreads();
        if (lat16 && bi != bj) {  // the compared tile through the same LDS tile
#pragma unroll
            for (int i = 0; i < 16; ++i) tl[ty + 4 * i][tx] = la[i];
            __syncthreads();
            put16(bi * 64, bj * 64);
            __syncthreads();
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicAnd(ok, 0u);
}

// The adjacency indices of the entries a level plan's class CSRs read
// (latency <= wmax_ns, not a self-loop), for the one-call build's loss upload
// (only those losses cross PCIe).  One wave per row: pass 1 keeps the chunks'
// ballots in LDS, one atomic reserves the row's range, pass 2 writes the
// indices in row order.  Past `cap` entries are counted, not written.
template <bool IDENT>
__global__ __launch_bounds__(256) void lvl_index_kernel(uint32_t V, const uint64_t *__restrict__ row_ptr,
                                                        const uint32_t *__restrict__ col,
                                                        const uint64_t *__restrict__ lat, uint64_t wmax_ns,
                                                        uint32_t *__restrict__ idx, uint64_t cap,
                                                        unsigned long long *cursor) {
    __shared__ uint64_t bal[4][TR_CH];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t u = wave; u < V; u += nwaves) {
        const uint64_t b = row_ptr[u], e = row_ptr[u + 1];
        const uint32_t nch = (uint32_t)((e - b + 63) / 64);
        auto test = [&](uint32_t c) -> uint64_t {
            const uint64_t k = b + 64ull * c + lane;
            const uint64_t l = k < e ? lat[k] : ~0ull;
            return __ballot(l <= wmax_ns && (IDENT ? (uint32_t)(k - b) != u : col[k] != u));
        };
        uint32_t cnt = 0;
        for (uint32_t c0 = 0; c0 < nch; c0 += 4) {
            uint64_t m[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) m[q] = c0 + q < nch ? test(c0 + q) : 0ull;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (c0 + q < TR_CH && lane == 0) bal[wv][c0 + q] = m[q];
                cnt += (uint32_t)__popcll(m[q]);
            }
        }
        unsigned long long base = 0;
        if (cnt && lane == 0) base = atomicAdd(cursor, (unsigned long long)cnt);
        base = __shfl(base, 0);
        if (!cnt || base + cnt > cap) continue;  // uniform
        for (uint32_t c = 0; c < nch; ++c) {
            const uint64_t m = c < TR_CH ? bal[wv][c] : test(c);
            if (!m) continue;  // uniform
            if ((m >> lane) & 1ull) idx[base + (uint64_t)__popcll(m & below)] = (uint32_t)(b + 64ull * c + lane);
            base += (uint64_t)__popcll(m);
        }
    }
}

// symmetric plans' one-call build: every uploaded loss equals its mirror's
// (identity rows: entry u * V + v <-> v * V + u; the mirror is uploaded too,
// having the same latency); any difference clears *ok
__global__ void loss_mirror_check_kernel(const uint32_t *__restrict__ idx, uint64_t count, uint64_t V,
                                         const float *__restrict__ loss, uint32_t *ok) {
    bool bad = false;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < count;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = idx[i];
        bad |= __float_as_uint(loss[k]) != __float_as_uint(loss[(k % V) * V + k / V]);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicAnd(ok, 0u);
}

__global__ void loss_scatter_kernel(const uint32_t *__restrict__ idx, const float *__restrict__ val, uint64_t count,
                                    float *__restrict__ loss) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < count;
         i += (uint64_t)gridDim.x * blockDim.x)
        loss[idx[i]] = val[i];
}

// The kept class structure (level_keep): a plan's graph cannot change after
// its creation, so which pairs its run lists, in which class and where each
// list starts is settled once the probe has proved the bound B -- row u of the
// run's out-rows is the prefix "classes 1..B" of row u of the probe's class
// rows (lists are stored in class order inside a row).  Kept once at creation:
// the class offsets at the run's stride (d_kcls) and the heads as u16 columns
// (d_kcol), rows based by a scan of their kept counts; a run only reads the
// kept edges' losses and packs the entries (lvl_fill_kernel).
// Step 1: row u's kept count (cnt[V] = 0, so the scan's last value is the total).
__global__ void lvl_keep_count_kernel(uint32_t V, uint32_t pcls, uint32_t B, const uint32_t *__restrict__ poff,
                                      uint32_t *__restrict__ cnt) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u > V) return;
    // slot k of a row: the start of class k + 1 (slot pcls - 1: the row's end; B <= pcls - 1)
    cnt[u] = u < V ? poff[(uint64_t)u * pcls + B] - poff[(uint64_t)u * pcls] : 0u;
}

// Step 2, one wave a vertex: the run's class offsets (rcls a vertex, lvl_out_kernel's
// layout: classes past B empty; written twice, the in-rows being the out-rows)
// from the probe's (pcls a vertex), and the prefix's heads as u16.
__global__ __launch_bounds__(256) void lvl_keep_kernel(uint32_t V, uint32_t pcls, uint32_t rcls, uint32_t B,
                                                       const uint32_t *__restrict__ poff,
                                                       const uint64_t *__restrict__ pent,
                                                       const uint32_t *__restrict__ base,
                                                       uint32_t *__restrict__ koff, uint16_t *__restrict__ kcol) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint64_t vc1 = (uint64_t)V * rcls + 1;
    for (uint32_t u = wave; u < V; u += nwaves) {
        const uint32_t *po = poff + (uint64_t)u * pcls;
        const uint32_t p0 = po[0], cnt = po[B] - p0, kb = base[u];
        if (lane < rcls) {
            const uint32_t o = kb + (lane < B ? po[lane] - p0 : cnt);
            koff[(uint64_t)u * rcls + lane] = o;
            koff[vc1 + (uint64_t)u * rcls + lane] = o;
        }
        for (uint32_t i = lane; i < cnt; i += 64) kcol[kb + i] = (uint16_t)pent[p0 + i];
    }
    if (wave == 0 && lane == 0) {  // the arrays' last word: the total
        const uint32_t total = base[V];
        koff[vc1 - 1] = total;
        koff[2 * vc1 - 1] = total;
    }
}

// The run's pass over a kept structure, one wave a row: the kept heads v of row
// u, their losses gathered (identity rows: loss[row_ptr[u] + v], FILL_UNR x 64
// of a row in flight: a C3 row's ~330 all go out before the first is used) and
// the entries stored at the kept indices, the bits lvl_out_kernel's put stores
// (CE4: 4-byte entries, *ovf set where a difference does not fit).
constexpr int FILL_UNR = 8;
template <bool CE4>
__global__ __launch_bounds__(256) void lvl_fill_kernel(uint32_t V, uint32_t cls, uint32_t vb,
                                                       const uint64_t *__restrict__ row_ptr,
                                                       const float *__restrict__ loss,
                                                       const uint32_t *__restrict__ koff,
                                                       const uint16_t *__restrict__ kcol, uint64_t *__restrict__ ce_out,
                                                       unsigned long long *ovf) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    bool over = false;
    for (uint32_t u = wave; u < V; u += nwaves) {
        const uint32_t b = koff[(uint64_t)u * cls], e = koff[(uint64_t)u * cls + cls - 1];
        const float *lrow = loss + row_ptr[u];
        for (uint32_t i0 = b + lane; i0 < e; i0 += 64 * FILL_UNR) {
            uint32_t v[FILL_UNR];
            float ls[FILL_UNR];
#pragma unroll
            for (int r = 0; r < FILL_UNR; ++r) v[r] = i0 + 64 * r < e ? kcol[i0 + 64 * r] : 0u;
#pragma unroll
            for (int r = 0; r < FILL_UNR; ++r) ls[r] = i0 + 64 * r < e ? lrow[v[r]] : 0.0f;
#pragma unroll
            for (int r = 0; r < FILL_UNR; ++r) {
                if (i0 + 64 * r >= e) continue;
                const float eb = 1.0f - ls[r];  // (1f32 - other.packet_loss), mod.rs:328
                if constexpr (CE4) {
                    // (a loss outside [0, 1] or a NaN wraps the difference past every field: it overflows too)
                    const uint32_t d = 0x3f800000u - __float_as_uint(eb);
                    over |= (d >> (32u - vb)) != 0;
                    reinterpret_cast<uint32_t *>(ce_out)[i0 + 64 * r] = v[r] | d << vb;
                } else {
                    ce_out[i0 + 64 * r] = ((uint64_t)__float_as_uint(eb) << 32) | v[r];
                }
            }
        }
    }
    if (CE4 && over) atomicOr(ovf, 1ull);
}

// the adjacency indices of a kept structure's entries (identity rows), row by
// row: the one-call build's needed losses without another pass over the latencies
__global__ __launch_bounds__(256) void lvl_keep_index_kernel(uint32_t V, uint32_t cls,
                                                             const uint64_t *__restrict__ row_ptr,
                                                             const uint32_t *__restrict__ koff,
                                                             const uint16_t *__restrict__ kcol,
                                                             uint32_t *__restrict__ idx, unsigned long long total,
                                                             unsigned long long *cnt) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t u = wave; u < V; u += nwaves) {
        const uint32_t b = koff[(uint64_t)u * cls], e = koff[(uint64_t)u * cls + cls - 1];
        const uint32_t r = (uint32_t)row_ptr[u];
        for (uint32_t i = b + lane; i < e; i += 64) idx[i] = r + kcol[i];
    }
    if (wave == 0 && lane == 0) *cnt = total;
}

// ------------------------------------------------------------ level solve
#if LOSS_COUNT
__device__ unsigned long long solve_cnt[8];  // diagnostic builds: [1] edge visits, [4] [6] [7] phase ticks: init, levels, out
__device__ unsigned long long lvl_cnt[8][5];  // level solve, per level (<= 7): ticks plan+compact / walk / collect, items, rows
__constant__ uint32_t lvl_diag;                // level solve ablations (SRT_LVL_DIAG)
#endif
#define LOSS_TICK(slot) LOSS_TICK_TO(solve_cnt, slot)
// the packed push: 1 keeps the state probe of the head's key as the select's
// predicate (a read before every min; C3 4.29 ms a step), 0 mins
// unconditionally (4.32; A/B builds)
#ifndef SRT_PK_PROBE
#define SRT_PK_PROBE 1
#endif
// The lean stages (`lean`, LVL_LEAN_* of srt_internal.h; SRT_LVL_LEAN=0: none).
// LIST_T: a push-only level of the packed row with at most so many items is
// walked LIST_LPI lanes an item and lists its members as they are hit, instead
// of a scan of the row for them (`lean` carries it in its high half, 0: never).
#ifndef SRT_LIST_T
#define SRT_LIST_T 16
#endif
constexpr uint32_t LIST_T = SRT_LIST_T;
// (a wider workgroup -- level_ce4_wide_kernel's 640 or 768 threads -- walks a
// listed level with its first 512 threads, the lanes an item staying 32)
constexpr uint32_t LIST_NT = 512;                 // threads that walk a listed level
constexpr uint32_t LIST_LPI = LIST_NT / LIST_T;  // lanes an item of a listed level
static_assert(LIST_T >= 1 && LIST_T * LIST_LPI == LIST_NT && LIST_NT <= PACK_NT,
              "a listed level's items share the narrowest workgroup evenly");
// The wave walk of the other push-only levels of the packed row (LVL_LEAN_WAVE):
// WAVE_B: items of a batch, dealt to the waves by a counter; WAVE_D: 64-entry
// passes in flight; WAVE_U: passes folded together (C3: 8 / 4 3.49 ms the solve,
// 4 / 2 3.65, 4 / 1 3.79, 12 / 4 3.78; 32 items a batch +0.14).  56 items a
// batch, not a lane's 64: a batch's passes are read in windows of 64, a lane a
// pass, and C3's class-1 lists (55 entries on average, one in ten of two
// passes) make about 70 passes of 64 items -- a second window of a few passes
// with a ring fill and drain of its own -- and 61.6 of 56, one window nine
// times in ten (r12, the solve: 64 items 3.389 ms, 60 3.405, 58 3.344, 56 3.299,
// 54 3.300, 52 3.309, 48 3.339).  At 768 threads a workgroup (r13, the solve
// 2.81 ms) 8 / 4 / 56 stays: 4 / 2 and 48 items the same, 8 / 2 +0.05, 64 items
// +0.07; a scalar-base entry address +0.04; a min only where the candidate is
// below the probed key: a region a min +0.01, one region a group of four +0.30,
// branch-free +1.65 (profiles/r13_level_wide).
#ifndef SRT_WAVE_B
#define SRT_WAVE_B 56
#endif
#ifndef SRT_WAVE_D
#define SRT_WAVE_D 8
#endif
#ifndef SRT_WAVE_U
#define SRT_WAVE_U 4
#endif
constexpr uint32_t WAVE_B = SRT_WAVE_B;
constexpr int WAVE_D = SRT_WAVE_D, WAVE_U = SRT_WAVE_U;
// LVL_LEAN_PULL: a level behind an unsettled list of at most V / PULL_LIST_DIV
// vertices collects over the list (a 2-byte L2 read, a key probe and a barrier a
// step of a workgroup's threads) instead of the row (16 B of keys a quad).  4:
// reasoned, not measured -- at a quarter of the row the list's steps are the
// row's, each behind a global read; C3's lists are a few hundred vertices, one step.
constexpr uint32_t PULL_LIST_DIV = 4;
static_assert(WAVE_B >= 1 && WAVE_B <= 64, "a batch's items: a lane each");
static_assert(WAVE_U >= 1 && WAVE_D % WAVE_U == 0, "the ring is folded in whole groups");
// probe != nullptr: no table; probe[2 + k] = the largest level over the
// in-use columns of row k (0xffff if one is unreached by level lcap), the u64
// at probe[0] += the edges walked.
// SP (VW = 2): the class lists walked as one stream of chunks a lane group,
// software-pipelined (see the walk below).
// PK (SP, CLSN 16, lcap <= PACK_LMAX): the packed row of srt_rowfold.h, 4.5 B
// a vertex, so that two 512-thread workgroups share a CU where the 8-B row
// allows one of 1,024 (16k vertices: 73,984 B against 131,328).  A 5-B row (u8
// level + f32 loss) does not fit twice: 2 x (256 + 5 x 16,384 + 544 B static)
// = 165,440 B > 163,840; nor do two workgroups of 1,024 threads: 8 waves a SIMD
// allow 64 VGPRs and the walk holds 104.  A vertex's key takes a hit's
// candidate by one atomicMin(1 << 30 | loss bits): state 3 -> 1 and the min
// over the tight in-edges at once (no level store a hit); a settled key (state
// 0) is below every candidate and skipped by its state.  The candidate's bits
// are masked to 30, so the state is exact whatever the losses are; the table's
// bits are the unpacked row's for losses in [0, 1], which every path to a plan
// enforces before a result is returned: the host scan (CsrStats::badloss_k,
// srt_api.cpp reference_errors), or -- the losses left to the device --
// first_bad_loss / the device range check (join_loss_check), whose error
// replaces the build's result.  The collect pass moves the keys of state 1 to
// state 0 and writes their 4-bit levels, a thread the word of its own quad
// (plain stores); the members go to mem_all + blockIdx.x * V (L2-resident, as
// level_q_kernel's).  spread: K lane groups an item in small levels (below).
// CE4 (PK; level_ce4_kernel): the class entries are the 4-byte form of
// lvl_out_kernel<..., CE4>, at the same indices; every walker decodes v = x &
// mask, bits(1 - e) = 0x3f800000 - (x >> vb), the 8-byte entry's fields bit for
// bit.
// The body is shared: level_solve_kernel runs it on 8-byte entries,
// level_ce4_kernel (the packed row alone) on 4-byte ones.
template <int LPT, int UNR, uint32_t CLSN, int VW, bool NT, bool SP, bool PK, bool CE4>
__device__ __forceinline__ void level_solve_body(
    uint32_t V, const uint32_t *__restrict__ nodes, uint32_t n, uint32_t row0, uint32_t row1,
    const uint32_t *__restrict__ cls_out, const uint32_t *__restrict__ cls_in, const uint64_t *__restrict__ ce_out,
    const uint64_t *__restrict__ ce_in, uint32_t lcap, uint64_t g, const uint64_t *__restrict__ sl_lat,
    const float *__restrict__ sl_loss, uint64_t *__restrict__ out_lat, float *__restrict__ out_loss,
    unsigned long long *stats, const uint32_t *__restrict__ row_list, void *__restrict__ out32,
    float *__restrict__ out32_loss, bool stage16, uint32_t *__restrict__ probe,
    unsigned long long *__restrict__ visit_cnt, bool idn, unsigned long long *row_ctr, uint16_t *mem_all,
    bool spread, uint32_t lean, uint32_t vb) {
    static_assert(!PK || (SP && CLSN == 16), "the packed row: the pipelined walk, levels <= PACK_LMAX");
    static_assert(!CE4 || PK, "4-byte class entries: the packed row's walks");
    const uint32_t vmask4 = (1u << vb) - 1u;  // CE4: an entry's vertex bits
    // CE4: a 4-byte entry as the 8-byte one's halves (.x the vertex, .y the bits of 1 - e)
    auto dec4 = [&](uint32_t xw) -> uint2 { return make_uint2(xw & vmask4, 0x3f800000u - (xw >> vb)); };
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long red_min[16], red_cnt[16], red_vis[16];
    __shared__ uint32_t dyn_k;
    __shared__ uint32_t red_max[16];
    constexpr uint32_t WCN = CLSN - 1;
    __shared__ uint32_t plan_end[WCN + 1];
    __shared__ uint64_t plan_push;
    __shared__ uint32_t plan_pull;
    __shared__ uint32_t cur[2][2];  // [level parity]: unsettled compaction, level collection
    __shared__ uint32_t cur_w[2];   // CE4, [level parity]: a deferred member list's cursor (scan_nib)
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem);  // hist[l]: end of level l in mem (l <= 31)
    uint16_t *lrow = reinterpret_cast<uint16_t *>(smem + SOLVE_HIST);
    uint32_t *prow = reinterpret_cast<uint32_t *>(smem + lds_prow_off(SOLVE_HIST, V));
    uint16_t *mem = PK ? mem_all + (uint64_t)blockIdx.x * V : reinterpret_cast<uint16_t *>(smem + lds_mem_off(SOLVE_HIST, V));
    uint32_t *key = reinterpret_cast<uint32_t *>(smem + SOLVE_HIST);  // PK: state | loss bits
    uint16_t *lev = reinterpret_cast<uint16_t *>(smem + pack_lev_off(V));  // PK: the levels of quad k in word k
    uint32_t *lev32 = reinterpret_cast<uint32_t *>(smem + pack_lev_off(V));  // ... the words of quads 2 k, 2 k + 1
    const uint32_t list_t = PK ? lean >> 16 : 0u;
    auto lev_of = [&](uint32_t v) -> uint32_t { return ((uint32_t)lev[v >> 2] >> (4 * (v & 3u))) & 0xfu; };
    const uint16_t LINF = 0xffffu;
    const uint32_t FINF = 0x7f800000u;  // +inf bits
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
    const uint32_t grp = tid / LPT, sub = tid % LPT, ngrp = nt / LPT;
    const uint64_t below = (1ull << lane) - 1ull;
    // The launch's minimum, unreached and visit counts live in the static LDS
    // reductions (a wave's slot, its lane 0 the only writer), folded in at each
    // row's end: none of them holds registers across the walk.
    if (tid < 16) {
        red_min[tid] = ~0ull;
        red_cnt[tid] = red_vis[tid] = 0;
    }
    // CE4: the row passes' stages (LVL_LEAN_SCAN / DEFER / PULL of srt_internal.h; uniform)
    const bool rows_scan = CE4 && (lean & LVL_LEAN_SCAN), rows_defer = CE4 && (lean & LVL_LEAN_DEFER);
    const bool rows_pull = CE4 && (lean & LVL_LEAN_PULL);
    bool clean = false;  // PK: the output pass before left every key and level unreached (uniform)
    const uint32_t nrows = row_list ? row1 : row1 - row0;
    // rows dealt by a counter (row_ctr != nullptr; else statically, row k to
    // workgroup k mod grid): a workgroup takes its next row while it writes
    // the row before (the atomic's latency behind the output phase), so a CU
    // whose rows ran long takes fewer; every workgroup makes exactly one fetch
    // past the last row
    unsigned long long kn = 0;
    auto fetch = [&]() -> uint32_t {
        if (tid == 0) dyn_k = (uint32_t)(kn < nrows ? kn : nrows);
        __syncthreads();
        return dyn_k;
    };
    if (row_ctr && tid == 0) kn = atomicAdd(&row_ctr[0], 1ull);
    uint32_t k0 = blockIdx.x;
    if (row_ctr) k0 = fetch();
    for (uint32_t k = k0; k < nrows; k = row_ctr ? fetch() : k + gridDim.x) {
        uint64_t mn = ~0ull;
        uint32_t unreach = 0, vis32 = 0;  // this row's, a lane (a row's entries and columns are < 2^32)
        const uint32_t i = row_list ? row_list[k] : row0 + k;
        const uint32_t s = nodes[i];
#if LOSS_COUNT
        unsigned long long tk0 = wall_clock64();
#endif
        // 1. every vertex unreached, s at level 0 (petgraph's zero score);
        // four vertices a thread a step (8-B level and 16-B loss stores)
        if (PK && clean) {
            // the row before's output pass stored the unreached pattern behind its reads: s alone is patched
            if (tid == 0) {
                key[s] = 0u;
                lev[s >> 2] = (uint16_t)(0xffffu & ~(0xfu << (4 * (s & 3u))));
            }
        } else if constexpr (PK) {
            // (the last quad's vertices past V stay unreached / 0xF: never read)
            for (uint32_t v4 = 4 * tid; v4 < V; v4 += 4 * nt) {
                const uint32_t q = s - v4;  // s among them: state 0, loss 0, level 0
                lev[v4 >> 2] = (uint16_t)(q < 4u ? 0xffffu & ~(0xfu << (4 * q)) : 0xffffu);
                if (v4 + 3 < V) {
                    *reinterpret_cast<uint4 *>(key + v4) =
                        make_uint4(q == 0 ? 0u : ~0u, q == 1 ? 0u : ~0u, q == 2 ? 0u : ~0u, q == 3 ? 0u : ~0u);
                } else {
                    for (uint32_t v = v4; v < V; ++v) key[v] = v == s ? 0u : ~0u;
                }
            }
        } else
        for (uint32_t v4 = 4 * tid; v4 < V; v4 += 4 * nt) {
            if (v4 + 3 < V) {
                uint2 lw = make_uint2(0xffffffffu, 0xffffffffu);
                uint4 pw = make_uint4(FINF, FINF, FINF, FINF);
                if (s - v4 < 4u) {  // s among them: level 0, loss 0 (selects, no indexed lvalue)
                    const uint32_t q = s - v4;
                    lw.x &= q == 0 ? 0xffff0000u : q == 1 ? 0x0000ffffu : 0xffffffffu;
                    lw.y &= q == 2 ? 0xffff0000u : q == 3 ? 0x0000ffffu : 0xffffffffu;
                    pw.x = q == 0 ? 0u : pw.x;
                    pw.y = q == 1 ? 0u : pw.y;
                    pw.z = q == 2 ? 0u : pw.z;
                    pw.w = q == 3 ? 0u : pw.w;
                }
                *reinterpret_cast<uint2 *>(lrow + v4) = lw;
                *reinterpret_cast<uint4 *>(prow + v4) = pw;
            } else {
                for (uint32_t v = v4; v < V; ++v) {
                    lrow[v] = v == s ? (uint16_t)0 : LINF;
                    prow[v] = v == s ? 0u : FINF;
                }
            }
        }
        if (tid == 0) {
            hist[0] = 1;
            mem[0] = (uint16_t)s;
            cur[1][0] = cur[1][1] = 0;
        }
        __syncthreads();
        LOSS_TICK(4)
        uint32_t settled = 1;
        // the vertices v with lrow[v] == want appended to mem[at + cur[par][ci]
        // ...) in any order: four a thread a step (one 8-B level read), one
        // LDS atomic a wave a step
        // (CE4, list = false: the members are counted alone -- in the wave, one
        // LDS atomic a wave a pass -- and their range of mem stays unwritten)
        auto compact = [&](uint16_t want, uint32_t at, uint32_t par, int ci, bool list) {
            uint32_t acc = 0;
            for (uint32_t v4 = 4 * tid; v4 < V; v4 += 4 * nt) {
                uint32_t fm = 0;
                if constexpr (PK) {
                    const uint32_t in = V - v4 >= 4u ? 0xfu : (1u << (V - v4)) - 1u;  // the quad's vertices < V
                    const uint32_t lw = lev[v4 >> 2];
                    if (want == LINF) {  // unsettled: the level still 0xF
                        fm = ((uint32_t)((lw & 0xfu) == 0xfu) | (uint32_t)((lw & 0xf0u) == 0xf0u) << 1 |
                              (uint32_t)((lw & 0xf00u) == 0xf00u) << 2 | (uint32_t)((lw & 0xf000u) == 0xf000u) << 3) & in;
                    } else {  // entered this level (state 1): settled, the state cleared, the level written
                        uint32_t nl = lw;
                        uint32_t kv[4];
                        if (in == 0xfu) {
                            const uint4 k4 = *reinterpret_cast<const uint4 *>(key + v4);
                            kv[0] = k4.x, kv[1] = k4.y, kv[2] = k4.z, kv[3] = k4.w;
                        } else {
#pragma unroll
                            for (uint32_t q = 0; q < 4; ++q) kv[q] = (in >> q) & 1u ? key[v4 + q] : ~0u;
                        }
#pragma unroll
                        for (uint32_t q = 0; q < 4; ++q)
                            if ((kv[q] >> 30) == 1u) {
                                fm |= 1u << q;
                                kv[q] &= PACK_LOSS;
                                nl = (nl & ~(0xfu << (4 * q))) | (uint32_t)want << (4 * q);
                            }
                        if (fm) {
                            lev[v4 >> 2] = (uint16_t)nl;
                            if (in == 0xfu) {
                                *reinterpret_cast<uint4 *>(key + v4) = make_uint4(kv[0], kv[1], kv[2], kv[3]);
                            } else {
#pragma unroll
                                for (uint32_t q = 0; q < 4; ++q)
                                    if ((in >> q) & 1u) key[v4 + q] = kv[q];
                            }
                        }
                    }
                } else if (v4 + 3 < V) {
                    const uint2 w = *reinterpret_cast<const uint2 *>(lrow + v4);
                    fm = (uint32_t)((w.x & 0xffffu) == want) | (uint32_t)((w.x >> 16) == want) << 1 |
                         (uint32_t)((w.y & 0xffffu) == want) << 2 | (uint32_t)((w.y >> 16) == want) << 3;
                } else {
                    for (uint32_t q = 0; q < 4; ++q)
                        if (v4 + q < V && lrow[v4 + q] == want) fm |= 1u << q;
                }
                if (CE4 && !list) {
                    acc += (uint32_t)__popc(fm);
                    continue;
                }
                uint32_t tot = 0, bel = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint64_t m = __ballot((fm >> q) & 1u);
                    tot += (uint32_t)__popcll(m);
                    bel += (uint32_t)__popcll(m & below);
                }
                if (!tot) continue;  // uniform
                uint32_t b = 0;
                if (lane == 0) b = atomicAdd(&cur[par][ci], tot);
                b = __shfl(b, 0);
                uint32_t pos = at + b + bel;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if ((fm >> q) & 1u) mem[pos++] = (uint16_t)(v4 + q);
            }
            if (CE4 && !list) {
                for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
                if (lane == 0 && acc) atomicAdd(&cur[par][ci], acc);
            }
        };
        // CE4: the vertices < V whose 4-bit level is `nib` appended to mem[at + *ctr
        // ...) in any order, a thread a 16-byte word of 32 levels: "some nibble of x
        // equals nib" is y & y >> 1 & y >> 2 & y >> 3 & 0x11111111 of y = ~(x ^ nib in
        // every nibble), so a word without one costs a dozen instructions and the
        // per-vertex work runs only where a word hits.  A wave that hits takes its
        // range by one LDS atomic (the lanes' counts summed by shuffles: a lane's own
        // atomic on the one counter cost a level of 2,818 members 2.7 us a row).
        // The levels' region is whole 16-byte words (solve_lds_bytes rounds it up to
        // 16 B: V / 32 words, rounded up); the nibbles past V in the last one -- the
        // last quad's 0xF, the padding's anything -- are masked.
        auto scan_nib = [&](uint32_t nib, uint32_t at, uint32_t *ctr) {
            const uint32_t pat = nib * 0x11111111u;
            const uint4 *lev128 = reinterpret_cast<const uint4 *>(smem + pack_lev_off(V));
            for (uint32_t w0 = (uint32_t)wv << 6; 32u * w0 < V; w0 += nt) {  // uniform in the wave
                const uint32_t w = w0 + lane;
                uint32_t h[4] = {0u, 0u, 0u, 0u};
                if (32u * w < V) {
                    const uint4 x4 = lev128[w];
                    h[0] = x4.x, h[1] = x4.y, h[2] = x4.z, h[3] = x4.w;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        uint32_t y = ~(h[q] ^ pat);
                        y &= y >> 1;
                        y &= y >> 2;
                        h[q] = y & 0x11111111u;  // bit 4 i: vertex 32 w + 8 q + i is at nib
                    }
                    if (32u * w + 32u > V) {  // the row's last word
#pragma unroll
                        for (uint32_t q = 0; q < 4; ++q) {
                            const uint32_t b = 32u * w + 8u * q, rem = V > b ? V - b : 0u;
                            if (rem < 8u) h[q] &= (1u << (4u * rem)) - 1u;
                        }
                    }
                }
                const uint32_t cnt = (uint32_t)(__popc(h[0]) + __popc(h[1]) + __popc(h[2]) + __popc(h[3]));
                if (!__ballot(cnt != 0u)) continue;  // uniform
                uint32_t incl = cnt;
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(incl, o);
                    if (lane >= o) incl += y;
                }
                uint32_t b = 0;
                if (lane == 63) b = atomicAdd(ctr, incl);
                uint32_t pos = at + (uint32_t)__shfl(b, 63) + incl - cnt;
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q)
                    for (uint32_t m = h[q]; m; m &= m - 1u)
                        mem[pos++] = (uint16_t)(32u * w + 8u * q + ((uint32_t)__builtin_ctz(m) >> 2));
            }
        };
        // 2. levels in increasing latency
        for (uint32_t l = 1; l <= lcap && settled < V; ++l) {
            const uint32_t U = V - settled, par = l & 1u;
            if (tid == 0) {
                uint32_t run = 0, pl = 0;
                uint64_t pm = 0;
                for (uint32_t w = 1; w <= WCN; ++w) {
                    uint32_t items = 0;
                    if (w <= l) {
                        const uint32_t j = l - w, nj = hist[j] - (j ? hist[j - 1] : 0u);
                        if (nj && nj <= U) {
                            pm |= 1ull << w;
                            items = nj;
                        } else if (nj) {
                            pl = 1;
                            items = U;
                        }
                    }
                    run += items;
                    plan_end[w] = run;
                }
                plan_push = pm;
                plan_pull = pl;
                cur[par][0] = cur[par][1] = 0;
                if constexpr (CE4) cur_w[par] = 0;
            }
            __syncthreads();
            const uint32_t T = plan_end[WCN];
            const uint64_t pm = plan_push;
            // no tail level l - w (w <= WCN, every class) holds a vertex: the
            // levels >= l are all empty (uniform)
            if (T == 0) break;
#if LOSS_COUNT
            unsigned long long lt0 = wall_clock64();
#define LVL_TICK(q)                                                                    \
    if (tid == 0 && l < 8) {                                                           \
        const unsigned long long lt1 = wall_clock64();                                 \
        atomicAdd(&lvl_cnt[l][q], lt1 - lt0);                                          \
        lt0 = lt1;                                                                     \
    }
            if (tid == 0 && l < 8) {
                atomicAdd(&lvl_cnt[l][3], (unsigned long long)T);
                atomicAdd(&lvl_cnt[l][4], 1ull);
            }
#else
#define LVL_TICK(q)
#endif
            if (plan_pull) {
                // the unsettled vertices into mem[settled, V) (any order)
                if (rows_scan) scan_nib(0xfu, settled, &cur[par][0]);
                else compact(LINF, settled, par, 0, true);
                __syncthreads();
            }
            LVL_TICK(0)
            // item t: its class w (searched up from the w passed in -- a lane
            // group's items come in increasing t, so from its last item's:
            // one LDS read, not up to WCN dependent ones), vertex and list
            auto item = [&](uint32_t t, uint32_t &w, uint32_t &x, uint32_t &e0, uint32_t &e1) {
                while (t >= plan_end[w]) ++w;
                const uint32_t m = t - (w > 1 ? plan_end[w - 1] : 0u), j = l - w;
                const bool push = (pm >> w) & 1ull;
                x = mem[push ? (j ? hist[j - 1] : 0u) + m : settled + m];
                const uint32_t *cl = push ? cls_out : cls_in;
                e0 = cl[(uint64_t)x * CLSN + w - 1];
                e1 = cl[(uint64_t)x * CLSN + w];
            };
            // PK: a push-only level of few items (uniform) does not scan the row for its
            // members: LIST_LPI lanes an item walk its list entry by entry, the hit's min
            // is the returning form, and the one lane that finds the head unreached
            // (state 3; every later hit finds state 1) appends it to the members
            bool listed = false;
            if constexpr (PK) listed = T <= list_t && !plan_pull;
            // ... and one of more items is walked a wave an item (LVL_LEAN_WAVE; uniform)
            bool waved = false;
            if constexpr (PK) waved = (lean & LVL_LEAN_WAVE) && T > list_t && !plan_pull;
            if (PK && listed) {
                const uint32_t t = tid / LIST_LPI, ls = tid % LIST_LPI;
                if (t < T) {
                    uint32_t w = 1, x, e0, e1;
                    item(t, w, x, e0, e1);
                    vis32 += ls == 0 ? e1 - e0 : 0u;
                    const float onem = 1.0f - __uint_as_float(key[x] & PACK_LOSS);
                    for (uint32_t e = e0 + ls; e < e1; e += LIST_LPI) {
                        uint2 wd;
                        if constexpr (CE4) {
                            wd = dec4(reinterpret_cast<const uint32_t *>(ce_out)[e]);
                        } else {
                            wd = reinterpret_cast<const uint2 *>(ce_out)[e];
                        }
                        const uint32_t o = wd.x;
                        const uint32_t b = __float_as_uint(1.0f - __fmul_rn(onem, __uint_as_float(wd.y)));
                        if (key[o] > PACK_LOSS && atomicMin(&key[o], 1u << 30 | (b & PACK_LOSS)) >= 3u << 30)
                            mem[settled + atomicAdd(&cur[par][1], 1u)] = (uint16_t)o;
                    }
                }
            } else if (PK && waved) {
                // One wave an item: what a lane group of the chunk walk below works out
                // in vector registers a chunk (which item and chunk come next, the
                // entry address, the slot bounds) is uniform in the wave here and is
                // scalar work.  Batches of `bs` items are dealt by the level's counter
                // (cur[par][0]: a push-only level compacts no unsettled list); lane i of
                // a batch fetches item t0 + i (its list and 1 - loss of its vertex).
                // The batch's lists then go by as one stream of passes of 64 entries, a
                // lane an entry, the mins under one exec mask: lane p works out pass
                // p's list place, length and 1 - loss once a batch, and a pass costs
                // three readlanes and no branch.  A pass is loaded WAVE_D passes ahead
                // of its fold, a ring in registers; every step loads (lanes past the
                // list its last entry, steps past the last pass that pass again), so
                // the loads in flight can be counted.  WAVE_U passes are folded
                // together (their probes, then their mins), so that one's LDS latency
                // hides behind the others'.  The candidate is the chunk walk's; its min
                // goes out where the chunk walk's select keeps it.
                constexpr int D = WAVE_D, U = WAVE_U;
                const uint32_t Tu = __builtin_amdgcn_readfirstlane(T);
                const uint32_t per = (Tu + (uint32_t)nw - 1) / (uint32_t)nw;  // (the workgroup's own waves: 8, 10 or 12)
                const uint32_t bs = per < WAVE_B ? per : WAVE_B;  // a small level: every wave a share
                for (;;) {
                    uint32_t bi = 0;
                    if (lane == 0) bi = atomicAdd(&cur[par][0], 1u);
                    const uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane(bi) * bs;
                    if (t0 >= Tu) break;
                    const uint32_t nb = Tu - t0 < bs ? Tu - t0 : bs;
                    uint32_t w = 1, x = 0, e0 = 0, e1 = 0;
                    float onem = 0.0f;
                    if ((uint32_t)lane < nb) {
                        item(t0 + lane, w, x, e0, e1);
                        onem = 1.0f - __uint_as_float(key[x] & PACK_LOSS);
                    }
                    const uint32_t len = e1 - e0;  // (lanes past the batch: 0)
                    vis32 += len;
                    // the batch's passes in list order: pass p lies in the item whose
                    // running count of passes is the first above p (a search over the
                    // lanes' inclusive counts), a window of 64 passes a lane each
                    const uint32_t np = (len + 63u) >> 6;
                    uint32_t incl = np;
                    for (int o = 1; o < 64; o <<= 1) {
                        const uint32_t y = __shfl_up(incl, o);
                        if (lane >= o) incl += y;
                    }
                    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane(incl, 63);
                    for (uint32_t win = 0; win < total; win += 64u) {
                    const uint32_t p = win + lane;
                    uint32_t it = 0;  // the items whose passes all lie before p (<= 63)
#pragma unroll
                    for (uint32_t sb = 32; sb; sb >>= 1)
                        if ((uint32_t)__shfl(incl, it + sb - 1u) <= p) it += sb;
                    const uint32_t il = __shfl(len, it);
                    const uint32_t j = p - ((uint32_t)__shfl(incl, it) - ((il + 63u) >> 6));  // pass j of item `it`
                    // pass p (a lane past the last: never read): first entry, entries from it on, 1 - loss
                    const uint32_t pb = (uint32_t)__shfl(e0, it) + 64u * j, pr = il - 64u * j;
                    const uint32_t pom = __shfl(__float_as_uint(onem), it);
                    const uint32_t nq = total - win < 64u ? total - win : 64u;
                    typename std::conditional<CE4, uint32_t, uint2>::type ring[D];  // (CE4: one register a pass)
                    uint32_t rrem[D], rom[D];  // a ring slot's entries (0: none) and 1 - loss, uniform
                    auto issue = [&](int r, uint32_t q) {
                        const uint32_t qc = q < nq ? q : nq - 1u;
                        const uint32_t rm = (uint32_t)__builtin_amdgcn_readlane(pr, qc);
                        rrem[r] = q < nq ? rm : 0u;
                        rom[r] = (uint32_t)__builtin_amdgcn_readlane(pom, qc);
                        const uint32_t o = (uint32_t)lane < rm - 1u ? (uint32_t)lane : rm - 1u;
                        const uint32_t pq = (uint32_t)__builtin_amdgcn_readlane(pb, qc);
                        if constexpr (CE4) {
                            ring[r] = reinterpret_cast<const uint32_t *>(ce_out)[pq + o];  // 256 B a pass
                        } else {
                            ring[r] = reinterpret_cast<const uint2 *>(ce_out + pq)[o];
                        }
                    };
                    auto entry = [&](int r) -> uint2 {
                        if constexpr (CE4) {
                            return dec4(ring[r]);
                        } else {
                            return ring[r];
                        }
                    };
#pragma unroll
                    for (int r = 0; r < D; ++r) issue(r, r);
                    for (uint32_t q0 = 0; q0 < nq; q0 += D) {
#pragma unroll
                        for (int r0 = 0; r0 < D; r0 += U) {
                            // (every lane holds an entry of the list: the probes and the
                            // candidates need no mask, the mins alone do)
#if SRT_PK_PROBE
                            uint32_t ko[U];
#pragma unroll
                            for (int u = 0; u < U; ++u) ko[u] = key[entry(r0 + u).x];
#endif
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const uint2 wd = entry(r0 + u);
                                const uint32_t b = __float_as_uint(1.0f - __fmul_rn(__uint_as_float(rom[r0 + u]), __uint_as_float(wd.y)));
#if SRT_PK_PROBE
                                if ((uint32_t)lane < rrem[r0 + u] && ko[u] > PACK_LOSS)
#else
                                if ((uint32_t)lane < rrem[r0 + u])
#endif
                                    atomicMin(&key[wd.x], 1u << 30 | (b & PACK_LOSS));
                            }
#pragma unroll
                            for (int u = 0; u < U; ++u) issue(r0 + u, q0 + r0 + u + D);
                        }
                    }
                    }
                }
            } else
            if constexpr (SP) {
                // The level's items as one stream of chunks a lane group (CH
                // entries of one item's class list, UNR pairs a lane): the next
                // chunk's entry loads go out before this chunk's level probes
                // and folds, so their latency hides behind the LDS work, and an
                // item's offsets are read one item ahead.  Push and pull chunks
                // run apart (push is uniform in an item and, but at a class
                // boundary, in a wave), without a per-entry direction test.
                static_assert(VW == 2, "the pipelined walk loads entry pairs");
                constexpr uint32_t CH = UNR * LPT * 2;
                constexpr int NE = UNR * 2;
                // (CE4: an entry pair is 8 B, the even entry 8-B aligned)
                typedef typename std::conditional<CE4, uint2, uint4>::type pair_t;
                auto load = [&](pair_t *d, uint32_t w, uint32_t b) {
                    const uint64_t *ce = ((pm >> w) & 1ull) ? ce_out : ce_in;
#pragma unroll
                    for (int q = 0; q < UNR; ++q) {
                        if constexpr (CE4) {
                            d[q] = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint32_t *>(ce) + b + (sub + q * LPT) * 2);
                        } else {
                            d[q] = *reinterpret_cast<const uint4 *>(ce + b + (sub + q * LPT) * 2);
                        }
                    }
                };
                // a small level (2 T <= lane groups) in a workgroup alone on its
                // CU (1,024 threads: nothing else hides its latency): K groups an
                // item, group g taking item g mod T's chunks g div T, + K, + 2K,
                // ... (one item a group), so its few lists are walked in one or
                // two steps instead of one chunk a step by one group (C3 4.40 ->
                // 4.26 ms; C2's 4 workgroups a CU: 0.334 -> 0.351 ms, so not there;
                // the packed row's two workgroups a CU: C3 solve 4.225 -> 4.194 ms,
                // so there too -- `spread`)
                const uint32_t K = (PK ? spread : nt == LOSS_NT) && 2 * T <= ngrp ? ngrp / T : 1u;
                const uint32_t CHS = K * CH;  // a group's chunk stride in an item
                uint32_t ct = K > 1 ? (grp < T * K ? grp % T : T) : grp, cw = 1, cx = 0, ce0 = 0, ce1 = 0;
                uint32_t pw = 1, px = 0, pe0 = 0, pe1 = 0;  // the group's next item
                if (ct < T) item(ct, cw, cx, ce0, ce1);
                pw = cw;
                if (ct + ngrp < T) item(ct + ngrp, pw, px, pe0, pe1);
                uint32_t cb = (ce0 & ~1u) + (K > 1 ? grp / T : 0u) * CH;
                pair_t cur[UNR];
                if (ct < T && cb < ce1) load(cur, cw, cb);  // (a chunk past a short list: nothing to load)
                while (ct < T) {
                    // the next chunk: this item's next one, or the next item's first
                    uint32_t nt2 = ct, nw2 = cw, nx2 = cx, ne02 = ce0, ne12 = ce1, nb = cb + CHS;
                    const bool adv = nb >= ce1;
                    if (adv) {
                        nt2 = ct + ngrp;
                        nw2 = pw;
                        nx2 = px;
                        ne02 = pe0;
                        ne12 = pe1;
                        nb = pe0 & ~1u;
                    }
                    pair_t nxt[UNR];
                    if (nt2 < T) load(nxt, nw2, nb);
                    if (adv && nt2 + ngrp < T) item(nt2 + ngrp, pw, px, pe0, pe1);
                    if (cb < ce1) {
                        uint64_t wd[NE];
                        uint32_t o[NE];
                        bool ok[NE];
                        // the lane's slots: slot s (pair q = s / 2 at 2 LPT q) holds
                        // entry a0 + s, inside the list from s_lo on and below s_hi
                        // (s_lo <= 1: the chunk starts at the even entry at or
                        // below e0) -- one compare a slot but the first
                        const uint32_t a0 = cb + 2 * sub;
                        const int32_t s_lo = (int32_t)(ce0 - a0), s_hi = (int32_t)(ce1 - a0);
#pragma unroll
                        for (int q = 0; q < UNR; ++q) {
                            if constexpr (CE4) {
                                const uint2 a = dec4(cur[q].x), c = dec4(cur[q].y);
                                wd[2 * q] = ((uint64_t)a.y << 32) | a.x;
                                wd[2 * q + 1] = ((uint64_t)c.y << 32) | c.x;
                            } else {
                                wd[2 * q] = ((uint64_t)cur[q].y << 32) | cur[q].x;
                                wd[2 * q + 1] = ((uint64_t)cur[q].w << 32) | cur[q].z;
                            }
                            ok[2 * q] = 2 * LPT * q < s_hi && (q > 0 || s_lo <= 0);
                            ok[2 * q + 1] = 2 * LPT * q + 1 < s_hi;
                        }
                        // every entry of [e0, e1) is walked once, also under the K
                        // spread: the lane group that takes an item's first chunk
                        // counts the whole list
                        vis32 += sub == 0 && cb == (ce0 & ~1u) ? ce1 - ce0 : 0u;
                        if constexpr (PK) {
                            // A slot outside the list aims at the item's own
                            // vertex: settled on push, unsettled on pull, so it is
                            // no hit and its min is a no-op.
#pragma unroll
                            for (int q = 0; q < NE; ++q) o[q] = ok[q] ? (uint32_t)wd[q] : cx;
                            if ((pm >> cw) & 1ull) {
                                // push: the head's key takes state 1 and the min of
                                // the candidates.  Branch-free: a candidate is
                                // above every settled key (state 0 < 1 << 30) and
                                // all ones lowers no key, so the NE mins go out
                                // back to back without an exec-mask region each.
                                const float onem = 1.0f - __uint_as_float(key[cx] & PACK_LOSS);
                                uint32_t c[NE];
#if SRT_PK_PROBE
                                uint32_t ko[NE];
#pragma unroll
                                for (int q = 0; q < NE; ++q) ko[q] = key[o[q]];
#endif
#pragma unroll
                                for (int q = 0; q < NE; ++q) {
                                    const float r = __uint_as_float((uint32_t)(wd[q] >> 32));
                                    const uint32_t b = __float_as_uint(1.0f - __fmul_rn(onem, r));
#if SRT_PK_PROBE
                                    c[q] = ko[q] > PACK_LOSS ? 1u << 30 | (b & PACK_LOSS) : ~0u;
#else
                                    c[q] = ok[q] ? 1u << 30 | (b & PACK_LOSS) : ~0u;
#endif
                                }
#pragma unroll
                                for (int q = 0; q < NE; ++q) atomicMin(&key[o[q]], c[q]);
                            } else {
                                // pull: the tail's 4-bit level against j (<= 13, never
                                // the unsettled 0xF); a tail at j is settled.  The
                                // tails' losses are read for every slot (any o is a
                                // vertex), the lane's candidates folded in registers.
                                const uint32_t j = l - cw;
                                uint32_t lo4[NE], ku[NE];
#pragma unroll
                                for (int q = 0; q < NE; ++q) lo4[q] = lev_of(o[q]);
#pragma unroll
                                for (int q = 0; q < NE; ++q) ku[q] = key[o[q]];
                                uint32_t best = ~0u;
#pragma unroll
                                for (int q = 0; q < NE; ++q) {
                                    const float r = __uint_as_float((uint32_t)(wd[q] >> 32));
                                    const float lu = __uint_as_float(ku[q] & PACK_LOSS);
                                    const uint32_t b = __float_as_uint(1.0f - __fmul_rn(1.0f - lu, r));
                                    const uint32_t c = lo4[q] == j ? 1u << 30 | (b & PACK_LOSS) : ~0u;
                                    best = c < best ? c : best;
                                }
                                if (best != ~0u) atomicMin(&key[cx], best);
                            }
                        } else {
#pragma unroll
                            for (int q = 0; q < NE; ++q) o[q] = ok[q] ? (uint32_t)wd[q] : 0u;
                            uint16_t lo_[NE];
#pragma unroll
                            for (int q = 0; q < NE; ++q) lo_[q] = lrow[o[q]];
                            if ((pm >> cw) & 1ull) {
                                // push: x in N_j, its class-w out-edges x -> v, v
                                // unsettled or at l: v enters level l (stored once),
                                // its loss min-folded by an LDS atomic
                                const float onem = 1.0f - __uint_as_float(prow[cx]);
#pragma unroll
                                for (int q = 0; q < NE; ++q)
                                    if (ok[q] && lo_[q] >= (uint16_t)l) {
                                        const float r = __uint_as_float((uint32_t)(wd[q] >> 32));
#if LOSS_COUNT
                                        if (!(lvl_diag & 2) && lo_[q] > (uint16_t)l) lrow[o[q]] = (uint16_t)l;
                                        if (!(lvl_diag & 1))
                                            atomicMin(&prow[o[q]], __float_as_uint(1.0f - __fmul_rn(onem, r)));
#else
                                        if (lo_[q] > (uint16_t)l) lrow[o[q]] = (uint16_t)l;
                                        atomicMin(&prow[o[q]], __float_as_uint(1.0f - __fmul_rn(onem, r)));
#endif
                                    }
                            } else {
                                // pull: x unsettled, its class-w in-edges u -> x, u in N_j
                                const uint32_t j = l - cw;
#pragma unroll
                                for (int q = 0; q < NE; ++q)
                                    if (ok[q] && lo_[q] == (uint16_t)j) {
                                        const float r = __uint_as_float((uint32_t)(wd[q] >> 32));
                                        lrow[cx] = (uint16_t)l;
                                        const float c = 1.0f - __fmul_rn(1.0f - __uint_as_float(prow[o[q]]), r);
                                        atomicMin(&prow[cx], __float_as_uint(c));
                                    }
                            }
                        }
                    }
                    ct = nt2;
                    cw = nw2;
                    cx = nx2;
                    ce0 = ne02;
                    ce1 = ne12;
                    cb = nb;
#pragma unroll
                    for (int q = 0; q < UNR; ++q) cur[q] = nxt[q];
                }
            } else {
                uint32_t nw_ = 1, nx = 0, ne0 = 0, ne1 = 0;
                if (grp < T) item(grp, nw_, nx, ne0, ne1);
                for (uint32_t t = grp; t < T; t += ngrp) {
                    const uint32_t w = nw_, x = nx, e0 = ne0, e1 = ne1, j = l - w;
                    if (t + ngrp < T) item(t + ngrp, nw_, nx, ne0, ne1);
                    const bool push = (pm >> w) & 1ull;
                    const uint64_t *ce = push ? ce_out : ce_in;
                    // push: x in N_j, its class-w out-edges x -> v, v unsettled or at l;
                    // pull: x unsettled, its class-w in-edges u -> x, u in N_j
                    const float onem = push ? 1.0f - __uint_as_float(prow[x]) : 0.0f;
                    constexpr int NE = UNR * VW;
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
#pragma unroll
                        for (int q = 0; q < NE; ++q) {
                            vis32 += ok[q];
                            const bool hit = ok[q] && (push ? lo_[q] >= (uint16_t)l : lo_[q] == (uint16_t)j);
                            if (hit) {
                                // the head enters level l (every writer stores l; a
                                // head already at l is not stored again), its loss
                                // min-folded by an LDS atomic (reading the loss first
                                // and skipping the atomic when it cannot lower it
                                // measured slower: C3 walk 49 -> 56 us a row)
                                const float r = __uint_as_float((uint32_t)(wd[q] >> 32));
                                if (push) {
#if LOSS_COUNT
                                    // diagnostic builds: lvl_diag bit 0 drops the loss atomics,
                                    // bit 1 the level stores (wrong tables; timing only)
                                    if (!(lvl_diag & 2) && lo_[q] != (uint16_t)l) lrow[o[q]] = (uint16_t)l;
                                    if (!(lvl_diag & 1))
                                        atomicMin(&prow[o[q]], __float_as_uint(1.0f - __fmul_rn(onem, r)));
#else
                                    if (lo_[q] != (uint16_t)l) lrow[o[q]] = (uint16_t)l;
                                    atomicMin(&prow[o[q]], __float_as_uint(1.0f - __fmul_rn(onem, r)));
#endif
                                } else {
                                    lrow[x] = (uint16_t)l;
                                    const float c = 1.0f - __fmul_rn(1.0f - __uint_as_float(prow[o[q]]), r);
                                    atomicMin(&prow[x], __float_as_uint(c));
                                }
                            }
                        }
                    }
                }
            }
            __syncthreads();  // every head of level l found
            LVL_TICK(1)
            // N_l (the vertices now at level l) -> mem[settled, ...)
            if (PK && listed) {
                // the listed members alone: the state cleared, the 4-bit level by an atomic on
                // the 32-bit word of the vertex's quad pair (up to 8 members share it)
                const uint32_t got = cur[par][1];
                for (uint32_t m = tid; m < got; m += nt) {
                    const uint32_t v = mem[settled + m];
                    key[v] &= PACK_LOSS;
                    atomicAnd(&lev32[v >> 3], ~((0xfu ^ l) << (4 * (v & 7u))));
                }
            } else if (rows_pull && plan_pull && U <= V / PULL_LIST_DIV) {
                // A level behind an unsettled list (mem[settled, settled + U), written before the
                // walk): every vertex that entered the level -- pushed or pulled -- was unsettled
                // then, so the members are the list's vertices of state 1, and a short list is
                // walked instead of the row.  State 1 -> 0 and the level as the listed collect's;
                // the members are packed to the list's front in place: a step's appends land
                // below (step + 1) nt, where every read was made before the step's barrier.
                uint32_t nx = tid < U ? mem[settled + tid] : 0u;
                for (uint32_t b0 = 0; b0 < U; b0 += nt) {  // uniform
                    const uint32_t m = b0 + tid, v = nx;
                    if (m + nt < U) nx = mem[settled + m + nt];
                    bool hit = false;
                    if (m < U) {
                        const uint32_t kv = key[v];
                        hit = (kv >> 30) == 1u;
                        if (hit) {
                            key[v] = kv & PACK_LOSS;
                            atomicAnd(&lev32[v >> 3], ~((0xfu ^ l) << (4 * (v & 7u))));
                        }
                    }
                    __syncthreads();
                    const uint64_t bm = __ballot(hit);
                    if (!bm) continue;  // uniform in the wave
                    uint32_t b = 0;
                    if (lane == 0) b = atomicAdd(&cur[par][1], (uint32_t)__popcll(bm));
                    b = __shfl(b, 0);
                    if (hit) mem[settled + b + (uint32_t)__popcll(bm & below)] = (uint16_t)v;
                }
            } else {
                // A level's list is read only by a later level that pushes from it, and the plan
                // above pushes from N_j only where nj <= U; U only falls, and right behind this
                // collect it is V - settled - nl.  So a level of nl > V - settled - nl members can
                // never be pushed from: its range of mem stays reserved (hist and every index as
                // they are) and unwritten.  One that can is listed behind the barrier by the wide
                // scan for its level.  Exact, not a heuristic: the test is the plan's own.
                compact((uint16_t)l, settled, par, 1, !rows_defer);
                if (rows_defer) {
                    __syncthreads();
                    const uint32_t nl = cur[par][1];
                    if (nl && nl <= V - settled - nl) scan_nib(l, settled, &cur_w[par]);
                }
            }
            __syncthreads();
            LVL_TICK(2)
            settled += cur[par][1];
            if (tid == 0) hist[l] = settled;
        }
        __syncthreads();  // hist / lrow final for the output
        LOSS_TICK(6)
        if (row_ctr && tid == 0) kn = atomicAdd(&row_ctr[0], 1ull);  // the next row
        // this row's counts into the wave's slots of the static reductions
        auto row_fold = [&]() {
            for (int off = 32; off > 0; off >>= 1) {
                const uint64_t o = __shfl_xor(mn, off);
                mn = o < mn ? o : mn;
                unreach += __shfl_xor(unreach, off);
                vis32 += __shfl_xor(vis32, off);  // (a row's visits: < 2^32 entries)
            }
            if (lane == 0) {
                red_min[wv] = mn < red_min[wv] ? mn : red_min[wv];
                red_cnt[wv] += unreach;
                red_vis[wv] += vis32;
            }
        };
        // 3. table row i (or staging slot k), or the probe's row maximum
        if (probe) {  // (probe rows run the unpacked row: their caps are 15, 31, 63)
            uint32_t rmax = 0;
            for (uint32_t j0 = tid; j0 < n; j0 += nt) {
                const uint32_t l = PK ? lev_of(nodes[j0]) : lrow[nodes[j0]];
                rmax = l > rmax ? l : rmax;
            }
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = __shfl_xor(rmax, off);
                rmax = o > rmax ? o : rmax;
            }
            if (lane == 0) red_max[wv] = rmax;
            __syncthreads();
            if (tid == 0) {
                uint32_t m = 0;
                for (int q = 0; q < nw; ++q) m = red_max[q] > m ? red_max[q] : m;
                probe[2 + k] = m;
            }
            row_fold();
            __syncthreads();
            continue;
        }
        uint64_t *ol = out_lat + (uint64_t)i * n;
        float *op = out_loss + (uint64_t)i * n;
        uint32_t *o32 = out32 && !stage16 ? reinterpret_cast<uint32_t *>(out32) + (uint64_t)k * n : nullptr;
        uint16_t *o16 = out32 && stage16 ? reinterpret_cast<uint16_t *>(out32) + (uint64_t)k * n : nullptr;
        float *o32p = out32_loss ? out32_loss + (uint64_t)k * n : nullptr;
        if (idn) {
            // every node in use, in node order (nodes[j] = j, n = V, n % 4 == 0):
            // four columns a thread a step -- one 8-B level and one 16-B loss
            // read from LDS, 16-B non-temporal stores
            typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
            // PK: the unreached pattern stored back behind a quad's reads (this loop covers the
            // row: n = V), so that the workgroup's next row patches its source alone
            const bool reinit = PK && (lean & LVL_LEAN_INIT);
            clean = reinit;
            for (uint32_t j4 = 4 * tid; j4 < n; j4 += 4 * nt) {
                // (PK: one 2-B word of levels, 0xF = unreached, and the 16 B of keys)
                const uint32_t l4 = PK ? lev[j4 >> 2] : 0u;
                const uint2 lw = PK ? make_uint2(0u, 0u) : *reinterpret_cast<const uint2 *>(lrow + j4);
                const uint4 pw = *reinterpret_cast<const uint4 *>((PK ? key : prow) + j4);
                if (reinit) {
                    lev[j4 >> 2] = (uint16_t)0xffffu;
                    *reinterpret_cast<uint4 *>(key + j4) = make_uint4(~0u, ~0u, ~0u, ~0u);
                }
                auto lv4 = [&](int q) -> uint32_t {
                    const uint32_t x = (l4 >> (4 * q)) & 0xfu;
                    return x == 0xfu ? (uint32_t)LINF : x;
                };
                const uint32_t lv[4] = {PK ? lv4(0) : lw.x & 0xffffu, PK ? lv4(1) : lw.x >> 16,
                                        PK ? lv4(2) : lw.y & 0xffffu, PK ? lv4(3) : lw.y >> 16};
                const uint32_t pv[4] = {pw.x, pw.y, pw.z, pw.w};  // (PK: settled keys, the loss bits as they are)
                uint64_t lu[4], latv[4];
                float lossv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (j4 + q == i) {
                        latv[q] = sl_lat[i];
                        lossv[q] = sl_loss[i];
                        lu[q] = latv[q] == ~0ull ? ~0ull : latv[q] / g;
                    } else if (lv[q] == LINF) {
                        ++unreach;
                        latv[q] = lu[q] = ~0ull;
                        lossv[q] = 1.0f;
                    } else {
                        lu[q] = lv[q];
                        latv[q] = lu[q] * g;
                        lossv[q] = __uint_as_float(pv[q]);
                    }
                    mn = latv[q] < mn ? latv[q] : mn;
                }
                const f32x4 lp = {lossv[0], lossv[1], lossv[2], lossv[3]};
                if (o32p) {
                    if (o16) {
                        const u16x4 lq = {(unsigned short)(latv[0] == ~0ull ? 0xffffu : lu[0]),
                                          (unsigned short)(latv[1] == ~0ull ? 0xffffu : lu[1]),
                                          (unsigned short)(latv[2] == ~0ull ? 0xffffu : lu[2]),
                                          (unsigned short)(latv[3] == ~0ull ? 0xffffu : lu[3])};
                        __builtin_nontemporal_store(lq, reinterpret_cast<u16x4 *>(o16 + j4));
                    } else if (o32) {
                        const u32x4 lq = {latv[0] == ~0ull ? ~0u : (unsigned)lu[0],
                                          latv[1] == ~0ull ? ~0u : (unsigned)lu[1],
                                          latv[2] == ~0ull ? ~0u : (unsigned)lu[2],
                                          latv[3] == ~0ull ? ~0u : (unsigned)lu[3]};
                        __builtin_nontemporal_store(lq, reinterpret_cast<u32x4 *>(o32 + j4));
                    }
                    __builtin_nontemporal_store(lp, reinterpret_cast<f32x4 *>(o32p + j4));
                } else if (NT) {
                    const u64x2 a = {latv[0], latv[1]}, c = {latv[2], latv[3]};
                    __builtin_nontemporal_store(a, reinterpret_cast<u64x2 *>(ol + j4));
                    __builtin_nontemporal_store(c, reinterpret_cast<u64x2 *>(ol + j4 + 2));
                    __builtin_nontemporal_store(lp, reinterpret_cast<f32x4 *>(op + j4));
                } else {
                    *reinterpret_cast<u64x2 *>(ol + j4) = u64x2{latv[0], latv[1]};
                    *reinterpret_cast<u64x2 *>(ol + j4 + 2) = u64x2{latv[2], latv[3]};
                    *reinterpret_cast<f32x4 *>(op + j4) = lp;
                }
            }
        } else
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
                    const uint16_t l = PK ? (lev_of(vv[q]) == 0xfu ? LINF : (uint16_t)lev_of(vv[q])) : lrow[vv[q]];
                    if (l == LINF) {
                        ++unreach;
                        latv = lu = ~0ull;
                        lossv = 1.0f;
                    } else {
                        lu = l;
                        latv = lu * g;
                        lossv = __uint_as_float(PK ? key[vv[q]] : prow[vv[q]]);
                    }
                }
                // streamed out without allocating in the caches (NT): the
                // class CSRs the walks read stay resident
                if (o32p) {
                    if (o16) __builtin_nontemporal_store(latv == ~0ull ? (uint16_t)0xffffu : (uint16_t)lu, o16 + j);
                    else if (o32) __builtin_nontemporal_store(latv == ~0ull ? ~0u : (uint32_t)lu, o32 + j);
                    __builtin_nontemporal_store(lossv, o32p + j);
                } else if (NT) {
                    __builtin_nontemporal_store(latv, ol + j);
                    __builtin_nontemporal_store(lossv, op + j);
                } else {
                    ol[j] = latv;
                    op[j] = lossv;
                }
                mn = latv < mn ? latv : mn;
            }
        }
        row_fold();
        __syncthreads();  // the next row rewrites the LDS rows
        LOSS_TICK(7)
    }
    __syncthreads();  // (a workgroup without a row: the slots' initial values)
    if (tid == 0) {
        unsigned long long m = red_min[0], c = red_cnt[0], vz = red_vis[0];
        for (int q = 1; q < nw; ++q) {
            m = red_min[q] < m ? red_min[q] : m;
            c += red_cnt[q];
            vz += red_vis[q];
        }
#if LOSS_COUNT
        if (!probe) atomicAdd(&solve_cnt[1], vz);
#endif
        if (probe) {
            if (vz) atomicAdd(reinterpret_cast<unsigned long long *>(probe), vz);
        } else {
            atomicMin(&stats[0], m);
            if (c) atomicAdd(&stats[1], c);
            if (visit_cnt && vz) atomicAdd(visit_cnt, vz);
        }
        // the last workgroup done (every fetch made) returns the counter to 0
        // for the next launch (memory-side atomics; the launch boundary orders it)
        if (row_ctr && atomicAdd(&row_ctr[1], 1ull) == gridDim.x - 1ull) {
            atomicExch(&row_ctr[0], 0ull);
            atomicExch(&row_ctr[1], 0ull);
        }
    }
}

template <int LPT, int UNR, uint32_t CLSN, int VW, bool NT, bool SP = false, bool PK = false>
__global__ __launch_bounds__(LOSS_NT) void level_solve_kernel(
    uint32_t V, const uint32_t *__restrict__ nodes, uint32_t n, uint32_t row0, uint32_t row1,
    const uint32_t *__restrict__ cls_out, const uint32_t *__restrict__ cls_in, const uint64_t *__restrict__ ce_out,
    const uint64_t *__restrict__ ce_in, uint32_t lcap, uint64_t g, const uint64_t *__restrict__ sl_lat,
    const float *__restrict__ sl_loss, uint64_t *__restrict__ out_lat, float *__restrict__ out_loss,
    unsigned long long *stats, const uint32_t *__restrict__ row_list, void *__restrict__ out32,
    float *__restrict__ out32_loss, bool stage16, uint32_t *__restrict__ probe,
    unsigned long long *__restrict__ visit_cnt, bool idn, unsigned long long *row_ctr, uint16_t *mem_all,
    bool spread, uint32_t lean) {
    level_solve_body<LPT, UNR, CLSN, VW, NT, SP, PK, false>(V, nodes, n, row0, row1, cls_out, cls_in, ce_out, ce_in, lcap, g,
                                                            sl_lat, sl_loss, out_lat, out_loss, stats, row_list, out32,
                                                            out32_loss, stage16, probe, visit_cnt, idn, row_ctr, mem_all,
                                                            spread, lean, 0u);
}

// The packed row on 4-byte class entries (vb: the bits of V - 1): the packed
// instantiation's arguments and the entry's vertex bits.
template <bool NT>
__global__ __launch_bounds__(LOSS_NT) void level_ce4_kernel(
    uint32_t V, const uint32_t *__restrict__ nodes, uint32_t n, uint32_t row0, uint32_t row1,
    const uint32_t *__restrict__ cls_out, const uint32_t *__restrict__ cls_in, const uint64_t *__restrict__ ce_out,
    const uint64_t *__restrict__ ce_in, uint32_t lcap, uint64_t g, const uint64_t *__restrict__ sl_lat,
    const float *__restrict__ sl_loss, uint64_t *__restrict__ out_lat, float *__restrict__ out_loss,
    unsigned long long *stats, const uint32_t *__restrict__ row_list, void *__restrict__ out32,
    float *__restrict__ out32_loss, bool stage16, uint32_t *__restrict__ probe,
    unsigned long long *__restrict__ visit_cnt, bool idn, unsigned long long *row_ctr, uint16_t *mem_all,
    bool spread, uint32_t lean, uint32_t vb) {
    level_solve_body<4, 4, 16, 2, NT, true, true, true>(V, nodes, n, row0, row1, cls_out, cls_in, ce_out, ce_in, lcap, g, sl_lat,
                                                        sl_loss, out_lat, out_loss, stats, row_list, out32, out32_loss,
                                                        stage16, probe, visit_cnt, idn, row_ctr, mem_all, spread, lean, vb);
}

// ... in workgroups of NTH = 640 or 768 threads, two a CU as well: 5 or 6 waves
// a SIMD instead of 4 on the same LDS, which the 4-byte-entry walk's registers
// allow (78 VGPRs of the 80 that six waves leave; the 8-byte walk's 126 do not)
// once the chunk walk keeps UNR = 2 entry pairs a lane in flight, not 4.  The
// wave walk runs at the same rate a wave, so its throughput follows the waves
// (r13, C3: the solve 3.31 ms at 512 threads, 3.03 at 640, 2.81 at 768).  The
// body takes its thread and wave counts from blockDim; the plan chooses NTH at
// its create (level_ce4_threads, knob SRT_LVL_CE4_NT).
constexpr uint32_t CE4_WIDE_NT[] = {640, 768};  // the wide instantiations' threads (level_ce4_kernel: PACK_NT)
template <bool NT, int NTH, int UNR>
__global__ __launch_bounds__(NTH, 2 * NTH / 256) void level_ce4_wide_kernel(
    uint32_t V, const uint32_t *__restrict__ nodes, uint32_t n, uint32_t row0, uint32_t row1,
    const uint32_t *__restrict__ cls_out, const uint32_t *__restrict__ cls_in, const uint64_t *__restrict__ ce_out,
    const uint64_t *__restrict__ ce_in, uint32_t lcap, uint64_t g, const uint64_t *__restrict__ sl_lat,
    const float *__restrict__ sl_loss, uint64_t *__restrict__ out_lat, float *__restrict__ out_loss,
    unsigned long long *stats, const uint32_t *__restrict__ row_list, void *__restrict__ out32,
    float *__restrict__ out32_loss, bool stage16, uint32_t *__restrict__ probe,
    unsigned long long *__restrict__ visit_cnt, bool idn, unsigned long long *row_ctr, uint16_t *mem_all,
    bool spread, uint32_t lean, uint32_t vb) {
    static_assert(NTH % 128 == 0 && NTH > (int)PACK_NT && NTH / 64 <= 16,
                  "two workgroups fill whole waves a SIMD; 16 reduction slots");
    level_solve_body<4, UNR, 16, 2, NT, true, true, true>(V, nodes, n, row0, row1, cls_out, cls_in, ce_out, ce_in, lcap, g, sl_lat,
                                                          sl_loss, out_lat, out_loss, stats, row_list, out32, out32_loss,
                                                          stage16, probe, visit_cnt, idn, row_ctr, mem_all, spread, lean, vb);
}

// ------------------------------------------------- quantized level solve
// The level solve for latencies that are not small integers of g (Shadow
// reads any unit down to ns, units.rs:377-388: C3ns has g = 1 ns and edges of
// 1-301 ms).  Buckets of width q <= the shortest edge (units): bucket k holds
// the vertices of L(s, v) in [k q, (k + 1) q), classes c = floor(w / q) >= 1.
// A tight predecessor u of v has L(s, u) <= L(s, v) - q, so it lies in an
// earlier bucket, and an edge of class c out of bucket j reaches bucket j + c
// or j + c + 1.  Processing the pairs (j, c) with j + c = k at step k (push
// along class-c out-edges of N_j, or pull into the unsettled set along class-c
// in-edges from tails in bucket j, the smaller end as in level_solve_kernel)
// therefore leaves every vertex whose key lands in bucket k final once step k
// is done: its candidates come from steps k - 1 and k only.  A vertex's key is
// one u64, L units << 32 | loss bits, min-ed by an LDS atomic: the
// lexicographic (latency, loss) order of the reference's Dijkstra (mod.rs:
// 305-340), over tails that are final when read.  Candidates past dcap (the
// probe's bound B) are dropped, so every key stored is settled by the last
// bucket, B / q.  Class entries: v in bits [0, vb), the weight's remainder
// w - c q in [vb, vb + rb), (1f32 - e) bits in [34, 64).  LDS: 8 B a vertex;
// the settled vertices in bucket order live in a per-workgroup global scratch
// (mem_all + blockIdx.x * V, L2-resident).  stage_mode: 0 the table, 2 u32
// units + f32 loss staging (row k at k * n), 3 8-byte records {units, loss
// bits}.  probe != nullptr: probe[2 + k] = the largest L units over the in-use
// columns of row k (~0 if one is unreached), the u64 at probe[0] += visits.
template <int LPT, int UNR, uint32_t CLSN, int VW, bool NT>
__global__ __launch_bounds__(LOSS_NT) void level_q_kernel(
    uint32_t V, const uint32_t *__restrict__ nodes, uint32_t n, uint32_t row0, uint32_t row1,
    const uint32_t *__restrict__ cls_out, const uint32_t *__restrict__ cls_in, const uint64_t *__restrict__ ce_out,
    const uint64_t *__restrict__ ce_in, uint32_t kcap, uint32_t dcap, uint32_t qw, uint32_t rb, uint32_t vb, uint64_t g,
    const uint64_t *__restrict__ sl_lat, const float *__restrict__ sl_loss, uint64_t *__restrict__ out_lat,
    float *__restrict__ out_loss, unsigned long long *stats, const uint32_t *__restrict__ row_list,
    void *__restrict__ stage, float *__restrict__ stage_loss, uint32_t stage_mode, uint32_t *__restrict__ probe,
    unsigned long long *__restrict__ visit_cnt, uint16_t *__restrict__ mem_all) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long red_min[16], red_cnt[16], red_vis[16];
    __shared__ uint32_t red_max[16];
    constexpr uint32_t WCN = CLSN - 1;
    __shared__ uint32_t plan_end[WCN + 1];
    __shared__ uint64_t plan_push;
    __shared__ uint32_t plan_pull;
    __shared__ uint32_t cur[2][2];
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem);  // hist[k]: end of bucket k in mem (k <= 31)
    unsigned long long *key = reinterpret_cast<unsigned long long *>(smem + SOLVE_HIST);
    uint16_t *mem = mem_all + (uint64_t)blockIdx.x * V;
    const unsigned long long KINF = ~0ull;
    const uint64_t vmask = (1ull << vb) - 1ull, rmask = (1ull << rb) - 1ull;
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
    const uint32_t grp = tid / LPT, sub = tid % LPT, ngrp = nt / LPT;
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t mn = ~0ull;
    unsigned long long unreach = 0, visits = 0;
    const uint32_t nrows = row_list ? row1 : row1 - row0;
    for (uint32_t k = blockIdx.x; k < nrows; k += gridDim.x) {
        const uint32_t i = row_list ? row_list[k] : row0 + k;
        const uint32_t s = nodes[i];
        for (uint32_t v = tid; v < V; v += nt) key[v] = v == s ? 0ull : KINF;
        if (tid == 0) {
            hist[0] = 1;
            mem[0] = (uint16_t)s;
            cur[1][0] = cur[1][1] = 0;
        }
        __syncthreads();
        uint32_t settled = 1;
        for (uint32_t b = 1; b <= kcap && settled < V; ++b) {
            const uint32_t U = V - settled, par = b & 1u;
            if (tid == 0) {
                uint32_t run = 0, pl = 0;
                uint64_t pm = 0;
                for (uint32_t c = 1; c <= WCN; ++c) {
                    uint32_t items = 0;
                    if (c <= b) {
                        const uint32_t j = b - c, nj = hist[j] - (j ? hist[j - 1] : 0u);
                        if (nj && nj <= U) {
                            pm |= 1ull << c;
                            items = nj;
                        } else if (nj) {
                            pl = 1;
                            items = U;
                        }
                    }
                    run += items;
                    plan_end[c] = run;
                }
                plan_push = pm;
                plan_pull = pl;
                cur[par][0] = cur[par][1] = 0;
            }
            __syncthreads();
            const uint32_t T = plan_end[WCN];
            const uint64_t pm = plan_push;
            const uint32_t lo = b * qw, hi = lo + qw;  // bucket b: latencies [lo, hi)
            if (T && plan_pull) {
                // the unsettled vertices (key at bucket >= b, or none) into mem[settled, V)
                for (uint32_t base = 0; base < V; base += nt) {
                    const uint32_t v = base + tid;
                    const bool f = v < V && (uint32_t)(key[v] >> 32) >= lo;
                    const uint64_t m = __ballot(f);
                    if (!m) continue;  // uniform
                    uint32_t o = 0;
                    if (lane == 0) o = atomicAdd(&cur[par][0], (uint32_t)__popcll(m));
                    o = __shfl(o, 0);
                    if (f) mem[settled + o + (uint32_t)__popcll(m & below)] = (uint16_t)v;
                }
                __syncthreads();
            }
            auto item = [&](uint32_t t, uint32_t &c, uint32_t &x, uint32_t &e0, uint32_t &e1) {
                c = 1;
                while (t >= plan_end[c]) ++c;
                const uint32_t m = t - (c > 1 ? plan_end[c - 1] : 0u), j = b - c;
                const bool push = (pm >> c) & 1ull;
                x = mem[push ? (j ? hist[j - 1] : 0u) + m : settled + m];
                const uint32_t *cl = push ? cls_out : cls_in;
                e0 = cl[(uint64_t)x * CLSN + c - 1];
                e1 = cl[(uint64_t)x * CLSN + c];
            };
            uint32_t nc_ = 1, nx = 0, ne0 = 0, ne1 = 0;
            if (grp < T) item(grp, nc_, nx, ne0, ne1);
            for (uint32_t t = grp; t < T; t += ngrp) {
                const uint32_t c = nc_, x = nx, e0 = ne0, e1 = ne1, j = b - c;
                if (t + ngrp < T) item(t + ngrp, nc_, nx, ne0, ne1);
                const bool push = (pm >> c) & 1ull;
                const uint64_t *ce = push ? ce_out : ce_in;
                const uint32_t cbase = c * qw, jlo = j * qw, jhi = jlo + qw;
                // push: x in bucket j (final), its class-c out-edges x -> v;
                // pull: x unsettled, its class-c in-edges u -> x from u in bucket j
                const unsigned long long kx = push ? key[x] : 0ull;
                const uint32_t dx = (uint32_t)(kx >> 32);
                const float onem = 1.0f - __uint_as_float((uint32_t)kx);
                unsigned long long best = KINF;
                constexpr int NE = UNR * VW;
                for (uint32_t e = VW == 2 ? e0 & ~1u : e0; e < e1; e += UNR * LPT * VW) {
                    uint64_t wd[NE];
                    uint32_t ei[NE], o[NE];
                    bool ok[NE];
                    load_entries<UNR, LPT, VW>(ce, e, sub, e0, e1, wd, ei, ok);
#pragma unroll
                    for (int q = 0; q < NE; ++q) o[q] = ok[q] ? (uint32_t)(wd[q] & vmask) : 0u;
                    unsigned long long ko[NE];
#pragma unroll
                    for (int q = 0; q < NE; ++q) ko[q] = key[o[q]];
#pragma unroll
                    for (int q = 0; q < NE; ++q) {
                        visits += ok[q];
                        const uint32_t w = cbase + (uint32_t)((wd[q] >> vb) & rmask);
                        const float r = __uint_as_float((uint32_t)(wd[q] >> 34));
                        if (push) {
                            const uint32_t d = dx + w;
                            const unsigned long long ck =
                                ((unsigned long long)d << 32) | __float_as_uint(1.0f - __fmul_rn(onem, r));
                            if (ok[q] && d <= dcap && ck < ko[q]) atomicMin(&key[o[q]], ck);
                        } else {
                            const uint32_t du = (uint32_t)(ko[q] >> 32), d = du + w;
                            // tail in bucket j (an unreached tail's ~0 is past every bucket)
                            if (ok[q] && du >= jlo && du < jhi && d <= dcap) {
                                const float lu = __uint_as_float((uint32_t)ko[q]);
                                const unsigned long long ck =
                                    ((unsigned long long)d << 32) | __float_as_uint(1.0f - __fmul_rn(1.0f - lu, r));
                                best = ck < best ? ck : best;
                            }
                        }
                    }
                }
                if (!push && best != KINF) atomicMin(&key[x], best);
            }
            __syncthreads();  // every key of bucket b final
            // N_b (the keys now in bucket b) -> mem[settled, ...)
            for (uint32_t base = 0; base < V; base += nt) {
                const uint32_t v = base + tid;
                const unsigned long long kv = v < V ? key[v] : KINF;
                const uint32_t dv = (uint32_t)(kv >> 32);
                const bool f = kv != KINF && dv >= lo && dv < hi;
                const uint64_t m = __ballot(f);
                if (!m) continue;  // uniform
                uint32_t o = 0;
                if (lane == 0) o = atomicAdd(&cur[par][1], (uint32_t)__popcll(m));
                o = __shfl(o, 0);
                if (f) mem[settled + o + (uint32_t)__popcll(m & below)] = (uint16_t)v;
            }
            __syncthreads();
            const uint32_t got = cur[par][1];
            // no tail in buckets b - WCN .. b and bucket b empty: every later
            // bucket is empty (uniform)
            if (!T && !got) break;
            settled += got;
            if (tid == 0) hist[b] = settled;
        }
        __syncthreads();  // keys final for the output
        if (probe) {
            uint32_t rmax = 0;
            for (uint32_t j0 = tid; j0 < n; j0 += nt) {
                const unsigned long long kv = key[nodes[j0]];
                const uint32_t l = kv == KINF ? ~0u : (uint32_t)(kv >> 32);
                rmax = l > rmax ? l : rmax;
            }
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = __shfl_xor(rmax, off);
                rmax = o > rmax ? o : rmax;
            }
            if (lane == 0) red_max[wv] = rmax;
            __syncthreads();
            if (tid == 0) {
                uint32_t m = 0;
                for (int q = 0; q < nw; ++q) m = red_max[q] > m ? red_max[q] : m;
                probe[2 + k] = m;
            }
            __syncthreads();
            continue;
        }
        uint64_t *ol = out_lat + (uint64_t)i * n;
        float *op = out_loss + (uint64_t)i * n;
        uint32_t *o32 = stage_mode == 2 ? reinterpret_cast<uint32_t *>(stage) + (uint64_t)k * n : nullptr;
        float *o32p = stage_mode == 2 ? stage_loss + (uint64_t)k * n : nullptr;
        uint2 *orec = stage_mode == 3 ? reinterpret_cast<uint2 *>(stage) + (uint64_t)k * n : nullptr;
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
                    const unsigned long long kv = key[vv[q]];
                    if (kv == KINF) {
                        ++unreach;
                        latv = lu = ~0ull;
                        lossv = 1.0f;
                    } else {
                        lu = kv >> 32;
                        latv = lu * g;
                        lossv = __uint_as_float((uint32_t)kv);
                    }
                }
                // a staged self-loop past the u32 field saturates; the
                // consumers rewrite the diagonal from the host's self-loops
                const uint32_t l32 = lu >= 0xffffffffull ? ~0u : (uint32_t)lu;
                if (orec) {
                    __builtin_nontemporal_store(((uint64_t)__float_as_uint(lossv) << 32) | l32,
                                                reinterpret_cast<uint64_t *>(orec) + j);
                } else if (o32) {
                    __builtin_nontemporal_store(l32, o32 + j);
                    __builtin_nontemporal_store(lossv, o32p + j);
                } else if (NT) {
                    __builtin_nontemporal_store(latv, ol + j);
                    __builtin_nontemporal_store(lossv, op + j);
                } else {
                    ol[j] = latv;
                    op[j] = lossv;
                }
                mn = latv < mn ? latv : mn;
            }
        }
        __syncthreads();  // the next row rewrites the LDS keys and the scratch
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(mn, off);
        mn = o < mn ? o : mn;
        unreach += __shfl_xor(unreach, off);
        visits += __shfl_xor(visits, off);
    }
    if (lane == 0) {
        red_min[wv] = mn;
        red_cnt[wv] = unreach;
        red_vis[wv] = visits;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = red_min[0], c = red_cnt[0], vz = red_vis[0];
        for (int q = 1; q < nw; ++q) {
            m = red_min[q] < m ? red_min[q] : m;
            c += red_cnt[q];
            vz += red_vis[q];
        }
        if (probe) {
            if (vz) atomicAdd(reinterpret_cast<unsigned long long *>(probe), vz);
        } else {
            atomicMin(&stats[0], m);
            if (c) atomicAdd(&stats[1], c);
            if (visit_cnt && vz) atomicAdd(visit_cnt, vz);
        }
    }
}

// The shortest non-self-loop edge latency (ns) min-ed into *out: one wave per
// adjacency row; the column is read only where the latency would lower the
// lane's minimum (the quantized level solve's bucket width)
__global__ __launch_bounds__(256) void edge_min_kernel(uint32_t V, const uint64_t *__restrict__ row_ptr,
                                                       const uint32_t *__restrict__ col,
                                                       const uint64_t *__restrict__ lat, unsigned long long *out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    uint64_t m = ~0ull;
    for (uint32_t u = wave; u < V; u += nwaves) {
        const uint64_t b = row_ptr[u], e = row_ptr[u + 1];
        for (uint64_t k = b + lane; k < e; k += 64) {
            const uint64_t l = lat[k];
            if (l < m && col[k] != u) m = l;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(m, off);
        m = o < m ? o : m;
    }
    if (lane == 0 && m != ~0ull) atomicMin(out, (unsigned long long)m);
}

// the level build's per-run counters in one launch (small memsets are a
// ~4.6 us fill kernel each on the device timeline): stats, the class max,
// the visit count; or (stats == nullptr) the class-CSR pass's cursor and max
__global__ void level_zero_kernel(unsigned long long *stats, unsigned long long *a, unsigned long long *b,
                                  unsigned long long *c = nullptr) {
    if (stats) {
        stats[0] = ~0ull;
        stats[1] = 0ull;
    }
    if (a) *a = 0ull;
    if (b) *b = 0ull;
    if (c) *c = 0ull;
}

}  // namespace

LevelCtx level_ctx(srt_plan *p) {
    LevelCtx c;
    c.device = p->device;
    c.stream = p->stream;
    c.V = p->V;
    c.n = p->n;
    c.g = p->kp.g;
    c.t_cls = p->t_cls;
    c.tcls = p->lvl_keep_run ? p->d_kcls : p->d_tcls;  // (a kept structure's offsets: level_keep)
    c.ce_out = p->d_tpk;
    c.ce_in = p->lvl_single ? p->d_tpk : p->d_tpk2;
    c.nodes = p->d_nodes;
    c.sl_lat = p->d_sl_lat;
    c.sl_loss = p->d_sl_loss;
    c.out_lat = p->d_out_lat;
    c.out_loss = p->d_out_loss;
    c.visits = p->d_lvisit;
    c.q = p->lvl_q;
    c.rb = p->lvl_rb;
    c.vb = p->lvl_vb;
    c.lmem = p->d_lmem;
    c.idn = p->ident_nodes && p->n == p->V && p->n % 4 == 0;
    c.nt_store = p->lvl_nt;
    c.sp = p->lvl_sp;
    c.pack = p->lvl_pack;
    c.spread = p->lvl_spread;
    c.ce4 = p->lvl_ce4_run;
    c.ce4_nt = p->lvl_ce4_nt;
    // (the packed row's listed levels: LIST_T items at most; SRT_LVL_LIST_T: fewer, A/B)
    const char *lt = std::getenv("SRT_LVL_LIST_T");
    const uint32_t list_t = std::min<uint32_t>(lt ? (uint32_t)std::atoi(lt) : LIST_T, LIST_T);
    c.lean = p->lvl_lean | (p->lvl_lean & LVL_LEAN_LIST ? list_t << 16 : 0u);
    // rows dealt by a counter (knob SRT_LVL_DYN=0: statically, A/B)
    const bool dyn = p->lvl_dyn;
    if (dyn && !p->d_rowctr) {
        if (hipMalloc(&p->d_rowctr, 2 * sizeof(unsigned long long)) != hipSuccess ||
            hipMemsetAsync(p->d_rowctr, 0, 2 * sizeof(unsigned long long), p->stream) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(p->d_rowctr);
            p->d_rowctr = nullptr;
        }
    }
    c.row_ctr = dyn ? p->d_rowctr : nullptr;
    return c;
}

void level_ce4_off(srt_plan *p) {
    p->lvl_ce4 = p->lvl_ce4_pending = false;
    const size_t at = p->desc.find(" ce=4");
    if (at != std::string::npos) p->desc.erase(at, 5);
}

uint32_t level_vbits(uint32_t V) {
    uint32_t vb = 1;
    while ((1u << vb) < V) ++vb;
    return vb;
}

// level_grid's arithmetic: the workgroups whose LDS rows a CU holds (160 KB,
// 2 KB a workgroup for its static LDS and the allocation's granule)
int level_rows_per_cu(uint32_t V, bool quant, bool packed) {
    return (int)((160 * 1024) / (solve_lds_bytes(V, quant, packed) + 2048));
}

namespace {
// ------------------------------------------------------------ level solve
// a run of p at its bound fills a kept class structure (level_keep): the plan is still symmetric
bool level_keep_applies(const srt_plan *p) {
    return p->lvl_kept && p->lvl_sym && !p->lvl_q && p->lvl_kbound == p->kp.lmax;
}

// what both class-CSR builds allocate: class offsets and counts, cursor, class max
srt_status level_csr_arrays(srt_plan *p, uint64_t vc1, srt_err *err) {
    uint64_t cap_cur = p->d_tcursor ? 1 : 0, cap_mw = p->d_tmaxw ? 1 : 0;
    srt_status st = ensure_class_arrays(p, vc1, err);
    if (st == SRT_OK) st = grow(&p->d_tcursor, &cap_cur, 1, err, "hipMalloc(level cursor)");
    if (st == SRT_OK) st = grow(&p->d_tmaxw, &cap_mw, 1, err, "hipMalloc(level max)");
    return st;
}

// lvl_out_kernel over adjacency rows [u0, u1) at the bound wns (ns): ident =
// identity rows of a symmetric plan (out-rows only: no in-row counts), l16 =
// they read the u16-unit copy p->d_lat16.  Class offsets to `offsets`, entries
// to `entries` (slots below `cap`, from the cursor's value on).
// ce4: the 4-byte entries of the packed row's walk (ident, with_loss, q = 0; vb = level_vbits(V)), overflow word
// p->d_lvisit[1].
void launch_lvl_out(srt_plan *p, bool with_loss, bool ident, bool l16, uint32_t u0, uint32_t u1, uint64_t wns,
                    uint32_t cls, uint32_t q, uint32_t vb, uint32_t *offsets, uint64_t *entries, uint64_t cap,
                    bool ce4 = false) {
    const auto kern = ce4    ? (l16 ? lvl_out_kernel<true, false, true, true, true> : lvl_out_kernel<true, false, true, false, true>)
                      : !ident ? (with_loss ? lvl_out_kernel<true> : lvl_out_kernel<false>)
                      : l16  ? (with_loss ? lvl_out_kernel<true, false, true, true> : lvl_out_kernel<false, false, true, true>)
                             : (with_loss ? lvl_out_kernel<true, false, true> : lvl_out_kernel<false, false, true>);
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(8192, (u1 - u0 + 3) / 4));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, p->stream, u0, u1, p->d_row_ptr, p->d_col, p->d_lat,
                       with_loss ? p->d_loss : (const float *)nullptr, p->kp.g, 1.0 / (double)p->kp.g, wns, cls, q, vb,
                       offsets, p->d_tccnt, entries, cap, p->d_tcursor, (unsigned long long *)p->d_tmaxw,
                       l16 ? p->d_lat16 : (const uint16_t *)nullptr, ce4 ? p->d_lvisit + 1 : (unsigned long long *)nullptr);
}

// The class CSRs of the graph's edges of latency <= wmax units (self-loops
// dropped), classes = exact weights 1..wmax <= WC: out-rows straight from the
// adjacency (lvl_out_kernel), in-rows by a scan of their counts and one walk
// of the out-rows (lvl_in_kernel).  The entry arrays hold p->lvl_cap entries:
// the first call (the create-time probe, wmax = min(31, max edge)) counts,
// sizes them and runs again; every later call prunes at the probe's bound <=
// that wmax, so its count fits and nothing waits for the host.
// ce4: a symmetric plan's out-rows as 4-byte entries (the packed row's run; the
// overflow word p->d_lvisit[1] is zeroed with the cursor) -- p->lvl_ce4_run says
// whether this build wrote them.
srt_status level_csr(srt_plan *p, uint64_t wmax, bool with_loss, srt_err *err, bool ce4 = false) {
    hipStream_t M = p->stream;
    const uint32_t V = p->V;
    const uint32_t q = p->lvl_q;
    const uint64_t ncls = q ? wmax / q : wmax;
    const uint32_t cls = ncls < 16 ? 16 : ncls < 32 ? 32 : 64;
    const uint64_t vc1 = (uint64_t)V * cls + 1;
    srt_status st = level_csr_arrays(p, vc1, err);
    if (st != SRT_OK) return st;
    if (!p->h_tcount) {
        const hipError_t e = hipHostMalloc((void **)&p->h_tcount, 4 * sizeof(uint64_t), 0);
        if (e != hipSuccess) return fail(err, e, "hipHostMalloc");
    }
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(8192, (V + 3) / 4));
    const uint64_t wns = wmax * p->kp.g;
    // symmetric plans (lvl_sym_tile_kernel: identity rows, mirrored pairs --
    // their losses too when the entries carry them): out-rows only
    const bool single = with_loss ? p->lvl_sym : p->lvl_sym_lat;
    p->lvl_single = single;
    const bool use4 = ce4 && single && with_loss && !q && p->d_lvisit;
    p->lvl_ce4_run = use4;
    const uint32_t vb = q ? p->lvl_vb : use4 ? level_vbits(V) : 32u;
    // a kept class structure (level_keep): the lists and their offsets stand since
    // creation, this run's losses are filled into them -- one launch, no pass over
    // the adjacency, no cursor, no offsets copy.  (4-byte entries: the caller has
    // zeroed the overflow word, level_run)
    p->lvl_keep_run = false;
    if (with_loss && wmax == p->kp.lmax && level_keep_applies(p) && p->lvl_kstride == cls) {
        cspan_begin(p);
        hipLaunchKernelGGL(use4 ? lvl_fill_kernel<true> : lvl_fill_kernel<false>, dim3(blocks), dim3(256), 0, M, V, cls, vb,
                           p->d_row_ptr, p->d_loss, p->d_kcls, p->d_kcol, p->d_tpk,
                           use4 ? p->d_lvisit + 1 : (unsigned long long *)nullptr);
        cspan_end(p);
        p->lvl_keep_run = true;
        p->t_cls = cls;
        p->t_q = 1;
        p->t_level = true;
        p->t_edges = p->lvl_cap;  // (as the adjacency pass reports it: the probe's count)
        return SRT_OK;
    }
    auto out_pass = [&]() {
        if (!single)  // in-row counts, then in-row cursors (out-rows-only plans count none)
            (void)hipMemsetAsync(p->d_tccnt, 0, 2 * vc1 * 4, M);
        hipLaunchKernelGGL(level_zero_kernel, dim3(1), dim3(1), 0, M, (unsigned long long *)nullptr,
                           (unsigned long long *)p->d_tcursor, (unsigned long long *)p->d_tmaxw,
                           use4 ? p->d_lvisit + 1 : (unsigned long long *)nullptr);
        // symmetric plans have identity rows (lvl_sym_tile_kernel); theirs may read
        // the u16-unit copy (the symmetry check's; wmax < 0xffff units)
        launch_lvl_out(p, with_loss, single, single && p->d_lat16, 0u, V, wns, cls, q, vb, p->d_tcls, p->d_tpk, p->lvl_cap,
                       use4);
    };
    // first call (the create-time probe): entry arrays of the caller's
    // estimate (p->lvl_est; +1024: the solve's 2-entry loads read up to UNR *
    // LPT * 2 entries past a class's end), one pass, the count read back; an
    // estimate too small (or none) sizes them by the count and runs again.
    // lvl_cap = the count: every later call prunes at a bound <= this wmax
    auto size_arrays = [&](uint64_t entries) -> srt_status {
        uint64_t ca = 0, cb = 0;
        (void)hipFree(p->d_tpk);
        (void)hipFree(p->d_tpk2);
        p->d_tpk = p->d_tpk2 = nullptr;
        p->t_cap = 0;
        srt_status s2;
        // symmetric plans read the in-rows through the out-rows: no second array
        // (allocated below when a later run needs in-rows after all)
        if ((s2 = grow(&p->d_tpk, &ca, entries + 1024, err, "hipMalloc(level out-rows)")) != SRT_OK ||
            (!single && (s2 = grow(&p->d_tpk2, &cb, entries + 1024, err, "hipMalloc(level in-rows)")) != SRT_OK))
            return s2;
        p->lvl_cap = entries;
        return SRT_OK;
    };
    const bool first = !p->lvl_cap;
    if (first && p->lvl_est && (st = size_arrays(p->lvl_est)) != SRT_OK) return st;
    cspan_begin(p);
    out_pass();
    cspan_end(p);
    if (first) {
        hipError_t e = hipMemcpyAsync(p->h_tcount, p->d_tcursor, sizeof(uint64_t), hipMemcpyDeviceToHost, M);
        if (e == hipSuccess) e = hipStreamSynchronize(M);
        if (e != hipSuccess) return fail(err, e, "level edge count");
        const uint64_t count = std::max<uint64_t>(p->h_tcount[0], 1);
        if (count > p->lvl_cap) {
            if ((st = size_arrays(count)) != SRT_OK) return st;
            cspan_begin(p);
            out_pass();
            cspan_end(p);
        }
        p->lvl_cap = count;
    }
    if (single) {
        // symmetric plan (lvl_sym_tile_kernel): the in-rows are the out-rows;
        // their offsets copied, the entries read through the same array
        // (level_ctx)
        cspan_begin(p);
        const hipError_t e = hipMemcpyAsync(p->d_tcls + vc1, p->d_tcls, vc1 * 4, hipMemcpyDeviceToDevice, M);
        cspan_end(p);
        if (e != hipSuccess) return fail(err, e, "class offsets (symmetric)");
    } else {
        if (!p->d_tpk2) {  // a symmetric plan whose run needs in-rows (its losses did not mirror)
            uint64_t cb = 0;
            if ((st = grow(&p->d_tpk2, &cb, p->lvl_cap + 1024, err, "hipMalloc(level in-rows)")) != SRT_OK) return st;
        }
        if ((st = scan_scratch(p, (size_t)vc1, err)) != SRT_OK) return st;  // allocated outside the timed span
        cspan_begin(p);
        if ((st = exclusive_scan_u32(p, p->d_tccnt, p->d_tcls + vc1, (size_t)vc1, err)) != SRT_OK) return st;
        const uint64_t vmask = q ? (1ull << vb) - 1ull : 0xffffffffull;
        hipLaunchKernelGGL(lvl_in_kernel, dim3(blocks), dim3(256), 0, M, V, cls, vmask, p->d_tcls, p->d_tpk,
                           p->d_tcls + vc1, p->d_tccnt + vc1, p->d_tpk2);
        cspan_end(p);
    }
    p->t_cls = cls;
    p->t_q = 1;
    p->t_level = true;
    p->t_edges = p->lvl_cap;  // the probe's count (an upper bound at the run's smaller wmax)
    return SRT_OK;
}

__global__ void set_u64_kernel(unsigned long long *p, unsigned long long v) { *p = v; }

// The class CSR of a symmetric level plan (identity rows, mirrored pairs:
// out-rows only) built sharded over W ranks: the fixed per-graph work of a
// row-sharded build, which every rank paid whole before (C3: 0.63 ms of an
// 8-rank share of ~1.4 ms).  Rank r builds the out-rows of vertices [r vr,
// (r + 1) vr) into entry slot r (entries [r C, (r + 1) C), its cursor starting
// at r C, so the class offsets it writes are absolute) and its offsets into
// offset slot r; one all-gather of each (in place, C entries and vr * cls
// offsets a rank -- C3, 8 ranks: ~5 MB + 128 KB a rank) and every rank holds
// the whole class CSR.  C = the largest slice's entry count, measured once (a
// counting pass per slice and an all-gather of the counts) at the first run.
// comm == nullptr: the measurement form (srt_plan_shard_rows with
// SRT_LVL_SHARD_EMU=1, one GPU): the first run builds every slice, later runs
// rebuild the own slice only and wait out a modelled all-gather
// (SRT_FW_EMU_AG_US + received bytes / SRT_FW_EMU_AG_GBPS, as the FW emulation).
srt_status level_csr_sharded(srt_plan *p, uint64_t wmax, bool with_loss, uint32_t W, uint32_t r, srt_comm *comm,
                             srt_err *err) {
    hipStream_t M = p->stream;
    const uint32_t V = p->V, vr = (V + W - 1) / W;
    const uint32_t cls = wmax < 16 ? 16 : wmax < 32 ? 32 : 64;
    const uint64_t vc1 = (uint64_t)V * cls + 1;
    uint64_t cap_cnt = p->d_lvl_counts ? W : 0;
    srt_status st = level_csr_arrays(p, vc1, err);
    if (st != SRT_OK ||
        (st = grow(&p->d_lvl_offstage, &p->lvl_offstage_cap, (uint64_t)W * vr * cls, err,
                   "hipMalloc(class offset slots)")) != SRT_OK ||
        (st = grow(&p->d_lvl_counts, &cap_cnt, W, err, "hipMalloc(slice counts)")) != SRT_OK)
        return st;
    const uint64_t wns = wmax * p->kp.g;
    auto slice = [&](uint32_t s, uint64_t base, uint64_t cap, uint64_t *entries) {
        hipLaunchKernelGGL(set_u64_kernel, dim3(1), dim3(1), 0, M, p->d_tcursor, (unsigned long long)base);
        launch_lvl_out(p, with_loss, true, false, std::min(V, s * vr), std::min(V, (s + 1) * vr), wns, cls, 0u, 32u,
                       p->d_lvl_offstage, entries, cap);
    };
    const bool emu = comm == nullptr;
    if (!p->lvl_seg_cap) {
        // sizing: every slice counted (cap 0: nothing written); the measured
        // form counts all W here, a rank its own and all-gathers the counts
        std::vector<unsigned long long> cnt(W, 0);
        for (uint32_t s = 0; s < W; ++s) {
            if (!emu && s != r) continue;
            slice(s, 0, 0, p->d_tpk);
            const hipError_t e = hipMemcpyAsync(p->d_lvl_counts + s, p->d_tcursor, 8, hipMemcpyDeviceToDevice, M);
            if (e != hipSuccess) return fail(err, e, "slice count");
        }
        if (!emu && (st = comm_allgather_inplace(comm, p->d_lvl_counts, 8, M, err)) != SRT_OK) return st;
        hipError_t e = hipMemcpyAsync(cnt.data(), p->d_lvl_counts, 8ull * W, hipMemcpyDeviceToHost, M);
        if (e == hipSuccess) e = hipStreamSynchronize(M);
        if (e != hipSuccess) return fail(err, e, "slice counts");
        uint64_t C = 1;
        for (uint32_t s = 0; s < W; ++s) C = std::max<uint64_t>(C, cnt[s]);
        (void)hipFree(p->d_tpk);
        (void)hipFree(p->d_tpk2);
        p->d_tpk = p->d_tpk2 = nullptr;
        uint64_t ca = 0;
        if ((st = grow(&p->d_tpk, &ca, C * W + 1024, err, "hipMalloc(level out-rows)")) != SRT_OK) return st;
        p->lvl_seg_cap = C;
        p->lvl_cap = C * W;
        p->lvl_emu_built = false;
    }
    const uint64_t C = p->lvl_seg_cap;
    cspan_begin(p);
    if (emu && !p->lvl_emu_built) {  // the measured form's first run: every rank's slice
        for (uint32_t s = 0; s < W; ++s) slice(s, s * C, (s + 1) * C, p->d_tpk);
        p->lvl_emu_built = true;
    } else {
        slice(r, (uint64_t)r * C, (uint64_t)(r + 1) * C, p->d_tpk);
        if (emu) {
            emu_allgather(p->device, W, (double)C * 8 + (double)vr * cls * 4, M);
        } else if ((st = comm_allgather_inplace(comm, p->d_tpk, C * 8, M, err)) != SRT_OK ||
                   (st = comm_allgather_inplace(comm, p->d_lvl_offstage, (uint64_t)vr * cls * 4, M, err)) != SRT_OK) {
            return st;
        }
    }
    // the offsets, out-rows and (symmetric) in-rows alike
    hipError_t e = hipMemcpyAsync(p->d_tcls, p->d_lvl_offstage, (uint64_t)V * cls * 4, hipMemcpyDeviceToDevice, M);
    if (e == hipSuccess)
        e = hipMemcpyAsync(p->d_tcls + vc1, p->d_lvl_offstage, (uint64_t)V * cls * 4, hipMemcpyDeviceToDevice, M);
    cspan_end(p);
    if (e != hipSuccess) return fail(err, e, "class offsets (sharded)");
    p->lvl_single = true;
    p->lvl_keep_run = false;
    p->lvl_ce4_run = false;  // the slice exchange moves 8-byte entries
    p->t_cls = cls;
    p->t_q = 1;
    p->t_level = true;
    p->t_edges = C * W;
    return SRT_OK;
}

// the packed row's instantiation (16 class offsets, the pipelined walk)
auto pick_packed_kernel(bool nt_store) {
    return nt_store ? level_solve_kernel<4, 4, 16, 2, true, true, true> : level_solve_kernel<4, 4, 16, 2, false, true, true>;
}
// ... on 4-byte class entries
// (threads: PACK_NT, or one of CE4_WIDE_NT with the chunk walk at two entry pairs a lane)
auto pick_ce4_kernel(bool nt_store, uint32_t threads = PACK_NT) {
    static_assert(CE4_WIDE_NT[0] == 640 && CE4_WIDE_NT[1] == 768, "the instantiations below");
    return threads == 768   ? (nt_store ? level_ce4_wide_kernel<true, 768, 2> : level_ce4_wide_kernel<false, 768, 2>)
           : threads == 640 ? (nt_store ? level_ce4_wide_kernel<true, 640, 2> : level_ce4_wide_kernel<false, 640, 2>)
                            : (nt_store ? level_ce4_kernel<true> : level_ce4_kernel<false>);
}

// Workgroups of a level solve launch over `rows` rows (one row per
// workgroup at a time; the LDS row decides how many fit a CU)
uint32_t level_grid(int device, uint32_t V, bool quant, uint32_t rows, uint32_t *nt_out, uint32_t pack,
                    uint32_t pack_nt = PACK_NT) {
    // the packed row: PACK_NT threads a workgroup (pack_nt: the 4-byte-entry
    // kernel's own count), `pack` workgroups a CU (what the runtime said of the
    // kernel's registers and this LDS row at the create)
    if (pack) {
        if (nt_out) *nt_out = pack_nt;
        return std::max<uint32_t>(1, std::min<uint32_t>(rows, (uint32_t)cu_count(device) * pack));
    }
    // workgroups a CU's LDS holds, then the fewest threads a workgroup (256,
    // 512 or 1024) that still fill the CU's 2,048 thread slots: more rows in
    // flight a CU for small graphs (C2, 4k: 4 x 512 threads 0.39 ms a solve
    // against 2 x 1024 0.50 ms; 4 x 256 0.39), one 1,024-thread workgroup for
    // C3's 128 KB rows
    const int lds_cu = std::max(1, level_rows_per_cu(V, quant, false));
    uint32_t nt = 256;
    while (nt < LOSS_NT && (int)(2048 / nt) > lds_cu) nt *= 2;
    const int per_cu = std::max(1, std::min(2048 / (int)nt, lds_cu));
    if (nt_out) *nt_out = nt;
    return std::max<uint32_t>(1, std::min<uint32_t>(rows, (uint32_t)(cu_count(device) * per_cu)));
}

// The instantiation for a class table of t_cls offsets a vertex: 4 lanes an
// item, 4 entry pairs in flight a lane with 16 classes, 2 with 32 or 64.
// nt_store: table rows by non-temporal stores (knob SRT_LVL_NT=0: plain, A/B).
// sp: the pipelined walk (knob SRT_LVL_SP=0: the per-item walk, A/B).  Measured
// at C3 (same box): branch-free hits through a per-lane dummy word 4.83 ms, the
// same as the pipelined walk; lane groups x pairs in flight 4x4 (kept) 4.79,
// 2x4 5.22, 8x2 5.50, 4x2 5.57, 2x2 6.09 ms
template <bool NT, bool SP>
auto solve_kernel_for(uint32_t t_cls) {
    return t_cls == 16   ? level_solve_kernel<4, 4, 16, 2, NT, SP>
           : t_cls == 32 ? level_solve_kernel<4, 2, 32, 2, NT, SP>
                         : level_solve_kernel<4, 2, 64, 2, NT, SP>;
}
auto pick_solve_kernel(uint32_t t_cls, bool nt_store, bool sp) {
    return sp ? (nt_store ? solve_kernel_for<true, true>(t_cls) : solve_kernel_for<false, true>(t_cls))
              : (nt_store ? solve_kernel_for<true, false>(t_cls) : solve_kernel_for<false, false>(t_cls));
}
template <bool NT>
auto q_kernel_for(uint32_t t_cls) {
    return t_cls == 16   ? level_q_kernel<4, 4, 16, 2, NT>
           : t_cls == 32 ? level_q_kernel<4, 2, 32, 2, NT>
                         : level_q_kernel<4, 2, 64, 2, NT>;
}
auto pick_q_kernel(uint32_t t_cls, bool nt_store) {
    return nt_store ? q_kernel_for<true>(t_cls) : q_kernel_for<false>(t_cls);
}

// level_solve_kernel (or level_q_kernel, c.q > 0) over rows [r0, r1) (or the
// row list) of the context c (probe: no table, reverse = in- and out-CSRs
// swapped: distances TO the row's node); lcap = the bound B in units.
// stage_mode 0: the table; 1: u16 latency units + f32 loss staging, row k of
// the job at k * n; 2: u32 units + loss; 3: 8-byte records (quantized only)
void launch_solve_ctx(const LevelCtx &c, unsigned long long *d_stats, const uint32_t *list, uint32_t r0, uint32_t r1,
                      uint32_t lcap, bool reverse, uint32_t *probe, void *stage, float *stage_loss,
                      uint32_t stage_mode) {
    const uint32_t V = c.V, rows = list ? r1 : r1 - r0;
    if (!rows) return;
    const bool quant = c.q != 0;
    // the packed row: table and staged rows of a plan that chose it (the probe
    // rows' caps are past its 4-bit levels)
    const uint32_t pack = !quant && !probe && c.sp && c.t_cls == 16 && lcap <= PACK_LMAX && c.lmem ? c.pack : 0u;
    uint32_t nt = 0;
    const uint32_t ce4_nt = pack && c.ce4 && c.ce4_nt ? c.ce4_nt : PACK_NT;  // (the overflow repeat, 8-byte entries: PACK_NT)
    const uint32_t grid = level_grid(c.device, V, quant, rows, &nt, pack, ce4_nt);
    const size_t lds = solve_lds_bytes(V, quant, pack != 0);
    const uint64_t vc1 = (uint64_t)V * c.t_cls + 1;
    const uint32_t *co = c.tcls, *ci = c.tcls + vc1;
    const uint64_t *eo = c.ce_out, *ei = c.ce_in;
    if (reverse) {
        std::swap(co, ci);
        std::swap(eo, ei);
    }
    if (quant) {
        const auto kern = pick_q_kernel(c.t_cls, c.nt_store);
        (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(LDS_BUDGET - 4096));
        const uint32_t kcap = std::min<uint32_t>(lcap / c.q, LWC);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), lds, c.stream, V, c.nodes, c.n, list ? 0u : r0, r1, co, ci,
                           eo, ei, kcap, lcap, c.q, c.rb, c.vb, c.g, c.sl_lat, c.sl_loss, c.out_lat, c.out_loss, d_stats,
                           list, stage, stage_loss, stage_mode, probe, c.visits, c.lmem);
        return;
    }
    if (pack && c.ce4) {  // (4-byte entries are written only for a run on the packed row: level_run)
        const auto k4 = pick_ce4_kernel(c.nt_store, nt);
        (void)hipFuncSetAttribute((const void *)k4, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_BUDGET - 4096));
        hipLaunchKernelGGL(k4, dim3(grid), dim3(nt), lds, c.stream, V, c.nodes, c.n, list ? 0u : r0, r1, co, ci, eo, ei, lcap,
                           c.g, c.sl_lat, c.sl_loss, c.out_lat, c.out_loss, d_stats, list, stage_mode ? stage : nullptr,
                           stage_mode ? stage_loss : nullptr, stage_mode == 1, probe, c.visits, c.idn, c.row_ctr, c.lmem,
                           c.spread, c.lean, level_vbits(V));
        return;
    }
    const auto kern = pack ? pick_packed_kernel(c.nt_store) : pick_solve_kernel(c.t_cls, c.nt_store, c.sp);
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_BUDGET - 4096));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), lds, c.stream, V, c.nodes, c.n, list ? 0u : r0, r1, co, ci, eo, ei,
                       lcap, c.g, c.sl_lat, c.sl_loss, c.out_lat, c.out_loss, d_stats, list,
                       stage_mode ? stage : nullptr, stage_mode ? stage_loss : nullptr, stage_mode == 1, probe,
                       c.visits, c.idn, c.row_ctr, pack ? c.lmem : (uint16_t *)nullptr, c.spread, c.lean);
}

// the per-workgroup scratch of the quantized solve and of the packed row
// (p->d_lmem): every workgroup a launch may have, V u16 each
srt_status level_scratch(srt_plan *p, srt_err *err) {
    if (!p->lvl_q && !p->lvl_pack) return SRT_OK;
    return grow(&p->d_lmem, &p->lmem_cap, level_scratch_bytes(p->device, p->V, p->lvl_q != 0, p->lvl_pack) / 2, err,
                "hipMalloc(level scratch)");
}

srt_status launch_solve(srt_plan *p, unsigned long long *d_stats, const RowJob &job, uint32_t lcap, bool reverse,
                        uint32_t *probe, srt_err *err) {
    srt_status st = level_scratch(p, err);
    if (st != SRT_OK) return st;
    const uint32_t r0 = job.list ? 0u : job.range ? job.r0 : p->row0;
    const uint32_t r1 = job.list ? job.count : job.range ? job.r1 : p->row1;
    launch_solve_ctx(level_ctx(p), d_stats, job.list, r0, r1, lcap, reverse, probe, job.out32_loss ? job.out32 : nullptr,
                     job.out32_loss, job.out32_loss ? (p->stage16 ? 1u : 2u) : 0u);
    return SRT_OK;
}

}  // namespace

// Create-time proof for the level solve: the pruned graph's (edges <= wmax
// units) distances from and to K <= 8 in-use nodes s, spread over the node
// list, by probe rows.  Every in-use u, v has d(u, v) <= d(u, s) + d(s, v) <=
// in-ecc(s) + out-ecc(s) for each s (pruned distances bound the real ones from
// above), so *bound = the smallest such sum; ~0 when every s misses an in-use
// node within wmax levels one way or the other.  *visits: the edges a
// forward probe row walked on average (the AUTO price).  p->lvl_q > 0: the
// quantized solve's buckets of q units; the bound must keep every class and
// bucket <= 31 (B < 32 q).
srt_status level_probe(srt_plan *p, uint64_t wmax, uint32_t wc, uint64_t *bound, uint64_t *visits, srt_err *err) {
    *bound = ~0ull;
    *visits = 0;
    if (!p->n) return SRT_OK;
    p->lvl_cap = 0;  // a new bound: count and size the entry arrays again
    // the estimate: latencies spread evenly up to the longest edge, twice over
    {
        const uint64_t maxu = p->lvl_maxu ? p->lvl_maxu : wmax;
        const double f = std::min(1.0, 2.0 * (double)wmax / (double)std::max<uint64_t>(maxu, 1));
        p->lvl_est = (uint64_t)((double)p->n_adj * f) + 65536;
    }
    srt_status st = level_csr(p, wmax, false, err);
    if (st != SRT_OK) return st;
    const uint32_t K = std::min<uint32_t>(8, p->n);
    uint32_t rows[8];
    for (uint32_t k = 0; k < K; ++k) rows[k] = (uint32_t)((uint64_t)k * p->n / K);
    uint32_t *d_pr = nullptr;
    hipError_t e = hipMalloc(&d_pr, 48 * sizeof(uint32_t));  // fwd [0, 16), rev [16, 32), rows [32, 40)
    if (e != hipSuccess) return fail(err, e, "hipMalloc(level probe)");
    uint32_t h[32] = {};
    (void)hipMemsetAsync(d_pr, 0, 32 * sizeof(uint32_t), p->stream);
    e = hipMemcpyAsync(d_pr + 32, rows, K * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream);
    RowJob job;
    job.list = d_pr + 32;
    job.count = K;
    const uint64_t LQ = (uint64_t)(wc + 1) * (p->lvl_q ? p->lvl_q : 1) - 1;  // the largest bound the solve takes
    // distances up to LQ (not only up to wmax: a path of short edges may be
    // longer than the longest edge)
    const uint32_t cap = (uint32_t)LQ;
    if (e == hipSuccess) {
        cspan_begin(p);
        st = launch_solve(p, nullptr, job, cap, false, d_pr, err);
        if (st == SRT_OK) st = launch_solve(p, nullptr, job, cap, true, d_pr + 16, err);
        cspan_end(p);
        if (st != SRT_OK) {
            (void)hipStreamSynchronize(p->stream);
            (void)hipFree(d_pr);
            return st;
        }
        e = hipMemcpyAsync(h, d_pr, sizeof h, hipMemcpyDeviceToHost, p->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    (void)hipFree(d_pr);
    if (e != hipSuccess) return fail(err, e, "level probe");
    uint64_t vis = 0;
    std::memcpy(&vis, h, 8);
    *visits = vis / K;
    for (uint32_t k = 0; k < K; ++k)
        if (h[2 + k] <= cap && h[18 + k] <= cap && (uint64_t)h[2 + k] + h[18 + k] <= LQ)  // classes <= wc
            *bound = std::min<uint64_t>(*bound, (uint64_t)h[2 + k] + h[18 + k]);
    if (std::getenv("SRT_TRACE"))
        std::fprintf(stderr,
                     "[srt] level probe: %llu edges <= %llu units, q %u, %u rows, bound %lld, %llu visits a row\n",
                     (unsigned long long)p->t_edges, (unsigned long long)wmax, p->lvl_q, K,
                     *bound == ~0ull ? -1ll : (long long)*bound, (unsigned long long)*visits);
    return SRT_OK;
}

// The level solve's build (SRT_ALGO_LEVEL): the class CSRs of the edges <=
// kp.lmax units (the probe's bound), then the rows -- in chunks of
// fold_chunk_rows when the one-call build downloads behind them (ev_fold), as
// fw_loss's fold.  A sharded plan solves its own rows [row0, row1).
namespace {
// Sharded level solve (comm bound): this rank's rows (d_lrows, by
// build_loss_rows) solved in tail_q chunks into the staging as u16 latency
// units + f32 loss (6 B a pair, half the table's 12), chunk c's rows
// all-gathered on the comm stream behind chunk c + 1's solve and expanded into
// every rank's table behind its all-gather -- the sharded FW tail's pipeline
// with the solve in place of the fold.
srt_status level_sharded(srt_plan *p, unsigned long long *d_stats, srt_err *err) {
    const uint32_t W = (uint32_t)p->comm->nranks, r = (uint32_t)p->comm->rank;
    p->stage16 = p->lvl_q == 0;  // quantized: u32 units
    p->stage_loss_only = false;
    const uint32_t q = p->tail_q, cr = p->tail_cr, lcap = (uint32_t)p->kp.lmax;
    const size_t cbytes = (size_t)cr * p->n * 4, lbytes = (size_t)cr * p->n * (p->stage16 ? 2 : 4);
    hipStream_t M = p->stream, C = p->comm_stream;
    srt_status st;
    if ((st = ensure_row_staging(p, W, err)) != SRT_OK ||
        (st = ensure_events(p->ev, 2 * (size_t)q, (unsigned)hipEventDisableSystemFence, err)) != SRT_OK)
        return st;
    for (uint32_t c = 0; c < q; ++c) {
        const size_t slot = ((size_t)c * W + r) * cr;
        RowJob job;
        job.list = p->d_lrows + slot;
        job.count = p->lrow_cnt[r] > c * cr ? std::min(cr, p->lrow_cnt[r] - c * cr) : 0u;
        job.out32 = reinterpret_cast<uint8_t *>(p->d_slat) + slot * p->n * (p->stage16 ? 2 : 4);
        job.out32_loss = p->d_sloss + slot * p->n;
        (void)hipEventRecord(p->ev[2 * c], M);
        if ((st = launch_solve(p, d_stats, job, lcap, false, nullptr, err)) != SRT_OK) return st;
        (void)hipEventRecord(p->ev[2 * c + 1], M);
        p->p3_launches++;
        p->p3_work += (double)job.count * p->n;
        (void)hipEventRecord(p->ev_tail[c], M);
        (void)hipStreamWaitEvent(C, p->ev_tail[c], 0);
        const size_t base = (size_t)c * W * cr * p->n;
        if ((st = comm_allgather_inplace(p->comm,
                                         reinterpret_cast<uint8_t *>(p->d_slat) + base * (p->stage16 ? 2 : 4), lbytes, C,
                                         err)) != SRT_OK ||
            (st = comm_allgather_inplace(p->comm, p->d_sloss + base, cbytes, C, err)) != SRT_OK)
            return st;
        (void)hipEventRecord(p->ev_tail[q + c], C);
    }
    expand_chunks_behind(p, W);
    p->shard_tail = true;
    return SRT_OK;
}
}  // namespace

srt_status level_prepare(srt_plan *p, srt_err *err) { return level_csr(p, p->kp.lmax, true, err); }

srt_status level_keep(srt_plan *p, srt_err *err) {
    static_assert(LEVEL_V_MAX <= 65536, "kept heads are u16");
    p->lvl_kept = 0;
    p->lvl_keep_run = false;
    const uint32_t V = p->V;
    const uint64_t B = p->kp.lmax;
    // out-rows only (identity rows, mirrored latencies), exact classes, heads that fit u16,
    // and the probe's class rows at hand (out-rows only as well: its last build was loss-free)
    if (!p->lvl_sym_lat || !p->ident_rows || p->lvl_q || V > 65536 || !p->lvl_cap || !p->lvl_single || !p->d_tcls ||
        !p->d_tpk || !p->d_tccnt)
        return SRT_OK;
    const uint32_t pcls = p->t_cls;                            // the probe's offsets a vertex
    const uint32_t rcls = B < 16 ? 16 : B < 32 ? 32 : 64;      // the run's (level_csr)
    if (B < 1 || B >= pcls || p->tcls_cap < 2ull * V + 2) return SRT_OK;
    hipStream_t M = p->stream;
    const uint64_t vc1 = (uint64_t)V * rcls + 1;
    uint32_t *cnt = p->d_tccnt, *base = p->d_tccnt + V + 1;  // (the in-row counts: out-rows-only plans count none)
    srt_status st = scan_scratch(p, (size_t)V + 1, err);
    if (st != SRT_OK) return st;
    cspan_begin(p);
    hipLaunchKernelGGL(lvl_keep_count_kernel, dim3((V + 256) / 256), dim3(256), 0, M, V, pcls, (uint32_t)B, p->d_tcls, cnt);
    st = exclusive_scan_u32(p, cnt, base, (size_t)V + 1, err);
    cspan_end(p);
    if (st != SRT_OK) return st;
    uint32_t total = 0;
    hipError_t e = hipMemcpyAsync(&total, base + V, 4, hipMemcpyDeviceToHost, M);
    if (e == hipSuccess) e = hipStreamSynchronize(M);
    if (e != hipSuccess) return fail(err, e, "level keep (count)");
    if (!total || total > p->lvl_cap) return SRT_OK;
    (void)hipFree(p->d_kcls);
    (void)hipFree(p->d_kcol);
    p->d_kcls = nullptr;
    p->d_kcol = nullptr;
    uint64_t ca = 0, cb = 0;
    if ((st = grow(&p->d_kcls, &ca, 2 * vc1, err, "hipMalloc(kept class offsets)")) != SRT_OK ||
        (st = grow(&p->d_kcol, &cb, (uint64_t)total + 1024, err, "hipMalloc(kept columns)")) != SRT_OK)
        return st;
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(8192, (V + 3) / 4));
    cspan_begin(p);
    hipLaunchKernelGGL(lvl_keep_kernel, dim3(blocks), dim3(256), 0, M, V, pcls, rcls, (uint32_t)B, p->d_tcls, p->d_tpk, base,
                       p->d_kcls, p->d_kcol);
    cspan_end(p);
    if ((e = hipGetLastError()) != hipSuccess) return fail(err, e, "level keep");
    p->lvl_kept = total;
    p->lvl_kstride = rcls;
    p->lvl_kbound = B;
    if (std::getenv("SRT_TRACE"))
        std::fprintf(stderr, "[srt] level keep: %llu of %llu entries, classes <= %llu\n", (unsigned long long)total,
                     (unsigned long long)p->lvl_cap, (unsigned long long)B);
    return SRT_OK;
}

void level_solve_stage(const LevelCtx &c, uint32_t r0, uint32_t r1, uint32_t lmax, void *stage_lat,
                       float *stage_loss, uint32_t stage_mode, unsigned long long *d_stats) {
    launch_solve_ctx(c, d_stats, nullptr, r0, r1, lmax, false, nullptr, stage_lat, stage_loss, stage_mode);
}

size_t level_scratch_bytes(int device, uint32_t V, bool quant, uint32_t pack) {
    return quant || pack ? (size_t)level_grid(device, V, quant, ~0u, nullptr, quant ? 0u : pack) * V * 2 : 0;
}

int level_pack_fit(uint32_t V, bool nt_store, bool ce4, uint32_t threads) {
    if (!threads || !ce4) threads = PACK_NT;
    const void *kern = ce4 ? (const void *)pick_ce4_kernel(nt_store, threads) : (const void *)pick_packed_kernel(nt_store);
    int wgs = 0;
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_BUDGET - 4096)) !=
            hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, kern, (int)threads, solve_lds_bytes(V, false, true)) !=
            hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return wgs;
}

bool level_ce4_threads_valid(uint32_t threads) {
    return threads == PACK_NT || threads == CE4_WIDE_NT[0] || threads == CE4_WIDE_NT[1];
}

uint32_t level_ce4_threads(uint32_t V, bool nt_store, uint32_t forced) {
    const int fit512 = level_pack_fit(V, nt_store, true, PACK_NT);
    if (fit512 < 2) return 0;
    const int fit640 = level_pack_fit(V, nt_store, true, CE4_WIDE_NT[0]), fit768 = level_pack_fit(V, nt_store, true, CE4_WIDE_NT[1]);
    const uint32_t widest = fit768 >= 2 ? CE4_WIDE_NT[1] : fit640 >= 2 ? CE4_WIDE_NT[0] : PACK_NT;
    const uint32_t threads = forced ? forced : widest;
    if (std::getenv("SRT_TRACE"))
        std::fprintf(stderr, "[srt] level ce4: %u threads a workgroup%s (workgroups a CU: 768 x%d, 640 x%d, 512 x%d)\n", threads,
                     forced ? " (forced)" : "", fit768, fit640, fit512);
    return threads;
}

void level_loss_index(srt_plan *p, uint32_t *d_idx, uint64_t cap, unsigned long long *d_cnt, hipStream_t s) {
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(8192, (p->V + 3) / 4));
    if (p->lvl_kept && !p->lvl_q && p->lvl_kbound == p->kp.lmax && p->lvl_kept <= cap) {  // the kept structure lists them
        hipLaunchKernelGGL(lvl_keep_index_kernel, dim3(blocks), dim3(256), 0, s, p->V, p->lvl_kstride, p->d_row_ptr,
                           p->d_kcls, p->d_kcol, d_idx, (unsigned long long)p->lvl_kept, d_cnt);
        return;
    }
    (void)hipMemsetAsync(d_cnt, 0, sizeof *d_cnt, s);
    // identity rows: the column is the entry's place in its row (no column loads)
    hipLaunchKernelGGL(p->ident_rows ? lvl_index_kernel<true> : lvl_index_kernel<false>, dim3(blocks), dim3(256), 0, s,
                       p->V, p->d_row_ptr, p->d_col, p->d_lat, p->kp.lmax * p->kp.g, d_idx, cap, d_cnt);
}

void loss_scatter(const uint32_t *d_idx, const float *d_val, uint64_t count, float *d_loss, hipStream_t s) {
    if (count)
        hipLaunchKernelGGL(loss_scatter_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (count + 255) / 256)),
                           dim3(256), 0, s, d_idx, d_val, count, d_loss);
}

void loss_mirror_check(const uint32_t *d_idx, uint64_t count, uint64_t V, const float *d_loss, uint32_t *d_ok,
                       hipStream_t s) {
    if (count)
        hipLaunchKernelGGL(loss_mirror_check_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (count + 255) / 256)),
                           dim3(256), 0, s, d_idx, count, V, d_loss, d_ok);
}

srt_status level_sym_check(srt_plan *p, uint64_t wmax_units, bool with_loss, bool *sym, srt_err *err) {
    *sym = false;
    if (!p->V || p->n_adj != (uint64_t)p->V * p->V || !p->ident_rows) return SRT_OK;
    uint32_t *d_ok = nullptr;
    hipError_t e = hipMalloc(&d_ok, 4);
    if (e != hipSuccess) return fail(err, e, "hipMalloc(symmetry flag)");
    uint32_t one = 1;
    e = hipMemcpyAsync(d_ok, &one, 4, hipMemcpyHostToDevice, p->stream);
    const uint64_t nb = (p->V + 63) / 64;
    // every latency below 0xffff units and rows of a multiple of 4 entries: the
    // check also writes the adjacency's u16-unit copy, which the class-CSR
    // passes stream instead of the u64 latencies (a quarter of the bytes; C3
    // 16k: out-rows 538 -> 309 us a build, the check 542 -> 854 us once).  From
    // 8,192 vertices: at C2's 4k it measured 0.01-0.02 ms slower a build
    const char *k16 = std::getenv("SRT_LAT16");  // knob: 0 = never, 1 = at any size (A/B, tests)
    const int kv16 = k16 ? std::atoi(k16) : -1;
    const bool want16 = wmax_units < 0xffff && p->V % 4 == 0 && kv16 != 0 && (kv16 == 1 || p->V >= 8192);
    (void)hipFree(p->d_lat16);
    p->d_lat16 = nullptr;
    if (e == hipSuccess && want16 && hipMalloc(&p->d_lat16, p->n_adj * 2) != hipSuccess) {
        (void)hipGetLastError();
        p->d_lat16 = nullptr;  // no room: the u64 latencies are streamed
    }
    cspan_begin(p);
    if (e == hipSuccess)
        hipLaunchKernelGGL(lvl_sym_tile_kernel, dim3((uint32_t)std::min<uint64_t>(nb * (nb + 1) / 2, 8192)), dim3(256),
                           0, p->stream, p->V, p->d_lat, with_loss ? p->d_loss : nullptr, wmax_units * p->kp.g, d_ok,
                           p->d_lat16, 1.0 / (double)p->kp.g);
    cspan_end(p);
    uint32_t ok = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&ok, d_ok, 4, hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    (void)hipFree(d_ok);
    if (e != hipSuccess) return fail(err, e, "symmetry check");
    *sym = ok != 0;
    if (!*sym) {  // only symmetric plans' out-rows read it
        (void)hipFree(p->d_lat16);
        p->d_lat16 = nullptr;
    }
    return SRT_OK;
}

// The shortest non-self-loop edge of the plan's graph, ns (~0: none)
srt_status level_min_edge(srt_plan *p, uint64_t *min_ns, srt_err *err) {
    *min_ns = ~0ull;
    unsigned long long *d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof *d);
    if (e != hipSuccess) return fail(err, e, "hipMalloc(edge min)");
    (void)hipMemsetAsync(d, 0xff, sizeof *d, p->stream);
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(8192, (p->V + 3) / 4));
    cspan_begin(p);
    hipLaunchKernelGGL(edge_min_kernel, dim3(blocks), dim3(256), 0, p->stream, p->V, p->d_row_ptr, p->d_col, p->d_lat,
                       d);
    cspan_end(p);
    e = hipMemcpyAsync(min_ns, d, sizeof *d, hipMemcpyDeviceToHost, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    (void)hipFree(d);
    return e == hipSuccess ? SRT_OK : fail(err, e, "edge min");
}

void level_stats_init(unsigned long long *d_stats, hipStream_t s) {
    hipLaunchKernelGGL(level_zero_kernel, dim3(1), dim3(1), 0, s, d_stats, d_stats + 2, (unsigned long long *)nullptr);
}

srt_status level_run(srt_plan *p, unsigned long long *d_stats, srt_err *err) {
    if (!p->ev_loss0) {
        (void)hipEventCreate(&p->ev_loss0);
        (void)hipEventCreate(&p->ev_loss1);
    }
    (void)hipEventRecord(p->ev_loss0, p->stream);
    p->shard_tail = false;
    p->tail_expanded = false;
    p->stage16 = false;
    // symmetric integer-level plans sharded over ranks build the class CSR
    // sharded too (level_csr_sharded); the others build it whole
    const bool sym_int = p->lvl_sym && !p->lvl_q && p->ident_rows;
    srt_status st;
    if (!p->d_lvisit) {  // [0] the visit count, [1] the 4-byte entries' overflow word
        const hipError_t e = hipMalloc(&p->d_lvisit, 2 * sizeof(unsigned long long));
        if (e != hipSuccess) return fail(err, e, "hipMalloc(visit counter)");
        (void)hipMemsetAsync(p->d_lvisit, 0, 2 * sizeof(unsigned long long), p->stream);
    }
    // 4-byte class entries: a plan that chose them (lvl_ce4), its rows on the
    // packed row (launch_solve_ctx's conditions) and read where they are built --
    // not exchanged between ranks, nor downloaded behind the solve (the repeat
    // after an overflow is srt_plan_sync's and srt_plan_fetch's)
    const bool ce4 = p->lvl_ce4 && sym_int && p->lvl_pack && p->lvl_sp && p->kp.lmax <= PACK_LMAX && !p->comm &&
                     !p->fold_chunk_rows;
    bool zeroed = false;
    if (sym_int && ((p->comm && p->comm->nranks > 1) || (p->row_shard && p->lvl_emu_ranks > 1)))
        level_ce4_off(p);  // the sharded class CSR exchanges 8-byte entries
    if (sym_int && p->comm && p->comm->nranks > 1)
        st = level_csr_sharded(p, p->kp.lmax, true, (uint32_t)p->comm->nranks, (uint32_t)p->comm->rank, p->comm, err);
    else if (sym_int && p->row_shard && p->lvl_emu_ranks > 1)
        st = level_csr_sharded(p, p->kp.lmax, true, p->lvl_emu_ranks,
                               (uint32_t)((uint64_t)p->row0 * p->lvl_emu_ranks / std::max<uint32_t>(p->n, 1)), nullptr,
                               err);
    else {
        // a kept class structure: the run's counters zeroed ahead of the fill, the
        // 4-byte entries' overflow word with them (nothing else writes the class max)
        const bool kept = level_keep_applies(p);
        if (kept)
            hipLaunchKernelGGL(level_zero_kernel, dim3(1), dim3(1), 0, p->stream, d_stats,
                               (unsigned long long *)p->d_tmaxw, p->d_lvisit,
                               ce4 ? p->d_lvisit + 1 : (unsigned long long *)nullptr);
        st = level_csr(p, p->kp.lmax, true, err, ce4);
        zeroed = kept && st == SRT_OK && p->lvl_keep_run;
    }
    if (st != SRT_OK) return st;
    p->lvl_ce4_pending = p->lvl_ce4_run;
    if (!zeroed)
        hipLaunchKernelGGL(level_zero_kernel, dim3(1), dim3(1), 0, p->stream, d_stats, (unsigned long long *)p->d_tmaxw,
                           p->d_lvisit);
#if LOSS_COUNT
    {
        const uint32_t dg = std::getenv("SRT_LVL_DIAG") ? (uint32_t)std::atoi(std::getenv("SRT_LVL_DIAG")) : 0u;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(lvl_diag), &dg, sizeof dg);
    }
#endif
    p->p3_launches = 0;
    p->p3_work = 0.0;
    p->p3_tiles = 0;
    if (p->comm) {
        st = level_sharded(p, d_stats, err);
        (void)hipEventRecord(p->ev_loss1, p->stream);
        return st;
    }
    const uint32_t lcap = (uint32_t)p->kp.lmax;
    // the solve launches are the plan's timed dominant launches (event pairs,
    // srt_plan_kernel_stats; work = the table pairs they write)
    const uint32_t cr = p->fold_chunk_rows ? p->fold_chunk_rows : std::max<uint32_t>(1, p->row1 - p->row0);
    const uint32_t nc = (p->row1 - p->row0 + cr - 1) / cr;
    if ((st = ensure_events(p->ev, 2 * (size_t)nc, (unsigned)hipEventDisableSystemFence, err)) != SRT_OK) return st;
    if (p->fold_chunk_rows && (st = ensure_events(p->ev_fold, nc, hipEventDisableTiming, err)) != SRT_OK) return st;
    for (uint32_t c = 0; c < nc; ++c) {
        RowJob job;
        job.range = true;
        job.r0 = p->row0 + c * cr;
        job.r1 = std::min(p->row1, job.r0 + cr);
        (void)hipEventRecord(p->ev[2 * c], p->stream);
        if ((st = launch_solve(p, d_stats, job, lcap, false, nullptr, err)) != SRT_OK) return st;
        (void)hipEventRecord(p->ev[2 * c + 1], p->stream);
        p->p3_launches++;
        p->p3_work += (double)(job.r1 - job.r0) * p->n;
        if (p->fold_chunk_rows) (void)hipEventRecord(p->ev_fold[c], p->stream);
    }
    (void)hipEventRecord(p->ev_loss1, p->stream);
#if LOSS_COUNT
    {  // diagnostic builds (-DLOSS_COUNT=1): totals of every level solve so far
        unsigned long long c[8];
        (void)hipStreamSynchronize(p->stream);
        (void)hipMemcpyFromSymbol(c, HIP_SYMBOL(solve_cnt), sizeof c);
        const double rows = (double)(p->row1 - p->row0);
        std::fprintf(stderr, "[srt] level solve (cumulative): visits %llu, us per row per CU: init %.2f levels %.2f out %.2f\n",
                     c[1], c[4] * 0.01 / rows, c[6] * 0.01 / rows, c[7] * 0.01 / rows);
        unsigned long long lc[8][5];
        (void)hipMemcpyFromSymbol(lc, HIP_SYMBOL(lvl_cnt), sizeof lc);
        for (int l = 1; l < 8; ++l)
            if (lc[l][4])
                std::fprintf(stderr, "[srt]   level %d: rows %llu items/row %.0f us/row: plan %.2f walk %.2f collect %.2f\n", l,
                             lc[l][4], (double)lc[l][3] / lc[l][4], lc[l][0] * 0.01 / lc[l][4],
                             lc[l][1] * 0.01 / lc[l][4], lc[l][2] * 0.01 / lc[l][4]);
    }
#endif
    return SRT_OK;
}

// srt_init: loads this unit's code object (srt::preload_kernels)
hipError_t preload_level() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&level_zero_kernel));
}

}  // namespace srt
