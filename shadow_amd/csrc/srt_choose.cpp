// srt_choose.cpp -- the host decisions of plan creation (srt_choose.h): pure
// functions of the scanned graph, the device's free memory and the knobs.
#include "srt_choose.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <queue>
#include <thread>

namespace srt {

unsigned __int128 proved_bound(const CsrStats &cs, uint32_t V, uint64_t ecc_units) {
    return ecc_units != ~0ull ? (unsigned __int128)ecc_units : (unsigned __int128)(V ? V - 1 : 0) * max_units(cs);
}

// Choose the closure's key representation and prove it exact.
//
// Keys are path latencies in units of g = gcd of all edge latencies (latency
// only: the loss is recomputed exactly by the loss pass, so no loss bits share
// the key).  Lmax bounds every shortest-path latency: the longest edge for a
// complete graph (a direct edge bounds every pair), else (V-1) * max edge --
// or, tighter, in-eccentricity + out-eccentricity of one node that reaches
// and is reached by every node (fw_ecc_bound: d(u,v) <= d(u,s) + d(s,v)).
// Edges longer than Lmax are then stored saturated at INF (the init kernels).
// Exactness does not depend on the schedule's read order: (1) every stored
// value only decreases from its initial value <= INF, so each operand is <=
// INF and a candidate (sum of two) is <= 2 INF, which the key type holds
// without wrapping (u16 lanes: 0xFFFE; u32: 2^32 - 2) -- no candidate is ever
// corrupted, whatever the grouped / look-ahead / sharded schedules read; (2) a
// candidate below INF is the exact length of a real walk, so no stored value
// drops below the true distance d; (3) the schedule's values are never above
// the sequential Floyd-Warshall's (its candidates are formed from operands at
// least as tight), which ends at d.  So the closure ends at d exactly when
// every finite d < INF -- Lmax < INF.  The test below asks for 2 Lmax + 1 <
// INF, a margin kept from the r01 packed (latency, loss) keys.  Below 2^53 the
// keys may be f64 (v_add_f64 / v_min_f64), below 2^62 u64, and below
// KEY32_INF (2^31 - 1) u32; u16 below KEY16_INF.  Lmax < 2^32 - 1
// additionally lets the loss pass keep latencies as u32.  Knob
// SRT_FW_KEY=u32|f64|u64 (measurement / A-B parity only) skips the narrower
// representations.
bool choose_key_params(const CsrStats &cs, uint32_t V, uint64_t ecc_units, const Knob<int> &fw_key, KeyParams *kp,
                       int *key_type, bool *f16, std::string *why) {
    kp->g = cs.gcd;
    const uint64_t maxu = max_units(cs);
    unsigned __int128 Lmax = cs.complete ? (unsigned __int128)maxu : (unsigned __int128)(V ? V - 1 : 0) * maxu;
    // the eccentricity bound (fw_ecc_bound), when the sweeps found one
    if (ecc_units != ~0ull && (unsigned __int128)ecc_units < Lmax) Lmax = ecc_units;
    kp->lmax = Lmax > (unsigned __int128)~0ull ? ~0ull : (uint64_t)Lmax;
    kp->lat32 = Lmax < 0xffffffffull;
    // knob SRT_FW_KEY = u16 / u32 / f64 / u64: the narrowest key allowed (A/B, tests)
    const bool force = fw_key.set;
    const bool allow16 = !force || fw_key.v == KEY_U16;
    const int min_type = force && (fw_key.v == KEY_U64 || fw_key.v == KEY_F64) ? fw_key.v : KEY_U32;
    *f16 = false;
    if (allow16 && 2 * Lmax + 1 < (unsigned __int128)srt::KEY16_INF) {
        *key_type = srt::KEY_U16;
        // f16 integer arithmetic on the same 2-byte keys (0.75 VALU slot per
        // relaxation instead of 1): every finite distance < 1024 = F16 INF,
        // so candidates stay <= 2048, exact in f16 (the FW kernels).  SRT_FW_KEY=u16
        // keeps integer arithmetic (A/B parity tests).
        *f16 = !force && Lmax < 1024;
        return true;
    }
    if (min_type <= srt::KEY_U32 && 2 * Lmax + 1 < (unsigned __int128)srt::KEY32_INF) {
        *key_type = srt::KEY_U32;
        return true;
    }
    if (min_type <= srt::KEY_F64 && 2 * Lmax + 1 < ((unsigned __int128)1 << 53)) {
        *key_type = srt::KEY_F64;
        return true;
    }
    if (2 * Lmax + 1 < ((unsigned __int128)1 << 62)) {
        *key_type = srt::KEY_U64;
        return true;
    }
    *why = "the latency range does not fit a 62-bit exact key";
    return false;
}

// Sparse SSSP key (the packed-key sweeps): latency in units of g in the high 32 bits.
// A stored value is a simple path (<= V-1 edges) and a candidate adds one
// edge, so V * max_edge_latency / g < 2^32 - 1 keeps every sum exact and
// below the all-ones "unreached" key.
bool sssp_params(const CsrStats &cs, uint32_t V, std::string *why) {
    if ((unsigned __int128)V * max_units(cs) >= 0xffffffffull) {
        *why = "V * max edge latency exceeds the 32-bit latency field of the SSSP key";
        return false;
    }
    return true;
}

// Family prices for AUTO, seconds on one MI355X, from the measured rates of
// DESIGN.md 4 (rest launches by key type, r03 profiles; sparse builds r04).
// Dense: Vp^3 relaxations (half on the triangle schedule: 2-byte keys on a
// symmetric graph), at least ~80 us a 128-pivot round (the chain: C2 4k), plus
// the exact-loss fold (C3: 7.0 ms for 16k x 16k pairs).  Sparse: one unit per
// (source, in-edge or vertex) visited, at the C4 rate of the frontier sweeps
// (u16 latencies) or of the packed-key sweeps, at least ~1 ms a launch of
// sources (its ~60 dependent sweeps).
double price_fw(uint32_t Vp, uint32_t n, uint32_t V, int key_type, bool f16, bool sym) {
    const double rate = f16                          ? 4.3e13   // C3 rest: 1.45 ms / 6.26e10
                        : key_type == srt::KEY_U16 ? 3.3e13     // 1.90 ms (r02)
                        : key_type == srt::KEY_U32 ? 1.25e13    // 4.82-5.19 ms
                        : key_type == srt::KEY_F64 ? 8e12       // ~half the u32 mix, not profiled
                                                   : 4e12;      // u64: ~1/3 of u32's mix, not profiled
    const bool tri = sym && (f16 || key_type == srt::KEY_U16);
    const double relax = (double)Vp * Vp * Vp * (tri ? 0.5 : 1.0);
    return std::max(relax / rate, (double)(Vp / 128) * 80e-6) + (double)n * V * 2.6e-11;
}
// Level solve: a row walks the probe row's edge count plus ~4 passes over
// the row's V levels (init, the level collections), at the level fold's
// measured cost per visit (C3: 4.56 ms for 16k rows of ~160k visits), and
// writes its 12-byte table row.
double price_level(uint32_t n, uint32_t V, uint64_t visits) {
    return (double)n * ((double)visits + 4.0 * V) * 1.8e-12 + (double)n * n * 12.0 / 5e12 + 3e-4;
}
double price_sparse(uint32_t n, uint64_t n_in, uint32_t V, bool frontier) {
    const double units = (double)n * ((double)n_in + V);
    const double per = frontier ? 1.19e-11 : 1.73e-11;  // C4: 9e10 units in 1.07 s / 1.56 s
    const double launches = std::ceil((double)n / (frontier ? 8192.0 : 4096.0));
    return std::max(units * per, launches * 1e-3);
}

FamilyPick pick_family(uint32_t want, bool fw_ok, bool sssp_ok, bool lvl_ok, double t_fw, double t_sssp,
                       double t_lvl) {
    FamilyPick r;
    if (want == SRT_ALGO_FW) {
        if (fw_ok) r.algo = SRT_ALGO_FW;
    } else if (want == SRT_ALGO_SSSP) {
        if (sssp_ok) r.algo = SRT_ALGO_SSSP;
    } else if (want == SRT_ALGO_LEVEL) {
        if (lvl_ok) r.algo = SRT_ALGO_LEVEL;
    } else {
        if (!fw_ok) t_fw = 1e300;
        if (!sssp_ok) t_sssp = 1e300;
        if (!lvl_ok) t_lvl = 1e300;
        char pr[128];
        std::snprintf(pr, sizeof pr, " auto-price=fw:%.3gms,sparse:%.3gms,level:%.3gms", t_fw < 1e299 ? t_fw * 1e3 : -1.0,
                      t_sssp < 1e299 ? t_sssp * 1e3 : -1.0, t_lvl < 1e299 ? t_lvl * 1e3 : -1.0);
        r.note = pr;
        if (fw_ok || sssp_ok || lvl_ok)
            r.algo = t_lvl <= std::min(t_fw, t_sssp) ? SRT_ALGO_LEVEL : t_sssp < t_fw ? SRT_ALGO_SSSP : SRT_ALGO_FW;
    }
    return r;
}

LevelQuantum level_quantum(uint64_t min_edge_units, uint32_t vb) {
    LevelQuantum r;
    // an entry keeps the remainder w - c q (< q) in 34 - vb bits;
    // latencies up to 64 q stay below 2^31
    r.q = std::min<uint64_t>(std::min<uint64_t>(min_edge_units, 1ull << (34 - vb)), 1ull << 25);
    while ((1ull << r.rb) < r.q) ++r.rb;
    return r;
}

SsspGroups sssp_groups(uint32_t n, uint32_t V, uint64_t free_bytes) {
    // R words of 64 sources per lane (one wave walks a vertex's in-edges
    // once for 64*R sources), and as many groups in flight as ~256 MB of
    // path state allows (Infinity Cache sized), never more than the rows need
    const uint32_t words = std::max<uint32_t>(1, (n + 63) / 64);
    // Many groups in flight amortise each sweep's launch and latency chain
    // and the convergence tail (C4, measured: 192 MB of path state 3.0 s,
    // 1.6 GB 1.73 s, 6.4 GB 1.53 s, 12.8 GB 1.49 s), capped at 1/8 of the
    // free HBM.
    uint64_t budget_mb = 6400;
    if (free_bytes) budget_mb = std::max<uint64_t>(64, std::min<uint64_t>(budget_mb, (free_bytes >> 20) / 8));
    const uint32_t R = words >= 4 ? 4 : words >= 2 ? 2 : 1;
    const uint64_t per_group = (uint64_t)V * 64 * 8 * R;
    uint64_t G = std::max<uint64_t>(1, (budget_mb << 20) / std::max<uint64_t>(per_group, 1));
    G = std::min<uint64_t>(G, (words + R - 1) / R);
    G = std::min<uint64_t>(G, 256);
    SsspGroups r;
    r.R = R;
    r.nb = (uint32_t)(G * R);
    return r;
}

FrontierGeometry frontier_geometry(uint32_t n, uint32_t V, uint64_t block_bytes, uint64_t free_bytes,
                                   bool latency_symmetric, const CreateKnobs &k) {
    // blocks in flight: as many as half the free HBM holds (C4: ~0.7 GB a
    // block, capped at 64 = 32k sources), never more than the rows need;
    // knob SRT_SSSP_FR_NB (measurement)
    const uint64_t bb = block_bytes;
    uint64_t nb = 64;
    if (free_bytes) nb = std::min<uint64_t>(nb, std::max<uint64_t>(1, (free_bytes / 2) / std::max<uint64_t>(bb, 1)));
    // launches of equal size (C4: 196 blocks as 4 x 49, not 64+64+64+4 --
    // a small last launch pays a full run of sweeps: 0.70 -> 0.68 s)
    const uint64_t all_blocks = std::max<uint32_t>(1, (n + 511) / 512);
    nb = (all_blocks + (all_blocks + nb - 1) / nb - 1) / ((all_blocks + nb - 1) / nb);
    if (k.sssp_fr_nb.set) nb = std::max<uint64_t>(1, k.sssp_fr_nb.v);
    nb = std::min<uint64_t>(nb, all_blocks);
    FrontierGeometry r;
    r.nb = (uint32_t)nb;
    // undirected (latency-symmetric) graphs: L(s, v) = L(v, s), so every
    // launch starts from the exact columns of the earlier launches' rows
    // (the frontier's fr_sym_copy_kernel) -- which needs the latencies
    // of all rows resident: n * V * 2 B (C4: 20 GB), if a quarter of the
    // free HBM holds them.  Knob SRT_SSSP_SYM=0 (A/B, tests).
    r.sym = !(k.sssp_sym.set && k.sssp_sym.v == 0) && all_blocks > nb && all_blocks * V * 1024ull <= free_bytes / 4 &&
            latency_symmetric;
    // a smaller first launch: the only one whose latency phase starts
    // from the sources alone (C4, 4 launches: 49+49+49+49 blocks 0.488 s,
    // 12+61+61+62 0.463, 20+... 0.465, 28+... 0.463); ~1/12 of the
    // blocks, the rest keep the launch count, so their buffers grow to
    // hold them.  Knob SRT_FR_FIRST = blocks (0: equal launches; A/B).
    if (r.sym) {
        const uint64_t f = k.fr_first.set ? k.fr_first.v : all_blocks / 12, launches = (all_blocks + nb - 1) / nb;
        if (f > 0 && f < nb && launches >= 2) {
            const uint64_t rest = (all_blocks - f + launches - 2) / (launches - 1);
            if (rest <= 64 && rest * bb <= free_bytes / 2) {
                nb = std::max(nb, rest);
                r.first = (uint32_t)f;
                r.nb = (uint32_t)nb;
            }
        }
    }
    r.lblocks = r.sym ? (uint32_t)all_blocks : (uint32_t)nb;
    return r;
}

// Pull-form adjacency for the sweep: for every v, the entries u -> v of every
// row u (petgraph edges(u): directed outgoing / undirected incident), minus
// self-loops (they never shorten a path; the diagonal is the raw self-loop).
void build_in_edges(const srt_csr *g, uint64_t gunit, uint64_t n_in, std::vector<uint64_t> *ptr,
                    std::vector<srt::InEdge> *edges) {
    const uint32_t V = g->n_nodes;
    ptr->assign((size_t)V + 1, 0);
    for (uint32_t u = 0; u < V; ++u)
        for (uint64_t k = g->row_ptr[u]; k < g->row_ptr[u + 1]; ++k)
            if (g->col[k] != u) (*ptr)[g->col[k] + 1]++;
    for (uint32_t v = 0; v < V; ++v) (*ptr)[v + 1] += (*ptr)[v];
    edges->resize(std::max<uint64_t>(n_in, 1));
    std::vector<uint64_t> fill(ptr->begin(), ptr->end() - 1);
    for (uint32_t u = 0; u < V; ++u)
        for (uint64_t k = g->row_ptr[u]; k < g->row_ptr[u + 1]; ++k) {
            const uint32_t v = g->col[k];
            if (v == u) continue;
            srt::InEdge e;
            e.u = u;
            e.w = (uint32_t)(g->lat_ns[k] / gunit);
            e.eb = 1.0f - g->loss[k];
            e.pad = 0;
            (*edges)[fill[v]++] = e;
        }
}

// Is the latency adjacency symmetric (every u -> v of latency w has a v -> u of
// latency w, as multisets -- petgraph undirected graphs are)?  Then every
// shortest latency is symmetric, L(s, v) = L(v, s), which the frontier sweeps
// use to seed a launch from the rows of the earlier ones.  Per vertex: the
// in-edges (u, w) against the out-row (col, lat / g), both sorted; host threads
// over vertex ranges.
bool latency_symmetric(const srt_csr *g, const std::vector<uint64_t> &in_ptr, const std::vector<srt::InEdge> &in_edge,
                       uint64_t gunit) {
    const uint32_t V = g->n_nodes;
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<uint8_t> bad(nt, 0);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            std::vector<uint64_t> a, b;
            for (uint32_t v = (uint32_t)((uint64_t)V * t / nt); v < (uint32_t)((uint64_t)V * (t + 1) / nt) && !bad[t];
                 ++v) {
                a.clear();
                b.clear();
                for (uint64_t k = in_ptr[v]; k < in_ptr[v + 1]; ++k)
                    a.push_back((uint64_t)in_edge[k].u << 32 | in_edge[k].w);
                for (uint64_t k = g->row_ptr[v]; k < g->row_ptr[v + 1]; ++k)
                    if (g->col[k] != v) b.push_back((uint64_t)g->col[k] << 32 | (uint32_t)(g->lat_ns[k] / gunit));
                if (a.size() != b.size()) {
                    bad[t] = 1;
                    break;
                }
                std::sort(a.begin(), a.end());
                std::sort(b.begin(), b.end());
                if (a != b) bad[t] = 1;
            }
        });
    for (auto &x : th) x.join();
    for (uint8_t x : bad)
        if (x) return false;
    return true;
}

// Source order of the sparse sweeps: the level order of a shortest-latency
// tree from the highest-degree vertex (then from the lowest-numbered vertex
// not yet reached): the root, its tree children, theirs, ... each parent's
// children together.  The sweeps put table rows in this order into their
// words, lanes (8 sources) and 128-B lines (32 sources); sources at the same
// tree depth under nearby parents reach most targets along paths of the same
// hop count, so a word's labels change at the same vertices in the same
// sweeps.  C4's graph (tools measurement on the host, hop counts of the
// shortest-path trees of 32-source lines over all targets): 3.1 distinct hop
// counts a line in this order, 9.7 in plain breadth-first order from the same
// root, 7.5 in tree depth-first order.  Measured on C4: loss sweeps 266 -> 214
// ms a build; but as the order of the launches (which sources come first) it
// costs the symmetric seeding (latency sweeps 94 -> 142 ms), so the frontier
// composes launches in breadth-first order (hop_rank) and orders rows within a
// launch by this rank.
// plain breadth-first discovery order from the same root (knob SRT_SSSP_ORDER=2, A/B)
std::vector<uint32_t> hop_rank(const srt_csr *g) {
    const uint32_t V = g->n_nodes;
    std::vector<uint32_t> rank(V, ~0u), q;
    q.reserve(V);
    uint32_t start = 0;
    uint64_t best = 0;
    for (uint32_t u = 0; u < V; ++u)
        if (g->row_ptr[u + 1] - g->row_ptr[u] > best) best = g->row_ptr[u + 1] - g->row_ptr[u], start = u;
    uint32_t next = 0;
    for (uint32_t root = start, scan = 0; next < V;) {
        if (rank[root] == ~0u) {
            rank[root] = next++;
            q.push_back(root);
            for (size_t h = q.size() - 1; h < q.size(); ++h)
                for (uint64_t k = g->row_ptr[q[h]]; k < g->row_ptr[q[h] + 1]; ++k) {
                    const uint32_t v = g->col[k];
                    if (v < V && rank[v] == ~0u) {
                        rank[v] = next++;
                        q.push_back(v);
                    }
                }
        }
        while (scan < V && rank[scan] != ~0u) ++scan;
        root = scan;
    }
    return rank;
}

std::vector<uint32_t> spt_rank(const srt_csr *g) {
    const uint32_t V = g->n_nodes, NONE = ~0u;
    std::vector<uint32_t> rank(V, NONE), first(V, NONE), last(V, NONE), sib(V, NONE), q;
    std::vector<uint64_t> dist(V, ~0ull);
    std::vector<uint32_t> pred(V, NONE);
    std::vector<uint8_t> done(V, 0);
    q.reserve(V);
    uint32_t start = 0;
    uint64_t best = 0;
    for (uint32_t u = 0; u < V; ++u)
        if (g->row_ptr[u + 1] - g->row_ptr[u] > best) best = g->row_ptr[u + 1] - g->row_ptr[u], start = u;
    typedef std::pair<uint64_t, uint32_t> Item;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    uint32_t next = 0;
    for (uint32_t root = start, scan = 0; next < V;) {
        if (rank[root] == NONE) {
            // Dijkstra over the adjacency's latencies; a vertex joins its
            // parent's child list when settled (children in settle order)
            dist[root] = 0;
            heap.push({0, root});
            while (!heap.empty()) {
                const Item it = heap.top();
                heap.pop();
                const uint32_t u = it.second;
                if (done[u] || it.first != dist[u]) continue;
                done[u] = 1;
                if (u != root) {
                    const uint32_t pu = pred[u];
                    if (last[pu] == NONE) first[pu] = u;
                    else sib[last[pu]] = u;
                    last[pu] = u;
                }
                for (uint64_t k = g->row_ptr[u]; k < g->row_ptr[u + 1]; ++k) {
                    const uint32_t v = g->col[k];
                    if (v >= V || done[v]) continue;
                    const uint64_t d = it.first + g->lat_ns[k];
                    if (d < dist[v]) {
                        dist[v] = d;
                        pred[v] = u;
                        heap.push({d, v});
                    }
                }
            }
            // the tree's level order
            q.clear();
            q.push_back(root);
            rank[root] = next++;
            for (size_t h = 0; h < q.size(); ++h)
                for (uint32_t c = first[q[h]]; c != NONE; c = sib[c]) {
                    rank[c] = next++;
                    q.push_back(c);
                }
        }
        while (scan < V && rank[scan] != NONE) ++scan;
        root = scan;
    }
    return rank;
}

FrontierOrder frontier_vertex_order(const srt_csr *g, const uint32_t *nodes, uint32_t n, std::vector<uint64_t> *in_ptr_,
                                    std::vector<InEdge> *in_edge_) {
    // Hub-spreading vertex order for the frontier sweeps: a wave works
    // through a 64-vertex chunk item by item, so a chunk of hubs (BA
    // graphs number them first: C4's vertices 0..63 have ~1000
    // in-edges each) would keep one wave busy for the whole sweep
    // (measured: C4 1.71 s -> 1.07 s with the hubs dealt out).  The
    // cpb highest in-degree vertices go to slot 0 of the cpb chunks,
    // one each; every other vertex keeps its relative order (BA graphs'
    // id locality: neighbours of similar age gather similar rows).
    std::vector<uint64_t> &in_ptr = *in_ptr_;
    std::vector<InEdge> &in_edge = *in_edge_;
    const uint32_t V = g->n_nodes, cpb = (V + 63) / 64;
    std::vector<uint32_t> order(V), pi(V, ~0u);
    for (uint32_t v = 0; v < V; ++v) order[v] = v;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return in_ptr[a + 1] - in_ptr[a] > in_ptr[b + 1] - in_ptr[b];
    });
    // (measured, C4: no hubs dealt 1.30 s, the top 64 0.95 s, one per chunk 0.80 s)
    const uint32_t H = V >= 64 * cpb ? cpb : (V > cpb ? cpb - 1 : 0);  // chunks with a full slot 0
    std::vector<uint8_t> hub(V, 0);
    for (uint32_t h = 0; h < H; ++h) {
        pi[order[h]] = h * 64;
        hub[order[h]] = 1;
    }
    for (uint32_t v = 0, pos = 0; v < V; ++v) {
        if (hub[v]) continue;
        while (pos % 64 == 0 && pos / 64 < H) ++pos;  // slot 0 of a hub chunk
        pi[v] = pos++;
    }
    FrontierOrder r;
    std::vector<uint64_t> ip((size_t)V + 1, 0), &op = r.row_ptr;
    op.assign((size_t)V + 1, 0);
    for (uint32_t v = 0; v < V; ++v) {
        ip[pi[v] + 1] = in_ptr[v + 1] - in_ptr[v];
        uint64_t d = 0;
        for (uint64_t k = g->row_ptr[v]; k < g->row_ptr[v + 1]; ++k) d += g->col[k] != v;
        op[pi[v] + 1] = d;
    }
    for (uint32_t v = 0; v < V; ++v) {
        ip[v + 1] += ip[v];
        op[v + 1] += op[v];
    }
    std::vector<InEdge> ie(in_edge.size());
    std::vector<uint32_t> &oc = r.col;
    oc.resize(std::max<uint64_t>(op[V], 1));
    for (uint32_t v = 0; v < V; ++v) {
        uint64_t o = ip[pi[v]];
        for (uint64_t k = in_ptr[v]; k < in_ptr[v + 1]; ++k, ++o) {
            ie[o] = in_edge[k];
            ie[o].u = pi[in_edge[k].u];
        }
        o = op[pi[v]];
        for (uint64_t k = g->row_ptr[v]; k < g->row_ptr[v + 1]; ++k)
            if (g->col[k] != v) oc[o++] = pi[g->col[k]];
    }
    in_ptr.swap(ip);
    in_edge.swap(ie);
    r.fnodes.resize(n);
    for (uint32_t i = 0; i < n; ++i) r.fnodes[i] = pi[nodes[i]];
    return r;
}

bool choose_row_packed(bool quant, uint64_t lmax, bool sp, const Knob<int> &pack, int rows_unpacked, int rows_packed,
                       int fit_rt) {
    const bool valid = !quant && lmax <= 14 && sp && fit_rt >= 2;
    if (!valid || (pack.set && pack.v == 0)) return false;
    if (pack.set && pack.v == 1) return true;
    return rows_unpacked < 2 && rows_packed >= 2;
}

std::string describe_level(uint64_t g, uint32_t q, uint64_t lmax, uint32_t V, uint32_t n, uint64_t visits, bool sym,
                           bool lat16, bool packed) {
    char d[200];
    const char *rows = sym ? (packed  ? (lat16 ? " rows=sym lat16 row=packed" : " rows=sym row=packed")
                              : lat16 ? " rows=sym lat16"
                                      : " rows=sym")
                           : (packed ? " row=packed" : "");
    if (q)
        std::snprintf(d, sizeof d, "level:u32 g=%llu q=%u lmax=%llu(probe) V=%u n=%u visits=%llu loss=in-solve%s",
                      (unsigned long long)g, q, (unsigned long long)lmax, V, n, (unsigned long long)visits, rows);
    else
        std::snprintf(d, sizeof d, "level:u16 g=%llu lmax=%llu(probe) V=%u n=%u visits=%llu loss=in-solve%s",
                      (unsigned long long)g, (unsigned long long)lmax, V, n, (unsigned long long)visits, rows);
    return d;
}

std::string describe_fw(bool f16, int key_type, const KeyParams &kp, bool complete, uint64_t ecc_units, uint32_t V,
                        uint32_t n, bool glds, bool band) {
    char d[200];
    std::snprintf(d, sizeof d, "fw:%s B=%d g=%llu lmax=%llu%s V=%u n=%u stage=%s band=%d loss=tight-dag%s",
                  f16                   ? "f16key"
                  : key_type == KEY_U16 ? "u16key"
                  : key_type == KEY_U32 ? "u32key"
                  : key_type == KEY_F64 ? "f64key"
                                        : "u64key",
                  FW_B, (unsigned long long)kp.g, (unsigned long long)kp.lmax,
                  complete ? "(complete)" : ecc_units != ~0ull && ecc_units == kp.lmax ? "(ecc)" : "(V-1)", V, n,
                  glds ? "glds" : "reg", (int)band, kp.lat32 ? "/u32" : "/u64");
    return d;
}

std::string describe_sssp(uint64_t g, uint32_t V, uint32_t n, uint64_t n_in, uint32_t R, uint32_t groups,
                          uint32_t delta, bool table_order) {
    char d[256];
    std::snprintf(d, sizeof d, "sssp:lat32|f32 g=%llu V=%u n=%u E_in=%llu R=%u groups=%u delta=%u order=%s",
                  (unsigned long long)g, V, n, (unsigned long long)n_in, R, groups, delta,
                  table_order ? "table" : "bfs");
    return d;
}

std::string describe_frontier(uint64_t g, uint64_t ecc_units, uint32_t V, uint32_t n, uint64_t n_in, uint32_t blocks,
                              uint32_t first, bool table_order, bool tree_order, bool sym) {
    char d[160];
    std::snprintf(d, sizeof d,
                  "sssp:frontier u16|f32 g=%llu lmax=%llu%s V=%u n=%u E_in=%llu blocks=%u first=%u order=%s seed=%s",
                  (unsigned long long)g, (unsigned long long)(ecc_units != ~0ull ? ecc_units : 0),
                  ecc_units != ~0ull ? "(ecc)" : "(V-1)", V, n, (unsigned long long)n_in, blocks, first,
                  table_order ? "table" : tree_order ? "bfs+tree" : "bfs", sym ? "sym" : "none");
    return d;
}

}  // namespace srt
