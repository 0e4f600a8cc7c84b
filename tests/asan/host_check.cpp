// host_check.cpp -- the GPU-free host code of libsrt and the oracle under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_sanitize.py builds
// it with tests/asan/Makefile and runs it on the CPU).  It drives:
//   * srt_gml.cpp   GML ingest: generated graphs, truncations and byte flips
//   * srt_scan.cpp  the CSR scan: random CSRs with planted errors, on threads
//   * srt_xz.cpp    the .xz decoder: the blobs named on the command line
//                   (made by Python's liblzma) intact, truncated and flipped
//   * srt_ip.cpp    IpAssignment and the resolver's host lookups, threaded
//   * srt_routing.cpp RoutingInfo: path / counters from 8 threads over
//                   a compact table (the device build is replaced by
//                   routing_build below, which fills a host table)
//   * the oracle    GML parse + Dijkstra + direct paths
//   * srt_choose.cpp plan creation's host decisions: key proofs, family
//                   choice, launch geometry, in-edges, symmetry, the
//                   frontier's vertex order, on generated graphs
// Any sanitizer report aborts the process (halt_on_error); exit 0 = clean.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/srt.h"
#include "../../oracle/srt_oracle.h"
#include "../../shadow_amd/csrc/srt_choose.h"
#include "../../shadow_amd/csrc/srt_internal.h"
#include "../../shadow_amd/csrc/srt_scan.h"

#define CHECK(c, ...)                                         \
    do {                                                      \
        if (!(c)) {                                           \
            std::fprintf(stderr, "CHECK failed: " __VA_ARGS__); \
            std::fprintf(stderr, "\n");                       \
            std::exit(1);                                     \
        }                                                     \
    } while (0)

// ---- stand-ins for the device build the RoutingInfo code links against ----
// (the harness has no GPU: these fill the table on the host)
namespace srt {
void init_wait() {}
srt_status routing_build(const srt_csr *, const uint32_t *, uint32_t n, const srt_opts *, CompactTable *t,
                         uint64_t *min_latency, srt_err *) {
    t->bytes = SRT_RI_REC6;
    t->n = n;
    t->g = 1000;
    t->lat16 = static_cast<uint16_t *>(std::malloc(std::max<size_t>((size_t)n * n, 1) * 2));
    t->loss = static_cast<float *>(std::malloc(std::max<size_t>((size_t)n * n, 1) * 4));
    for (size_t k = 0; k < (size_t)n * n; ++k) {
        t->lat16[k] = (uint16_t)(1 + k % 300);
        t->loss[k] = (float)(k % 97) / 1000.0f;
    }
    t->diag.assign(n, srt_path{7, 0.5f, 0});
    *min_latency = 1000;
    return SRT_OK;
}
}  // namespace srt
extern "C" srt_status srt_get_direct_paths(const srt_csr *, const uint32_t *, uint32_t, srt_path *, uint64_t *,
                                           const srt_opts *, srt_err *) {
    return SRT_ERR_UNSUPPORTED;
}
extern "C" srt_status srt_plan_fetch(srt_plan *, srt_path *, uint64_t *, srt_err *) { return SRT_ERR_UNSUPPORTED; }

namespace {

std::string gml(uint32_t n, std::mt19937_64 &rng, bool directed) {
    std::string s = std::string("graph [\n  directed ") + (directed ? "1" : "0") + "\n";
    for (uint32_t i = 0; i < n; ++i) s += "  node [\n    id " + std::to_string(i * 3 + 1) + "\n    host_bandwidth_up \"1 Gbit\"\n  ]\n";
    const char *units[] = {"ms", "us", "ns", "s", "m", "h", "μs", ""};
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = directed ? 0 : i; j < n; ++j) {
            if (i != j && rng() % 3 == 0) continue;
            s += "  edge [\n    source " + std::to_string(i * 3 + 1) + "\n    target " + std::to_string(j * 3 + 1) +
                 "\n    latency \"" + std::to_string(1 + rng() % 300) + " " + units[rng() % 8] + "\"\n";
            if (rng() % 2) s += "    packet_loss 0." + std::to_string(rng() % 1000) + "\n";
            s += "  ]\n";
        }
    return s + "]\n";
}

void check_gml(std::mt19937_64 &rng) {
    int ok = 0, bad = 0;
    for (int it = 0; it < 60; ++it) {
        std::string t = gml(2 + rng() % 24, rng, rng() % 2);
        if (it % 3 == 1) t.resize(rng() % t.size());                     // truncated
        if (it % 3 == 2) t[rng() % t.size()] = (char)(rng() % 256);     // a flipped byte
        srt_gml *g = nullptr;
        srt_err e{};
        if (srt_gml_parse(t.data(), t.size(), &g, &e) == SRT_OK) {
            srt_csr c{};
            CHECK(srt_gml_csr(g, &c) == SRT_OK, "csr");
            uint64_t sum = 0;
            for (uint64_t k = 0; k < c.n_adj; ++k) sum += c.col[k] + c.lat_ns[k];
            (void)sum;
            srt_gml_free(g);
            ++ok;
        } else {
            ++bad;
        }
        char err[256];
        or_graph *og = or_gml_parse(t.data(), t.size(), err, sizeof err);
        if (og) or_graph_free(og);
    }
    std::printf("gml: %d parsed, %d rejected\n", ok, bad);
}

void check_scan(std::mt19937_64 &rng) {
    for (int it = 0; it < 20; ++it) {
        const uint32_t V = 50 + rng() % 300;
        std::vector<uint64_t> rp(V + 1, 0), lat;
        std::vector<uint32_t> col;
        std::vector<float> loss;
        for (uint32_t u = 0; u < V; ++u) {
            const uint32_t d = rng() % 40;
            for (uint32_t k = 0; k < d; ++k) {
                col.push_back(rng() % (V + (it % 5 == 0 ? 3 : 0)));  // sometimes out of range
                lat.push_back((rng() % 300) * 1000000ull + (it % 7 == 0 ? rng() % 2 : 0));
                loss.push_back(it % 4 == 0 && rng() % 50 == 0 ? 1.5f : (float)(rng() % 100) / 1000.f);
            }
            rp[u + 1] = col.size();
        }
        srt_csr c{V, 0, col.size(), rp.data(), col.data(), lat.data(), loss.data(), nullptr};
        srt::CsrStats cs;
        srt::csr_scan(&c, &cs, true);
        (void)srt::first_bad_loss(&c);
    }
    std::printf("scan: ok\n");
}

std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> b;
    FILE *f = std::fopen(path, "rb");
    if (!f) return b;
    int c;
    while ((c = std::fgetc(f)) != EOF) b.push_back((uint8_t)c);
    std::fclose(f);
    return b;
}

void check_xz(int argc, char **argv, std::mt19937_64 &rng) {
    int good = 0, rejected = 0;
    for (int a = 1; a < argc; ++a) {
        const std::vector<uint8_t> blob = slurp(argv[a]);
        CHECK(!blob.empty(), "read %s", argv[a]);
        for (int v = 0; v < 12; ++v) {
            std::vector<uint8_t> b = blob;
            if (v >= 1 && v <= 4) b.resize(rng() % b.size());
            if (v >= 5) b[rng() % b.size()] ^= (uint8_t)(1u << (rng() % 8));
            uint8_t *out = nullptr;
            size_t n = 0;
            srt_err e{};
            if (srt_xz_decompress(b.data(), b.size(), &out, &n, &e) == SRT_OK) {
                ++good;
                srt_free(out);
            } else {
                ++rejected;
            }
        }
    }
    std::printf("xz: %d decoded, %d rejected\n", good, rejected);
}

void check_ip(std::mt19937_64 &rng) {
    srt_ip_assignment *ia = nullptr;
    CHECK(srt_ip_assignment_create(&ia) == SRT_OK, "ia");
    for (int k = 0; k < 3000; ++k) {
        if (rng() % 4 == 0) {
            srt_err e{};
            (void)srt_ip_assignment_assign_ip(ia, (uint32_t)(rng() % 500), (uint32_t)rng(), &e);
        } else {
            (void)srt_ip_assignment_assign(ia, (uint32_t)(rng() % 500));
        }
    }
    std::vector<uint32_t> nodes(srt_ip_assignment_get_nodes(ia, nullptr, 0));
    srt_ip_assignment_get_nodes(ia, nodes.data(), (uint32_t)nodes.size());
    srt_ip_resolver *r = nullptr;
    srt_err e{};
    CHECK(srt_ip_resolver_create(ia, nodes.data(), (uint32_t)nodes.size(), &r, &e) == SRT_OK, "resolver");
    std::vector<uint32_t> ips(400000);
    for (auto &x : ips) x = (uint32_t)rng();
    std::vector<int32_t> rows(ips.size());
    CHECK(srt_ip_resolve_rows(r, ips.data(), ips.size(), rows.data()) == SRT_OK, "resolve");
    srt_ip_resolver_destroy(r);
    srt_ip_assignment_destroy(ia);
    std::printf("ip: ok\n");
}

void check_routing_info() {
    const uint32_t n = 300;
    std::vector<uint32_t> ids(n), nodes(n);
    std::vector<uint64_t> rp(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) ids[i] = 5 * i + 2, nodes[i] = i;
    srt_csr c{n, 0, 0, rp.data(), nullptr, nullptr, nullptr, ids.data()};
    srt_routing_info *ri = nullptr;
    srt_err e{};
    CHECK(srt_routing_info_build(&c, nodes.data(), n, 1, nullptr, &ri, &e) == SRT_OK, "build: %s", e.msg);
    std::vector<std::thread> th;
    std::atomic<uint64_t> hits{0};
    for (int t = 0; t < 8; ++t)
        th.emplace_back([&, t] {
            std::mt19937 r(t);
            for (int k = 0; k < 200000; ++k) {
                const uint32_t a = 5 * (r() % (n + 3)) + 2, b = 5 * (r() % n) + 2;
                srt_path p;
                if (srt_routing_info_path(ri, a, b, &p) == SRT_OK) hits++;
                srt_routing_info_increment_packet_count(ri, a, b);
            }
        });
    for (auto &x : th) x.join();
    std::vector<uint64_t> counts((size_t)n * n, 3);
    srt_routing_info_add_packet_counts(ri, counts.data());
    std::vector<srt_path> full((size_t)n * n);
    srt_routing_info_copy_table(ri, full.data());
    uint64_t mn = 0;
    CHECK(srt_routing_info_smallest_latency_ns(ri, &mn) == 1, "min");
    srt_routing_info_destroy(ri);
    std::printf("routing info: %llu paths\n", (unsigned long long)hits.load());
}

void check_oracle(std::mt19937_64 &rng) {
    const std::string t = gml(40, rng, false);
    char err[256];
    or_graph *og = or_gml_parse(t.data(), t.size(), err, sizeof err);
    CHECK(og, "oracle parse: %s", err);
    const uint32_t n = or_graph_num_nodes(og), m = or_graph_num_edges(og);
    std::vector<uint32_t> ids(n), src(m), dst(m), nodes(n);
    std::vector<uint64_t> lat(m);
    std::vector<float> loss(m);
    or_graph_node_ids(og, ids.data());
    or_graph_edges(og, src.data(), dst.data(), lat.data(), loss.data());
    for (uint32_t i = 0; i < n; ++i) nodes[i] = i;
    or_edge_list el{n, m, src.data(), dst.data(), lat.data(), loss.data(), or_graph_directed(og)};
    std::vector<uint64_t> ol((size_t)n * n);
    std::vector<float> op((size_t)n * n);
    or_err e{};
    for (int mode = 0; mode < 2; ++mode)
        (void)or_compute_shortest_paths(&el, ids.data(), nodes.data(), n, n, ol.data(), op.data(), 4, mode, &e);
    (void)or_get_direct_paths(&el, ids.data(), nodes.data(), n, ol.data(), op.data(), &e);
    or_graph_free(og);
    std::printf("oracle: ok\n");
}

// ---- plan creation's host decisions (srt_choose.cpp) ----

// a graph as its adjacency entries (u, v, latency, loss), in row order
struct Adj {
    uint32_t V = 0;
    std::vector<uint64_t> rp, lat;
    std::vector<uint32_t> col;
    std::vector<float> loss;
    srt_csr csr() { return srt_csr{V, 0, col.size(), rp.data(), col.data(), lat.data(), loss.data(), nullptr}; }
};
struct Entry {
    uint32_t u, v;
    uint64_t lat;
    float loss;
};
Adj adj_of(uint32_t V, std::vector<Entry> es) {
    std::stable_sort(es.begin(), es.end(), [](const Entry &a, const Entry &b) { return a.u < b.u; });
    Adj a;
    a.V = V;
    a.rp.assign((size_t)V + 1, 0);
    for (const Entry &e : es) {
        a.rp[e.u + 1]++;
        a.col.push_back(e.v);
        a.lat.push_back(e.lat);
        a.loss.push_back(e.loss);
    }
    for (uint32_t u = 0; u < V; ++u) a.rp[u + 1] += a.rp[u];
    return a;
}
// both directions of undirected edges (a, b), a != b, plus one self-loop per vertex
std::vector<Entry> undirected(uint32_t V, const std::vector<std::pair<uint32_t, uint32_t>> &edges, std::mt19937_64 &rng) {
    std::vector<Entry> es;
    for (uint32_t v = 0; v < V; ++v) es.push_back({v, v, 1 + rng() % 50, 0.f});
    for (const auto &e : edges) {
        const uint64_t l = 1 + rng() % 50;
        const float p = (float)(rng() % 100) / 1000.f;
        es.push_back({e.first, e.second, l, p});
        es.push_back({e.second, e.first, l, p});
    }
    return es;
}
// preferential attachment: every new vertex joins m distinct earlier ones, by degree
std::vector<std::pair<uint32_t, uint32_t>> ba_edges(uint32_t V, uint32_t m, std::mt19937_64 &rng) {
    std::vector<std::pair<uint32_t, uint32_t>> edges;
    std::vector<uint32_t> ends;
    for (uint32_t v = 1; v <= m; ++v) edges.push_back({0, v}), ends.push_back(0), ends.push_back(v);
    for (uint32_t v = m + 1; v < V; ++v) {
        std::vector<uint32_t> t;
        while (t.size() < m) {
            const uint32_t x = ends[rng() % ends.size()];
            if (std::find(t.begin(), t.end(), x) == t.end()) t.push_back(x);
        }
        for (uint32_t x : t) edges.push_back({x, v}), ends.push_back(x), ends.push_back(v);
    }
    return edges;
}
std::vector<std::pair<uint32_t, uint32_t>> ring_edges(uint32_t V, uint32_t chords, std::mt19937_64 &rng) {
    std::vector<std::pair<uint32_t, uint32_t>> edges;
    for (uint32_t v = 0; v < V; ++v) edges.push_back({v, (v + 1) % V});
    for (uint32_t k = 0; k < chords; ++k) {
        const uint32_t a = rng() % V, b = rng() % V;
        if (a != b) edges.push_back({a, b});
    }
    return edges;
}

typedef std::tuple<uint32_t, uint32_t, uint32_t, float> EdgeKey;  // (source, target, latency units, 1 - loss)

void check_vertex_order(Adj a) {
    const uint32_t V = a.V;
    srt_csr c = a.csr();
    uint64_t n_in = 0;
    for (uint32_t u = 0; u < V; ++u)
        for (uint64_t k = a.rp[u]; k < a.rp[u + 1]; ++k) n_in += a.col[k] != u;
    std::vector<uint64_t> in_ptr;
    std::vector<srt::InEdge> in_edge;
    srt::build_in_edges(&c, 1, n_in, &in_ptr, &in_edge);
    CHECK(in_ptr[V] == n_in, "in-edge count");
    const std::vector<uint64_t> ptr0 = in_ptr;
    const std::vector<srt::InEdge> edge0 = in_edge;
    std::vector<uint32_t> nodes(V);
    for (uint32_t v = 0; v < V; ++v) nodes[v] = v;
    const srt::FrontierOrder fo = srt::frontier_vertex_order(&c, nodes.data(), V, &in_ptr, &in_edge);
    const std::vector<uint32_t> &pi = fo.fnodes;  // the nodes are 0 .. V-1: fnodes is pi itself
    // a permutation
    std::vector<uint8_t> hit(V, 0);
    for (uint32_t v = 0; v < V; ++v) {
        CHECK(pi[v] < V && !hit[pi[v]], "V=%u: pi is no permutation at %u", V, v);
        hit[pi[v]] = 1;
    }
    // the H = V / 64 full chunks get the H vertices of highest in-degree
    // (the lower id first among equals) at their slot 0, in that order
    const uint32_t H = V / 64;
    std::vector<uint32_t> by_deg(V);
    for (uint32_t v = 0; v < V; ++v) by_deg[v] = v;
    std::stable_sort(by_deg.begin(), by_deg.end(),
                     [&](uint32_t x, uint32_t y) { return ptr0[x + 1] - ptr0[x] > ptr0[y + 1] - ptr0[y]; });
    std::vector<uint8_t> hub(V, 0);
    for (uint32_t h = 0; h < H; ++h) {
        CHECK(pi[by_deg[h]] == h * 64, "V=%u: hub %u (vertex %u) sits at %u", V, h, by_deg[h], pi[by_deg[h]]);
        hub[by_deg[h]] = 1;
    }
    // every other vertex keeps its relative order
    uint32_t last = 0;
    bool first = true;
    for (uint32_t v = 0; v < V; ++v) {
        if (hub[v]) continue;
        CHECK(first || pi[v] > last, "V=%u: vertex %u out of order", V, v);
        CHECK(!(pi[v] % 64 == 0 && pi[v] / 64 < H), "V=%u: vertex %u in a hub's slot", V, v);
        last = pi[v];
        first = false;
    }
    // the permuted in-edges are the input's, renumbered
    std::vector<EdgeKey> want, got;
    for (uint32_t v = 0; v < V; ++v)
        for (uint64_t k = ptr0[v]; k < ptr0[v + 1]; ++k)
            want.emplace_back(pi[edge0[k].u], pi[v], edge0[k].w, edge0[k].eb);
    CHECK(in_ptr.size() == (size_t)V + 1 && in_ptr[0] == 0 && in_ptr[V] == n_in, "V=%u: permuted in_ptr", V);
    for (uint32_t x = 0; x < V; ++x) {
        CHECK(in_ptr[x] <= in_ptr[x + 1], "V=%u: permuted in_ptr decreases", V);
        for (uint64_t k = in_ptr[x]; k < in_ptr[x + 1]; ++k) got.emplace_back(in_edge[k].u, x, in_edge[k].w, in_edge[k].eb);
    }
    std::sort(want.begin(), want.end());
    std::sort(got.begin(), got.end());
    CHECK(want == got, "V=%u: permuted in-edges differ", V);
    // the out-CSR is the permuted adjacency without self-loops, each row in its order
    CHECK(fo.row_ptr.size() == (size_t)V + 1 && fo.row_ptr[0] == 0 && fo.row_ptr[V] == n_in, "V=%u: out row_ptr", V);
    CHECK(fo.col.size() == std::max<uint64_t>(n_in, 1), "V=%u: out col size", V);
    for (uint32_t v = 0; v < V; ++v) {
        uint64_t o = fo.row_ptr[pi[v]];
        for (uint64_t k = a.rp[v]; k < a.rp[v + 1]; ++k)
            if (a.col[k] != v) {
                CHECK(o < fo.row_ptr[pi[v] + 1] && fo.col[o] == pi[a.col[k]], "V=%u: out row of %u", V, v);
                ++o;
            }
        CHECK(o == fo.row_ptr[pi[v] + 1], "V=%u: out row length of %u", V, v);
    }
}

void check_symmetry(std::mt19937_64 &rng) {
    const uint32_t V = 200;
    const std::vector<Entry> es = undirected(V, ba_edges(V, 3, rng), rng);
    auto symmetric = [&](const std::vector<Entry> &e) {
        Adj a = adj_of(V, e);
        srt_csr c = a.csr();
        std::vector<uint64_t> in_ptr;
        std::vector<srt::InEdge> in_edge;
        srt::build_in_edges(&c, 1, e.size() - V, &in_ptr, &in_edge);
        // every in-edge is an adjacency entry, with its latency and 1 - loss
        for (uint32_t v = 0; v < V; ++v)
            for (uint64_t k = in_ptr[v]; k < in_ptr[v + 1]; ++k) {
                bool found = false;
                for (uint64_t j = a.rp[in_edge[k].u]; j < a.rp[in_edge[k].u + 1] && !found; ++j)
                    found = a.col[j] == v && a.lat[j] == in_edge[k].w && 1.0f - a.loss[j] == in_edge[k].eb;
                CHECK(found && in_edge[k].u != v, "in-edge %u -> %u is no adjacency entry", in_edge[k].u, v);
            }
        return srt::latency_symmetric(&c, in_ptr, in_edge, 1);
    };
    CHECK(symmetric(es), "an undirected graph is latency-symmetric");
    size_t k = V;  // the first entry past the self-loops: one direction of an edge
    std::vector<Entry> one = es;
    one[k].lat += 1;
    CHECK(!symmetric(one), "one direction's latency changed");
    std::vector<Entry> cut = es;
    cut.erase(cut.begin() + (long)k + 1);  // its reverse
    CHECK(!symmetric(cut), "one reverse edge removed");
}

void check_pick_family() {
    const uint32_t algos[] = {SRT_ALGO_FW, SRT_ALGO_SSSP, SRT_ALGO_LEVEL};
    for (int ok = 0; ok < 8; ++ok)
        for (int w = 0; w < 3; ++w) {
            const srt::FamilyPick f = srt::pick_family(algos[w], ok & 1, ok & 2, ok & 4, 3.0, 2.0, 1.0);
            CHECK(f.algo == ((ok >> w) & 1 ? (int)algos[w] : -1) && f.note.empty(), "forced family %d, ok %d", w, ok);
        }
    auto pick = [](double fw, double sp, double lv, int ok = 7) {
        return srt::pick_family(SRT_ALGO_AUTO, ok & 1, ok & 2, ok & 4, fw, sp, lv).algo;
    };
    CHECK(pick(1e-3, 2e-3, 3e-3) == SRT_ALGO_FW, "AUTO: fw cheapest");
    CHECK(pick(2e-3, 1e-3, 3e-3) == SRT_ALGO_SSSP, "AUTO: sparse cheapest");
    CHECK(pick(2e-3, 3e-3, 1e-3) == SRT_ALGO_LEVEL, "AUTO: level cheapest");
    CHECK(pick(1e-3, 1e-3, 1e-3) == SRT_ALGO_LEVEL, "AUTO: level on a tie");
    CHECK(pick(1e-3, 1e-3, 2e-3) == SRT_ALGO_FW, "AUTO: fw on a tie with sparse");
    CHECK(pick(1e-3, 2e-3, 3e-3, 6) == SRT_ALGO_SSSP, "AUTO: the cheapest available");
    CHECK(pick(1e-3, 2e-3, 3e-3, 4) == SRT_ALGO_LEVEL, "AUTO: the only one available");
    CHECK(pick(1e-3, 2e-3, 3e-3, 0) == -1, "AUTO: none available");
    const srt::FamilyPick f = srt::pick_family(SRT_ALGO_AUTO, true, false, true, 1e-3, 2e-3, 0.5e-3);
    CHECK(f.note == " auto-price=fw:1ms,sparse:-1ms,level:0.5ms", "note '%s'", f.note.c_str());
}

void check_geometry() {
    const srt::CreateKnobs none;
    // C4: 100k sources = 196 blocks, launches of 16 + 3 x 60
    const uint64_t bb = 100000ull * (1024 + 2048 + 152) + 600000ull * 72, ample = 256ull << 30;
    srt::FrontierGeometry f = srt::frontier_geometry(100000, 100000, bb, ample, true, none);
    CHECK(f.nb == 60 && f.first == 16 && f.lblocks == 196 && f.sym, "C4 geometry: nb=%u first=%u lblocks=%u", f.nb,
          f.first, f.lblocks);
    // not symmetric: 4 equal launches of 49, their latencies only
    f = srt::frontier_geometry(100000, 100000, bb, ample, false, none);
    CHECK(f.nb == 49 && f.first == 0 && f.lblocks == 49 && !f.sym, "C4 directed: nb=%u first=%u", f.nb, f.first);
    srt::CreateKnobs k;
    k.sssp_fr_nb.set = true, k.sssp_fr_nb.v = 2;
    k.fr_first.set = true, k.fr_first.v = 1;
    f = srt::frontier_geometry(1300, 1300, 1300ull * 3224 + 7800ull * 72, ample, true, k);
    CHECK(f.nb == 2 && f.first == 1 && f.lblocks == 3 && f.sym, "first=1 geometry: nb=%u first=%u lblocks=%u", f.nb,
          f.first, f.lblocks);
    k.sssp_sym.set = true, k.sssp_sym.v = 0;
    f = srt::frontier_geometry(1300, 1300, 1300ull * 3224 + 7800ull * 72, ample, true, k);
    CHECK(f.nb == 2 && f.first == 0 && f.lblocks == 2 && !f.sym, "sym=0 geometry: nb=%u first=%u", f.nb, f.first);
    // free memory unknown: the 64-block cap stays (79 blocks as 40 + 39), no seeding
    f = srt::frontier_geometry(40000, 40000, bb, 0, true, none);
    CHECK(f.nb == 40 && f.first == 0 && f.lblocks == 40 && !f.sym, "unknown memory: nb=%u", f.nb);
    f = srt::frontier_geometry(64 * 512, 40000, bb, 0, true, none);
    CHECK(f.nb == 64, "the cap: nb=%u", f.nb);
    // little memory: one block a launch
    f = srt::frontier_geometry(100000, 100000, bb, bb, true, none);
    CHECK(f.nb == 1 && f.lblocks == 1 && !f.sym, "little memory: nb=%u", f.nb);

    srt::SsspGroups g = srt::sssp_groups(100, 500, 0);  // 2 words: one group of R = 2
    CHECK(g.R == 2 && g.nb == 2, "groups: R=%u nb=%u", g.R, g.nb);
    g = srt::sssp_groups(100000, 100000, 0);  // 6400 MB / (V * 64 * 8 * 4) = 32 groups
    CHECK(g.R == 4 && g.nb == 128, "C4 groups: R=%u nb=%u", g.R, g.nb);
    g = srt::sssp_groups(100000, 100000, 8ull << 30);  // 1/8 of 8 GB: 5 groups
    CHECK(g.R == 4 && g.nb == 20, "small-memory groups: R=%u nb=%u", g.R, g.nb);

    srt::LevelQuantum q = srt::level_quantum(1000000, 14);  // C3ns: edges >= 1 ms in ns units
    CHECK(q.q == 1000000 && q.rb == 20, "quantum: q=%llu rb=%u", (unsigned long long)q.q, q.rb);
    CHECK(srt::level_quantum(1, 14).q < 2 && srt::level_quantum(0, 14).q < 2, "no quantized solve");
    q = srt::level_quantum(1ull << 40, 15);  // capped by the entry's 34 - vb remainder bits
    CHECK(q.q == 1ull << 19 && q.rb == 19, "capped quantum: q=%llu rb=%u", (unsigned long long)q.q, q.rb);
}

// a complete 2-node graph whose longest edge is L ns beside 1 ns self-loops
// (gcd 1): Lmax = L units
void check_key(uint64_t L, int forced, int want_type, bool want_f16, bool want_ok = true) {
    std::vector<Entry> es = {{0, 0, 1, 0.f}, {0, 1, L, 0.f}, {1, 0, L, 0.f}, {1, 1, 1, 0.f}};
    Adj a = adj_of(2, es);
    srt_csr c = a.csr();
    srt::CsrStats cs;
    srt::csr_scan(&c, &cs, true);
    CHECK(cs.complete && cs.gcd == 1 && cs.maxlat == L, "scan of the key graph");
    srt::Knob<int> key;
    if (forced >= 0) key.set = true, key.v = forced;
    srt::KeyParams kp{};
    int type = -1;
    bool f16 = false;
    std::string why;
    const bool ok = srt::choose_key_params(cs, 2, ~0ull, key, &kp, &type, &f16, &why);
    CHECK(ok == want_ok, "L=%llu: key %s", (unsigned long long)L, ok ? "chosen" : "refused");
    if (!ok) return;
    CHECK(type == want_type && f16 == want_f16 && kp.g == 1 && kp.lmax == L && kp.lat32 == (L < 0xffffffffull),
          "L=%llu forced %d: type %d f16 %d", (unsigned long long)L, forced, type, (int)f16);
}

void check_keys() {
    using namespace srt;
    // 2 Lmax + 1 against KEY16_INF, KEY32_INF, 2^53 and 2^62; f16 below 1024
    check_key(1023, -1, KEY_U16, true);
    check_key(1024, -1, KEY_U16, false);
    check_key((KEY16_INF - 1) / 2 - 1, -1, KEY_U16, false);
    check_key((KEY16_INF - 1) / 2, -1, KEY_U32, false);
    check_key((KEY32_INF - 1) / 2 - 1, -1, KEY_U32, false);
    check_key((KEY32_INF - 1) / 2, -1, KEY_F64, false);
    check_key((1ull << 52) - 1, -1, KEY_F64, false);
    check_key(1ull << 52, -1, KEY_U64, false);
    check_key((1ull << 61) - 1, -1, KEY_U64, false);
    check_key(1ull << 61, -1, KEY_U64, false, false);
    // a forced key: never f16, never narrower than asked
    check_key(1023, KEY_U16, KEY_U16, false);
    check_key(1023, KEY_U32, KEY_U32, false);
    check_key(1023, KEY_F64, KEY_F64, false);
    check_key(1023, KEY_U64, KEY_U64, false);
    check_key((KEY32_INF - 1) / 2, KEY_U16, KEY_F64, false);
    // not complete: (V-1) * max edge, or the eccentricity bound when it is tighter
    CsrStats cs;
    cs.gcd = 10, cs.maxlat = 1000, cs.complete = false;
    CHECK(proved_bound(cs, 11, ~0ull) == 1000 && proved_bound(cs, 11, 70) == 70 && proved_bound(cs, 0, ~0ull) == 0,
          "proved bound");
    KeyParams kp{};
    int type = -1;
    bool f16 = false;
    std::string why;
    CHECK(choose_key_params(cs, 101, ~0ull, Knob<int>(), &kp, &type, &f16, &why) && kp.lmax == 10000 && !f16, "(V-1)");
    CHECK(choose_key_params(cs, 101, 700, Knob<int>(), &kp, &type, &f16, &why) && kp.lmax == 700 && f16, "(ecc)");
    CHECK(sssp_params(cs, 101, &why) && max_units(cs) == 100, "sparse key");
    cs.maxlat = 0xffffffffull * 10;
    CHECK(!sssp_params(cs, 1, &why), "sparse key overflow");
}

void check_choose(std::mt19937_64 &rng) {
    check_vertex_order(adj_of(600, undirected(600, ba_edges(600, 3, rng), rng)));
    check_vertex_order(adj_of(130, undirected(130, ring_edges(130, 0, rng), rng)));
    for (uint32_t V : {63u, 64u, 65u}) check_vertex_order(adj_of(V, undirected(V, ring_edges(V, 40, rng), rng)));
    check_symmetry(rng);
    check_pick_family();
    check_geometry();
    check_keys();
    // the source orders are permutations
    Adj a = adj_of(700, undirected(700, ba_edges(700, 2, rng), rng));
    srt_csr c = a.csr();
    for (const std::vector<uint32_t> &rank : {srt::hop_rank(&c), srt::spt_rank(&c)}) {
        std::vector<uint8_t> hit(a.V, 0);
        for (uint32_t v = 0; v < a.V; ++v) {
            CHECK(rank[v] < a.V && !hit[rank[v]], "source order is no permutation");
            hit[rank[v]] = 1;
        }
    }
    std::printf("choose: ok\n");
}

}  // namespace

int main(int argc, char **argv) {
    std::mt19937_64 rng(2026);
    check_gml(rng);
    check_scan(rng);
    check_xz(argc, argv, rng);
    check_ip(rng);
    check_routing_info();
    check_oracle(rng);
    check_choose(rng);
    std::printf("host_check: clean\n");
    return 0;
}
