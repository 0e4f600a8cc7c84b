// srt_choose.h -- the host decisions of plan creation (srt_choose.cpp): key
// proofs, family prices and choice, launch geometry, the sparse graph's
// in-edges, symmetry, source and vertex orders, and describe()'s strings.
// Every function takes its inputs as arguments: no device call, no
// environment variable (srt_api.cpp's read_create_knobs fills CreateKnobs),
// so tests/asan/host_check.cpp drives all of it on the CPU.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "srt_internal.h"
#include "srt_scan.h"

namespace srt {

// an environment knob: unset, or its parsed value
template <typename T>
struct Knob {
    bool set = false;
    T v{};
};

// The environment variables plan creation reads, parsed once at the start of
// every create (they may change between two creates of one process).
struct CreateKnobs {
    bool fw_no_ecc = false;       // SRT_FW_NO_ECC (presence): no eccentricity proof, the (V-1) * max edge bound
    Knob<int> level;              // SRT_LEVEL: 0 keeps AUTO off the level solve (A/B, tests)
    Knob<int> lvl_sym;            // SRT_LVL_SYM: 0 = always build the in-rows (A/B, tests)
    Knob<int> level_q;            // SRT_LEVEL_Q: 0 = integer levels only (A/B, tests)
    Knob<int> lvl_nt;             // SRT_LVL_NT: 0 = the level solve's table rows by plain stores (A/B, tests)
    Knob<int> lvl_sp;             // SRT_LVL_SP: 0 = its per-item walk, not the pipelined one (A/B, tests)
    Knob<int> lvl_dyn;            // SRT_LVL_DYN: 0 = its rows dealt statically, not by a counter (A/B, tests)
    Knob<int> lvl_pack;           // SRT_LVL_PACK: 0 = never its packed LDS row, 1 = wherever the layout is valid (A/B, tests)
    Knob<int> lvl_ce4;            // SRT_LVL_CE4: 0 = never the packed row's 4-byte class entries, 1 = wherever the packed row runs on a symmetric plan (A/B, tests); unset: with the packed row the plan chose itself (SRT_LVL_PACK unset)
    Knob<int> lvl_ce4_nt;         // SRT_LVL_CE4_NT: 512, 640 or 768 = the threads of the 4-byte-entry kernel's workgroups (A/B, tests; any other value is refused); unset: the widest that fits twice a CU
    Knob<int> lvl_keep;           // SRT_LVL_KEEP: 0 = every run builds its class rows from the adjacency (A/B, tests); unset or 1 = kept from the probe's wherever eligible (level_keep)
    Knob<int> lvl_spread;        // SRT_LVL_SPREAD: 0 = the packed row's small levels one lane group an item (A/B)
    Knob<int> lvl_lean;           // SRT_LVL_LEAN: 0 = full-row passes around every level's walk (A/B, tests); unset or 1 = the lean
                                  // stages kept (LVL_LEAN_KEPT); an even value > 1 = that mask of LVL_LEAN_* stages (A/B; 6 = without
                                  // the wave walk of the big push levels; 14 = without the row stages LVL_LEAN_ROWS, 16 .. 64)
    Knob<int> fw_p1;              // SRT_FW_P1: u16/f16 phase 1, 1 = two FW steps per barrier, 0 = one (A/B)
    Knob<int> fw_emulate_ranks;   // SRT_FW_EMULATE_RANKS: rank 0's share of an N-rank schedule (measurement only)
    Knob<bool> fw_band;           // SRT_FW_BAND=1: grouped launches in banded tile order
    Knob<int> fw_key;             // SRT_FW_KEY=u16|u32|f64|u64: the narrowest key allowed, as a KeyType (A/B, tests)
    Knob<int> sssp_key;           // SRT_SSSP_KEY: 64 keeps the packed-key sweep (A/B, tests)
    Knob<int> sssp_order;         // SRT_SSSP_ORDER: source order of the sweep's words, 0 = table order (default 1)
    Knob<double> sssp_delta;      // SRT_SSSP_DELTA: delta-stepping bucket width, x the mean in-edge latency
    Knob<int> sssp_act;           // SRT_SSSP_ACT: 0 turns target activation off, k > 1: from sweep k
    Knob<long long> sssp_fr_nb;   // SRT_SSSP_FR_NB: frontier blocks per launch (measurement)
    Knob<int> sssp_fr_grid;       // SRT_SSSP_FR_GRID: frontier sweep workgroups (measurement)
    Knob<int> sssp_sym;           // SRT_SSSP_SYM: 0 = no symmetric seeding (A/B, tests)
    Knob<long long> fr_first;     // SRT_FR_FIRST: blocks of the first frontier launch (0: equal launches; A/B)
    Knob<int> upload_piece;       // SRT_UPLOAD_PIECE: log2 entries per piece, forces the pipelined upload on (tests)
};

// the longest edge in units of the latency gcd
inline uint64_t max_units(const CsrStats &cs) { return cs.maxlat / cs.gcd; }

// The proved bound on every finite shortest-path latency, units of g: the
// eccentricity bound when the sweeps found one (ecc_units != ~0), else
// (V-1) * max edge.
unsigned __int128 proved_bound(const CsrStats &cs, uint32_t V, uint64_t ecc_units);

bool choose_key_params(const CsrStats &cs, uint32_t V, uint64_t ecc_units, const Knob<int> &fw_key, KeyParams *kp,
                       int *key_type, bool *f16, std::string *why);
bool sssp_params(const CsrStats &cs, uint32_t V, std::string *why);

double price_fw(uint32_t Vp, uint32_t n, uint32_t V, int key_type, bool f16, bool sym);
double price_level(uint32_t n, uint32_t V, uint64_t visits);
double price_sparse(uint32_t n, uint64_t n_in, uint32_t V, bool frontier);

// The family of a create: the asked one when it is available, AUTO's cheapest
// (level on a tie with the cheaper closure, FW on a tie with sparse); algo -1:
// none applies.  note: AUTO's " auto-price=" suffix of describe().
struct FamilyPick {
    int algo = -1;
    std::string note;
};
FamilyPick pick_family(uint32_t want, bool fw_ok, bool sssp_ok, bool lvl_ok, double t_fw, double t_sssp,
                       double t_lvl);

// Quantized level solve: bucket width q (units of g; < 2: no quantized solve)
// and the remainder bits rb of a class entry, from the shortest edge and the
// vertex bits vb of an entry (level_vbits).
struct LevelQuantum {
    uint64_t q = 0;
    uint32_t rb = 0;
};
LevelQuantum level_quantum(uint64_t min_edge_units, uint32_t vb);

// Packed-key sweeps: R words of 64 sources per lane, nb = groups x R words in
// flight.  free_bytes: the device's free memory, 0 when unknown.
struct SsspGroups {
    uint32_t R = 1, nb = 1;
};
SsspGroups sssp_groups(uint32_t n, uint32_t V, uint64_t free_bytes);

// Frontier sweeps: nb 512-source blocks per launch, a first launch of `first`
// blocks (0: equal launches), lblocks blocks of resident latencies, sym =
// launches seed from the earlier ones' rows.  block_bytes: device memory of
// one block (frontier_block_bytes); free_bytes as above.
struct FrontierGeometry {
    uint32_t nb = 1, first = 0, lblocks = 1;
    bool sym = false;
};
FrontierGeometry frontier_geometry(uint32_t n, uint32_t V, uint64_t block_bytes, uint64_t free_bytes,
                                   bool latency_symmetric, const CreateKnobs &k);

void build_in_edges(const srt_csr *g, uint64_t gunit, uint64_t n_in, std::vector<uint64_t> *ptr,
                    std::vector<InEdge> *edges);
bool latency_symmetric(const srt_csr *g, const std::vector<uint64_t> &in_ptr, const std::vector<InEdge> &in_edge,
                       uint64_t gunit);
std::vector<uint32_t> hop_rank(const srt_csr *g);
std::vector<uint32_t> spt_rank(const srt_csr *g);

// The frontier sweeps' hub-spreading vertex order pi: in_ptr / in_edge are
// permuted in place (rows and sources renumbered); row_ptr / col are the
// renumbered out-CSR without self-loops and fnodes[i] = pi[nodes[i]].
struct FrontierOrder {
    std::vector<uint64_t> row_ptr;
    std::vector<uint32_t> col;
    std::vector<uint32_t> fnodes;
};
FrontierOrder frontier_vertex_order(const srt_csr *g, const uint32_t *nodes, uint32_t n, std::vector<uint64_t> *in_ptr,
                                    std::vector<InEdge> *in_edge);

// The LDS row of an integer level plan: packed (4.5 B a vertex, two 512-thread
// workgroups a CU) or not.  The layout is valid for a plan that is not
// quantized, whose bound is <= 14 (4-bit levels), with the pipelined walk on,
// and whose packed kernel the runtime keeps two workgroups a CU of (fit_rt:
// level_pack_fit).  Knob 0: never; 1: wherever valid; unset: where it doubles
// the rows a CU -- the unpacked row allows fewer than two workgroups a CU by
// the launch's arithmetic (rows_unpacked: level_rows_per_cu) and the packed
// row two (rows_packed).
bool choose_row_packed(bool quant, uint64_t lmax, bool sp, const Knob<int> &pack, int rows_unpacked, int rows_packed,
                       int fit_rt);

// describe() of a plan, by family
std::string describe_level(uint64_t g, uint32_t q, uint64_t lmax, uint32_t V, uint32_t n, uint64_t visits, bool sym,
                           bool lat16, bool packed = false);
std::string describe_fw(bool f16, int key_type, const KeyParams &kp, bool complete, uint64_t ecc_units, uint32_t V,
                        uint32_t n, bool glds, bool band);
std::string describe_sssp(uint64_t g, uint32_t V, uint32_t n, uint64_t n_in, uint32_t R, uint32_t groups,
                          uint32_t delta, bool table_order);
std::string describe_frontier(uint64_t g, uint64_t ecc_units, uint32_t V, uint32_t n, uint64_t n_in, uint32_t blocks,
                              uint32_t first, bool table_order, bool tree_order, bool sym);

}  // namespace srt
