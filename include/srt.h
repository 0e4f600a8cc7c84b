/*
 * srt.h -- C ABI of the MI355X-native Shadow routing-table build ("srt").
 *
 * This is the drop-in boundary behind Shadow's Rust network-graph API.  Each
 * entry point names the reference interface it replaces (paths relative to the
 * Shadow v3.1.0 tree, see INTEGRATION.md for the Rust-side binding):
 *
 *   srt_compute_shortest_paths  <- NetworkGraph::compute_shortest_paths
 *                                  src/main/network/graph/mod.rs:183-228
 *   srt_get_direct_paths        <- NetworkGraph::get_direct_paths
 *                                  src/main/network/graph/mod.rs:230-252
 *   min_latency_ns out-params   <- RoutingInfo::get_smallest_latency_ns
 *                                  src/main/network/graph/mod.rs:474-476
 *   srt_packet_batch            <- Worker::send_packet decision
 *                                  src/main/core/worker.rs:326-410 (+ :539-553)
 *   srt_gml_parse               <- NetworkGraph::parse / gml_parser::parse
 *                                  src/main/network/graph/mod.rs:134-181
 *   srt_gml_parse_file          <- load_network_graph + read_xz
 *                                  src/main/network/graph/mod.rs:479-509
 *   srt_ip_assignment_* / srt_ip_resolver_* / srt_packet_batch_ip
 *                               <- IpAssignment (mod.rs:352-420) and the
 *                                  send path's lookups (worker.rs:539-553)
 *   srt_xoshiro_* / srt_host_node_seed
 *                               <- Host::random (host.rs:122, 233) seeding
 *                                  (sim_config.rs:47-53, 222-244)
 *   srt_routing_info_*          <- generate_routing_info + RoutingInfo
 *                                  src/main/core/sim_config.rs:424-461,
 *                                  src/main/network/graph/mod.rs:428-477
 *
 * Conventions (mirroring the reference's FFI: plain C types, no exceptions
 * across the boundary, caller-owned outputs):
 *   - All pointers in srt_csr / outputs are HOST pointers unless a function
 *     says "device".  Inputs are borrowed for the duration of the call.
 *   - Node references are petgraph NodeIndex values (0..n_nodes-1, GML order).
 *   - out[i*n + j] is the path nodes[i] -> nodes[j] (row-major over the
 *     caller's in-use node list, which may be in any order).
 *   - Every function returns an srt_status and fills *err (may be NULL) with
 *     the reference's error text for NO_EDGE / MULTI_EDGE.
 *   - Library functions are thread-compatible: concurrent calls on different
 *     srt_plan objects are fine; one plan is used by one thread at a time.
 */
#ifndef SRT_H
#define SRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_ABI_VERSION 4

typedef enum {
    SRT_OK = 0,
    SRT_ERR_NO_EDGE = 1,      /* "No edge connecting node {a} to {b}"   (mod.rs:267-268) */
    SRT_ERR_MULTI_EDGE = 2,   /* "More than one edge connecting node {a} to {b}" (:270-274) */
    SRT_ERR_DISCONNECTED = 3, /* reference panics: assert_eq!(paths.len(), n^2) (:219) */
    SRT_ERR_INVALID = 4,      /* bad arguments / parse error */
    SRT_ERR_HIP = 5,          /* HIP runtime failure */
    SRT_ERR_OOM = 6,
    SRT_ERR_UNSUPPORTED = 7,
    SRT_ERR_COMM = 8, /* RCCL failure */
} srt_status;

typedef struct {
    int32_t code;
    uint32_t a_id; /* GML ids named in NO_EDGE / MULTI_EDGE messages */
    uint32_t b_id;
    char msg[256];
} srt_err;

/* The graph as petgraph holds it: for every NodeIndex u, the EdgeReferences of
 * graph.edges(u) (directed: outgoing; undirected: all incident edges, the far
 * endpoint as `col`, self-loops once).  Parallel edges are allowed. */
typedef struct {
    uint32_t n_nodes;
    uint32_t directed;        /* informational; adjacency already encodes it */
    uint64_t n_adj;           /* number of adjacency entries */
    const uint64_t *row_ptr;  /* n_nodes + 1 */
    const uint32_t *col;      /* n_adj */
    const uint64_t *lat_ns;   /* n_adj, latency already converted to ns (mod.rs:336) */
    const float *loss;        /* n_adj, packet_loss in [0,1] */
    const uint32_t *node_ids; /* n_nodes GML ids (error text); NULL = use NodeIndex */
} srt_csr;

/* #[repr(C)] mirror of PathProperties (mod.rs:296-303), 16 bytes */
typedef struct {
    uint64_t latency_ns;
    float packet_loss;
    uint32_t _pad;
} srt_path;

/* FW: blocked min-plus Floyd-Warshall on the latencies + the exact-loss fold
 * (dense graphs); SSSP: batched multi-source sweeps (sparse graphs); LEVEL:
 * per-source bucket (Dial) Dijkstra over the edges of at most B units, B a
 * proved bound on every shortest path (dense graphs of small diameter in units
 * of the latency gcd); AUTO: the cheapest that applies, priced from measured
 * rates (the plan description names the choice and the prices) */
typedef enum { SRT_ALGO_AUTO = 0, SRT_ALGO_FW = 1, SRT_ALGO_SSSP = 2, SRT_ALGO_LEVEL = 3 } srt_algo;

typedef struct {
    uint32_t algo;   /* srt_algo */
    int32_t device;  /* HIP device ordinal (the first one when n_gpus > 1), -1 = current */
    uint32_t flags;  /* SRT_OPT_* */
    uint32_t n_gpus; /* 0 or 1: one GPU; N > 1: the build (srt_compute_shortest_paths,
                        srt_routing_info_build) shards over devices device .. device+N-1
                        with one host thread each in the calling process (srt_comm_init_local) */
} srt_opts;
/* flags: every one of the n_gpus ranks on `device` (tests the multi-GPU schedules on one GPU) */
#define SRT_OPT_SAME_DEVICE 1u

/* ------------------------------------------------------------------ info */
int srt_abi_version(void);
/* number of visible HIP devices (0 when no GPU); never fails */
int srt_device_count(void);

/* ------------------------------------------------------ one-shot host API */
/* compute_shortest_paths over the in-use nodes.  out: n*n entries (caller
 * allocated).  *min_latency_ns (may be NULL) = get_smallest_latency_ns() of the
 * resulting table, diagonal included. */
srt_status srt_compute_shortest_paths(const srt_csr *g, const uint32_t *nodes, uint32_t n,
                                      srt_path *out, uint64_t *min_latency_ns,
                                      const srt_opts *opts, srt_err *err);

/* get_direct_paths: table = the unique edge between every ordered pair. */
srt_status srt_get_direct_paths(const srt_csr *g, const uint32_t *nodes, uint32_t n,
                                srt_path *out, uint64_t *min_latency_ns, const srt_opts *opts,
                                srt_err *err);

/* ---------------------------------------------- device-resident plan API */
/* A plan holds the graph and the routing table in HBM so a caller (bench,
 * multi-GPU driver, the packet stage) can time or chain the build without
 * PCIe copies.  Table layout in HBM: SoA, row-major n*n: u64 latency_ns and
 * f32 packet_loss. */
typedef struct srt_plan srt_plan;

/* Uploads the graph, validates self-loops of the in-use nodes (mod.rs:210-217)
 * and chooses the kernel family; no shortest-path work yet. */
srt_status srt_plan_create(const srt_csr *g, const uint32_t *nodes, uint32_t n,
                           const srt_opts *opts, srt_plan **plan, srt_err *err);
/* Full routing build on the plan's stream; blocks until done. */
srt_status srt_plan_run(srt_plan *plan, srt_err *err);
/* Same, enqueue only (caller synchronises with srt_plan_sync). */
srt_status srt_plan_run_async(srt_plan *plan, srt_err *err);
srt_status srt_plan_sync(srt_plan *plan, srt_err *err);
/* Post-run: connectivity check + min latency; copies the table out if out != NULL. */
srt_status srt_plan_fetch(srt_plan *plan, srt_path *out, uint64_t *min_latency_ns,
                          srt_err *err);
/* device pointers of the table (valid until srt_plan_destroy) */
srt_status srt_plan_table(srt_plan *plan, uint64_t **d_latency_ns, float **d_packet_loss,
                          uint32_t *n);
/* human-readable kernel/representation choice, e.g. "fw:packed64 g=1000000 qb=38 s=30" */
const char *srt_plan_describe(const srt_plan *plan);
/* hipStream_t of the plan (as void*) */
void *srt_plan_stream(srt_plan *plan);
/* Timing of the last run's dominant kernel (FW phase-3 "rest" launches or the
 * SSSP sweep): summed ms and number of launches, measured with HIP events on
 * the plan's stream; dominant_work = relaxations those launches performed;
 * total_ms = the whole build on the device. */
srt_status srt_plan_kernel_stats(const srt_plan *plan, double *dominant_ms,
                                 uint64_t *dominant_launches, double *dominant_work,
                                 double *total_ms);
/* Phase breakdown of the last run (HIP events on the plan's streams). */
typedef struct {
    double total_ms;            /* the whole build on the device */
    double dominant_ms;         /* FW phase-3 rest launches / SSSP sweeps, summed */
    uint64_t dominant_launches;
    double dominant_work;       /* relaxations (FW) / algorithmic bytes (SSSP) of those launches */
    double loss_ms;             /* dense: exact-loss pass (tight-edge CSR + fold), 0 for SSSP */
    uint64_t tight_edges;       /* dense: edges of the tight-edge CSR */
    uint32_t sharded_tail;      /* dense, comm bound: 1 = the loss pass ran on this rank's own
                                   closure rows (no key all-gather; tight-edge lists and
                                   u32 + f32 table rows exchanged), 0 = replicated */
    uint32_t sparse_split;      /* reserved, 0 (an earlier split latency/loss sweep, removed) */
    uint64_t sparse_sweeps;     /* sparse: sweep launches of the last run, summed over its source
                                   launches (each covers every group in flight) */
    uint32_t loss_fold;         /* dense: 1 = the level fold (tight edges walked by weight class
                                   from the smaller latency level), 0 = the single-direction scan */
    uint32_t reserved0;
    uint64_t edge_visits;       /* level solve: class-CSR entries the last run's rows walked (ABI 2) */
    double create_device_ms;    /* device work of srt_plan_create, once per graph: bound proofs, the
                                   level probes, the symmetry check (ABI 4) */
} srt_timing;
srt_status srt_plan_timing(const srt_plan *plan, srt_timing *out);
/* C tiles (128 x 128 keys) the last FW run's dominant launches loaded and
 * stored, summed over those launches (0 for the SSSP sweep): the algorithmic
 * C traffic is tiles x 128^2 x 2 x sizeof(key). */
srt_status srt_plan_kernel_tiles(const srt_plan *plan, uint64_t *dominant_tiles);
void srt_plan_destroy(srt_plan *plan);

/* -------------------------------------------------------- multi-GPU (RCCL) */
/* One process per GPU.  Rank 0 calls srt_comm_unique_id, ships the 128 bytes
 * to the other ranks (e.g. torch.distributed broadcast), then every rank calls
 * srt_comm_init on its device.  A plan bound to a communicator computes only
 * its own source rows and all-gathers the table over xGMI. */
typedef struct srt_comm srt_comm;
srt_status srt_comm_unique_id(uint8_t out[128], srt_err *err);
srt_status srt_comm_init(const uint8_t id[128], int nranks, int rank, int device,
                         srt_comm **comm, srt_err *err);
void srt_comm_destroy(srt_comm *comm);
/* Host-callback transport with the same semantics (used to run the sharded
 * build over any host-side collective, e.g. torch.distributed/gloo in tests).
 * Each callback is invoked with the plan's stream idle and must have completed
 * the collective on the DEVICE buffer before returning 0.
 *   bcast:     d_buf[0..bytes) from rank `root` to all ranks;
 *   allgather: in place, rank r contributes d_buf[r*bytes_per_rank ..). */
typedef int (*srt_bcast_fn)(void *user, void *d_buf, uint64_t bytes, int root);
typedef int (*srt_allgather_fn)(void *user, void *d_buf, uint64_t bytes_per_rank);
srt_status srt_comm_init_callbacks(int nranks, int rank, srt_bcast_fn bcast,
                                   srt_allgather_fn allgather, void *user, srt_comm **comm,
                                   srt_err *err);
/* In-process transport: nranks communicators (comms[0 .. nranks)) for nranks
 * host threads of THIS process, rank r on devices[r] (NULL: device r; a device
 * may repeat -- several ranks on one GPU, for testing the schedules).  Every
 * rank's plan is driven by its own thread; collectives stay stream-ordered
 * (events + one peer-read kernel, peer access enabled between the devices).
 * Up to 16 ranks.  srt_comm_abort releases the other ranks of a failed one. */
srt_status srt_comm_init_local(int nranks, const int32_t *devices, srt_comm **comms, srt_err *err);
void srt_comm_abort(srt_comm *comm);
/* Binds the plan to a communicator: from now on srt_plan_run computes only
 * this rank's block-rows of the closure, broadcasts each round's pivot
 * block-row from its owner and all-gathers the path keys at the end, so every
 * rank holds the full table.  The communicator must outlive the plan. */
srt_status srt_plan_bind_comm(srt_plan *plan, srt_comm *comm, srt_err *err);
/* Row sharding without an exchange, for plans whose source rows are
 * independent (LEVEL and SSSP: one Dijkstra per source, the rayon fan-out of
 * mod.rs:190-208): from now on srt_plan_run computes only table rows
 * [rank*n/nranks, (rank+1)*n/nranks) (other rows are not written) and the
 * connectivity check / min latency of srt_plan_fetch cover those rows;
 * srt_plan_fetch refuses `out` (read the rows through srt_plan_table).  The
 * multi-process form of srt_opts.n_gpus: each rank's rows stay in its HBM or go
 * to the host over its own link, no collective.  FW plans (the closure needs
 * every pivot row): SRT_ERR_UNSUPPORTED -- bind a communicator instead. */
srt_status srt_plan_shard_rows(srt_plan *plan, int nranks, int rank, srt_err *err);

/* ------------------------------------------------------- packet delivery */
/* One outgoing inter-host packet, in the source host's send order. */
typedef struct {
    uint32_t src_host; /* index of the source host's RNG state */
    uint32_t src_row;  /* table row of the source host's node */
    uint32_t dst_row;  /* table column of the destination host's node */
    uint32_t payload_size;
    uint64_t t_ns; /* emulated time at send */
} srt_pkt;

/* PacketDeliveryStatusFlags (src/main/routing/packet.minimal.h:24-36): the send
 * decision's two, the inbound router stage's five, the interface's one
 * (PDS_SND_INTERFACE_SENT, packet.minimal.h:21) of the outbound relay stage
 * and its two of the receive stage (packet.minimal.h:27-28), the UDP socket's
 * three of srt_udprecv */
enum {
    SRT_PDS_NONE = 0,
    SRT_PDS_SND_CREATED = 1u << 1, /* the UDP send stage's: pull_out_packet made the packet (packet.minimal.h:15) */
    SRT_PDS_SND_INTERFACE_SENT = 1u << 7,
    SRT_PDS_INET_SENT = 1u << 8,
    SRT_PDS_INET_DROPPED = 1u << 9,
    SRT_PDS_ROUTER_ENQUEUED = 1u << 10,
    SRT_PDS_ROUTER_DEQUEUED = 1u << 11,
    SRT_PDS_ROUTER_DROPPED = 1u << 12,
    SRT_PDS_RCV_INTERFACE_RECEIVED = 1u << 13,
    SRT_PDS_RCV_INTERFACE_DROPPED = 1u << 14,
    SRT_PDS_RCV_SOCKET_PROCESSED = 1u << 15, /* the UDP receive stage's three (packet.minimal.h:29-32) */
    SRT_PDS_RCV_SOCKET_DROPPED = 1u << 16,
    SRT_PDS_RCV_SOCKET_BUFFERED = 1u << 18,
    SRT_PDS_RELAY_CACHED = 1u << 21,
    SRT_PDS_RELAY_FORWARDED = 1u << 22
};

typedef struct {
    uint64_t round_end_ns;
    uint64_t bootstrap_end_ns;
    uint64_t sim_end_ns;
} srt_round;

/* Batched Worker::send_packet decision for one scheduling round, on the device.
 * All pointers are DEVICE pointers on the plan's device.  Packets must be
 * grouped by source host: host_pkt_ptr[h]..host_pkt_ptr[h+1] are host h's
 * packets in send order (n_hosts + 1 entries).  rng: 4 x u64 xoshiro256++ state
 * per host, advanced in place by one draw per non-completed packet.
 * flags/deliver: per packet.  counters (may be NULL): n*n u64 per-path packet
 * counts (RoutingInfo::increment_packet_count).  stats (device, 2 x u64):
 * [0] = min latency of sent packets (runahead), [1] = min deliver time
 * (next event time); both UINT64_MAX when nothing was sent, and they are
 * min-combined with their previous contents (initialise to UINT64_MAX). */
srt_status srt_packet_batch(srt_plan *plan, const srt_pkt *d_pkts, const uint32_t *d_host_pkt_ptr,
                            uint32_t n_hosts, uint64_t n_pkts, uint64_t *d_rng,
                            const srt_round *round, uint32_t *d_flags, uint64_t *d_deliver,
                            uint64_t *d_counters, uint64_t *d_stats, srt_err *err);

/* Batched Worker::push_packet_to_host (worker.rs:629-639) for the packets
 * srt_packet_batch marked SENT: each becomes Event::new_packet
 * (core/work/event.rs:20-31) whose src_host_event_id is its source host's
 * next event id (Host::get_new_event_id, host.rs:691-695) in send order, and
 * each destination host's events come out in its event queue's pop order:
 * deliver time, then source host id, then event id (event.rs:85-150).  Host
 * index order (the packet grouping of srt_packet_batch) is HostId order.
 * All pointers are DEVICE pointers.  dst_host: destination host of every
 * packet (< n_dst_hosts).  event_base: per source host, its next event id
 * (advanced in place by its number of sent packets).  Outputs: event_id per
 * packet (UINT64_MAX for packets not sent); order[0 .. n_sent): the sent
 * packets' indices grouped by destination host, each group in pop order;
 * dst_ptr[0 .. n_dst_hosts]: group offsets (dst_ptr[n_dst_hosts] = n_sent).
 * Asynchronous on the plan's stream (it never waits for the device): each
 * destination's group is sorted in on-chip memory; a group of more than 1024
 * events, or a sent packet whose destination is out of range, is flagged:
 * call srt_packet_events_status before reading the results (it redoes a batch
 * with a big group exactly).  The unsent tail of order[] is unspecified. */
srt_status srt_packet_events(srt_plan *plan, const uint32_t *d_host_pkt_ptr, uint32_t n_hosts, uint64_t n_pkts,
                             const uint32_t *d_flags, const uint64_t *d_deliver, const uint32_t *d_dst_host,
                             uint32_t n_dst_hosts, uint64_t *d_event_base, uint64_t *d_event_id,
                             uint32_t *d_order, uint32_t *d_dst_ptr, srt_err *err);
/* Synchronises the plan's stream: SRT_ERR_INVALID ("destination host index
 * out of range") if an srt_packet_events call since the last check met one;
 * if the last call had a destination group too big for the on-chip sort,
 * redoes that call's sort exactly (its arrays must still be valid) and
 * returns SRT_OK; else SRT_OK. */
srt_status srt_packet_events_status(srt_plan *plan, srt_err *err);

/* -------------------------------------------------------- in-flight store */
/* What joins the rounds to each other: Worker::send_packet clamps every
 * deliver time to the round's end or later (worker.rs:396-400), and
 * srt_inbound_run takes only the arrivals of its window, so the packets a
 * round's event push numbered wait here, on the device, until a window reaches
 * their deliver time.  The store keeps per packet its deliver time, source
 * host, event id, destination host, total size and a 64-bit tag of the
 * caller's (36 bytes), in one flat pool; a pop takes every stored packet with
 * deliver < until_ns and hands them out as one window's batch in final order:
 * grouped by destination host, each group in its event queue's pop order --
 * deliver time, then source host id, then event id (core/work/event.rs:85-150),
 * each compared as a full-width unsigned integer.  Event ids are unique per
 * source host, so the key is a total order and the outputs are a pure function
 * of the SET of stored packets; the order inside the pool is unspecified.
 * ABI: additive to version 4; detect the stage by its symbols. */
typedef struct srt_flight srt_flight;

#define SRT_FLIGHT_POOL_OVERFLOW   1u  /* more packets in flight than pool_cap: the excess is NOT stored (counted) */
#define SRT_FLIGHT_OUT_OVERFLOW    2u  /* more packets due than out_cap: the pop took NOTHING, the pool is unchanged */
#define SRT_FLIGHT_BAD_HOST        4u  /* a sent packet's dst_host >= n_dst_hosts: not stored */
#define SRT_FLIGHT_LATE_PUSH       8u  /* a pushed deliver time < the last pop's until_ns: stored, comes out at the next pop */
#define SRT_FLIGHT_TIME_REGRESSION 16u /* a pop's until_ns < the previous pop's */

/* A store for n_dst_hosts destination hosts and at most pool_cap (<= 2^31)
 * packets in flight, on the plan's device and stream, or, with plan == NULL,
 * host-only: every array argument of the other calls is then a HOST pointer
 * and the calls complete before they return.  Both forms run the same step.
 * Memory of the instance, in bytes, one allocation, nothing per call:
 *   pool_cap * 108 + ceil(n_dst_hosts / 2) * 8 + 56
 * (the pool twice, 2 * 36 bytes a packet: a pop compacts the survivors from one
 * half into the other; 32 bytes a packet of staging, where a window's records
 * lie grouped by destination before they are ordered, and 4 of its slot there;
 * per destination a count; the state words).  Destroy the instance before its
 * plan. */
srt_status srt_flight_create(srt_plan *plan, uint32_t n_dst_hosts, uint64_t pool_cap,
                             srt_flight **out, srt_err *err);

/* After srt_packet_events of a round, its arguments and outputs as they are:
 * d_host_pkt_ptr (n_src_hosts + 1 entries), n_pkts (< 2^31), d_flags,
 * d_deliver, d_dst_host and d_event_id, plus every packet's total size
 * (payload plus headers, what srt_inbound_run wants).  The store takes exactly
 * the packets with flags[p] == SRT_PDS_INET_SENT, the test the event push
 * applies; a packet's source host is the segment of host_pkt_ptr it lies in
 * (host index order is HostId order).  d_tag (may be NULL) is opaque and comes
 * back with the packet; without it the tag is the push's base + batch index,
 * the base being the running count of all earlier pushes' n_pkts, returned in
 * *tag_base (HOST pointer, may be NULL).  A destination >= n_dst_hosts is
 * flagged (BAD_HOST) and skipped.  A packet for which the pool has no room is
 * flagged (POOL_OVERFLOW) and counted in n_lost; nothing is written past the
 * pool, and which packets of an overflowing push are the lost ones is
 * unspecified.  A deliver time below the largest until_ns popped so far is
 * flagged (LATE_PUSH); the packet is stored and leaves with the next pop.
 * Asynchronous on the plan's stream: it never waits for the device. */
srt_status srt_flight_push(srt_flight *fl, const uint32_t *d_host_pkt_ptr, uint32_t n_src_hosts, uint64_t n_pkts,
                           const uint32_t *d_flags, const uint64_t *d_deliver, const uint32_t *d_dst_host,
                           const uint64_t *d_event_id, const uint32_t *d_total_size,
                           const uint64_t *d_tag /* may be NULL: tag_base + batch index */,
                           uint64_t *tag_base /* host pointer, may be NULL, like seq_base elsewhere */, srt_err *err);

/* One window: every stored packet with deliver < until_ns leaves the store.
 * Outputs, out_cap entries each but d_w_dst_ptr (n_dst_hosts + 1): the group
 * offsets d_w_dst_ptr (d_w_dst_ptr[n_dst_hosts] = the number popped), and in
 * final order d_w_deliver, d_w_total_size, d_w_src_host, d_w_event_id, d_w_tag;
 * d_w_order is the identity 0 .. n_popped, so that d_w_order, d_w_dst_ptr,
 * d_w_deliver and d_w_total_size go into srt_inbound_run as they are with
 * n_pkts = out_cap (the inbound stage bounds its walk by min(dst_ptr[n_hosts],
 * n_pkts) on the device): no host round trip between the two calls.  Entries
 * past the number popped are not written.  If more packets are due than
 * out_cap the pop is void: nothing leaves, every d_w_dst_ptr entry is 0, the
 * call is flagged (OUT_OVERFLOW) and srt_flight_status reports the true due
 * count in n_popped, so that the caller can pop again with room; there is no
 * partial window.  Survivors stay.  until_ns must not decrease (a smaller one
 * is flagged TIME_REGRESSION and still takes what lies before it).  A
 * destination group of any size comes out exact in the same call; one of more
 * than 256 packets is ranked in quadratic time by one workgroup.
 * Asynchronous on the plan's stream: it never waits for the device. */
srt_status srt_flight_pop(srt_flight *fl, uint64_t until_ns,
                          uint32_t *d_w_order, uint32_t *d_w_dst_ptr /* n_dst_hosts + 1 */,
                          uint64_t *d_w_deliver, uint32_t *d_w_total_size, uint32_t *d_w_src_host,
                          uint64_t *d_w_event_id, uint64_t *d_w_tag, uint64_t out_cap, srt_err *err);

/* Synchronises the stream.  *flags (may be NULL): the SRT_FLIGHT_* conditions
 * met since the last status call (then cleared); *n_popped: the last pop's due
 * count, void or not; *n_stored: packets in the store; *n_lost: packets lost to
 * POOL_OVERFLOW since create (all may be NULL).  SRT_ERR_INVALID, with a message
 * that names every flag set, when any was; else SRT_OK. */
srt_status srt_flight_status(srt_flight *fl, uint32_t *flags, uint64_t *n_popped, uint64_t *n_stored,
                             uint64_t *n_lost, srt_err *err);
void srt_flight_destroy(srt_flight *fl);

/* --------------------------------------------------- inbound router stage */
/* What the destination host does with the packet events srt_packet_events
 * ordered, batched over hosts: each packet event pushes its packet into the
 * host's upstream Router, a CoDel queue (network/router/mod.rs:57-61,
 * router/codel_queue.rs: TARGET 10 ms, INTERVAL 100 ms, no length limit), and
 * the host's relay_inet_in drains that queue into the network interface under
 * a token bucket sized from bandwidth_down (network/relay/mod.rs:200-287,
 * relay/token_bucket.rs: 1 ms refills of max(1, bytes_per_second / 1000),
 * capacity one refill + CONFIG_MTU; host.rs:303-305, 855-858, 977-979).  At
 * one host, events run in time order and at equal times every packet event
 * runs before the relay's forward task (core/work/event.rs:102-110).  The
 * stage decides which packets the router drops (ROUTER_DROPPED) and when every
 * other packet reaches the interface (RELAY_FORWARDED at forward_ns); it is
 * exact, state included, and a pure function of the arrival order, the deliver
 * times, the packet sizes and each host's download bandwidth.
 * OUT OF SCOPE: the CPU-delay model that reschedules events (host.rs:820-848),
 * the loopback relay (is_local is always false here; the outbound relay is the
 * srt_outbound stage below), and what a TCP socket does with the packet: the
 * interface's receive side up to the socket hand-off is the srt_deliver stage
 * below, a UDP socket's receive buffer and reads the srt_udprecv stage.
 * ABI: additive to version 4; detect the stage by its symbols. */
typedef struct srt_inbound srt_inbound;

/* a packet of an EARLIER call that left the stage in this one */
typedef struct {
    uint64_t seq;        /* its call's seq_base + its batch index */
    uint64_t forward_ns; /* UINT64_MAX unless forwarded */
    uint32_t status;     /* SRT_PDS_* */
    uint32_t dst_host;
} srt_inbound_late;

/* one host's state (tests, checkpoints, event-id accounting) */
typedef struct {
    uint64_t balance;             /* TokenBucket */
    uint64_t last_refill_ns;
    uint64_t interval_end_ns;     /* CoDelQueue; UINT64_MAX = None */
    uint64_t drop_next_ns;        /* UINT64_MAX = None */
    uint64_t current_drop_count;
    uint64_t previous_drop_count;
    uint64_t queue_len;           /* packets in the CoDel queue */
    uint64_t bytes_stored;
    uint64_t task_ns;             /* pending forward task; UINT64_MAX = relay Idle */
    uint64_t tasks_scheduled;     /* forward tasks scheduled so far: each took one of the
                                     host's event ids (Host::get_new_event_id) */
    uint32_t mode;                /* 0 Store, 1 Drop */
    uint32_t cached;              /* 1: the relay holds a cached next_packet */
    uint32_t overflow;            /* 1: this host's ring overflowed, its results are invalid */
    uint32_t reserved0;
} srt_inbound_host_state;

/* srt_inbound_status flags */
#define SRT_INBOUND_RING_OVERFLOW 1u   /* a host held more unresolved packets than queue_cap */
#define SRT_INBOUND_LATE_OVERFLOW 2u   /* more late records than late_cap (the rest are lost) */
#define SRT_INBOUND_TIME_REGRESSION 4u /* an arrival earlier than the previous call's until_ns */
#define SRT_INBOUND_OVERSIZE 8u        /* a packet larger than its host's token bucket can hold: the
                                          reference would reschedule it for ever; here its forward
                                          task is tried once a call (task_ns moved to until_ns) */
#define SRT_INBOUND_AFTER_UNTIL 16u    /* an arrival at or after until_ns: not taken (status 0) */

/* State for n_hosts destination hosts on the plan's device and stream, or,
 * with plan == NULL, a host-only instance: every array argument of the other
 * calls is then a HOST pointer and the calls complete before they return.
 * Both forms run the same per-host step.  bw_down_bytes_per_s: HOST pointer,
 * each host's requested bandwidth_down in bits / 8.  queue_cap: packets a
 * host may hold unresolved (queued) across calls; the rings take
 * n_hosts * queue_cap * 24 bytes.  Buckets start full, last refill at 0.
 * Destroy the instance before its plan (it runs on the plan's stream). */
srt_status srt_inbound_create(srt_plan *plan, uint32_t n_hosts, const uint64_t *bw_down_bytes_per_s,
                              uint32_t queue_cap, srt_inbound **out, srt_err *err);
/* One scheduling window.  d_order / d_dst_ptr: srt_packet_events' outputs
 * (dst_ptr has n_hosts + 1 entries, n_hosts as at create); d_deliver: the
 * deliver times; d_total_size: every packet's payload plus headers; all
 * indexed by batch index, n_pkts of them (order[] holds dst_ptr[n_hosts]).
 * The batch's arrivals must lie in the window [previous call's until_ns,
 * until_ns): every one of them is pushed at its deliver time and every forward
 * task with a time < until_ns runs.  An earlier arrival is flagged
 * (TIME_REGRESSION); an arrival at or after until_ns belongs to a later window
 * and is NOT taken -- its status stays 0, it is not pending, and the call is
 * flagged (AFTER_UNTIL) so that the caller feeds it again with that window.
 * Before bootstrap_end_ns the bucket is not touched (worker.rs:489-491).
 * Outputs, per batch packet: d_status (0 for a packet that is not in
 * order[] or was not taken; ENQUEUED | DROPPED; ENQUEUED | DEQUEUED | FORWARDED, plus CACHED
 * if the relay ever held it back; still in the stage at until_ns: ENQUEUED,
 * or ENQUEUED | DEQUEUED | CACHED for the relay's cached packet) and
 * d_forward_ns (UINT64_MAX unless forwarded).  A packet still in the stage
 * stays there under the sequence number *seq_base + batch index (seq_base,
 * host pointer, may be NULL: the running count of all earlier calls' n_pkts).
 * Packets of earlier calls that leave in this one are appended to d_late
 * (late_cap records, any order) and counted in *d_late_count (written by the
 * call; beyond late_cap: SRT_INBOUND_LATE_OVERFLOW).
 * Asynchronous on the plan's stream, like srt_packet_events. */
srt_status srt_inbound_run(srt_inbound *ib, const uint32_t *d_order, const uint32_t *d_dst_ptr,
                           const uint64_t *d_deliver, const uint32_t *d_total_size, uint64_t n_pkts,
                           uint64_t until_ns, uint64_t bootstrap_end_ns, uint32_t *d_status,
                           uint64_t *d_forward_ns, srt_inbound_late *d_late, uint32_t late_cap,
                           uint32_t *d_late_count, uint64_t *seq_base, srt_err *err);
/* Synchronises the stream.  *flags (may be NULL): the SRT_INBOUND_* conditions
 * met since the last status call (then cleared); *n_pending (may be NULL):
 * packets still in the stage.  SRT_ERR_INVALID when a flag is set (a ring
 * overflow never writes out of bounds: the host is marked in its state and
 * only its results are invalid), else SRT_OK. */
srt_status srt_inbound_status(srt_inbound *ib, uint32_t *flags, uint64_t *n_pending, srt_err *err);
/* Synchronises and copies every host's state to out[n_hosts] (HOST pointer). */
srt_status srt_inbound_state(srt_inbound *ib, srt_inbound_host_state *out, srt_err *err);
/* apply_control_law's increment, round(1e8 / sqrt(count)) in f64 with count 0
 * as 1 (codel_queue.rs:287-300), for counts[0 .. n) (HOST pointers), evaluated
 * where the instance runs (on the device for a plan's instance).  use_table
 * != 0: as the stage evaluates it (a host-built table below 1024, f64 above);
 * 0: the f64 path for every count. */
srt_status srt_inbound_control_law(srt_inbound *ib, const uint64_t *counts, uint64_t n, int use_table,
                                   uint64_t *increments, srt_err *err);
void srt_inbound_destroy(srt_inbound *ib);

/* ----------------------------------------------- interface receive stage */
/* What the destination host's interface does with the packets the inbound
 * router forwarded, batched over hosts: networkinterface_push
 * (host/network/network_interface.c:140-202, called from
 * Relay::forward_until_blocked, network/relay/mod.rs:260-270) marks the packet
 * RCV_INTERFACE_RECEIVED, looks its socket up in the host's associations --
 * the specific key (protocol, destination port, source ip, source port) first,
 * then the wildcard (protocol, destination port, 0, 0) -- and hands the packet
 * to that socket, or marks it RCV_INTERFACE_DROPPED.  One call takes ONE
 * srt_inbound_run call's results (per-packet status / forward_ns in window
 * order, and the late list) and returns the per-host delivery list: exactly
 * the packets with RELAY_FORWARDED, grouped by destination host, each host's
 * in the order its interface receives them, which is the relay's forward order
 * and the CoDel queue's FIFO order -- the host's late packets by ascending seq,
 * then its batch packets by ascending position in the window -- each with its
 * socket.  forward_ns is nondecreasing along every host's list for results of
 * a correct inbound call (an invariant, not a sort key).  Windows are taken in
 * final order (order[] the identity, as srt_flight_pop emits them), so the
 * stage needs only d_dst_ptr and a packet's seq is seq_base + its position.
 * The lookup uses the associations AS THEY STAND AT THE CALL, for late packets
 * too: the reference looks up at push time, not at enqueue time.  Key fields
 * are compared verbatim as integers (ports and addresses in network byte
 * order).  A packet whose peer is 0:0 hits the wildcard key on the first probe,
 * as in the reference, where the two keys are the same string.
 * LIMIT: associations change only between calls.  The reference can associate
 * or disassociate as a consequence of a delivery inside the window (a TCP
 * close, say); a caller that disassociates a socket mid-window must treat the
 * window's later deliveries to that socket as the lookup would, or split the
 * window there.
 * OUT OF SCOPE: what a TCP socket does with the packet, the loopback relay,
 * the CPU-delay model.  (A UDP socket's receive buffer and its reads are the
 * srt_udprecv stage below, which takes this stage's list as it is; the
 * tracker's byte counts of the internet interface are the srt_tracker stage,
 * pcap capture the srt_pcap stage.)
 * ABI: additive to version 4; detect the stage by its symbols. */
typedef struct srt_deliver srt_deliver;

#define SRT_PROTO_TCP 1u /* ProtocolType PTCP (host/protocol.h:11) */
#define SRT_PROTO_UDP 2u /* PUDP */

/* what the lookup needs from a packet, 16 bytes; `user` is opaque and comes back */
typedef struct {
    uint32_t peer_ip_be;    /* the packet's source address */
    uint16_t peer_port_be;  /* its source port */
    uint16_t local_port_be; /* its destination port */
    uint32_t protocol;      /* SRT_PROTO_*; any other value matches no association */
    uint32_t user;
} srt_rx_meta;

/* one socket association of a host's interface, 20 bytes; the wildcard has peer 0:0 */
typedef struct {
    uint32_t host;
    uint32_t protocol; /* SRT_PROTO_TCP or SRT_PROTO_UDP */
    uint32_t peer_ip_be;
    uint16_t local_port_be;
    uint16_t peer_port_be;
    uint32_t socket; /* < 2^31, the caller's name for the socket */
} srt_assoc;

#define SRT_DELIVER_OUT_OVERFLOW 1u /* more delivered packets than out_cap: nothing past out_cap written */
#define SRT_DELIVER_LOG_OVERRUN  2u /* a late packet's seq is older than the log holds: a placeholder record */
#define SRT_DELIVER_NOTE_OVERRUN 4u /* a tag the note ring no longer (or not yet) holds: a placeholder record */
#define SRT_DELIVER_BAD_HOST     8u /* a late record's dst_host >= n_hosts: skipped */

/* An instance for n_hosts destination hosts on the plan's device and stream,
 * or, with plan == NULL, host-only: every array argument named d_ is then a
 * HOST pointer and the calls complete before they return.  Both forms run the
 * same step.  Memory of the instance, in bytes:
 *   32 + n_hosts * 12 + note_cap * 16 + log_cap * 32 + slots * 16
 * (the state words; per host three counts; the note ring of srt_rx_meta; the
 * seq log of {tag, meta, valid}; the association table, slots being the
 * smallest power of two >= max(table_slots_min, 2) that keeps the load at or
 * below 1/2 -- it doubles when the associations outgrow it and never shrinks),
 * on the device, plus the table once more in pinned host memory and the
 * authoritative associations on the host.  Nothing is allocated per call; only
 * the first run after the table has doubled waits for the stream and
 * reallocates the device copy.  note_cap and log_cap are at most 2^31.
 * Destroy the instance before its plan. */
srt_status srt_deliver_create(srt_plan *plan, uint32_t n_hosts, uint32_t table_slots_min, uint64_t note_cap,
                              uint64_t log_cap, srt_deliver **out, srt_err *err);

/* networkinterface_associate / networkinterface_disassociate
 * (network_interface.c:77-116) for a batch of n associations (HOST pointer),
 * between calls of srt_deliver_run.  The authoritative table lives on the
 * host; the device copy is rebuilt on the host and uploaded on the stream by
 * the next srt_deliver_run, and only when the associations have changed since
 * the last upload.  associate: a key that exists already -- in the table or
 * twice in the batch -- a host >= n_hosts, a socket >= 2^31 or a protocol that
 * is neither SRT_PROTO_TCP nor SRT_PROTO_UDP returns SRT_ERR_INVALID and
 * changes NOTHING (the reference asserts there is no collision).
 * disassociate: the socket field is ignored and a missing key is a no-op (the
 * reference tolerates it, network_interface.c:106-112). */
srt_status srt_deliver_associate(srt_deliver *dl, const srt_assoc *assoc, uint64_t n, srt_err *err);
srt_status srt_deliver_disassociate(srt_deliver *dl, const srt_assoc *assoc, uint64_t n, srt_err *err);

/* The lookup of the stage for n (host, meta) pairs against the same table, on
 * the host (HOST pointers): sockets[k] is the socket, or UINT32_MAX.  For
 * packets that never reach the inbound stage (SRT_OUT_LOCAL), and for tests. */
srt_status srt_deliver_lookup(srt_deliver *dl, const uint32_t *hosts, const srt_rx_meta *meta, uint64_t n,
                              uint32_t *sockets, srt_err *err);

/* The same lookup for n (< 2^31) records in device arrays, asynchronous on the
 * plan's stream: the table is uploaded first if the associations have changed
 * since the last upload, as srt_deliver_run does it, then one thread a record
 * probes it.  A host >= n_hosts gives UINT32_MAX.  On a host-only instance it
 * is srt_deliver_lookup.  With it the SRT_OUT_LOCAL packets of an outbound
 * call go to srt_tracker_rx_flat without a read-back.  KNOWN GAP: the order of
 * those packets among themselves stays the caller's; srt_outbound_run returns
 * their send time and no rank. */
srt_status srt_deliver_lookup_flat(srt_deliver *dl, const uint32_t *d_hosts, const srt_rx_meta *d_meta, uint64_t n,
                                   uint32_t *d_sockets, srt_err *err);

/* The table as the next run sees it (all may be NULL): associations, slots,
 * the longest probe sequence of a stored key (1: every key in its home slot)
 * and whether a chain runs past the table's end. */
srt_status srt_deliver_table_stats(srt_deliver *dl, uint64_t *n_assoc, uint32_t *n_slots, uint32_t *max_probe,
                                   uint32_t *wrapped, srt_err *err);

/* After a round's srt_flight_push with d_tag == NULL: the round's metas, d_meta[i]
 * for batch packet i, whose tag is tag_base + i (tag_base as the push returned
 * it), go into the instance's ring at tag % note_cap.  tag_base must not lie
 * below the previous note's end (SRT_ERR_INVALID).  A tag is readable iff tag <
 * note_end && note_end - tag <= note_cap, note_end being the last note's
 * tag_base + n_pkts: size note_cap to the packets pushed while a packet may be
 * in flight or in its window.  n_pkts < 2^31.  Asynchronous on the plan's
 * stream. */
srt_status srt_deliver_note(srt_deliver *dl, const srt_rx_meta *d_meta, uint64_t n_pkts, uint64_t tag_base,
                            srt_err *err);

/* One delivery, for the srt_inbound_run call just made.  d_dst_ptr (n_hosts + 1
 * entries) and d_tag are srt_flight_pop's d_w_dst_ptr and d_w_tag, d_status and
 * d_forward_ns the inbound call's outputs, seq_base the value it returned,
 * d_late / late_cap (< 2^31) / d_late_count its late list, of which
 * min(*d_late_count, late_cap) records are used.  n_pkts (< 2^31) is the
 * inbound call's n_pkts and may be the flight pop's out_cap: the walk is
 * bounded by walked = min(d_dst_ptr[n_hosts], n_pkts) on the device, so there
 * is no host round trip between pop, inbound and deliver.
 * Outputs: d_out_host_ptr[0 .. n_hosts] is the grouping, [n_hosts] the number
 * delivered; parallel to it in delivery order d_out_socket (UINT32_MAX: no
 * socket), d_out_forward_ns, d_out_tag, d_out_user and d_out_status (the
 * inbound status plus RCV_INTERFACE_RECEIVED, and RCV_INTERFACE_DROPPED when
 * no socket took the packet), out_cap entries each.  With more delivered
 * packets than out_cap the call is flagged OUT_OVERFLOW, nothing is written
 * past out_cap and every d_out_host_ptr entry is held at out_cap at most, so
 * that a consumer stays inside the arrays; the records of such a call, and
 * which of the record flags below it raises, are unspecified, and
 * srt_deliver_status still reports the true count.
 * The seq log: a batch packet that stays in the inbound stage (ROUTER_ENQUEUED
 * without RELAY_FORWARDED or ROUTER_DROPPED) has {tag, meta} written at
 * (seq_base + i) % log_cap iff walked - i <= log_cap; a late packet's record is
 * read back iff seq_base + n_pkts - seq <= log_cap, else the call is flagged
 * LOG_OVERRUN.  Both are distances from the end of the call's range, so a slot
 * read is never one this call writes.  Size log_cap to the sequence numbers
 * handed out (n_pkts a call) while a packet may stay queued.
 * Placeholders: a delivered packet whose meta cannot be had -- LOG_OVERRUN, or
 * NOTE_OVERRUN, when its tag was not readable in the note ring at this call
 * (batch) or at the call that logged it (late; both calls are flagged) -- is
 * emitted in its place with socket = UINT32_MAX, user = UINT32_MAX, the inbound
 * status unchanged (no RCV_ bit: not looked up) and tag = UINT64_MAX if the tag
 * is lost too.  A late record with dst_host >= n_hosts is flagged BAD_HOST and
 * skipped.  Every write is range-checked first: a flagged call never writes
 * out of bounds.  A host's late run of any length comes out ordered in the
 * same call; one of more than 256 records is ranked in quadratic time by one
 * workgroup.
 * Asynchronous on the plan's stream: it never waits for the device and reads
 * nothing back. */
srt_status srt_deliver_run(srt_deliver *dl, const uint32_t *d_dst_ptr, uint64_t n_pkts, const uint64_t *d_tag,
                           const uint32_t *d_status, const uint64_t *d_forward_ns, uint64_t seq_base,
                           const srt_inbound_late *d_late, uint32_t late_cap, const uint32_t *d_late_count,
                           uint32_t *d_out_host_ptr, uint32_t *d_out_socket, uint64_t *d_out_forward_ns,
                           uint64_t *d_out_tag, uint32_t *d_out_user, uint32_t *d_out_status, uint64_t out_cap,
                           srt_err *err);
/* Synchronises the stream.  *flags (may be NULL): the SRT_DELIVER_* conditions
 * met since the last status call (then cleared); *n_delivered: the last run's
 * delivered packets; *n_no_socket: those of them (written) that no socket took
 * (both may be NULL; the device form sums the hosts' counts here, with one
 * launch, so that no kernel of a run adds to a call-wide counter).
 * SRT_ERR_INVALID, with a message that names every flag set, when any was;
 * else SRT_OK. */
srt_status srt_deliver_status(srt_deliver *dl, uint32_t *flags, uint64_t *n_delivered, uint64_t *n_no_socket,
                              srt_err *err);
void srt_deliver_destroy(srt_deliver *dl);

/* --------------------------------------------------- outbound relay stage */
/* What the source host does before Worker::send_packet, batched over hosts:
 * the step that produces srt_pkt.t_ns and the per-host send order
 * srt_packet_batch requires.  When a socket has data,
 * notify_socket_has_packets (host/host.rs:988-1002) puts the socket into the
 * interface's queuing discipline unless it is there already
 * (networkinterface_wantsSend, host/network/network_interface.c:344-370) and
 * notifies relay_inet_out: an Idle relay schedules its forward task at the
 * current time (one host event id).  The task (Relay::forward_until_blocked,
 * network/relay/mod.rs:200-272) takes the relay's cached packet if it holds
 * one, else pops the interface (network_interface.c:205-340,
 * network_queuing_disciplines.c):
 *   FIFO (Q_DISC_MODE_FIFO, the default): of the sockets in the queue, the one
 *     whose NEXT packet has the smallest priority (Host::get_next_packet_priority,
 *     host.rs:715: distinct within a host); only socket heads are compared, a
 *     socket is a FIFO of its packets whatever their priorities.  Equal
 *     priorities within a host are a caller error: taken in arrival order.
 *   round robin: the socket at the head of a plain queue, pushed to its tail
 *     again if it still has data.
 * The popped packet gets INTERFACE_SENT.  A packet whose destination is the
 * interface's own address (SRT_OUT_LOCAL) is exempt from the bucket and is
 * pushed back into the interface; every other packet, unless now <
 * bootstrap_end_ns, needs conforming_remove(total_size) of a token bucket
 * sized from bandwidth_up (host.rs:299-302, relay/mod.rs:277-287,
 * relay/token_bucket.rs: 1 ms refills of max(1, bytes_per_second / 1000),
 * capacity one refill + CONFIG_MTU, full at time 0): if that fails the packet
 * is cached (RELAY_CACHED) and the task rescheduled after the returned
 * duration (one more event id), else it gets RELAY_FORWARDED and goes through
 * Router::push to Worker::send_packet at that moment (router/mod.rs:49-55,
 * 74-77): send_ns is srt_pkt.t_ns.
 * Event order at one host, the stage's contract: events run in time order, and
 * at equal times every arrival (socket-has-data), in the caller's list order,
 * runs before the forward task.  LIMIT: the reference orders local events of
 * equal time by event id, which the library does not own; a caller whose
 * socket-has-data events can follow a forward task of the same time must split
 * the window there.
 * The stage is exact, state included, and a pure function of each host's
 * arrival list (ready_ns, socket, priority, size, local flag), the qdisc and
 * bandwidth_up.
 * OUT OF SCOPE: how sockets produce packets (TCP buffers, retransmission; UDP's
 * send buffers are the srt_udpsend stage below, which holds this relay inside
 * it) and the CPU-delay model that reschedules events.  The loopback interface is
 * srt_loopback below.  A local packet pushed back into the interface is
 * received as srt_deliver_run receives a forwarded one: srt_deliver_lookup, or
 * srt_deliver_lookup_flat on the device, resolves its socket.
 * ABI: additive to version 4; detect the stage by its symbols. */
typedef struct srt_outbound srt_outbound;

#define SRT_QDISC_FIFO 0
#define SRT_QDISC_RR 1
#define SRT_OUT_LOCAL 1u /* srt_out_pkt.flags: destination is the interface's own address */

/* one packet a socket hands to the interface, 32 bytes */
typedef struct {
    uint64_t ready_ns;   /* time of the socket-has-data event */
    uint64_t priority;   /* Host::get_next_packet_priority value */
    uint32_t total_size; /* payload plus headers */
    uint32_t socket;     /* < max_sockets, an index local to the host */
    uint32_t flags;      /* SRT_OUT_LOCAL */
    uint32_t reserved;
} srt_out_pkt;

/* a packet of an EARLIER call that was forwarded in this one, 32 bytes */
typedef struct {
    uint64_t seq;       /* its call's seq_base + its batch index */
    uint64_t send_ns;
    uint64_t send_rank; /* UINT64_MAX for a local packet */
    uint32_t status;    /* SRT_PDS_* */
    uint32_t src_host;
} srt_outbound_late;

/* one host's state (tests, checkpoints, event-id accounting) */
typedef struct {
    uint64_t balance;         /* TokenBucket */
    uint64_t last_refill_ns;
    uint64_t task_ns;         /* pending forward task; UINT64_MAX = relay Idle */
    uint64_t tasks_scheduled; /* forward tasks scheduled so far: each took one host event id */
    uint64_t sent_total;      /* non-local packets forwarded so far = the next send_rank */
    uint64_t queue_len;       /* packets in the socket queues */
    uint32_t cached;          /* 1: the relay holds a cached next_packet */
    uint32_t overflow;        /* 1: this host's ring overflowed, its results are invalid */
} srt_outbound_host_state;

/* srt_outbound_status flags */
#define SRT_OUTBOUND_RING_OVERFLOW 1u   /* a host held more unresolved packets than queue_cap */
#define SRT_OUTBOUND_LATE_OVERFLOW 2u   /* more late records than late_cap (the rest are lost) */
#define SRT_OUTBOUND_TIME_REGRESSION 4u /* an arrival earlier than the previous call's until_ns */
#define SRT_OUTBOUND_OVERSIZE 8u        /* a non-local packet larger than its host's token bucket can
                                           hold: the reference would reschedule it for ever; here
                                           its forward task is tried once a call (task_ns moved to
                                           until_ns) */
#define SRT_OUTBOUND_AFTER_UNTIL 16u    /* an arrival at or after until_ns: not taken (status 0) */
#define SRT_OUTBOUND_BAD_SOCKET 32u     /* socket >= max_sockets: the packet is not taken (status 0) */

/* State for n_hosts source hosts on the plan's device and stream, or, with
 * plan == NULL, a host-only instance: every array argument of the other calls
 * is then a HOST pointer and the calls complete before they return.  Both
 * forms run the same per-host step.  bw_up_bytes_per_s: HOST pointer, each
 * host's requested bandwidth_up in bits / 8.  qdisc: SRT_QDISC_*, one for all
 * hosts.  max_sockets: sockets a host may name.  queue_cap (< 2^31 - 2):
 * packets a host may hold unresolved in its socket queues across calls.
 * Memory of the instance, in bytes:
 *   n_hosts * (96 + queue_cap * 32 + max_sockets * 12)
 * (state record; ring of carried-over packets; per socket an 8-byte head /
 * tail cursor and a 4-byte slot of the qdisc's socket queue), plus 4 bytes a
 * packet of the largest batch seen (the per-socket links).  Buckets start
 * full, last refill at 0.  Destroy the instance before its plan. */
srt_status srt_outbound_create(srt_plan *plan, uint32_t n_hosts, const uint64_t *bw_up_bytes_per_s, uint32_t qdisc,
                               uint32_t max_sockets, uint32_t queue_cap, srt_outbound **out, srt_err *err);
/* One scheduling window.  d_pkts: n_pkts (< 2^31) packets grouped by source
 * host, d_host_ptr[h] .. d_host_ptr[h+1] being host h's (n_hosts + 1 entries),
 * each host's in arrival order with nondecreasing ready_ns inside [previous
 * call's until_ns, until_ns).  Every arrival is pushed at its ready_ns and
 * every forward task with a time < until_ns runs.  An earlier arrival is
 * flagged (TIME_REGRESSION); an arrival at or after until_ns is NOT taken
 * (status 0, not pending, AFTER_UNTIL) and must be fed again with its window,
 * as must a packet with a bad socket once corrected.
 * Outputs, per batch packet: d_status (0: not taken, or still in a socket
 * queue and counted pending; INTERFACE_SENT | RELAY_CACHED: the relay's cached
 * packet at until_ns; INTERFACE_SENT | RELAY_FORWARDED, plus RELAY_CACHED if it
 * was ever held back: forwarded), d_send_ns (the forward time, UINT64_MAX
 * unless forwarded) and d_send_rank (the packet's position in its host's whole
 * send sequence since create: the counter is per host, continues across calls
 * and is advanced only by non-local forwarded packets; UINT64_MAX for local or
 * unforwarded packets).  Sorting a round's forwarded non-local packets, late
 * ones included, by (source host, send_rank) gives the send order
 * srt_packet_batch needs (srt_sendbatch_run below builds that batch on the
 * device, without a sort).  A packet still in the stage stays there under the
 * sequence number *seq_base + batch index (seq_base: host pointer, may be
 * NULL).  Packets of earlier calls that are forwarded in this one are appended
 * to d_late (late_cap records, any order) and counted in *d_late_count (written
 * by the call; beyond late_cap: SRT_OUTBOUND_LATE_OVERFLOW).
 * Asynchronous on the plan's stream, like srt_inbound_run. */
srt_status srt_outbound_run(srt_outbound *ob, const srt_out_pkt *d_pkts, const uint32_t *d_host_ptr, uint64_t n_pkts,
                            uint64_t until_ns, uint64_t bootstrap_end_ns, uint32_t *d_status, uint64_t *d_send_ns,
                            uint64_t *d_send_rank, srt_outbound_late *d_late, uint32_t late_cap,
                            uint32_t *d_late_count, uint64_t *seq_base, srt_err *err);
/* Synchronises the stream.  *flags (may be NULL): the SRT_OUTBOUND_* conditions
 * met since the last status call (then cleared); *n_pending (may be NULL):
 * packets still in the stage.  SRT_ERR_INVALID when a flag is set (a ring
 * overflow never writes out of bounds: the host is marked in its state and
 * only its results are invalid), else SRT_OK. */
srt_status srt_outbound_status(srt_outbound *ob, uint32_t *flags, uint64_t *n_pending, srt_err *err);
/* Synchronises and copies every host's state to out[n_hosts] (HOST pointer). */
srt_status srt_outbound_state(srt_outbound *ob, srt_outbound_host_state *out, srt_err *err);
/* d_seq[h] (n_hosts entries) = the sequence number of the packet host h's relay
 * holds cached at the end of the last srt_outbound_run, or UINT64_MAX when it
 * holds none.  Asynchronous on the plan's stream (host-only: a plain loop).
 * For srt_tracker_tx below. */
srt_status srt_outbound_cached_seq(srt_outbound *ob, uint64_t *d_seq, srt_err *err);
void srt_outbound_destroy(srt_outbound *ob);

/* ------------------------------------------------------ send-batch gather */
/* From srt_outbound_run's results to srt_packet_batch's input, on the device:
 * the forwarded non-local packets of one outbound call, late ones included,
 * as srt_pkt records grouped by source host, each host's in send_rank order,
 * with t_ns = send_ns.  No sort is involved: within one srt_outbound_run call
 * every rank a host hands out comes from its one counter, so a host's ranks of
 * the call are one contiguous run [first, first + count) and a packet's place
 * is host_base[h] + (rank - first[h]): a count and a minimum per host, a scan
 * over the hosts, a scatter.  The arrays of ONE outbound call go in together;
 * mixing calls breaks the run and is flagged (RANK_GAP).
 * ABI: additive to version 4; detect the stage by its symbols. */

/* what srt_pkt needs beyond what the outbound stage returns, 16 bytes */
typedef struct { uint32_t src_row, dst_row, payload_size, user; } srt_send_meta;
typedef struct srt_sendbatch srt_sendbatch;

#define SRT_SENDBATCH_OUT_OVERFLOW 1u /* more sent packets than out_cap: nothing past out_cap written */
#define SRT_SENDBATCH_RANK_GAP     2u /* a host's ranks are not one contiguous run (arrays of different calls mixed) */
#define SRT_SENDBATCH_LOG_OVERRUN  4u /* a late packet's seq is older than the log holds */
#define SRT_SENDBATCH_BAD_HOST     8u /* a late record's src_host >= n_hosts: skipped */

/* An instance for n_hosts source hosts on the plan's device and stream, or,
 * with plan == NULL, host-only: every array argument of srt_sendbatch_run is
 * then a HOST pointer and the calls complete before they return.  Both forms
 * run the same step.  The instance owns a log of log_cap srt_send_meta records
 * (16 bytes each) and 12 bytes of scratch a host; nothing is allocated per
 * call.  Destroy the instance before its plan. */
srt_status srt_sendbatch_create(srt_plan *plan, uint32_t n_hosts, uint64_t log_cap,
                                srt_sendbatch **out, srt_err *err);
/* One gather, for the srt_outbound_run call just made: d_host_ptr, n_pkts
 * (< 2^31), d_send_ns and d_send_rank are that call's arguments and outputs,
 * seq_base the value it returned, d_late / late_cap (< 2^31) / d_late_count its
 * late list, of which min(*d_late_count, late_cap) records are used (the count
 * runs past the cap on overflow).  d_meta[i] belongs to batch packet i; `user`
 * is opaque and comes back in d_out_user (typically the destination host
 * srt_packet_events wants).
 * The log keeps the meta of packets that stay in the outbound stage, addressed
 * by seq % log_cap.  A batch packet without a rank (send_rank == UINT64_MAX:
 * not forwarded in this call, or local) has its meta written at seq_base + i,
 * provided n_pkts - i <= log_cap; a late packet's meta is read back from the
 * log, and its seq is valid iff seq_base + n_pkts - seq <= log_cap, else the
 * call is flagged LOG_OVERRUN and the record is emitted with rows 0, payload 0
 * and user = UINT32_MAX.  The rule measures the distance from the END of this
 * call's sequence range, so a slot it reads is never one this call writes: it
 * does not depend on the order of the call's own writes.  Size log_cap to the
 * packets fed while a packet may stay queued (queue_cap packets a host at
 * most, over however many calls they take to drain).
 * Outputs: d_out_host_ptr[0 .. n_hosts] is the grouping, [n_hosts] the number
 * of sent packets; d_out_pkts[k] = {src_host, src_row, dst_row, payload_size,
 * t_ns = send_ns} in send order; d_out_user and d_out_seq are parallel to it
 * (seq_base + index for a batch packet, the late record's seq for a late one:
 * the caller can carry anything else along by it).  src_row and dst_row are
 * copied verbatim, so with addresses in them the same output is the srt_pkt_ip
 * input of srt_packet_batch_ip.  At most out_cap records are written; with
 * more sent packets the call is flagged OUT_OVERFLOW and every entry of
 * d_out_host_ptr is held at out_cap, so that a consumer stays inside the
 * arrays (srt_sendbatch_status still reports the true count).
 * Every write is range-checked first (rank - first < count, position <
 * out_cap, src_host < n_hosts): a flagged call never writes out of bounds.
 * No host round trip is needed before the send decision: srt_packet_batch
 * launches by hosts and reads packets only through its host_pkt_ptr, its n_pkts
 * only sizes scratch, so the caller may pass out_cap there, with d_flags and
 * d_deliver of out_cap entries.
 * Asynchronous on the plan's stream: it never waits for the device. */
srt_status srt_sendbatch_run(srt_sendbatch *sb, const uint32_t *d_host_ptr, uint64_t n_pkts,
                             const srt_send_meta *d_meta, const uint64_t *d_send_ns,
                             const uint64_t *d_send_rank, uint64_t seq_base,
                             const srt_outbound_late *d_late, uint32_t late_cap,
                             const uint32_t *d_late_count,
                             srt_pkt *d_out_pkts, uint32_t *d_out_host_ptr, uint32_t *d_out_user,
                             uint64_t *d_out_seq, uint64_t out_cap, srt_err *err);
/* Synchronises the stream.  *flags (may be NULL): the SRT_SENDBATCH_*
 * conditions met since the last status call (then cleared); *n_sent (may be
 * NULL): the last call's sent packets.  SRT_ERR_INVALID, with a message that
 * names every flag set, when any was; else SRT_OK. */
srt_status srt_sendbatch_status(srt_sendbatch *sb, uint32_t *flags, uint64_t *n_sent, srt_err *err);
void srt_sendbatch_destroy(srt_sendbatch *sb);

/* --------------------------------------------------- tracker byte counters */
/* The tracker's heartbeat counters for the internet interface, on the device:
 * what tracker_addOutputBytes (called in networkinterface_pop,
 * host/network/network_interface.c:310-340) and tracker_addInputBytes (called
 * in networkinterface_push, :140-202) add up between two heartbeats
 * (host/tracker.c:24-48, 188-284), and what tracker_heartbeat logs as
 * "[shadow-heartbeat] [node]" and "[socket]" and then clears (:400-433,
 * 582-627).  A packet with payload > 0 is data, else control;
 * PDS_SND_TCP_RETRANSMITTED (SRT_TRK_RETRANS) selects the retransmit class.
 * Counts are kept per host and, separately, per socket slot, each in and out.
 * Only the REMOTE counters are kept: local means the loopback address, and on
 * the internet interface every packet is remote, one addressed to the
 * interface's own address (SRT_OUT_LOCAL) included, since its source is not
 * 127.0.0.1.
 * Output side: a packet is counted when the interface pops it, the moment it
 * gets SND_INTERFACE_SENT, before the relay may cache it and whether or not it
 * is forwarded later.  Input side: a packet is counted at networkinterface_push
 * and only if a socket took it (RCV_INTERFACE_DROPPED is not counted).
 * LIMITS: a call's packets all count in the current interval: the caller ends a
 * window at a heartbeat time and calls srt_tracker_heartbeat between windows.
 * The reference orders a heartbeat task and a packet event of the same instant
 * by event id, which the library does not own.
 * The LOCAL counters are the loopback interface's: srt_loopback below.
 * OUT OF SCOPE: the tracker's CPU, memory and socket-buffer lines.  (pcap
 * capture, at the same two points, is the srt_pcap stage below.)
 * ABI: additive to version 4; detect the stage by its symbols. */
typedef struct srt_tracker srt_tracker;

/* Counters (tracker.c:24-48) in the order of the heartbeat line, 80 bytes */
typedef struct {
    uint64_t packets_control;
    uint64_t bytes_control_header;
    uint64_t packets_control_retrans;
    uint64_t bytes_control_header_retrans;
    uint64_t packets_data;
    uint64_t bytes_data_header;
    uint64_t bytes_data_payload;
    uint64_t packets_data_retrans;
    uint64_t bytes_data_header_retrans;
    uint64_t bytes_data_payload_retrans;
} srt_trk_counters;

#define SRT_TRK_RETRANS 1u /* srt_trk_meta.flags: the packet's status has PDS_SND_TCP_RETRANSMITTED */

/* what the tracker needs from a packet beyond what the other stages return, 16 bytes */
typedef struct {
    uint32_t header_size;  /* packet_getHeaderSize */
    uint32_t payload_size; /* packet_getPayloadSize */
    uint32_t flags;        /* SRT_TRK_RETRANS */
    uint32_t socket_slot;  /* output side: the sending socket's slot (the input side takes srt_deliver's socket) */
} srt_trk_meta;

#define SRT_TRACKER_LOG_OVERRUN  1u /* a late or cached packet's seq is older than the log holds: not counted */
#define SRT_TRACKER_NOTE_OVERRUN 2u /* a placeholder delivery record, or a tag the note ring does not hold: skipped */
#define SRT_TRACKER_BAD_SOCKET   4u /* a socket slot >= n_sockets: counted at its host only */
#define SRT_TRACKER_BAD_HOST     8u /* a late or flat record's host >= n_hosts: skipped */

/* An instance for n_hosts hosts and n_sockets socket slots on the plan's device
 * and stream, or, with plan == NULL, host-only: every array argument named d_
 * is then a HOST pointer and the calls complete before they return.  Both forms
 * run the same step and agree bit for bit (all sums are integers).  The slots
 * are global and chosen by the caller: on the send side a packet's slot is
 * srt_trk_meta.socket_slot, on the receive side it is the socket
 * srt_deliver_run returns, so a caller who wants socket counters names its
 * associations by slot.  n_sockets == 0 switches the socket counters off.
 * Memory of the instance, in bytes:
 *   32 + n_hosts * 184 + n_sockets * 160 + (note_cap + log_cap) * 16
 * (the state words; per host the in and out records, two packet counts and
 * the remembered cached seq; per slot the in and out records; the note ring
 * and the seq log of srt_trk_meta), on the device, plus the records once more
 * on the host for the heartbeat.  Nothing is allocated per call.  n_hosts and
 * n_sockets are below 2^31, note_cap and log_cap at most 2^31.  Destroy the
 * instance before its plan. */
srt_status srt_tracker_create(srt_plan *plan, uint32_t n_hosts, uint32_t n_sockets, uint64_t note_cap,
                              uint64_t log_cap, srt_tracker **out, srt_err *err);

/* The output side, for the srt_outbound_run call just made: d_cached_seq is
 * what srt_outbound_cached_seq wrote after that call, d_host_ptr, n_pkts
 * (< 2^31) and d_status the call's arguments and output, seq_base the value it
 * returned, d_late / late_cap (< 2^31) / d_late_count its late list, of which
 * min(*d_late_count, late_cap) records are used.  d_meta[i] belongs to batch
 * packet i.  A packet is counted in the call in which the interface popped it:
 *   1. a batch packet whose d_status has SND_INTERFACE_SENT (forwarded, cached
 *      and SRT_OUT_LOCAL packets alike);
 *   2. a late record, unless its seq equals the seq this instance remembered
 *      as its host's cached packet at the end of the previous call: that
 *      packet was counted when it was popped;
 *   3. the packet the relay holds cached at the end of this call, if its seq is
 *      below seq_base and differs from the remembered one: queued in an earlier
 *      call, popped and held in this one, it is neither in the batch nor in
 *      the late list;
 *   4. then the remembered seq becomes the cached seq, or none.
 * So a packet cached over any number of calls is counted once, in the call
 * that popped it.  Call it once for every srt_outbound_run call, in order.
 * The seq log: a batch packet not popped in this call has its meta written at
 * (seq_base + i) % log_cap iff n_pkts - i <= log_cap; the meta of a late or
 * cached packet is read back iff its seq < seq_base and seq_base + n_pkts - seq
 * <= log_cap, else the call is flagged LOG_OVERRUN and that packet is not
 * counted.  Both are distances from the end of the call's range, the rule of
 * srt_sendbatch_run, so a slot read is never one this call writes.
 * A late record with src_host >= n_hosts is flagged BAD_HOST and skipped; a
 * socket_slot >= n_sockets (n_sockets > 0) is flagged BAD_SOCKET and the packet
 * counted at its host only.  Every write is range-checked first: a flagged call
 * never writes out of bounds.
 * Asynchronous on the plan's stream: it never waits for the device. */
srt_status srt_tracker_tx(srt_tracker *trk, const uint64_t *d_cached_seq, const uint32_t *d_host_ptr, uint64_t n_pkts,
                          const srt_trk_meta *d_meta, const uint32_t *d_status, uint64_t seq_base,
                          const srt_outbound_late *d_late, uint32_t late_cap, const uint32_t *d_late_count,
                          srt_err *err);

/* The round's metas under the flight tags of its push, for the input side:
 * the contract of srt_deliver_note (d_meta[i] has tag tag_base + i; tag_base
 * not below the previous note's end; a tag is readable iff tag < note_end &&
 * note_end - tag <= note_cap; n_pkts < 2^31; asynchronous). */
srt_status srt_tracker_note(srt_tracker *trk, const srt_trk_meta *d_meta, uint64_t n_pkts, uint64_t tag_base,
                            srt_err *err);

/* The input side: srt_deliver_run's outputs as they are (d_out_host_ptr of
 * n_hosts + 1 entries; d_out_socket, d_out_tag and d_out_status of out_cap
 * entries).  A record is counted iff its socket is not UINT32_MAX, at its host
 * and at the slot its socket names, with the meta noted under its tag.  A
 * placeholder record (no RCV_INTERFACE_RECEIVED in its status), or a tag the
 * note ring no longer holds, is skipped and flagged NOTE_OVERRUN.  The walk is
 * bounded by min(d_out_host_ptr[n_hosts], out_cap) on the device, so out_cap
 * may be the arrays' capacity: nothing is read back between deliver and
 * tracker.  Asynchronous on the plan's stream. */
srt_status srt_tracker_rx(srt_tracker *trk, const uint32_t *d_out_host_ptr, const uint32_t *d_out_socket,
                          const uint64_t *d_out_tag, const uint32_t *d_out_status, uint64_t out_cap, srt_err *err);

/* The input side for n (< 2^31) ungrouped records (host, socket, meta): the
 * SRT_OUT_LOCAL packets, which never reach the inbound stage, with the sockets
 * srt_deliver_lookup gave them.  A record is counted iff its socket is not
 * UINT32_MAX; a host >= n_hosts is skipped and flagged BAD_HOST.  Duplicate
 * (host, socket) pairs are summed.  Asynchronous on the plan's stream. */
srt_status srt_tracker_rx_flat(srt_tracker *trk, const uint32_t *d_host, const uint32_t *d_socket,
                               const srt_trk_meta *d_meta, uint64_t n, srt_err *err);

/* tracker_heartbeat (tracker.c:582-627) for a selection of hosts and socket
 * slots: synchronises the stream, returns the selected records and clears
 * exactly those (the reference's memset is per host, because hosts start at
 * different times).  hosts / sockets and the outputs are HOST pointers.  A NULL
 * selection means all (n_hosts / n_sockets records, in index order) and its
 * count is ignored; a selection of none is a non-NULL pointer with a count of
 * 0.  out_node_in[k] and out_node_out[k] belong to hosts[k], out_sock_in[k] and
 * out_sock_out[k] to sockets[k]; an output pointer may be NULL (the records are
 * still cleared).  An index out of range returns SRT_ERR_INVALID and clears
 * nothing; an index named twice is returned twice and cleared once. */
srt_status srt_tracker_heartbeat(srt_tracker *trk, const uint32_t *hosts, uint32_t n_sel_hosts,
                                 const uint32_t *sockets, uint32_t n_sel_sockets, srt_trk_counters *out_node_in,
                                 srt_trk_counters *out_node_out, srt_trk_counters *out_sock_in,
                                 srt_trk_counters *out_sock_out, srt_err *err);

/* Synchronises the stream.  *flags (may be NULL): the SRT_TRACKER_* conditions
 * met since the last status call (then cleared); *n_tx_counted / *n_rx_counted
 * (may be NULL): packets counted on the output / input side since create (the
 * device form sums the hosts' counts here, with one launch).  SRT_ERR_INVALID,
 * with a message that names every flag set, when any was; else SRT_OK. */
srt_status srt_tracker_status(srt_tracker *trk, uint32_t *flags, uint64_t *n_tx_counted, uint64_t *n_rx_counted,
                              srt_err *err);

/* _tracker_getCounterString (tracker.c:415-433): the twelve comma-separated
 * numbers of a heartbeat line -- packets-total, bytes-total, then the ten
 * fields in order -- so that a shim can emit the reference's line verbatim.
 * Host only.  Writes at most cap bytes, NUL included; returns the length the
 * whole string has (as snprintf does), or -1 on a NULL argument. */
int srt_tracker_counter_string(const srt_trk_counters *c, char *buf, size_t cap);
void srt_tracker_destroy(srt_tracker *trk);

/* ------------------------------------------------------ loopback interface */
/* What a host does with the packets its sockets send to 127.0.0.1: the
 * loopback interface's qdisc, relay_loopback, the receive and the tracker's
 * LOCAL counters, batched over hosts.  At one host, at one instant t:
 *   1. every socket-has-data event puts the socket into the loopback
 *      interface's qdisc unless it is there already (host/host.rs:988-1002,
 *      network_interface.c:344-370) and notifies the relay; an Idle relay
 *      schedules ONE forward task at t (relay/mod.rs:110-135: one host event
 *      id);
 *   2. the event-order contract of srt_outbound holds: at equal times every
 *      arrival, in the caller's list order, runs before the forward task.
 *      relay_loopback is RateLimit::Unlimited (host.rs:307-310) and every
 *      packet is local, so the task holds no bucket and caches no packet: it
 *      pops until the interface is empty (relay/mod.rs:200-272), in the
 *      qdisc's order (SRT_QDISC_FIFO / SRT_QDISC_RR as described above);
 *   3. each popped packet gets SND_INTERFACE_SENT and is counted by
 *      tracker_addOutputBytes in the LOCAL out-counters (its source is
 *      127.0.0.1), gets RELAY_FORWARDED and is pushed into the same interface
 *      with receive time t;
 *   4. the push (network_interface.c:140-202) adds RCV_INTERFACE_RECEIVED,
 *      looks up the specific then the wildcard key in the loopback
 *      interface's OWN association table, counts the packet in the LOCAL
 *      in-counters if a socket takes it, else adds RCV_INTERFACE_DROPPED.
 * So the interface is empty between instants and the stage carries no packet
 * from call to call: per host only the last instant seen and the number of
 * forward tasks, and the counters.
 * LIMIT: in the reference a delivery inside the task can make a socket produce
 * packets at the same instant (an ACK); the relay is Forwarding, so they join
 * the running task.  The library owns no sockets: the caller feeds such
 * packets in a FOLLOWING call with the same ready_ns.  They pop after
 * everything the earlier call held and take no further event id, which is
 * exact when the earlier packets had all been popped before the reply was
 * produced; otherwise the caller must split the instant.  A ready_ns of
 * UINT64_MAX is not an instant.  Equal priorities within a host's instant are
 * a caller error under FIFO (their order is then unspecified).
 * The heartbeat line: the reference prints
 * inbound-localhost-counters;outbound-localhost-counters;
 * inbound-remote-counters;outbound-remote-counters (tracker.c:453-519); the
 * first two are this stage's records, the last two srt_tracker's.
 * ABI: additive to version 4; detect the stage by its symbols. */
typedef struct srt_loopback srt_loopback;

#define SRT_LOOPBACK_TIME_ORDER 1u /* a ready_ns below its host's previous arrival: the host's span is not run */
#define SRT_LOOPBACK_BAD_SOCKET 2u /* socket >= max_sockets: the host's span is not run */
#define SRT_LOOPBACK_BAD_SLOT   4u /* a socket slot >= n_slots: that side of the packet is counted at its host only */

/* An instance for n_hosts hosts and n_slots socket slots on the plan's device
 * and stream, or, with plan == NULL, host-only: every array argument named d_
 * is then a HOST pointer and the calls complete before they return.  Both
 * forms run the same step and agree bit for bit.  qdisc: SRT_QDISC_*, one for
 * all hosts; max_sockets (> 0): sockets a host may name; the slots are
 * srt_tracker's (n_slots == 0 switches the slot counters off).
 * Memory of the instance, in bytes:
 *   32 + n_hosts * 184 + n_slots * 160
 * (the state words; per host the local in and out records, the last instant,
 * the task count and two packet counts of the last run; per slot the in and
 * out records), on the device, plus the records and the hosts' words once more
 * on the host, plus 16 bytes a packet of the largest batch seen: the sort key,
 * the begin of the packet's instant and the instant's end.  That scratch is the
 * one thing a call may allocate, when its batch is larger than any before (it
 * then waits for the stream once).  n_hosts and n_slots are below 2^31.
 * Destroy the instance before its plan. */
srt_status srt_loopback_create(srt_plan *plan, uint32_t n_hosts, uint32_t qdisc, uint32_t max_sockets,
                               uint32_t n_slots, srt_loopback **out, srt_err *err);

/* One call: the packets the hosts' sockets hand to the loopback interface.
 * dl: an srt_deliver instance of the same plan and n_hosts (else
 * SRT_ERR_INVALID) that holds the LOOPBACK interface's associations, kept with
 * srt_deliver_associate / _disassociate; the run uploads the table on the
 * stream when it has changed since the last upload, as srt_deliver_run does.
 * d_pkts: n_pkts (< 2^31) srt_out_pkt records grouped by host through
 * d_host_ptr (n_hosts + 1 entries), each host's in arrival order with
 * nondecreasing ready_ns; flags and total_size are ignored (every packet is
 * local).  d_rx_meta[i] and d_trk_meta[i] belong to batch packet i; d_trk_meta
 * may be NULL: nothing is counted then.  The walk is bounded on the device by
 * min(d_host_ptr[n_hosts], n_pkts): no host round trip precedes the call.
 * Outputs, n_pkts entries each, grouped by the INPUT's d_host_ptr (every packet
 * of an unflagged host is received); position k of host h's span, in the order
 * the interface receives: d_out_index[k] the packet's batch index,
 * d_out_socket[k] the socket or UINT32_MAX, d_out_recv_ns[k] the instant
 * (nondecreasing along the span), d_out_user[k] its rx_meta.user,
 * d_out_status[k] SND_INTERFACE_SENT | RELAY_FORWARDED | RCV_INTERFACE_RECEIVED,
 * plus RCV_INTERFACE_DROPPED when no socket took it.
 * Counters: every popped packet is counted on the out side at its host and at
 * d_trk_meta[i].socket_slot; on the in side iff a socket took it, at its host
 * and at the slot the returned socket names (srt_tracker_rx's convention), in
 * srt_tracker's classes.  A slot >= n_slots (n_slots > 0) raises BAD_SLOT and
 * that side of the packet is counted at its host only.
 * Tasks: one per host for each distinct instant; an arrival whose ready_ns
 * equals the host's last instant of an EARLIER call starts no new task (the
 * LIMIT above).
 * A host with a ready_ns below its previous arrival, in this call or an
 * earlier one (TIME_ORDER), or with a socket >= max_sockets (BAD_SOCKET) is
 * flagged: its state and counters stay untouched and its whole span is written
 * in identity order with status 0, socket UINT32_MAX, recv_ns UINT64_MAX and
 * the user copied.  The other hosts' results stay exact.  Every write is
 * range-checked first: a flagged call never reads or writes out of bounds.
 * An instant of any length is ordered in the same call, in time quadratic in
 * its length shared by the 8 or 64 lanes that own its host.
 * Asynchronous on the plan's stream: it reads nothing back. */
srt_status srt_loopback_run(srt_loopback *lb, srt_deliver *dl, const srt_out_pkt *d_pkts, const uint32_t *d_host_ptr,
                            uint64_t n_pkts, const srt_rx_meta *d_rx_meta, const srt_trk_meta *d_trk_meta,
                            uint32_t *d_out_index, uint32_t *d_out_socket, uint64_t *d_out_recv_ns,
                            uint32_t *d_out_user, uint32_t *d_out_status, srt_err *err);

/* srt_tracker_heartbeat for the local records, with its semantics throughout:
 * synchronises, returns the selected records and clears exactly those; a NULL
 * selection means all; an index out of range returns SRT_ERR_INVALID and clears
 * nothing; an index named twice is returned twice and cleared once.
 * srt_tracker_counter_string formats a record. */
srt_status srt_loopback_heartbeat(srt_loopback *lb, const uint32_t *hosts, uint32_t n_sel_hosts,
                                  const uint32_t *slots, uint32_t n_sel_slots, srt_trk_counters *out_node_in,
                                  srt_trk_counters *out_node_out, srt_trk_counters *out_slot_in,
                                  srt_trk_counters *out_slot_out, srt_err *err);

/* Synchronises; out_tasks[h] (n_hosts entries, HOST pointer): the forward tasks
 * host h's loopback relay has scheduled since create, each one host event id. */
srt_status srt_loopback_tasks(srt_loopback *lb, uint64_t *out_tasks, srt_err *err);

/* Synchronises the stream.  *flags (may be NULL): the SRT_LOOPBACK_* conditions
 * met since the last status call (then cleared); *n_received / *n_no_socket
 * (may be NULL): the last run's received packets and those of them no socket
 * took (the device form sums the hosts' counts here, with one launch).
 * SRT_ERR_INVALID, with a message that names every flag set, when any was;
 * else SRT_OK. */
srt_status srt_loopback_status(srt_loopback *lb, uint32_t *flags, uint64_t *n_received, uint64_t *n_no_socket,
                               srt_err *err);
void srt_loopback_destroy(srt_loopback *lb);

/* ------------------------------------------------------------ pcap capture */
/* The packet capture a host switches on with pcap_enabled / pcap_capture_size
 * (core/configuration.rs:558-577), built on the device: one byte stream a host,
 * the body of the file the reference's PcapWriter writes for an interface
 * (utility/pcap_writer.rs).  The capture points are the tracker's:
 * networkinterface_pop captures a packet right after SND_INTERFACE_SENT
 * (host/network/network_interface.c:310-340), networkinterface_push before the
 * socket hand-off, whether or not a socket takes the packet (:140-202).  One
 * instance is one interface class: a caller that captures the loopback
 * interfaces too makes a second instance.
 * A record is 16 + incl_len bytes (pcap_writer.rs:86-142,
 * network_interface.c:119-134), the header native endian:
 *   ts_sec  u32 = time_ns / 10^9          ts_usec  u32 = (time_ns % 10^9) / 1000
 *   incl_len u32 = min(capture_len, total)  orig_len u32 = total
 * with total = header_size + payload_len and header_size 28 for UDP, 40 for TCP,
 * 44 for TCP with the window-scale option (packet_getHeaderSize,
 * routing/packet.c:378-403, plus the 20-byte IP header).  Then the first
 * incl_len bytes of the packet as network/packet.rs:374-586 displays it, all
 * big endian.  IP: 45 00, total u16, id 00 00, 40 00, TTL 40, protocol, checksum
 * 00 00, source, destination.  TCP: ports, seq, ack (0 when ACK is not set),
 * the data-offset byte ((20 + options) / 4) << 4, the flag byte (tcp_flags &
 * 0x17: FIN 0x01, SYN 0x02, RST 0x04, ACK 0x10), window u16, checksum 0, urgent
 * 0, and with wscale_set the option 03 03 <wscale> 00.  UDP: ports, payload_len
 * + 8 as u16, checksum 0.  Then the payload.  The cut is at exactly capture_len
 * bytes (utility/give.rs), in the middle of a field or of the IP header if it
 * falls there; capture_len 0 leaves the 16-byte record header alone.
 * LIMIT: a host's sent and received packets of the same instant.  The reference
 * writes them in the order their events run, packet events before local ones
 * (core/work/event.rs:102-110), which is SRT_PCAP_RX_FIRST, the default; the
 * exact order at one instant depends on event ids, which the library does not
 * own (the tracker's caveat).  SRT_PCAP_TX_FIRST is the other choice.
 * ABI: additive to version 4; detect the stage by its symbols. */
typedef struct srt_pcap srt_pcap;

/* what the capture needs of a packet, 48 bytes */
typedef struct {
    uint64_t time_ns;     /* simulation time of the pop or the push */
    uint64_t payload_off; /* the payload's first byte in d_payload */
    uint32_t src_ip_be;   /* network byte order, as the IP assignment passes addresses */
    uint32_t dst_ip_be;
    uint16_t src_port_be; /* network byte order */
    uint16_t dst_port_be;
    uint32_t seq;         /* TCP, host order, as are ack and window */
    uint32_t ack;         /* written as 0 unless tcp_flags has ACK */
    uint16_t window;
    uint16_t payload_len;
    uint8_t protocol;     /* 6 TCP, 17 UDP */
    uint8_t tcp_flags;    /* wire bits; only 0x17 is used */
    uint8_t wscale;
    uint8_t wscale_set;   /* the window-scale option is present */
    uint32_t reserved;
} srt_pcap_rec;

#define SRT_PCAP_RX_FIRST 0u /* srt_pcap_create flags: at equal times a host's received packets come first */
#define SRT_PCAP_TX_FIRST 1u /* its sent packets come first */

#define SRT_PCAP_OVERFLOW     1u  /* the call's bytes exceed out_cap: d_host_off written, d_out untouched */
#define SRT_PCAP_BAD_PROTOCOL 2u  /* protocol neither 6 nor 17: skipped, 0 bytes */
#define SRT_PCAP_BAD_LENGTH   4u  /* header_size + payload_len > 65535: skipped */
#define SRT_PCAP_BAD_PAYLOAD  8u  /* payload_off + payload_len > payload_bytes: skipped */
#define SRT_PCAP_TIME_ORDER   16u /* a list decreases within a host, or starts before the host's last record */

/* An instance for n_hosts hosts on the plan's device and stream, or, with
 * plan == NULL, host-only: every array argument named d_ is then a HOST pointer
 * and the calls complete before they return.  Both forms run the same step and
 * agree byte for byte.  capture_len is the snap length of every host; enabled
 * (HOST pointer, n_hosts bytes, copied) says which hosts capture, NULL: all.
 * rec_cap bounds n_tx + n_rx of a call; flags is SRT_PCAP_RX_FIRST or
 * SRT_PCAP_TX_FIRST.  Memory of the instance, in bytes:
 *   40 + n_hosts * 32 + rec_cap * 16
 * (the state words; per host the last time, the call's largest time, its bytes,
 * its record count and the enabled byte; per record of a call its list entry,
 * size and byte offset), on the device.  Nothing is allocated per call.
 * n_hosts and rec_cap are below 2^31.  Destroy the instance before its plan. */
srt_status srt_pcap_create(srt_plan *plan, uint32_t n_hosts, uint32_t capture_len, const uint8_t *enabled,
                           uint64_t rec_cap, uint32_t flags, srt_pcap **out, srt_err *err);

/* One call formats the packets hosts sent (d_tx) and received (d_rx) in a span
 * of time.  Each list is grouped by host through a pointer array of n_hosts + 1
 * entries (ptr[0] == 0, nondecreasing), as every stage takes its batches, and is
 * nondecreasing in time_ns within a host.  d_*_idx is an optional indirection:
 * entry k of the list is d_tx[d_tx_idx[k]] (NULL: d_tx[k]), so srt_outbound's
 * send order or srt_deliver's output order is handed over without a gather; the
 * caller guarantees that every index names a record of its array.  n_tx and
 * n_rx may be the capacity of the lists: the walk is bounded by
 * min(ptr[n_hosts], n) on the device, so nothing is read back before the call.
 * n_tx + n_rx <= rec_cap.
 * Per host the two lists are merged stably by time_ns, equal times by the
 * create-time flag; every record becomes 16 + incl_len bytes; host h's bytes
 * are d_out[d_host_off[h] .. d_host_off[h + 1]), hosts in index order without
 * gaps, a host that does not capture with an empty range.  d_host_off has
 * n_hosts + 1 entries; d_out needs no alignment.  d_payload (payload_bytes
 * bytes) may be NULL only when capture_len <= 28, the shortest header, so that
 * no payload byte is reached; otherwise SRT_ERR_INVALID.
 * Conditions, collected for srt_pcap_status; every write is range-checked first:
 *   OVERFLOW      the call's bytes exceed out_cap: d_host_off is written in full
 *                 (the caller sizes a retry), no byte of d_out is written, the
 *                 hosts' last times and the counts do not advance;
 *   BAD_PROTOCOL, BAD_LENGTH, BAD_PAYLOAD: the record is skipped, 0 bytes;
 *   TIME_ORDER    a list decreases within a host, or a record is earlier than
 *                 the last time this instance wrote for its host: the record is
 *                 still written, in list order (its merge key is the largest
 *                 time of its list so far).
 * Asynchronous on the plan's stream, four launches: it never waits for the
 * device and reads nothing back. */
srt_status srt_pcap_run(srt_pcap *pc, const srt_pcap_rec *d_tx, const uint32_t *d_tx_idx,
                        const uint32_t *d_tx_host_ptr, uint64_t n_tx, const srt_pcap_rec *d_rx,
                        const uint32_t *d_rx_idx, const uint32_t *d_rx_host_ptr, uint64_t n_rx,
                        const uint8_t *d_payload, uint64_t payload_bytes, uint8_t *d_out, uint64_t out_cap,
                        uint64_t *d_host_off, srt_err *err);

/* Synchronises the stream.  *flags (may be NULL): the SRT_PCAP_* conditions met
 * since the last status call (then cleared); *n_records / *n_bytes (may be
 * NULL): records and bytes written since create.  SRT_ERR_INVALID, with a
 * message that names every flag set, when any was; else SRT_OK. */
srt_status srt_pcap_status(srt_pcap *pc, uint32_t *flags, uint64_t *n_records, uint64_t *n_bytes, srt_err *err);

/* The file side, host only.  srt_pcap_file_header: the 24 bytes a capture file
 * starts with (pcap_writer.rs:25-54, native endian: magic 0xA1B2C3D4, version
 * 2.4, thiszone 0, sigfigs 0, snaplen capture_len, linktype 101 LINKTYPE_RAW).
 * srt_pcap_open_files: paths has n_hosts entries, NULL: no file for that host;
 * each file is created or truncated, as File::create does, and gets the
 * header; files open from an earlier call are closed first.
 * srt_pcap_append_files: appends bytes[host_off[h] .. host_off[h + 1]) to host
 * h's file, for a call's d_out and d_host_off copied to the host.  The files
 * are closed by srt_pcap_destroy.  The reference names an interface's file
 * <dir>/<hostname>-<interface name>.pcap (network_interface.c:403-414); the
 * caller builds the paths. */
void srt_pcap_file_header(uint32_t capture_len, uint8_t out[24]);
srt_status srt_pcap_open_files(srt_pcap *pc, const char *const *paths, srt_err *err);
srt_status srt_pcap_append_files(srt_pcap *pc, const uint64_t *host_off, const uint8_t *bytes, srt_err *err);

/* the write pass's tile, in bytes: a workgroup assembles and stores that much of d_out at a time */
uint32_t srt_pcap_tile_bytes(void);
void srt_pcap_destroy(srt_pcap *pc);

/* ------------------------------------------------ UDP socket receive stage */
/* What a UDP socket does with the packets srt_deliver_run handed it, and what
 * the window's recvmsg calls get back, batched over socket slots:
 * UdpSocket::push_in_packet (host/descriptor/socket/inet/udp.rs:108-168),
 * recvmsg (:477-572), MessageBuffer (:1056-1134) and the SO_RCVBUF rule
 * (:900-925).  A socket's state is a FIFO of messages with a byte soft limit,
 * an optional connected peer, the receive time of the last message read, and
 * at most one blocked read.  The stage is exact, state included, and has no
 * feedback into the network.
 * The events of one socket in the window [previous until_ns, until_ns) run in
 * time order:
 *   push   a delivery record whose socket is this slot and whose status has
 *          RCV_INTERFACE_RECEIVED, at its forward_ns, in list order.  It gets
 *          RCV_SOCKET_PROCESSED; with a peer set and a source (ip, port) that
 *          differs from it, RCV_SOCKET_DROPPED; else if !(len_bytes <
 *          soft_limit), RCV_SOCKET_DROPPED; else the message {tag, recv_ns =
 *          forward_ns, payload_size, source, user} is appended, len_bytes +=
 *          payload_size, and it gets RCV_SOCKET_BUFFERED.  The limit is soft:
 *          a packet arriving one byte below it is accepted whole; a zero-length
 *          payload is buffered without changing len_bytes.  UDP never sets
 *          RCV_SOCKET_DELIVERED in the reference, nor does the stage.
 *   read   srt_udp_read at time_ns: an empty buffer answers -EWOULDBLOCK
 *          unless SRT_UDP_WAIT is set; otherwise the front message is taken
 *          (popped unless SRT_UDP_PEEK), copied = min(len, size), return_val =
 *          SRT_UDP_TRUNC ? size : copied, msg_flags has SRT_UDP_MSG_TRUNC iff
 *          copied < size, and the socket's last_read_recv_ns becomes the
 *          message's recv_ns, for peeks too (udp.rs:537-538).
 *   WAIT   the blocked syscall the reference re-runs when the socket turns
 *          READABLE (udp.rs:550-568): a WAIT read that finds the buffer empty is
 *          ARMED.  It completes at the first instant t at which a message is
 *          buffered, after every push of that socket with forward_ns == t (all
 *          packets of one relay forward task are pushed inside that task; the
 *          woken process runs in a later event of the same instant) and before
 *          the list's own reads of time t.  An armed read survives the call;
 *          its result is reported by the call that completes it: the arming
 *          call in d_results[r] with complete_ns = t, a later call as a record
 *          {read seq, result} appended to d_late.  One armed read a socket: a
 *          second WAIT read that finds the buffer empty meanwhile is flagged
 *          ARMED_TWICE and answered -EWOULDBLOCK.
 * At equal times pushes run before reads.
 * LIMIT: the reference orders a running process's syscall and a forward task of
 * the same instant by event id, which the library does not own.  A caller who
 * knows a read preceded a push of the same nanosecond splits the window there.
 * LIMIT: a host's loopback deliveries (srt_loopback) are not merged into the
 * same window here; a socket that receives on both interfaces in one window is
 * the caller's to order.
 * A record whose socket is UINT32_MAX, a placeholder record (no
 * RCV_INTERFACE_RECEIVED), a record whose slot is not open here (a TCP socket,
 * say: FOREIGN to this stage) and a record listed under a host that does not own
 * its slot pass through: d_rx_status[k] is deliver's status unchanged.
 * OUT OF SCOPE: TCP sockets and legacy_tcp, the send buffer, shutdown(2), the
 * CPU-delay model, the tracker's socket-buffer line (tcp.c only).
 * ABI: additive to version 4; detect the stage by its symbols. */
typedef struct srt_udprecv srt_udprecv;

/* what the socket needs from a packet, 16 bytes; `user` is opaque and comes back with the message */
typedef struct {
    uint32_t src_ip_be;
    uint16_t src_port_be;
    uint16_t reserved;
    uint32_t payload_size;
    uint32_t user;
} srt_udp_meta;

#define SRT_UDP_PEEK  0x2u     /* srt_udp_read.flags: MSG_PEEK */
#define SRT_UDP_TRUNC 0x20u    /* MSG_TRUNC: return the message's size, not the bytes copied */
#define SRT_UDP_WAIT  0x10000u /* a blocking call: neither MSG_DONTWAIT nor O_NONBLOCK */
#define SRT_UDP_MSG_TRUNC 0x20u /* srt_udp_result.msg_flags: MSG_TRUNC */

/* one recvmsg call, 24 bytes */
typedef struct {
    uint64_t time_ns;
    uint32_t slot;
    uint32_t len;   /* the sum of the iovecs' lengths */
    uint32_t flags; /* SRT_UDP_PEEK | SRT_UDP_TRUNC | SRT_UDP_WAIT */
    uint32_t user;  /* opaque, comes back as read_user */
} srt_udp_read;

#define SRT_UDP_NOT_TAKEN 0u /* srt_udp_result.status: the read was not run (READ_ORDER, or past the reads' bounds) */
#define SRT_UDP_DONE      1u /* return_val and the rest are the call's result */
#define SRT_UDP_ARMED     2u /* blocked: a later call reports it in d_late */

/* what one read returned, 56 bytes */
typedef struct {
    uint64_t tag;         /* the message's flight tag */
    uint64_t recv_ns;     /* when the interface received it (MessageRecvHeader.recv_time) */
    uint64_t complete_ns; /* when the call returned: its time_ns, or t for a read that blocked */
    int64_t return_val;   /* bytes, or -EWOULDBLOCK (-11), or -EBADF (-9) */
    uint32_t status;      /* SRT_UDP_NOT_TAKEN / DONE / ARMED */
    uint32_t msg_flags;   /* SRT_UDP_MSG_TRUNC or 0 */
    uint32_t src_ip_be;   /* the message's source: recvmsg's addr */
    uint16_t src_port_be;
    uint16_t reserved;
    uint32_t user;        /* the message's srt_udp_meta.user */
    uint32_t read_user;   /* the read's srt_udp_read.user */
} srt_udp_result;

/* an armed read of an EARLIER call that completed in this one, 64 bytes */
typedef struct {
    uint64_t seq; /* its call's read_seq_base + its index */
    srt_udp_result result;
} srt_udp_late;

#define SRT_UDPRECV_OPEN       1u /* value: recv_buf_size, the soft limit as given (UdpSocket::new, udp.rs:60-68) */
#define SRT_UDPRECV_CLOSE      2u /* drops what is buffered, disarms a waiting read */
#define SRT_UDPRECV_SET_PEER   3u /* connect: value = ip_be | (uint64_t)port_be << 32; 0 clears the peer */
#define SRT_UDPRECV_SET_RCVBUF 4u /* value: optval; the limit becomes min(max(optval * 2, 2048), 2^28) (udp.rs:910-924) */

/* one configuration step of a socket slot, 16 bytes */
typedef struct {
    uint32_t op;
    uint32_t slot;
    uint64_t value;
} srt_udprecv_op;

#define SRT_UDPRECV_RING_OVERFLOW 1u  /* a socket held more than ring_cap messages at the end of a call */
#define SRT_UDPRECV_LATE_OVERFLOW 2u  /* more late records than late_cap */
#define SRT_UDPRECV_NOTE_OVERRUN  4u  /* a tag the note ring does not hold: the record is skipped */
#define SRT_UDPRECV_BAD_SOCKET    8u  /* a read's slot is >= n_sockets, not its host's, or not open: -EBADF */
#define SRT_UDPRECV_READ_ORDER    16u /* a read outside the window or decreasing within its host: not taken */
#define SRT_UDPRECV_ARMED_TWICE   32u /* a WAIT read while the socket has an armed one: -EWOULDBLOCK */

#define SRT_UDPRECV_MARK_RING 1u /* srt_udprecv_socket_state.overflow bits */
#define SRT_UDPRECV_MARK_NOTE 2u

/* a socket slot's state, 48 bytes; UINT64_MAX: none */
typedef struct {
    uint64_t len_bytes;
    uint64_t soft_limit;
    uint64_t last_read_recv_ns; /* recv_time_of_last_read_packet */
    uint64_t armed_seq;         /* the blocked read's sequence number */
    uint32_t n_msgs;
    uint32_t peer_ip_be;
    uint16_t peer_port_be;
    uint8_t open;
    uint8_t overflow; /* SRT_UDPRECV_MARK_*: the slot's results are invalid since */
    uint32_t reserved;
} srt_udprecv_socket_state;

/* An instance for n_hosts hosts on the plan's device and stream, or, with plan
 * == NULL, host-only: every array argument named d_ is then a HOST pointer and
 * the calls complete before they return.  Both forms run the same step and
 * agree byte for byte.  Host h owns the global socket slots [socket_ptr[h],
 * socket_ptr[h + 1]) (HOST pointer, n_hosts + 1 entries, copied; socket_ptr[0]
 * == 0, nondecreasing, else SRT_ERR_INVALID); they are the slots srt_tracker
 * uses: a caller names its associations by slot, so srt_deliver_run's
 * d_out_socket is the slot.  n_sockets = socket_ptr[n_hosts] and n_hosts are
 * below 2^31.  ring_cap (below 2^31) is the number of messages a socket may
 * hold buffered ACROSS calls; inside a call a socket's queue is as long as the
 * call's list makes it.  note_cap is at most 2^31.  late_cap_hint, the largest
 * late_cap the caller means to pass, is checked (below 2^31) and sizes nothing
 * yet.  Memory of the instance, in bytes:
 *   round16(48 + n_sockets * 88) + n_sockets * ring_cap * 32 + note_cap * 16
 *      + max(n_sockets, 1024) * 16 + 16 + out_cap * 32
 * (the state words and the late count of a caller that passes none, 48, and
 * per slot its 88-byte state record, together rounded up to a multiple of 16;
 * per slot its ring of messages; the note ring of srt_udp_meta; the
 * configuration steps of one launch; 16 spare bytes; a 32-byte staged record
 * per delivery record of the largest out_cap seen), on the device.  The
 * staged records are the one thing that grows: the first run, and a run with a
 * larger out_cap than any before,
 * wait for the stream and reallocate them; no other run allocates or waits.
 * Destroy the instance before its plan. */
srt_status srt_udprecv_create(srt_plan *plan, uint32_t n_hosts, const uint32_t *socket_ptr, uint32_t ring_cap,
                              uint64_t note_cap, uint32_t late_cap_hint, srt_udprecv **out, srt_err *err);

/* Socket configuration between runs: n steps (HOST pointer), applied in list
 * order, one launch on the plan's stream for every n_sockets (at least 1024)
 * steps.  EVERY call first waits for the stream's earlier work (the instance
 * keeps one sorted copy of the steps on the host), so batch a window's steps
 * into one call.  A slot >= n_sockets or an unknown op returns SRT_ERR_INVALID
 * and changes NOTHING.  OPEN gives an empty buffer, len_bytes 0, no peer, no last
 * read time, no mark; on an open slot it does the same.  Every other step on a
 * slot that is not open is ignored.  A limit set below the current len_bytes
 * leaves has_space() false until reads drain the buffer. */
srt_status srt_udprecv_config(srt_udprecv *ur, const srt_udprecv_op *ops, uint64_t n, srt_err *err);

/* srt_deliver_note's and srt_tracker_note's contract for srt_udp_meta: after a
 * round's srt_flight_push with d_tag == NULL, d_meta[i] for batch packet i,
 * whose tag is tag_base + i, goes into the instance's ring at tag % note_cap.
 * tag_base must not lie below the previous note's end (SRT_ERR_INVALID).  A tag
 * is readable iff tag < note_end && note_end - tag <= note_cap.  n_pkts < 2^31.
 * Asynchronous on the plan's stream. */
srt_status srt_udprecv_note(srt_udprecv *ur, const srt_udp_meta *d_meta, uint64_t n_pkts, uint64_t tag_base,
                            srt_err *err);

/* One call per srt_deliver_run call, in order, on that call's outputs as they
 * are: the walk over the delivery list is bounded on the device by
 * min(d_out_host_ptr[n_hosts], out_cap), so nothing is read back between the
 * two stages.  The window's reads are grouped by host through d_read_host_ptr
 * (n_hosts + 1 entries; may be NULL when n_reads == 0), within a host in issue
 * order with nondecreasing time_ns; n_reads (< 2^31) may be the list's
 * capacity, the walk is bounded by min(d_read_host_ptr[n_hosts], n_reads).  A
 * read's sequence number is *read_seq_base + its index (read_seq_base, host
 * pointer, may be NULL: the running count of all earlier calls' n_reads).
 * until_ns must not lie below the previous call's (SRT_ERR_INVALID).
 * PRECONDITION: d_out_host_ptr and d_read_host_ptr start at 0 and are
 * nondecreasing, as srt_deliver_run emits the first.  With pointers that
 * decrease every access still stays inside the arrays, but which records and
 * reads a slot sees is then unspecified and the device and host-only forms
 * need not agree; nothing flags it.
 * Outputs: d_rx_status[k] for every walked record k, deliver's status OR the
 * socket's bits; d_results[r] for every r < n_reads; d_late (late_cap records,
 * any order) and *d_late_count (written by the call; beyond late_cap:
 * LATE_OVERFLOW); d_first_readable_ns[slot] for every slot: the time of the
 * socket's first empty -> non-empty transition in this call, else UINT64_MAX
 * (what wakes poll / epoll waiters).
 * Conditions, collected for srt_udprecv_status; every write is range-checked
 * first, a flagged call never writes out of bounds:
 *   RING_OVERFLOW  the newest messages beyond ring_cap are lost, the socket is
 *                  marked in its state and only its results are invalid;
 *   LATE_OVERFLOW  the records beyond late_cap are lost;
 *   NOTE_OVERRUN   the record is skipped (status unchanged), the socket marked;
 *   BAD_SOCKET     the read is answered -EBADF, whatever its time;
 *   READ_ORDER     a read below the previous until_ns, at or after until_ns,
 *                  or below an earlier read of its host's list that lies in the
 *                  window: not taken, status SRT_UDP_NOT_TAKEN;
 *   ARMED_TWICE    answered -EWOULDBLOCK.
 * Asynchronous on the plan's stream, two launches: it does not wait for the
 * device, except where the staged records grow (srt_udprecv_create). */
srt_status srt_udprecv_run(srt_udprecv *ur, const uint32_t *d_out_host_ptr, const uint32_t *d_out_socket,
                           const uint64_t *d_out_forward_ns, const uint64_t *d_out_tag, const uint32_t *d_out_status,
                           uint64_t out_cap, const uint32_t *d_read_host_ptr, const srt_udp_read *d_reads,
                           uint64_t n_reads, uint64_t *read_seq_base, uint64_t until_ns, uint32_t *d_rx_status,
                           srt_udp_result *d_results, srt_udp_late *d_late, uint32_t late_cap, uint32_t *d_late_count,
                           uint64_t *d_first_readable_ns, srt_err *err);

/* Synchronises the stream and sums the sockets' counts with one launch.
 * *flags (may be NULL): the SRT_UDPRECV_* conditions met since the last status
 * call (then cleared); *n_processed / *n_buffered / *n_dropped (may be NULL):
 * packets the sockets processed, buffered and dropped since create.
 * SRT_ERR_INVALID, with a message that names every flag set, when any was;
 * else SRT_OK. */
srt_status srt_udprecv_status(srt_udprecv *ur, uint32_t *flags, uint64_t *n_processed, uint64_t *n_buffered,
                              uint64_t *n_dropped, srt_err *err);

/* Synchronises and copies every slot's state to out[n_sockets] (HOST pointer). */
srt_status srt_udprecv_state(srt_udprecv *ur, srt_udprecv_socket_state *out, srt_err *err);

/* the bytes of delivery records (32 each, staged) and reads (24 each) a wave of 64 slots holds in LDS:
 * its hosts' records if they fit, their reads if they fit what is left; a list that does not fit is
 * walked in device memory instead */
uint32_t srt_udprecv_window_bytes(void);
void srt_udprecv_destroy(srt_udprecv *ur);

/* ---------------------------------------------------------- UDP send side */
/* Where a packet's path starts: a host's UDP sockets' send buffers and its
 * outbound relay, fused into one step per host, because the two feed each
 * other: buffer space depends on when the relay popped each message, pop times
 * on the qdisc and the token bucket, those on what sendmsg accepted.  The stage
 * is srt_outbound's relay (above: qdisc, bucket, cached packet, event ids, send
 * ranks) with UdpSocket::sendmsg (host/descriptor/socket/inet/udp.rs:327-475),
 * pull_out_packet (:170-195), peek_next_packet_priority / has_data_to_send
 * (:197-203), MessageBuffer (:1056-1134), the SO_SNDBUF rule (:874-899), TIOCOUTQ
 * (:597-603, len_bytes of the state), shutdown (:767-788) and close (:229-240)
 * inside it, and Host::get_next_packet_priority (host/host.rs:715-720, the
 * counter starts at 1).  Its per-call outputs have srt_outbound_run's formats, so
 * srt_sendbatch_run, srt_tracker_tx and everything behind them run on them
 * unchanged.  It is exact, state included.
 * State per host: everything srt_outbound keeps, next_priority, the host's own
 * IPv4 address.  State per global socket slot (host h owns [socket_ptr[h],
 * socket_ptr[h + 1]), srt_udprecv's and srt_tracker's slots): open, shut_wr,
 * soft_limit, len_bytes, n_msgs, the bound (ip, port), the peer or none, at most
 * one armed (blocked) send, a FIFO of messages {seq, priority, payload_size,
 * local}.
 * The events of one host in the window [previous until_ns, until_ns) run in
 * time order.
 *   sendmsg  srt_udp_send at time_ns, the checks in the reference's order:
 *     1. slot >= n_sockets, not this host's, or not open: -EBADF (BAD_SOCKET);
 *     2. shut_wr: -EPIPE (-32);
 *     3. the destination is the given one with SRT_UDPSEND_HAS_ADDR, else the
 *        peer, else -EDESTADDRREQ (-89);
 *     4. len > 65507: -EMSGSIZE (-90);
 *     5. slot not bound: NOT taken (UNBOUND).  The implicit bind of udp.rs:373-403
 *        draws a port from the host RNG: the caller binds through
 *        srt_udpsend_config and feeds the call again;
 *     6. destination 127.0.0.1, or a slot bound to 127.0.0.1: NOT taken
 *        (LOOPBACK): that traffic is srt_loopback's;
 *     7. !(len_bytes < soft_limit): -EWOULDBLOCK (-11), or with SRT_UDPSEND_WAIT
 *        the call is ARMED.  The limit is soft: a message is accepted whole while
 *        len_bytes < soft_limit; a zero-length message is accepted, or refused,
 *        by the same test and does not change len_bytes;
 *     8. accepted: priority = next_priority++, source = the bound address with
 *        0.0.0.0 replaced by the host's address, len_bytes += len, the message
 *        joins the slot's FIFO, the slot the qdisc unless it is in it, an Idle
 *        relay schedules its forward task at this time (tasks_scheduled += 1),
 *        return_val = len, local = (destination ip == the host's address).
 *   forward task  srt_outbound's, with total_size = payload + 28
 *     (routing/packet.c:382, core/definitions.h:102-113).  A pop runs
 *     pull_out_packet: len_bytes -= payload, n_msgs -= 1, the packet gets
 *     SND_CREATED.  If the slot had no space before the pop and has space after
 *     it, the slot turned WRITABLE at this instant: the first such time of the
 *     call goes to d_first_writable_ns[slot] (what wakes poll / epoll waiters; an
 *     open slot's only), and an armed send's wake-up is queued.  A packet the
 *     relay pops and then caches has already left the send buffer.
 *   wake-ups  the armed sends whose sockets turned writable during a forward
 *     task are run again from check 2, after that task returns (the forward loop
 *     keeps the interface until it blocks or empties; the woken process is a
 *     later event of the same instant), at the task's time, in the order of the
 *     pops that woke them.  An accepted one is an arrival at that time: an Idle
 *     relay schedules a new forward task at the same instant (tasks_scheduled +=
 *     1), a relay that holds a cached packet does nothing.  The result goes to
 *     d_results[i] with complete_ns = t when the arming call is this one, else to
 *     a late result record {seq, result}.  One armed send a socket: a second WAIT
 *     call that finds no space meanwhile is flagged ARMED_TWICE and answered
 *     -EWOULDBLOCK.
 *   raw arrival  SRT_UDPSEND_RAW: a packet handed over ready-made by a socket
 *     the stage does not model (TCP sharing the interface).  Its slot is a slot
 *     of the host that is NOT open here (else BAD_SOCKET, not taken); len is its
 *     total_size, priority comes from the record, SRT_UDPSEND_LOCAL from the
 *     flags.  No buffer check, the counter untouched, always accepted; it takes
 *     part in the qdisc and the relay like any packet and gets no SND_CREATED.  A
 *     host with only raw arrivals produces byte for byte what srt_outbound_run
 *     produces for the same list.
 * Equal times at one host: the list's calls of time t in list order, then the
 * forward task of t, then its wake-ups, then a further forward task of t if one
 * was scheduled: srt_outbound's contract extended.
 * LIMIT: the reference orders a running process's syscall and a forward task of
 * one instant by event id, which the library does not own; the caller splits
 * the window where it knows better.
 * LIMIT: priorities drawn by other sockets of the host (TCP) inside a window:
 * the caller sets the counter between calls (SET_NEXT_PRIORITY) and splits the
 * window at such draws.
 * OUT OF SCOPE: TCP and legacy_tcp, payload bytes (sizes only), the implicit bind
 * and its RNG draw, IP_PKTINFO, the CPU-delay model, the loopback interface.
 * ABI: additive to version 4; detect the stage by its symbols. */
typedef struct srt_udpsend srt_udpsend;

#define SRT_UDPSEND_HAS_ADDR 0x1u     /* srt_udp_send.flags: dst_ip_be / dst_port_be are given (sendto) */
#define SRT_UDPSEND_WAIT     0x10000u /* a blocking call: neither MSG_DONTWAIT nor O_NONBLOCK */
#define SRT_UDPSEND_RAW      0x20000u /* a ready-made packet of a socket the stage does not model */
#define SRT_UDPSEND_LOCAL    0x40000u /* RAW only: its destination is the interface's own address */

/* one sendmsg call, or one raw arrival, 40 bytes */
typedef struct {
    uint64_t time_ns;
    uint64_t priority; /* RAW only */
    uint32_t slot;
    uint32_t len; /* the sum of the iovecs' lengths; RAW: total_size */
    uint32_t dst_ip_be;
    uint16_t dst_port_be;
    uint16_t reserved;
    uint32_t flags; /* SRT_UDPSEND_HAS_ADDR | WAIT | RAW | LOCAL */
    uint32_t user;  /* opaque, comes back in the result */
} srt_udp_send;

#define SRT_UDPSEND_NOT_TAKEN 0u /* srt_udpsend_result.status: the call was not run; feed it again */
#define SRT_UDPSEND_DONE      1u /* return_val and the rest are the call's result */
#define SRT_UDPSEND_ARMED     2u /* blocked: a later call reports it in d_late_results */

/* what one call returned, 40 bytes */
typedef struct {
    uint64_t complete_ns; /* when the call returned: its time_ns, or t for a send that blocked */
    uint64_t priority;    /* the packet's, when accepted */
    int64_t return_val;   /* len, or -EBADF (-9), -EWOULDBLOCK (-11), -EPIPE (-32), -EDESTADDRREQ (-89), -EMSGSIZE (-90) */
    uint32_t status;      /* SRT_UDPSEND_NOT_TAKEN / DONE / ARMED */
    uint32_t src_ip_be;   /* the packet's source, when accepted */
    uint16_t src_port_be;
    uint16_t reserved;
    uint32_t user;
} srt_udpsend_result;

/* an armed send of an EARLIER call that completed in this one, 48 bytes */
typedef struct {
    uint64_t seq; /* its call's seq_base + its index */
    srt_udpsend_result result;
} srt_udpsend_late;

#define SRT_UDPSEND_OPEN              1u /* value: send_buf_size, the soft limit as given */
#define SRT_UDPSEND_CLOSE             2u /* new calls get -EBADF, an armed send is dropped; buffered messages still
                                            drain through the relay (udp.rs:229-240 drops only the association,
                                            the qdisc keeps its reference) */
#define SRT_UDPSEND_BIND              3u /* value: ip_be | (uint64_t)port_be << 32 */
#define SRT_UDPSEND_SET_PEER          4u /* connect: value as BIND; 0 clears the peer */
#define SRT_UDPSEND_SET_SNDBUF        5u /* value: optval; the limit becomes min(max(optval * 2, 4096), 2^28) */
#define SRT_UDPSEND_SHUT_WR           6u /* shutdown(SHUT_WR); ignored without a peer (ENOTCONN there) */
#define SRT_UDPSEND_SET_NEXT_PRIORITY 7u /* per HOST: the slot field names the host, value the counter */

/* one configuration step, 16 bytes */
typedef struct {
    uint32_t op;
    uint32_t slot;
    uint64_t value;
} srt_udpsend_op;

/* srt_udpsend_status flags */
#define SRT_UDPSEND_RING_OVERFLOW        1u    /* a socket held more than ring_cap messages at the end of a call */
#define SRT_UDPSEND_LATE_OVERFLOW        2u    /* more late packets than late_cap */
#define SRT_UDPSEND_TIME_REGRESSION      4u    /* a call earlier than the previous until_ns: not taken */
#define SRT_UDPSEND_OVERSIZE             8u    /* srt_outbound's rule for a packet its host's bucket can never hold */
#define SRT_UDPSEND_AFTER_UNTIL          16u   /* a call at or after until_ns: not taken */
#define SRT_UDPSEND_BAD_SOCKET           32u   /* -EBADF; a raw arrival: not taken */
#define SRT_UDPSEND_UNBOUND              64u   /* not taken: bind, then feed it again */
#define SRT_UDPSEND_LOOPBACK             128u  /* not taken: srt_loopback's traffic */
#define SRT_UDPSEND_ARMED_TWICE          256u  /* a WAIT call while the socket has an armed one: -EWOULDBLOCK */
#define SRT_UDPSEND_REOPEN_BUSY          512u  /* OPEN on a slot that still holds messages: ignored */
#define SRT_UDPSEND_LATE_RESULT_OVERFLOW 1024u /* more late results than late_results_cap */
#define SRT_UDPSEND_CALL_ORDER           2048u /* a call earlier than one before it in its host's list: not taken */

/* a socket slot's state, 48 bytes; UINT64_MAX: none */
typedef struct {
    uint64_t len_bytes; /* TIOCOUTQ */
    uint64_t soft_limit;
    uint64_t armed_seq; /* the blocked send's sequence number */
    uint32_t n_msgs;
    uint32_t bound_ip_be;
    uint32_t peer_ip_be;
    uint16_t bound_port_be;
    uint16_t peer_port_be;
    uint8_t open;
    uint8_t shut_wr;
    uint8_t bound;
    uint8_t has_peer;
    uint8_t overflow; /* 1: the slot's ring overflowed, its host's results are invalid since */
    uint8_t reserved0;
    uint16_t reserved1;
} srt_udpsend_socket_state;

/* one host's state: srt_outbound_host_state's fields, then the counter */
typedef struct {
    uint64_t balance;
    uint64_t last_refill_ns;
    uint64_t task_ns;
    uint64_t tasks_scheduled;
    uint64_t sent_total;
    uint64_t queue_len;
    uint32_t cached;
    uint32_t overflow;
    uint64_t next_priority;
} srt_udpsend_host_state;

/* An instance for n_hosts hosts on the plan's device and stream, or, with plan
 * == NULL, host-only: every array argument named d_ is then a HOST pointer and
 * the calls complete before they return.  Both forms run the same step and
 * agree byte for byte.  socket_ptr as for srt_udprecv_create; host_ip_be and
 * bw_up_bytes_per_s: HOST pointers, n_hosts entries; qdisc: SRT_QDISC_*.
 * ring_cap is the number of messages a socket may hold ACROSS calls; inside a
 * call a socket's queue is as long as the call's list makes it.  A host's
 * slots * (ring_cap + 1) and late_cap_hint are below 2^31 (SRT_ERR_INVALID);
 * late_cap_hint sizes nothing yet.  Memory of the instance, in bytes:
 *   64 + n_hosts * 112 + n_sockets * (88 + 4 + (ring_cap + 1) * 32)
 *      + (n_hosts + 1) * 4 + max(n_sockets + n_hosts, 1024) * 16 + n_calls * 32
 * (the call-wide words; per host its state record; per slot its state record,
 * its place in its host's qdisc array and its ring of messages with one spare
 * element for a woken send of an earlier call; socket_ptr; the configuration
 * steps of one launch; a 32-byte staged record per call of the largest n_calls
 * seen; each part rounded up to a multiple of 16, and 16 spare bytes), on the
 * device.  The staged records are the one thing that grows: the first run, and
 * a run with more calls than any before, wait for the stream and reallocate
 * them; no other run allocates or waits.  Buckets start full, last refill at
 * 0, next_priority at 1.  Destroy the instance before its plan. */
srt_status srt_udpsend_create(srt_plan *plan, uint32_t n_hosts, const uint32_t *socket_ptr, const uint32_t *host_ip_be,
                              const uint64_t *bw_up_bytes_per_s, uint32_t qdisc, uint32_t ring_cap,
                              uint32_t late_cap_hint, srt_udpsend **out, srt_err *err);

/* Configuration between runs: n steps (HOST pointer), applied in list order,
 * as srt_udprecv_config applies its own (every call first waits for the
 * stream: batch a window's steps into one call).  A slot >= n_sockets (a host
 * >= n_hosts for SET_NEXT_PRIORITY) or an unknown op returns SRT_ERR_INVALID
 * and changes NOTHING.  OPEN gives an empty, unbound, unconnected socket with
 * the limit as given; on a slot that still holds messages (open, or closed and
 * still draining) it is ignored and flagged REOPEN_BUSY.  Every other socket
 * step on a slot that is not open is ignored.  A limit set below len_bytes
 * leaves the socket without space until pops drain it. */
srt_status srt_udpsend_config(srt_udpsend *us, const srt_udpsend_op *ops, uint64_t n, srt_err *err);

/* One scheduling window.  d_calls: n_calls (< 2^31) records grouped by host
 * through d_call_host_ptr (n_hosts + 1 entries), each host's in issue order
 * with nondecreasing time_ns inside [previous until_ns, until_ns).  Every call
 * runs at its time_ns and every forward task with a time < until_ns runs.
 * Outputs: d_results[i] for every call; d_pds_status / d_send_ns / d_send_rank
 * [n_calls], d_late (late_cap records) / *d_late_count and *seq_base exactly as
 * srt_outbound_run defines them, indexed by call: a call that was not accepted
 * keeps status 0 and UINT64_MAX, an accepted one is a packet under the
 * sequence number *seq_base + its index (a UDP packet's status has SND_CREATED
 * from its pop on); d_late_results (late_results_cap records, any order) /
 * *d_late_results_count: the armed sends of earlier calls that completed;
 * d_first_writable_ns[slot] for every slot: see above, else UINT64_MAX.
 * Conditions, collected for srt_udpsend_status; every write is range-checked
 * first, a flagged call never writes out of bounds:
 *   RING_OVERFLOW    the newest messages beyond ring_cap are lost, the slot and
 *                    its host are marked and only that host's results are invalid;
 *   LATE_OVERFLOW, LATE_RESULT_OVERFLOW   the records beyond the cap are lost;
 *   TIME_REGRESSION, CALL_ORDER, AFTER_UNTIL   the call is not taken;
 *   OVERSIZE         srt_outbound's rule;
 *   BAD_SOCKET, UNBOUND, LOOPBACK, ARMED_TWICE   as above.
 * Asynchronous on the plan's stream, two launches: it does not wait for the
 * device, except where the staged records grow (srt_udpsend_create). */
srt_status srt_udpsend_run(srt_udpsend *us, const uint32_t *d_call_host_ptr, const srt_udp_send *d_calls,
                           uint64_t n_calls, uint64_t until_ns, uint64_t bootstrap_end_ns,
                           srt_udpsend_result *d_results, uint32_t *d_pds_status, uint64_t *d_send_ns,
                           uint64_t *d_send_rank, srt_outbound_late *d_late, uint32_t late_cap, uint32_t *d_late_count,
                           srt_udpsend_late *d_late_results, uint32_t late_results_cap, uint32_t *d_late_results_count,
                           uint64_t *d_first_writable_ns, uint64_t *seq_base, srt_err *err);

/* Synchronises the stream.  *flags (may be NULL): the SRT_UDPSEND_* conditions
 * met since the last status call (then cleared); *n_pending: packets still in
 * the stage after the last run; *n_accepted / *n_would_block / *n_armed: calls
 * accepted (raw arrivals and woken sends included), answered -EWOULDBLOCK, and
 * armed, since create.  SRT_ERR_INVALID, with a message that names every flag
 * set, when any was; else SRT_OK. */
srt_status srt_udpsend_status(srt_udpsend *us, uint32_t *flags, uint64_t *n_pending, uint64_t *n_accepted,
                              uint64_t *n_would_block, uint64_t *n_armed, srt_err *err);

/* Synchronises and copies every host's state to hosts[n_hosts] and every slot's
 * to socks[n_sockets] (HOST pointers; either may be NULL). */
srt_status srt_udpsend_state(srt_udpsend *us, srt_udpsend_host_state *hosts, srt_udpsend_socket_state *socks,
                             srt_err *err);

/* srt_outbound_cached_seq for this stage: d_seq[h] = the sequence number of the
 * packet host h's relay holds cached after the last run, or UINT64_MAX.
 * Asynchronous on the plan's stream.  For srt_tracker_tx. */
srt_status srt_udpsend_cached_seq(srt_udpsend *us, uint64_t *d_seq, srt_err *err);

/* The LDS a workgroup (one wave, 64 hosts) of the step kernel asks for, in
 * bytes: 1536 staged calls of 32 bytes (a wave whose hosts' calls are more is
 * walked in device memory instead), then 320 slot state records of 88 bytes and
 * their 320 qdisc entries (a wave whose hosts own more slots keeps them in
 * device memory): 78,592, two workgroups a CU. */
uint32_t srt_udpsend_window_bytes(void);
void srt_udpsend_destroy(srt_udpsend *us);

/* ---------------------------------------------------- IP assignment (a10) */
/* IpAssignment<u32> (src/main/network/graph/mod.rs:352-420): IPv4 address ->
 * GML node id.  Addresses cross the ABI in network byte order, as Shadow's C
 * exports pass them (in_addr_t, worker.rs:669-700).  Single-threaded use
 * (sim_config.rs:399-420 fills it once, on the main thread). */
typedef struct srt_ip_assignment srt_ip_assignment;
srt_status srt_ip_assignment_create(srt_ip_assignment **out);
void srt_ip_assignment_destroy(srt_ip_assignment *ia);
/* assign_ip (mod.rs:383-394): SRT_ERR_INVALID "IP address has already been
 * assigned" (IpPreviouslyAssignedError) when the address is taken */
srt_status srt_ip_assignment_assign_ip(srt_ip_assignment *ia, uint32_t node_id, uint32_t ipv4_be, srt_err *err);
/* assign (mod.rs:371-381): the next free address after the last one assign
 * handed out, from 11.0.0.1 upward, skipping *.0 and *.255 (:406-420);
 * returns it (network byte order) */
uint32_t srt_ip_assignment_assign(srt_ip_assignment *ia, uint32_t node_id);
/* get_node (mod.rs:397-399): 1 and *node_id, or 0 (None) */
int srt_ip_assignment_get_node(const srt_ip_assignment *ia, uint32_t ipv4_be, uint32_t *node_id);
/* get_nodes (mod.rs:402-404): the distinct assigned node ids, ascending, up to
 * cap of them into out (may be NULL); returns how many there are */
uint32_t srt_ip_assignment_get_nodes(const srt_ip_assignment *ia, uint32_t *out, uint32_t cap);
uint32_t srt_ip_assignment_size(const srt_ip_assignment *ia);

/* The assignment frozen against a routing table for the send path: IPv4 ->
 * table row (the row of the address's node; row_ids[i] = GML id of table row
 * i, e.g. the in-use nodes in srt_routing_info / srt_plan order).  Replaces the
 * two get_node lookups + the path() hash of every WorkerShared::latency /
 * reliability call (worker.rs:539-553).  Immutable: thread-safe. */
typedef struct srt_ip_resolver srt_ip_resolver;
srt_status srt_ip_resolver_create(const srt_ip_assignment *ia, const uint32_t *row_ids, uint32_t n_rows,
                                  srt_ip_resolver **out, srt_err *err);
void srt_ip_resolver_destroy(srt_ip_resolver *r);
/* host batch: rows[i] = table row of ips_be[i], -1 when the address is not
 * assigned or its node has no row (the reference's None) */
srt_status srt_ip_resolve_rows(const srt_ip_resolver *r, const uint32_t *ips_be, uint64_t n, int32_t *rows);

/* A packet by address: srt_pkt with the table row / column replaced by the
 * source / destination IPv4 (network byte order, packet_getSourceIP /
 * packet_getDestinationIP, worker.rs:341-345).  Same 24-byte layout. */
typedef struct {
    uint32_t src_host;
    uint32_t src_ip;
    uint32_t dst_ip;
    uint32_t payload_size;
    uint64_t t_ns;
} srt_pkt_ip;
/* srt_packet_batch with each packet's addresses resolved on the device
 * through `res` (its table is uploaded to the plan's device on first use).
 * Asynchronous like srt_packet_batch: a packet that is not completed and has
 * an address without a row (the reference's reliability(..).unwrap() panic,
 * worker.rs:359) is reported by the next srt_packet_status. */
srt_status srt_packet_batch_ip(srt_plan *plan, srt_ip_resolver *res, const srt_pkt_ip *d_pkts,
                               const uint32_t *d_host_pkt_ptr, uint32_t n_hosts, uint64_t n_pkts, uint64_t *d_rng,
                               const srt_round *round, uint32_t *d_flags, uint64_t *d_deliver, uint64_t *d_counters,
                               uint64_t *d_stats, srt_err *err);
/* Synchronises the plan's stream; SRT_ERR_INVALID if an srt_packet_batch_ip
 * since the last check met an unresolvable address, else SRT_OK. */
srt_status srt_packet_status(srt_plan *plan, srt_err *err);

/* ------------------------------------------------------ host RNG (a12) */
/* The host's Xoshiro256PlusPlus (host.rs:122, 233; rand_xoshiro 0.6.0) as the
 * 4 x u64 state srt_packet_batch advances.  Host-side helpers so the caller
 * can seed states, continue a stream on the host (the syscalls' draws,
 * host.rs:1373-1385) and check the hand-off; see INTEGRATION.md section 4. */
/* seed_from_u64 (SplitMix64 outputs as the four words) */
void srt_xoshiro_seed_from_u64(uint64_t seed, uint64_t state[4]);
/* count next_u64 draws (out may be NULL), state advanced in place */
void srt_xoshiro_next_u64(uint64_t state[4], uint64_t count, uint64_t *out);
/* a host's node_seed (sim_config.rs:47-53, 222-244): the first next_u64 of
 * seed_from_u64(general_seed) ^ DefaultHasher(hostname) (SipHash-1-3) */
uint64_t srt_host_node_seed(uint32_t general_seed, const char *hostname, size_t len);

/* ------------------------------------------------------------- RoutingInfo */
/* Dense RoutingInfo keyed by GML node ids: replaces the
 * HashMap<(u32,u32), PathProperties> and the RwLock<HashMap> packet counters of
 * RoutingInfo (mod.rs:428-477), and the NodeIndex -> GML id re-keying of every
 * pair in generate_routing_info (sim_config.rs:436-458): the table stays
 * row-major over the in-use nodes and a GML id -> row map resolves ids.
 * Thread-safe for concurrent path() / increment_packet_count() calls (worker
 * threads); build and destroy from one thread. */
typedef struct srt_routing_info srt_routing_info;

/* generate_routing_info (sim_config.rs:424-461) in one call: the in-use nodes
 * are NodeIndex values (node_id_to_index of the GML ids); use_shortest_paths
 * selects srt_compute_shortest_paths (mod.rs:183-228) or srt_get_direct_paths
 * (mod.rs:230-252); g->node_ids gives the GML ids (NULL: NodeIndex).  Errors
 * as those functions'. */
srt_status srt_routing_info_build(const srt_csr *g, const uint32_t *nodes, uint32_t n, int use_shortest_paths,
                                  const srt_opts *opts, srt_routing_info **out, srt_err *err);
/* The same over a plan that has run (srt_plan_run): fetches its table. */
srt_status srt_routing_info_from_plan(srt_plan *plan, srt_routing_info **out, srt_err *err);
/* RoutingInfo::path (mod.rs:444-446): SRT_OK and *out, or SRT_ERR_INVALID when
 * either GML id is not an in-use node (the reference's None). */
srt_status srt_routing_info_path(const srt_routing_info *ri, uint32_t src_id, uint32_t dst_id, srt_path *out);
/* RoutingInfo::increment_packet_count (mod.rs:449-456): saturating +1 (an id
 * that is not in use is ignored: the reference would panic on the missing
 * path when logging) */
void srt_routing_info_increment_packet_count(srt_routing_info *ri, uint32_t src_id, uint32_t dst_id);
/* adds a device round's per-pair counters (srt_packet_batch's n*n array,
 * copied to the host) into the counters, saturating */
void srt_routing_info_add_packet_counts(srt_routing_info *ri, const uint64_t *counts);
uint64_t srt_routing_info_packet_count(const srt_routing_info *ri, uint32_t src_id, uint32_t dst_id);
/* RoutingInfo::get_smallest_latency_ns (mod.rs:474-476): 0 = None (empty), 1 = *out set */
int srt_routing_info_smallest_latency_ns(const srt_routing_info *ri, uint64_t *out);
/* table row of a GML id (the srt_pkt src_row / dst_row of its host), -1 if not in use */
int64_t srt_routing_info_row(const srt_routing_info *ri, uint32_t gml_id);
uint32_t srt_routing_info_size(const srt_routing_info *ri);
/* Storage of the table.  srt_routing_info_build keeps the dense build's table
 * in the record form it was downloaded in and decodes in path(): 6 bytes a
 * pair (latency / g as u16 + f32 loss) for u16-key closures (C1-C3: 1.6 GB
 * at 16k nodes instead of 4.3 GB of srt_path), 8 bytes (u32 + f32) for other
 * closures whose latencies fit u32 units, else srt_path; the diagonal (the
 * raw self-loops) is kept apart. */
#define SRT_RI_PATH16 16  /* srt_path records */
#define SRT_RI_REC8 8     /* {latency / g u32, loss f32} */
#define SRT_RI_REC6 6     /* latency / g u16 array + loss f32 array */
int srt_routing_info_record_bytes(const srt_routing_info *ri);
/* the dense table as srt_path, row-major size x size, rows in in-use order
 * (read-only) -- only for SRT_RI_PATH16 storage, else NULL (use path() or
 * srt_routing_info_copy_table) */
const srt_path *srt_routing_info_table(const srt_routing_info *ri);
/* the whole table decoded into out[size * size] (any storage) */
void srt_routing_info_copy_table(const srt_routing_info *ri, srt_path *out);
void srt_routing_info_destroy(srt_routing_info *ri);

/* --------------------------------------------------------------- start-up */
/* Shadow builds the routing info once, at setup (sim_config.rs:136-140 ->
 * generate_routing_info, sim_config.rs:424-461), so that one call is a cold
 * one: it would pay the HIP runtime start, the load of this library's kernels
 * and the pinning of the transfer staging on top of the build.  srt_init does
 * those three on `device` (-1: the current device) and returns when done;
 * srt_init_async starts it on a library thread and returns at once, so the
 * simulator can call it first thing in main and parse its config and GML
 * graph meanwhile.  Every build (and srt_init) waits for a pending init.
 * Idempotent; errors of an async init surface in the next srt_init call.
 * Exit during an async init is safe without the caller's help: the calling
 * thread's exit (return from main, exit()) joins the init thread before any
 * atexit handler or static destructor runs.  srt_init_wait only waits for a
 * pending async init (no device work). */
srt_status srt_init(int device, srt_err *err);
void srt_init_async(int device);
void srt_init_wait(void);

/* --------------------------------------------------------------- GML ingest */
/* Parses Shadow GML text (gml-parser grammar + NetworkGraph validation) into a
 * library-owned graph; srt_gml_csr exposes its petgraph adjacency. */
typedef struct srt_gml srt_gml;
srt_status srt_gml_parse(const char *text, size_t len, srt_gml **out, srt_err *err);
srt_status srt_gml_csr(const srt_gml *g, srt_csr *csr);
void srt_gml_free(srt_gml *g);

/* load_network_graph's file sources (mod.rs:494-509) + NetworkGraph::parse:
 * reads `path`, decompresses it when xz != 0 (read_xz, mod.rs:479-492: the
 * .xz container with LZMA2 blocks and CRC32 / CRC64 / SHA-256 / no checks,
 * what lzma-rs 0.3.0 decodes), checks UTF-8 (String::from_utf8) and parses.
 * Errors carry the reference's contexts: "Failed to open file: \"{path}\""
 * / "Failed to read file: {path}" / "Failed to decompress file: ...". */
srt_status srt_gml_parse_file(const char *path, int xz, srt_gml **out, srt_err *err);
/* read_xz's decompression alone: *out (library-allocated, free with srt_free,
 * NUL-terminated for convenience) holds *out_len decompressed bytes */
srt_status srt_xz_decompress(const uint8_t *in, size_t len, uint8_t **out, size_t *out_len, srt_err *err);
void srt_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* SRT_H */
