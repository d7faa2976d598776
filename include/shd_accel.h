/*
 * shd_accel.h -- C ABI of the MI355X (gfx950) engine for Shadow's two data-parallel paths:
 *
 *   1. the routing build: lexicographic (latency, then packet loss) shortest paths over the
 *      GML network graph into the dense used-node RoutingInfo table, and the direct-path mode;
 *   2. the per-round inter-host packet relay: path latency/loss lookup, seeded per-host loss
 *      draw, delivery-time stamping, and the sort-merge of packet events into destination
 *      hosts' event queues.
 *
 * Plain C types only (no torch / HIP types); caller-owned host buffers unless a function says
 * "device".  No panic or C++ exception crosses this boundary: every entry point returns a
 * shd_status.  One shd_ctx per GPU; a context is not thread-safe (the reference calls the
 * routing build once from the setup thread and flushes the relay once per round from the
 * manager thread).
 *
 * Reference interfaces replaced (FlyearthR/shadow, Shadow 3.0.0):
 *   shd_routing_build      <- NetworkGraph::compute_shortest_paths / get_direct_paths
 *                             (src/main/network/graph/mod.rs:185-254), called from
 *                             generate_routing_info (src/main/core/sim_config.rs:424-461)
 *   shd_routing_lookup     <- RoutingInfo::path (graph/mod.rs:446-448),
 *                             WorkerShared::{latency,reliability} (src/main/core/worker.rs:529-543)
 *   shd_routing_smallest_latency <- RoutingInfo::get_smallest_latency_ns (graph/mod.rs:476-478)
 *   shd_relay_setup        <- WorkerShared tables built in Manager::run (core/manager.rs:309-332)
 *                             + per-host RNG / event-id counter (src/main/host/host.rs:218,580-584)
 *   shd_relay_round        <- the body of Worker::send_packet (src/main/core/worker.rs:328-413)
 *                             for every send of one scheduling round, flushed at the round
 *                             barrier (core/manager.rs:455-464), plus push_packet_to_host /
 *                             EventQueue::push (worker.rs:619-629, core/work/event_queue.rs:28-48)
 *   shd_path_packet_counts <- RoutingInfo::increment_packet_count / log_packet_counts
 *                             (graph/mod.rs:451-474)
 *   shd_offers_group       <- notify_socket_has_packets -> Relay::notify (relay/mod.rs:110-135), the
 *                             staging site: the thread running the host appends the offer to its stage
 */
#ifndef SHD_ACCEL_H
#define SHD_ACCEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHD_ABI_VERSION 12

typedef enum shd_status {
    SHD_OK = 0,
    SHD_ERR_NO_EDGE = 1,          /* "No edge connecting node {a} to {b}"      graph/mod.rs:267-270 */
    SHD_ERR_MULTI_EDGE = 2,       /* "More than one edge connecting node .."   graph/mod.rs:271-276 */
    SHD_ERR_UNREACHABLE = 3,      /* reference panics: assert paths.len()==n^2 graph/mod.rs:221 */
    SHD_ERR_LATENCY_OVERFLOW = 4, /* a path latency does not fit u64 ns (reference: overflow panic) */
    SHD_ERR_INVALID = 5,          /* bad argument (null pointer, index out of range, ...)          */
    SHD_ERR_HIP = 6,              /* HIP runtime failure                                           */
    SHD_ERR_NOMEM = 7,            /* host or device allocation failed                              */
    SHD_ERR_NO_HOST = 8,          /* "No host ID for dest address"              worker.rs:350-355 */
    SHD_ERR_STATE = 9             /* call order violated (e.g. relay before setup)                 */
} shd_status;

typedef struct shd_ctx shd_ctx;

/* Error detail; node ids are GML ids (graph/mod.rs:263-264 reports GML ids). */
typedef struct shd_error {
    int32_t code;      /* shd_status */
    uint32_t node_a;
    uint32_t node_b;
} shd_error;

/*
 * Network graph after GML parsing (NetworkGraph, graph/mod.rs:115-183).  Node indices are the
 * petgraph NodeIndex values (= GML node order); edges are in GML order.  edge_latency_ns is
 * ShadowEdge.latency converted to ns (units.rs:377-388), edge_packet_loss the raw f32.
 */
typedef struct shd_graph {
    uint32_t n_nodes;
    uint32_t n_edges;
    const uint32_t* edge_src;        /* node index, [n_edges] */
    const uint32_t* edge_dst;        /* node index, [n_edges] */
    const uint64_t* edge_latency_ns; /* [n_edges], > 0 */
    const float* edge_packet_loss;   /* [n_edges], in [0,1] */
    const uint32_t* node_ids;        /* GML id per node index [n_nodes]; NULL => id == index */
    int32_t directed;                /* GML 'directed' (default 0) */
} shd_graph;

/* Routing modes (network.use_shortest_path, configuration.rs:276; sim_config.rs:442-458). */
#define SHD_ROUTE_SHORTEST 0u
#define SHD_ROUTE_DIRECT 1u

/* Algorithm selection for SHD_ROUTE_SHORTEST (all produce identical bits). */
#define SHD_ALGO_AUTO 0u     /* dense graphs: 2-hop prune + SSSP; sparse: SSSP           */
#define SHD_ALGO_SSSP 1u     /* batched per-source label-correcting SSSP, labels in LDS   */
#define SHD_ALGO_PRUNED 2u   /* dense k-nearest 2-hop edge prune, then SSSP               */
#define SHD_ALGO_DELTA 3u    /* delta-stepping buckets inside the per-source SSSP         */
#define SHD_ALGO_BLOCKED 4u  /* blocked min-plus (Floyd-Warshall) latency + tight-DAG loss */

typedef struct shd_routing_info {
    uint32_t algo_used;        /* SHD_ALGO_* that ran */
    uint32_t wide_latency;     /* 1 if the u64-latency kernels ran (a path >= 2^32-1 ns) */
    uint64_t arcs;             /* arcs after parallel-edge reduction */
    uint64_t arcs_kept;        /* arcs after pruning (== arcs when no prune ran) */
    double ms_total;           /* device time of the last build (HIP events) */
    double ms_main;            /* device time of the dominant kernel; -1 when this call was not
                                  timed (shd_routing_set_timing) */
    double ms_minplus;         /* SHD_ALGO_BLOCKED: device time of the min-plus closure */
} shd_routing_info;

/* ---------------------------------------------------------------- context */
const char* shd_version(void);
const char* shd_status_str(shd_status st);
shd_ctx* shd_open(int device_ordinal, shd_status* st);
void shd_close(shd_ctx* ctx);
/* Stream for all device work of this context (a hipStream_t passed as void*; NULL => the
 * context's own stream).  Lets a caller order the engine behind its own stream. */
shd_status shd_set_stream(shd_ctx* ctx, void* hip_stream);
/* Tuning and testing knobs of this context (no reference counterpart).  No knob changes a result:
 * they pick grids, kernel variants or an equivalent fallback pipeline.  Every knob starts from the
 * environment variable SHD_<name>, read ONCE by shd_open, so the process environment cannot change
 * a context's grids between two calls; shd_set_knob overrides one for this context (value < 0: back
 * to the built-in default), shd_get_knob reads it (-1: the built-in default applies).  `name` is
 * spelled with or without the SHD_ prefix (e.g. "SSSP_SLOTS"); an unknown name is SHD_ERR_INVALID.
 * Relay pipeline knobs (RELAY_FORCE_*, RELAY_NO_LDS_MAP) apply from the next shd_relay_setup.
 * UPDATE_REPREPARES is a read-only counter: the shd_routing_update_edges calls of this context that
 * prepared the graph again in place of patching it (shd_set_knob refuses it). */
shd_status shd_set_knob(shd_ctx* ctx, const char* name, int64_t value);
shd_status shd_get_knob(const shd_ctx* ctx, const char* name, int64_t* value);

/* ---------------------------------------------------------------- routing build */
/*
 * Build rows [row_begin, row_end) of the n_used x n_used table (row-major in `used` order;
 * row_end == 0 means n_used).  lat_out/loss_out receive (row_end-row_begin) * n_used entries;
 * either may be NULL, in which case the table stays only device-resident in the context.
 * Diagonal = the node's single self-loop edge (graph/mod.rs:212-219).  Errors are reported
 * for the whole used set exactly as the reference: missing/multiple self-loop -> NO_EDGE /
 * MULTI_EDGE on the first such node in `used` order; unreachable pair -> UNREACHABLE.
 */
shd_status shd_routing_build(shd_ctx* ctx, const shd_graph* g, const uint32_t* used,
                             uint32_t n_used, uint32_t mode, uint32_t algo,
                             uint32_t row_begin, uint32_t row_end,
                             uint64_t* lat_out, float* loss_out, shd_error* err);

/*
 * Two-phase form of the same build (what a caller that rebuilds, shards or benchmarks uses):
 * shd_routing_prepare validates the graph and the used set, applies the self-loop rule and
 * uploads the arc CSR (device-resident in the context); shd_routing_run then computes rows
 * [row_begin, row_end) from the resident graph into device buffers on the context's stream
 * (NULL outputs => the context's resident table).  Errors as for shd_routing_build.
 */
shd_status shd_routing_prepare(shd_ctx* ctx, const shd_graph* g, const uint32_t* used,
                               uint32_t n_used, uint32_t mode, shd_error* err);
shd_status shd_routing_run(shd_ctx* ctx, uint32_t algo, uint32_t row_begin, uint32_t row_end,
                           uint64_t* d_lat_out, float* d_loss_out, shd_error* err);

/*
 * New weights for n edges of the context's prepared graph (shd_routing_prepare's or
 * shd_routing_build's), patched into the resident arc arrays: a network whose latencies drift or
 * whose links degrade or fail (packet_loss 1.0) is rebuilt by shd_routing_run alone, without a new
 * prepare.  (No reference counterpart: its RoutingInfo is built once, sim_config.rs:424-461.)
 * edge_index[i] is the edge's position in shd_graph's edge arrays (GML order); topology, used set,
 * mode and directedness stay as prepared.  Every later shd_routing_run, _run_next_hops,
 * _run_sharded and lookup after a run equals a fresh prepare of the modified graph bit for bit
 * (latency, loss bits, next hops, error codes with their node ids, shd_routing_info.arcs and
 * arcs_kept).
 *   Validation: the whole call is checked before anything changes; a refused call leaves the
 *     graph as it was.  SHD_ERR_STATE: no prepared graph.  SHD_ERR_INVALID: a NULL array with
 *     n > 0, an index >= n_edges, latency 0, loss outside [0, 1] or NaN (shd_routing_prepare's
 *     rules).  n == 0 is SHD_OK and does nothing.
 *   Duplicates: an edge named more than once takes its last entry.
 *   Arcs per edge: an undirected edge changes both of its arcs; a parallel edge only its own; a
 *     self-loop changes its node's diagonal entry (raw loss bits) if the node is used, and no arc.
 *   Resident table: not touched.  It stays the old network's until the next run, a relay on it
 *     keeps working until that run, and shd_routing_mirror follows its usual rule.
 *   Wide latencies (shortest mode): if some arc is >= 2^32 - 1 ns before the call, or an entry of
 *     the call is, the graph is prepared again from the context's own copies with the new weights
 *     (same results, a slower call; shd_get_knob counts such calls as UPDATE_REPREPARES).  Direct
 *     mode keeps the edges' u64 latencies and always patches in place.
 *   Cost: the first call after a prepare builds the edge -> arc map (O(n_edges log)); every later
 *     call is O(n) host work, 16 n bytes of upload and three launches, with one synchronisation.
 *   Communicator: no collective.  Under a communicator every rank applies the same updates.
 */
shd_status shd_routing_update_edges(shd_ctx* ctx, uint64_t n, const uint32_t* edge_index,
                                    const uint64_t* latency_ns, const float* packet_loss, shd_error* err);

/*
 * shd_routing_run plus next hops (the north star's; the reference keeps none: petgraph's
 * dijkstra returns scores only, graph/mod.rs:197-200).  Definition, identical for
 * every engine: pred(s, v) = the LOWEST node index u with an arc u -> v (u != v) whose final
 * label extended by that arc equals v's label bit for bit (latency and left-folded loss);
 * next_hop(s, d) = the node after s on d's pred chain, next_hop(s, s) = s (the self-loop), and
 * in direct mode the destination itself.  d_next_hop (device) receives (row_end - row_begin) x
 * n_used node indices (GML order); UINT32_MAX never appears in a successful build.
 */
shd_status shd_routing_run_next_hops(shd_ctx* ctx, uint32_t algo, uint32_t row_begin, uint32_t row_end,
                                     uint64_t* d_lat_out, float* d_loss_out, uint32_t* d_next_hop,
                                     shd_error* err);

/* As shd_routing_build, writing the rows straight into device buffers (hipMalloc'd or torch
 * tensors) on the context's stream; the call returns when the rows are complete. */
shd_status shd_routing_build_device(shd_ctx* ctx, const shd_graph* g, const uint32_t* used,
                                    uint32_t n_used, uint32_t mode, uint32_t algo,
                                    uint32_t row_begin, uint32_t row_end,
                                    uint64_t* d_lat_out, float* d_loss_out, shd_error* err);

shd_status shd_routing_last_info(const shd_ctx* ctx, shd_routing_info* info);

/* Time the dominant kernel on every `every`-th build (default 1 = every build; 0 = never).
 * The duration comes from HIP events recorded with that kernel's dispatch on the context's
 * stream; they cost a few microseconds of queue gap, which a caller timing many builds can
 * spread by sampling. */
shd_status shd_routing_set_timing(shd_ctx* ctx, uint32_t every);

/* Look up one pair of the resident table (row index relative to row_begin of the last build).
 * After shd_routing_mirror the lookup reads the pinned host mirror (no device round trip: what a
 * worker_getLatency-rate caller -- worker.rs:660-670, tcp.c:451-452 -- needs); otherwise it copies
 * the pair from the device. */
shd_status shd_routing_lookup(shd_ctx* ctx, uint32_t src_row, uint32_t dst_col,
                              uint64_t* latency_ns, float* packet_loss);
/* n lookups in one device gather and one copy (host arrays; any output may be NULL). */
shd_status shd_routing_lookup_batch(shd_ctx* ctx, uint64_t n, const uint32_t* src_row, const uint32_t* dst_col,
                                    uint64_t* latency_ns, float* packet_loss);
/* Keep a pinned host copy of the resident table (rows x cols x 12 B) for host-side lookups; it is
 * dropped with the resident table (the next build or prepare).  enable = 0 drops it. */
shd_status shd_routing_mirror(shd_ctx* ctx, int32_t enable);
shd_status shd_routing_smallest_latency(shd_ctx* ctx, uint64_t* latency_ns);

/*
 * assign_ips (src/main/core/sim_config.rs:399-420) with IpAssignment (graph/mod.rs:354-422),
 * host code: hosts in HostId order; ip_in[h] = the host's configured IPv4 address (host byte
 * order, 11.0.0.1 = 0x0B000001) or 0 for none (ip_in may be NULL: no host has one).  Configured
 * addresses are registered first (a repeat is SHD_ERR_INVALID, *err_host = that host: "IP address
 * has already been assigned"); every other host gets the next free address after the last one
 * handed out, from 11.0.0.1 on, skipping x.x.x.0 and x.x.x.255.  ip_out[n_hosts] receives every
 * host's address; used_gml (capacity n_hosts, may be NULL) the ids of the nodes that own an
 * address, ascending (IpAssignment::get_nodes, the `nodes` of generate_routing_info,
 * sim_config.rs:424-461), *n_used their count; host_col (may be NULL) each host's column in
 * that list -- the relay's host -> node map (shd_relay_setup).
 */
shd_status shd_assign_ips(uint32_t n_hosts, const uint32_t* node_gml_id, const uint32_t* ip_in,
                          uint32_t* ip_out, uint32_t* used_gml, uint32_t* n_used, uint32_t* host_col,
                          uint32_t* err_host);

/* ---------------------------------------------------------------- relay */
/*
 * Host tables for the relay: host -> used-node index (IpAssignment + RoutingInfo keys,
 * worker.rs:529-543), the n_nodes x n_nodes table (NULL => the context's resident table from
 * the last full routing build), each host's Xoshiro256++ state (4 x u64, host.rs:218) and next
 * event id (host.rs:580-584).  A relay set up on the resident table stops at the next
 * shd_routing_prepare / shd_routing_build / resident shd_routing_run (relay calls return
 * SHD_ERR_STATE until it is set up again); caller-passed tables are copied and stay valid.
 */
shd_status shd_relay_setup(shd_ctx* ctx, uint32_t n_hosts, const uint32_t* host_node,
                           uint32_t n_nodes, const uint64_t* lat, const float* loss,
                           const uint64_t* rng_state, const uint64_t* next_event_id);

/*
 * A new n_nodes x n_nodes table under a relay that keeps everything else (no reference
 * counterpart; the pair shd_routing_update_edges + resident shd_routing_run + shd_relay_retable
 * changes the network between two windows).  lat == loss == NULL: the context's resident table,
 * which must be a full build with n_nodes columns (else SHD_ERR_STATE); host arrays are copied as
 * in shd_relay_setup.
 *   Kept: the host -> node map, the stamp order, both buffers of RNG states and event ids, the
 *     bound of the event ids, the path packet counters (they go on accumulating), the sharding
 *     and the knobs read at setup.  Recomputed: the table's width (the pipeline choice) and its
 *     packed form.
 *   The call revives a relay that a resident run stopped.  SHD_ERR_STATE: a relay never set up,
 *     or set up before the context's communicator was created, replaced or (a sharded relay)
 *     destroyed: its shard and exchange buffers follow the communicator, so shd_relay_setup again.
 *   SHD_ERR_INVALID: n_nodes differs from the setup's; only one of the two arrays is NULL; or the
 *     runahead is set up and the new table's smallest latency is 0 (Runahead::new asserts a
 *     non-zero minimum).  A refused call leaves a running relay running on its old table.
 *   The table takes effect from the next round.  Queues, ledger, both stages and an open window
 *     are not touched: the call may come between shd_window_close and the next shd_window_open,
 *     or between an open and its close.
 *   Runahead: if it is set up, min_possible becomes the smallest latency of the table the relay
 *     now uses and the lowest used latency is forgotten (manager.rs:246-251 takes min_possible
 *     from RoutingInfo; a latency observed on the old network says nothing about the new one).
 *     The pending relay output's earliest deliver time is kept -- shd_runahead_setup would reset it.
 *   Communicator: local, no collective; every rank calls it.
 */
shd_status shd_relay_retable(shd_ctx* ctx, uint32_t n_nodes, const uint64_t* lat, const float* loss);

typedef struct shd_round {
    uint64_t round_end;      /* Worker::round_end_time */
    uint64_t sim_end;        /* WorkerShared::sim_end_time */
    uint64_t bootstrap_end;  /* WorkerShared::bootstrap_end_time */
} shd_round;

/*
 * One round's staged sends, grouped by source host: host h's sends are packets
 * [src_off[h], src_off[h+1]) in send order (src_off has n_hosts+1 entries).  chance may be
 * NULL: the engine then draws from the device-resident per-host streams; otherwise chance[i]
 * is the f64 the CPU drew from the host RNG at send time (worker.rs:365).
 */
typedef struct shd_batch {
    uint64_t n_packets;
    const uint32_t* src_off;
    const uint64_t* send_time;   /* emulated ns */
    const uint32_t* dst_host;    /* HostId after DNS resolution (worker.rs:350-355) */
    const uint32_t* payload;     /* packet_getPayloadSize */
    const double* chance;        /* optional */
} shd_batch;

#define SHD_PKT_SKIPPED 0u  /* now >= sim_end: returned before any effect (worker.rs:339-341) */
#define SHD_PKT_DROPPED 1u  /* PDS_INET_DROPPED (worker.rs:370-378) */
#define SHD_PKT_SENT 2u     /* PDS_INET_SENT + event pushed */

/*
 * Outputs (caller-owned host buffers, any may be NULL): status[n_packets]; the round's packet
 * events grouped by destination host in EventQueue pop order (event.rs:84-155):
 * ev_off[n_hosts+1], ev_deliver / ev_src / ev_seq / ev_pkt[n_sent] (ev_pkt = index of the
 * packet in the batch); min_deliver = min over sent deliver times (u64 max if none,
 * worker.rs:406); min_latency = min latency used (runahead.rs:60-115); n_sent.
 */
typedef struct shd_relay_out {
    uint8_t* status;
    uint32_t* ev_off;
    uint64_t* ev_deliver;
    uint32_t* ev_src;
    uint64_t* ev_seq;
    uint32_t* ev_pkt;
    uint64_t min_deliver;
    uint64_t min_latency;
    uint64_t n_sent;
    uint32_t n_dst;      /* destination hosts ev_off covers (ev_off has n_dst + 1 entries) */
    uint32_t n_events;   /* events in ev_* (= ev_off[n_dst]): n_sent on one GPU; a sharded round's
                            n_sent is the all-rank total, n_events what this rank received.  Both
                            are written by the relay calls; a caller building this struct for
                            shd_equeue_advance sets them (the queues check n_dst against their
                            host count and merge n_events events) */
} shd_relay_out;

shd_status shd_relay_round(shd_ctx* ctx, const shd_batch* batch, const shd_round* round,
                           shd_relay_out* out);

/* Device-buffer form (all pointers in shd_batch / shd_relay_out are device pointers; status,
 * ev_* must hold n_packets entries).  Used by the multi-GPU driver and the benchmark. */
shd_status shd_relay_round_device(shd_ctx* ctx, const shd_batch* d_batch, const shd_round* round,
                                  shd_relay_out* d_out);

/* ---------------------------------------------------------------- drop-in flush of staged sends */
/*
 * The round barrier of the drop-in (manager.rs:455-464) without any CPU reorder: the worker threads'
 * staging buffers go to the device as they are.  Each host runs on one worker thread per round
 * (scheduler/thread_per_core.rs:188-206), so its sends form ONE run (host, count) of consecutive
 * records in ONE stage (= one thread's buffer), in send order; stages and runs may come in any
 * order.  A staged send is 12 bytes (worker.rs:328-413 reads nothing else):
 *   time_off  now - time_base (ns; the round's window start is a natural time_base)
 *   dst       destination HostId (resolve_ip_to_host_id, worker.rs:350-355), | SHD_SEND_PAYLOAD
 *             when packet_getPayloadSize > 0 (the drop rule spares empty packets, :370)
 *   draw_hi   the source host's next_u64() >> 32 taken at send time -- in place of gen::<f64>()
 *             (:365), which consumes the same one next_u64, so the CPU stream advances as in the
 *             reference; the top 32 bits decide chance >= reliability exactly
 * The completed check (:334-341) stays on the CPU: staged sends have now < sim_end.
 * Outputs (host buffers; pinned -- shd_host_alloc -- for the link's full rate; any may be NULL):
 *   status2   2-bit SHD_PKT_* per send in stage order (stage 0's sends, then stage 1's, ...):
 *             send i in bits 2(i%4), 2(i%4)+1 of byte i/4; ceil(n/4) bytes
 *   ev_off    [n_hosts + 1]; events[ev_off[h], ev_off[h+1]) are host h's, in EventQueue order
 *   events    n_sent shd_event16 records
 *   seq_base  [n_hosts]: each host's first packet event id of this round (event id = seq_base[src]
 *             + seq_off)
 * Device RNG streams are not used (the draws are the CPU's); event ids, counters and the runahead
 * update as in shd_relay_round.  SHD_ERR_NO_HOST: a run's host or a destination is not a relay
 * host; SHD_ERR_INVALID: a host with two runs, or runs that do not cover a stage's records.
 *
 * Under a communicator of > 1 ranks (shd_relay_setup after it) every rank is handed the SAME
 * stages -- every worker thread's buffer, holding hosts of every shard -- and keeps its own hosts
 * [lo, hi) = shd_shard_range(n_hosts): the device groups every send (one pass, no CPU split), runs
 * its own hosts' sends through shd_relay_round_sharded and returns
 *   status2   every send in stage order: the own hosts' statuses, 0 for the other ranks' sends (an
 *             OR of the ranks' arrays gives every status)
 *   ev_off    [hi - lo + 1]; events: the own destinations' n_events events, seq_off relative to
 *             the source host's first id of the round and send = the index in stage order, for
 *             sources of any rank
 *   seq_base  entries [lo, hi) only (the ranks may share one array)
 *   min_deliver, min_latency, n_sent over all ranks.
 * A failed check (NO_HOST / INVALID runs) returns before the round's collectives on every rank
 * (they all see the same stages); a failure inside the round fails it on every rank.
 */
#define SHD_SEND_PAYLOAD 0x80000000u
typedef struct shd_send12 {
    uint32_t time_off;
    uint32_t dst;
    uint32_t draw_hi;
} shd_send12;

typedef struct shd_stage {
    uint32_t n_runs;
    const uint32_t* run_host;    /* [n_runs] source HostId of each run */
    const uint32_t* run_count;   /* [n_runs] its sends, consecutive in `sends` */
    uint64_t n_sends;
    const shd_send12* sends;     /* [n_sends] */
} shd_stage;

typedef struct shd_event16 {
    uint32_t deliver_off;   /* deliver time - round_end */
    uint32_t src_host;
    uint32_t seq_off;       /* src_host_event_id - seq_base[src_host] */
    uint32_t send;          /* the send's index in stage order */
} shd_event16;

/* 12-byte form (shd_flush_out.event_bytes = 12): the source host is left out -- the caller's
 * packet at index `send` already names it -- so 4 bytes less per event cross PCIe */
typedef struct shd_event12 {
    uint32_t deliver_off;
    uint32_t seq_off;
    uint32_t send;
} shd_event12;

/* Versioned: struct_size must be sizeof(shd_flush_out) as the caller's header declares it (round
 * 5 added n_events and event_bytes at the end; a caller built against that older layout has a
 * pointer here and is refused with SHD_ERR_INVALID instead of having fields read past its object). */
typedef struct shd_flush_out {
    uint32_t struct_size;   /* in: sizeof(shd_flush_out) */
    uint32_t event_bytes;   /* in: 16 (or 0) = shd_event16 records, 12 = shd_event12 records */
    uint8_t* status2;
    uint32_t* ev_off;
    shd_event16* events;        /* shd_event12 records when event_bytes = 12 */
    uint64_t* seq_base;
    uint64_t min_deliver;   /* as shd_relay_out (under a communicator: over all ranks) */
    uint64_t min_latency;
    uint64_t n_sent;
    uint64_t n_events;      /* events returned (= n_sent on one context; the own destinations' events
                               under a communicator) */
} shd_flush_out;

shd_status shd_relay_flush(shd_ctx* ctx, const shd_stage* stages, uint32_t n_stages, uint64_t time_base,
                           const shd_round* round, shd_flush_out* out);
/* Pinned host memory for staging buffers and outputs (hipHostMalloc); NULL on failure. */
void* shd_host_alloc(size_t bytes);
void shd_host_free(void* p);

/* ---------------------------------------------------------------- multi-GPU */
/*
 * The reference is one process whose manager thread runs every round to a barrier
 * (core/manager.rs:404-464); it has no multi-GPU path.  The engine shards the two paths along
 * their natural seams -- routing source rows, relay hosts by id -- over a communicator:
 *   shd_comm_init        one process per GPU, RCCL over xGMI; rank 0 makes the id with
 *                        shd_comm_unique_id and the caller hands it to every rank (MPI, a file,
 *                        torch.distributed ...); collective over the ranks
 *   shd_comm_init_local  every rank in this process (one host thread per rank must then drive
 *                        each sharded call concurrently): device copies between the contexts,
 *                        ordered by HIP events between their streams (no host stream syncs)
 *   shd_comm_init_host   ranks are processes the caller connects itself (MPI, gloo, sockets):
 *                        one all-to-all-v callback moves host bytes; the device bytes are staged
 *                        through pinned host memory around it (slower than RCCL: PCIe both ways)
 * Shards are contiguous blocks of ceil(total / n_ranks) (shd_shard_range).  Initialising or
 * destroying a communicator requires shd_relay_setup again.
 */
#define SHD_COMM_ID_BYTES 128
shd_status shd_comm_unique_id(uint8_t* id /* SHD_COMM_ID_BYTES */);
shd_status shd_comm_init(shd_ctx* ctx, int32_t n_ranks, int32_t rank, const uint8_t* id);
shd_status shd_comm_init_local(shd_ctx** ctxs, int32_t n_ranks);
/* The host transport of shd_comm_init_host.  all_to_allv: every rank calls it together; the
 * send_bytes[r] bytes at send + send_off[r] go to rank r (offsets may repeat: the same bytes to
 * several ranks), the recv_bytes[q] bytes from rank q land at recv + recv_off[q]; host memory,
 * the sizes already agree between the ranks.  Returns 0 on success (anything else fails the
 * call with SHD_ERR_HIP on this rank; the peers are the transport's to release). */
typedef struct shd_host_comm_ops {
    void* user;
    int (*all_to_allv)(void* user, const void* send, const uint64_t* send_bytes, const uint64_t* send_off,
                       void* recv, const uint64_t* recv_bytes, const uint64_t* recv_off);
} shd_host_comm_ops;
shd_status shd_comm_init_host(shd_ctx* ctx, int32_t n_ranks, int32_t rank, const shd_host_comm_ops* ops);
shd_status shd_comm_info(const shd_ctx* ctx, int32_t* n_ranks, int32_t* rank);
shd_status shd_comm_destroy(shd_ctx* ctx);
shd_status shd_shard_range(uint32_t total, int32_t n_ranks, int32_t rank, uint32_t* lo, uint32_t* hi);

/*
 * Routing build over the communicator (after shd_routing_prepare of the same graph on every
 * rank): each rank builds its source rows into its slice of the full table, then one
 * all-gather leaves the whole table on every rank (tables of at most SHD_SHARD_REPLICATE_MB MiB,
 * default 64, are instead built whole on every rank: no exchange; shares above 256 MB per rank
 * are exchanged in row chunks overlapping the build).  d_lat_full / d_loss_full are device buffers
 * of n_ranks * ceil(n_used / n_ranks) rows of n_used (rows >= n_used are padding).  Every rank
 * returns the same status: the lowest failing rank's error.  Replaces the rayon fan-out of
 * compute_shortest_paths (graph/mod.rs:192-210) across GPUs.
 */
shd_status shd_routing_run_sharded(shd_ctx* ctx, uint32_t algo, uint64_t* d_lat_full,
                                   float* d_loss_full, shd_error* err);

/*
 * One relay round over the communicator.  shd_relay_setup (after the communicator, same
 * arguments on every rank) makes this rank own hosts [lo, hi) = shd_shard_range(n_hosts):
 * their RNG streams, event ids and destination events.  d_batch holds the sends of the own
 * hosts only (src_off has hi - lo + 1 entries; host lo + k's sends are [src_off[k],
 * src_off[k+1])); d_out->status (device, n_packets) receives their statuses.  The round's
 * events for the own destinations come back in engine-owned device arrays, valid until the next
 * round: d_out->ev_off[hi - lo + 1] and ev_deliver / ev_src / ev_seq / ev_pkt (ev_pkt = the
 * packet's index in its sender rank's batch; the sender rank owns ev_src).  min_deliver,
 * min_latency and n_sent are reduced over all ranks.  A round that fails on any rank fails on
 * every rank with that rank's status and commits no host state anywhere.
 */
shd_status shd_relay_round_sharded(shd_ctx* ctx, const shd_batch* d_batch, const shd_round* round,
                                   shd_relay_out* d_out);

/* ---------------------------------------------------------------- destination event queues */
/*
 * Device-resident packet-event queues of this context's destination hosts:
 * WorkerShared::push_packet_to_host / EventQueue::push (worker.rs:619-629,
 * event_queue.rs:28-48) and the pop loop of Host::execute (host.rs:697-706) for packet events.
 * shd_equeue_advance merges a round's events (a relay output on the device, NULL for none) into
 * the pending queues and pops, per host, every event with deliver < window_end in EventQueue
 * order (time, src host, src event id; event.rs:84-155); later events stay pending for later
 * rounds.  The popped events are in engine-owned device arrays valid until the next advance.
 * tag = (number of the batch that carried the event << 32) | its ev_pkt in that batch.
 */
typedef struct shd_equeue_out {
    const uint32_t* off;        /* device [n_hosts + 1]: host h's events are [off[h], off[h+1]) */
    const uint64_t* deliver;    /* device [n_popped] */
    const uint32_t* src;
    const uint64_t* seq;
    const uint64_t* tag;
    uint64_t n_popped;
    uint64_t n_pending;         /* events left in the queues */
    uint64_t next_time;         /* earliest pending deliver time (EventQueue::next_event_time
                                   minimum over the hosts); UINT64_MAX when none is left */
} shd_equeue_out;

/* n_hosts = all hosts.  Under a communicator of > 1 ranks the queues hold this rank's destination
 * shard [lo, hi) = shd_shard_range(n_hosts) -- the hosts whose events shd_relay_round_sharded
 * returns here -- and every per-host array (the batch's ev_off, the popped off[]) covers those
 * hi - lo hosts.  A batch whose n_dst differs from the queues' host count is SHD_ERR_INVALID. */
shd_status shd_equeue_setup(shd_ctx* ctx, uint32_t n_hosts);
shd_status shd_equeue_advance(shd_ctx* ctx, const shd_relay_out* d_batch, uint64_t window_end,
                              shd_equeue_out* out);
/* Engine-owned device arrays (ev_off, ev_deliver, ev_src, ev_seq, ev_pkt; n_dst set) for up to
 * max_events events of the next round's relay output: pass them as the shd_relay_round_device
 * output (with the caller's status array), then to shd_equeue_advance, which adopts the batch as
 * a stored run without copying any of it.  Valid until that advance (or the next call). */
shd_status shd_equeue_batch_buffers(shd_ctx* ctx, uint64_t max_events, shd_relay_out* out);
/* The number the next non-NULL batch passed to shd_equeue_advance will get in its events' tags
 * (batch numbers count the non-NULL batches since shd_equeue_setup). */
shd_status shd_equeue_next_batch(shd_ctx* ctx, uint64_t* batch);
/* Host copies of the last advance's popped events (any pointer may be NULL). */
shd_status shd_equeue_copy_popped(shd_ctx* ctx, uint32_t* off, uint64_t* deliver, uint32_t* src,
                                  uint64_t* seq, uint64_t* tag);
/* Host copy of the pending queues (same layout; any pointer may be NULL). */
shd_status shd_equeue_pending(shd_ctx* ctx, uint32_t* off, uint64_t* deliver, uint32_t* src,
                              uint64_t* seq, uint64_t* tag, uint64_t* n_pending);

/* ---------------------------------------------------------------- round window */
/*
 * Runahead (src/main/core/scheduler/runahead.rs:12-115) kept in the context, and the next
 * scheduling window (SimController::manager_finished_current_round, controller.rs:86-111) from
 * the engine's own state.  shd_runahead_setup = Runahead::new(is_runahead_dynamic,
 * min_possible_latency, min_runahead_config) (manager.rs:246-251): min_possible_latency_ns = 0
 * takes RoutingInfo::get_smallest_latency_ns of the resident table; min_runahead_config_ns = 0
 * is None.  Every committed relay round (single or sharded; its min_latency reduced over all
 * ranks) then updates the lowest used latency when dynamic (update_lowest_used_latency,
 * worker.rs:380).  shd_round_window takes the caller's earliest non-packet event time
 * (UINT64_MAX: none) and the experiment end, and returns the window [start, end) the reference's
 * manager would open next: start = the minimum over that time, the pending queues' heads and the
 * last relay output not yet merged (manager.rs:430-464; UINT64_MAX = none, which is
 * EmulatedTime::MAX), end = min(start + runahead (saturating at EmulatedTime::MAX), end_time);
 * *running = start < end.  Under a communicator the minimum is reduced over all ranks: a
 * collective (every rank calls it, and every rank gets the same window).
 */
shd_status shd_runahead_setup(shd_ctx* ctx, int32_t dynamic, uint64_t min_possible_latency_ns,
                              uint64_t min_runahead_config_ns);
shd_status shd_runahead_get(const shd_ctx* ctx, uint64_t* runahead_ns);
shd_status shd_round_window(shd_ctx* ctx, uint64_t cpu_next_event_time, uint64_t end_time,
                            uint64_t* window_start, uint64_t* window_end, int32_t* running);
/* The window arithmetic alone (no context, no GPU): controller.rs:92-111 for a given minimum
 * next event time and runahead. */
shd_status shd_window_compute(uint64_t min_next_event_time, uint64_t runahead_ns, uint64_t end_time,
                              uint64_t* window_start, uint64_t* window_end, int32_t* running);

/* Copy bytes from an engine-owned device array (e.g. shd_equeue_out, a sharded relay output) to
 * host memory on the context's stream; returns when the copy is complete. */
shd_status shd_copy_to_host(shd_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* Read back the per-host RNG states / next event ids (e.g. to hand RNG use back to the CPU).
 * A sharded context's own hosts carry their current state, the others their setup state. */
shd_status shd_relay_get_host_state(shd_ctx* ctx, uint64_t* rng_state, uint64_t* next_event_id);

/* Per-path packet counters (RoutingInfo::increment_packet_count, graph/mod.rs:451-458): on by
 * default; the reference only reads them in log_packet_counts (never called), so a caller may
 * turn them off.  Counts accumulate over all rounds (n_nodes x n_nodes u64). */
shd_status shd_relay_set_counters(shd_ctx* ctx, int32_t enabled);
shd_status shd_path_packet_counts(shd_ctx* ctx, uint64_t* counts);

/* Which device pipeline ran the last successful round (diagnostics; no reference counterpart):
 * 7 = destination-bin placement, 3 = radix sort by destination, 1 = 64-bit records; 8 = a
 * sharded round whose pipeline-7 bins went to their destination ranks as stamped and were sorted
 * there (no packing or merge pass; otherwise a sharded round reports the local pipeline). */
shd_status shd_relay_last_pipeline(const shd_ctx* ctx, int32_t* pipeline);

/* ---------------------------------------------------------------------------------------
 * CoDel inbound router queues.  Replaces CoDelQueue::push / pop
 * (src/main/network/router/codel_queue.rs:125-306) for every host at once: one queue per host
 * stays on the device; a call replays a batch of operations, grouped by host, each host's in
 * time order.  A push carries (time, total size, packet id); a pop (size == SHD_CODEL_POP)
 * returns the next conforming packet or none, dropping per RFC 8289 as the reference does.
 * ------------------------------------------------------------------------------------- */
#define SHD_CODEL_POP 0xFFFFFFFFu

typedef struct shd_codel_ops {   /* device pointers */
    uint64_t n_ops;
    const uint32_t* host_off;    /* [n_hosts + 1] */
    const uint64_t* time;        /* [n_ops] emulated ns (the `now` argument) */
    const uint32_t* size;        /* [n_ops] packet total size for a push, SHD_CODEL_POP for a pop */
    const uint32_t* pkt;         /* [n_ops] packet id for a push (ignored for a pop) */
} shd_codel_ops;

typedef struct shd_codel_state {   /* one host's queue, for inspection (the reference's fields) */
    uint32_t len, mode;            /* mode: 0 Store, 1 Drop */
    uint32_t has_interval_end, has_drop_next;
    uint64_t interval_end, drop_next;
    uint64_t current_drop_count, previous_drop_count, total_bytes_stored;
} shd_codel_state;

/* (Re)create n_hosts empty queues holding up to `capacity` packets each. */
shd_status shd_codel_setup(shd_ctx* ctx, uint32_t n_hosts, uint32_t capacity);
/* Run a batch.  pop_out[k] = packet id a pop returned (SHD_CODEL_POP for none or for a push);
 * fate[id] = (op index << 2) | 1 (dequeued) or | 2 (dropped) for every packet this batch
 * dequeued or dropped (other entries untouched).  SHD_ERR_INVALID: a queue exceeded its
 * capacity or a packet id >= n_ids (the batch ran with the affected pushes/marks skipped), or the
 * reference panics: the control law (codel_queue.rs:287-300) of a time before SIMULATION_START
 * (to_abs_simtime) or with a result past EMUTIME_MAX = 2^64 - 2 (SimulationTime::saturating_add's
 * unwrap: no saturation there).  The queues are then left undefined: every later call returns
 * SHD_ERR_STATE until shd_codel_setup.
 * Times are EmulatedTimes, at most EMUTIME_MAX (2^64 - 1 is EMUTIME_INVALID).  interval_end =
 * now + INTERVAL saturates at EMUTIME_MAX (EmulatedTime::saturating_add); the standing delay and
 * the "dropping recently" span are saturating_duration_since: 0 when the earlier time is the
 * later one and when the difference is above SIMTIME_MAX = 17500059273709551614. */
shd_status shd_codel_run_device(shd_ctx* ctx, const shd_codel_ops* ops, uint32_t* pop_out,
                                uint64_t* fate, uint32_t n_ids);
shd_status shd_codel_get_state(shd_ctx* ctx, uint32_t host, shd_codel_state* out);

/* ---------------------------------------------------------------------------------------
 * Token-bucket relays.  Replaces TokenBucket::conforming_remove
 * (src/main/network/relay/token_bucket.rs:68-157) as Relay::forward_until_blocked calls it
 * (src/main/network/relay/mod.rs:200-287), for every relay at once: one bucket per relay stays
 * on the device; a call replays a batch of forwarding attempts, grouped by relay, each relay's
 * in time order.  An attempt is FORWARDED (value = the balance after it; UINT64_MAX for a relay
 * without a bucket), BLOCKED (value = the duration until it would conform; the relay is then
 * Pending until now + value, as forward_later schedules it) or SKIPPED (made while the relay
 * was Pending; value = the pending deadline).  Flag SHD_TB_EXEMPT: a local packet or one sent
 * while bootstrapping, forwarded without tokens (relay/mod.rs:224-229).
 * ------------------------------------------------------------------------------------- */
#define SHD_TB_FORWARDED 0
#define SHD_TB_BLOCKED 1
#define SHD_TB_SKIPPED 2
#define SHD_TB_EXEMPT 1u

typedef struct shd_tb_ops {     /* device pointers */
    uint64_t n_ops;
    const uint32_t* relay_off;  /* [n_relays + 1] */
    const uint64_t* time;       /* [n_ops] emulated ns (Worker::current_time) */
    const uint32_t* size;       /* [n_ops] packet total size (tokens to remove) */
    const uint8_t* flags;       /* [n_ops] SHD_TB_EXEMPT or 0 */
} shd_tb_ops;

typedef struct shd_tb_state {   /* one relay's bucket, for inspection (the reference's fields) */
    uint64_t capacity, balance, refill_increment, refill_interval, last_refill, pending_until;
} shd_tb_state;

/* (Re)create n_relays buckets (TokenBucket::new_inner, token_bucket.rs:37-60; full at start).
 * All three parameters 0 = no bucket (RateLimit::Unlimited); some but not all 0 is
 * SHD_ERR_INVALID (the reference's new() returns None and its caller unwraps), and so is a bucket
 * whose refill_interval_ns is above SIMTIME_MAX = 17500059273709551614 (no SimulationTime) or whose
 * last_refill is above EMUTIME_MAX = 2^64 - 2 (no EmulatedTime), before anything runs.  These rules
 * hold for the tb_* arrays of shd_inbound_setup and the outbound setups too.  Host arrays;
 * create_token_bucket (relay/mod.rs:291-302) is capacity = max(1, Bps/1000) + 1500,
 * increment = max(1, Bps/1000), interval = 1 ms. */
shd_status shd_tb_setup(shd_ctx* ctx, uint32_t n_relays, const uint64_t* capacity,
                        const uint64_t* refill_increment, const uint64_t* refill_interval_ns,
                        const uint64_t* last_refill);
/* Run a batch (device pointers); status[k] / value[k] per attempt.  SHD_ERR_INVALID where the
 * reference panics: a time before the bucket's last refill or more than SIMTIME_MAX after it
 * (duration_since, token_bucket.rs:128,152), or a conforming duration whose product or sum lies in
 * (SIMTIME_MAX, 2^64) (SimulationTime::saturating_mul / saturating_add saturate at SIMTIME_MAX only
 * when the u64 operation overflows; below that they unwrap); the batch still ran.  The token
 * product and sum saturate at 2^64 - 1; a blocked relay's deadline now + duration saturates at
 * EMUTIME_MAX (EmulatedTime::saturating_add). */
shd_status shd_tb_run_device(shd_ctx* ctx, const shd_tb_ops* ops, uint8_t* status, uint64_t* value);
shd_status shd_tb_get_state(shd_ctx* ctx, uint32_t relay, shd_tb_state* out);

/* ---------------------------------------------------------------------------------------
 * Inbound stage: the destination side after the event queues, for every host at once.  Per host
 * the device keeps a CoDel router queue, the inbound relay's token bucket and the relay's state
 * (the time of its outstanding forward task, the one packet it has cached) -- the stage's own
 * state: shd_codel_* and shd_tb_* keep their queues and buckets and behave as before.  One call
 * consumes a window's popped packet events, per host in order and merged with the host's own
 * forward task (a packet event runs before a task of the same time, event.rs:102-110):
 *   packet event at t   CoDelQueue::push(pkt, t) (Host::execute's packet branch, host.rs:742-746,
 *                       Router::route_incoming_packet), then Relay::notify (relay/mod.rs:110-135):
 *                       an Idle relay gets a task at t, a Pending one nothing
 *   task at T < window_end   Relay::forward_until_blocked (relay/mod.rs:200-272) at T: take the
 *                       cached packet or CoDelQueue::pop(T) (which may drop packets first, and
 *                       may return none: Idle); unless T < bootstrap_end or the host has no
 *                       bucket, conforming_remove(size) at T; Err(d) caches the packet and
 *                       schedules the next task at T + d (EmulatedTime saturating); otherwise
 *                       the packet is forwarded at T and the loop goes on
 * A task at T >= window_end stays outstanding for a later call.  Inbound packets are never local
 * (the router's address is UNSPECIFIED, host.rs:281-292).  Not covered: the reference's CPU-delay
 * model (host.rs:708-735) reschedules events on the CPU side; a caller that enables it cannot use
 * this stage.
 * ------------------------------------------------------------------------------------- */
#define SHD_INBOUND_FORWARDED 1   /* (pkt, T): the packet reaches the interface at T */
#define SHD_INBOUND_DROPPED 2     /* (pkt, T): dropped by the pop at T */

/* (Re)create n_hosts empty queues of up to `capacity` packets each, Idle relays and full
 * buckets.  The tb_* host arrays follow shd_tb_setup's rules (all three parameters 0: no bucket). */
shd_status shd_inbound_setup(shd_ctx* ctx, uint32_t n_hosts, uint32_t capacity,
                             const uint64_t* tb_capacity, const uint64_t* tb_refill_increment,
                             const uint64_t* tb_refill_interval_ns, const uint64_t* tb_last_refill);
/*
 * Advance every host over the window ending at window_end.  Device inputs: host h's events are
 * [d_off[h], d_off[h+1]) of d_time / d_size (total packet size) / d_pkt (packet id, not
 * UINT32_MAX); d_off and d_time may be shd_equeue_out.off and .deliver as they lie on the device
 * (n_events = n_popped; every pointer may be NULL when n_events is 0).  Input contract, per host:
 * times non-decreasing, every time < window_end and >= the previous call's window_end; for a host
 * with a bucket every size <= the bucket's capacity (the reference never sees a larger packet --
 * total size <= CONFIG_MTU -- and would reschedule it forever).  Outputs: one record per packet
 * that left the stage in this window, grouped by host in the order they happened (the drops of
 * a pop before the packet it returned), in engine-owned device arrays valid until the next
 * advance: host h's records are [out_off[h], out_off[h+1]) of out_pkt / out_time / out_kind
 * (SHD_INBOUND_*), *n_out in all.  *n_stored = packets still queued or cached; *next_task_time =
 * the earliest outstanding forward task over the hosts (UINT64_MAX: none).  The forward task is a
 * local event of its host: fold *next_task_time into shd_round_window's cpu_next_event_time.
 * Any output pointer may be NULL.  No collective: on a sharded context the arrays cover the
 * rank's own hosts, as the event queues' arrays do.
 * SHD_ERR_INVALID: the input contract is violated, d_off is not a CSR over n_events events, or a
 * queue exceeded its capacity -- every such input is refused by a check in the kernel, the
 * window has partly run, and every later call returns SHD_ERR_STATE until shd_inbound_setup; also
 * where the reference panics (the bucket's cases of shd_tb_run_device, the CoDel control law's of
 * shd_codel_run_device).  A window_end above EMUTIME_MAX = 2^64 - 2 is no time of the reference's:
 * a relay blocked for a saturated duration has its task at EMUTIME_MAX, which no window runs.  A
 * NULL array with
 * n_events > 0 or a window_end below the previous one is SHD_ERR_INVALID before anything runs.
 */
shd_status shd_inbound_advance(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time,
                               const uint32_t* d_size, const uint32_t* d_pkt, uint64_t n_events,
                               uint64_t window_end, uint64_t bootstrap_end,
                               const uint32_t** out_off, const uint32_t** out_pkt,
                               const uint64_t** out_time, const uint8_t** out_kind,
                               uint64_t* n_out, uint64_t* n_stored, uint64_t* next_task_time);
/* One host's state (any pointer may be NULL): *task_time UINT64_MAX = Idle; the cached packet;
 * the queue and the bucket in the structs of shd_codel_get_state / shd_tb_get_state
 * (pending_until = the task time, 0 when Idle).  SHD_ERR_STATE while the stage is not ready --
 * before shd_inbound_setup, or after a contract error until the next setup, as the advance;
 * SHD_ERR_INVALID: host >= n_hosts. */
shd_status shd_inbound_get_state(shd_ctx* ctx, uint32_t host, uint64_t* task_time, uint32_t* has_cached,
                                 uint32_t* cached_pkt, uint32_t* cached_size, shd_codel_state* codel,
                                 shd_tb_state* bucket);

/* ---------------------------------------------------------------------------------------
 * Outbound stage: the source side up to Worker::send_packet, for every host at once -- the
 * outbound relay relay_inet_out (host.rs:285-288, :871-880).  Per host the device keeps the
 * network interface's queue (the packets its sockets have offered and that have not left yet,
 * ordered by packet priority: the FIFO queuing discipline, network_interface.c:276-316,
 * network_queuing_disciplines.c:90-102, pops the socket whose head packet has the lowest
 * priority; priorities come from one per-host counter, host.rs:604-610, and every socket offers
 * its packets in increasing priority, so that is the lowest priority over all queued packets),
 * the outbound relay's token bucket, the relay's state (the time of its outstanding forward
 * task, the one packet it has cached) and the host's global id first_host + h -- the stage's own
 * state, apart from shd_inbound_* and shd_tb_*.  One call consumes a window's offers ("socket
 * data became sendable": notify_socket_has_packets, then Relay::notify), per host in order and
 * merged with the host's own forward task:
 *   offer at t <= task  (or the relay is Idle)  the packet is inserted by priority; an Idle relay
 *                       gets a task at t (notify -> forward_later(ZERO), relay/mod.rs:110-135),
 *                       a Pending one nothing.  An offer at the task's own time is inserted
 *                       before the task runs: the sends of one event accumulate (:124-126)
 *   task at T < window_end   Relay::forward_until_blocked (relay/mod.rs:200-272) at T: take the
 *                       cached packet or the lowest-priority queued one (none: Idle).  A packet
 *                       with dst == first_host + h is local (:222-230): it is forwarded at T
 *                       without the bucket and goes back to the interface (:262-265), a LOCAL
 *                       record, not sent.  Otherwise, unless T < bootstrap_end or the host has no
 *                       bucket, conforming_remove(size) at T; Err(d) caches the packet and
 *                       schedules the next task at T + d (EmulatedTime saturating); on success
 *                       the packet is sent at T, the instant Router::push calls
 *                       Worker::send_packet (router/mod.rs:49-55), and the loop goes on
 * A task at T >= window_end stays outstanding for a later call.  The cached packet is never
 * overtaken, not by a local packet and not by a lower priority (head-of-line blocking).
 * Exactness (FIFO): the merge is exact whenever a host's offers at one instant arrive in
 * increasing priority -- everything but a same-instant retransmission -- and also when the bucket
 * does not block at that instant.  Under SHD_QDISC_FIFO_SOCKETS (below) a same-instant
 * retransmission is exact as well: the order within a socket is the offer order, whatever the
 * priorities.  What stays inexact there is two events of one host at the same nanosecond, as
 * under round-robin.
 *
 * The queuing discipline is interface_qdisc (configuration.rs:396-397, :930-933), chosen at the
 * setup.  Under SHD_QDISC_ROUND_ROBIN (network_interface.c:235-273, :366-392;
 * network_queuing_disciplines.c:29-88) the host keeps the rrQueue instead: an ordered list of
 * distinct sockets, each with the packets it has offered in offer order (socket.c:434-467), a
 * socket in the list exactly while it has a packet queued.  An offer appends the packet to its
 * socket's and, if the socket is not in the rrQueue, pushes the socket at the tail
 * (networkinterface_wantsSend: find, else push).  A pop takes the head socket's first packet; the
 * socket goes back to the tail if it has more, else it leaves -- at the pop, before the relay
 * knows whether the bucket blocks, so while a packet sits in the relay's cache its socket has
 * already rotated.  Everything around the pop (notify, the merge, the cached packet, local
 * packets, bootstrapping, the bucket, the records) is the same code for both disciplines.
 * Exactness (round-robin): the merge is exact whenever a host's offers at one instant belong to
 * one event (one accumulation under relay/mod.rs:124-126) or to one socket.  Two events on one
 * host at the same nanosecond that offer on different sockets are rotated together here; in the
 * reference the first event's task may already have drained its packets.  Within a socket packets
 * leave in offer order: SHD_QDISC_FIFO and SHD_QDISC_ROUND_ROBIN see a socket as one list.
 *
 * The reference's sockets have two: a packet of priority 0 goes to the socket's control buffer,
 * every other one to its data buffer (socket.c:432-437), and peek and pull take the control buffer
 * first (socket.c:182-189, :466-467).  Every TCP control packet -- a pure ACK, SYN, FIN -- has
 * priority 0 (tcp.c:947-963; the host's counter starts at 1, host.rs:248), so a TCP host soon has
 * two packets of priority 0 queued, which SHD_QDISC_FIFO refuses.  SHD_QDISC_FIFO_SOCKETS and
 * SHD_QDISC_ROUND_ROBIN_SOCKETS model both buffers; an offer then carries the packet's priority
 * (0: control) and the offering socket's canonical handle (shd_outbound_advance_sockets).  Per
 * host: a set of sockets keyed by handle, each with a control list and a data list in offer order;
 * the socket's head is its first control packet if it has one, else its first data packet; a
 * socket is queued exactly while it has a packet.
 *   SHD_QDISC_FIFO_SOCKETS   the queue is the array heap of priority_queue.c:87-140, :189-208
 *       under network_queuing_disciplines.c:90-102: smaller(i, j) = !(key(i) > key(j)), key = the
 *       socket's head priority now, a tie "smaller" both ways.  Push appends and sifts up; pop
 *       swaps the root with the last entry, shrinks and sifts down (the right child when
 *       smaller(right, left)).  The discipline (network_interface.c:276-316) pops the root socket,
 *       pulls its head packet and pushes the socket again if it still has data, before the relay
 *       knows whether the bucket blocks.  A control packet offered to a socket that is in the heap
 *       changes its key where it stands, nothing is re-heapified: the send order is a function of
 *       the heap array, not "lowest priority first", and the device keeps that array.
 *   SHD_QDISC_ROUND_ROBIN_SOCKETS   the rrQueue as above, the pull taking the control list first.
 *
 * Not covered: the loopback relay (unlimited, every packet local), the pcap and tracker side
 * effects of networkinterface_pop, and the CPU-delay model (host.rs:708-735), as the inbound
 * stage.
 * ------------------------------------------------------------------------------------- */

/* QDiscMode (configuration.rs:396-397) */
#define SHD_QDISC_FIFO 0
#define SHD_QDISC_ROUND_ROBIN 1
/* the same two over sockets with a control and a data buffer (socket.c:432-437): the discipline
 * | 4.  (2 and 3 name nothing and stay SHD_ERR_INVALID.) */
#define SHD_QDISC_FIFO_SOCKETS 4
#define SHD_QDISC_ROUND_ROBIN_SOCKETS 5

/* (Re)create n_hosts empty queues of up to `capacity` packets each, Idle relays and full
 * buckets; host h's global id (what a packet's dst is compared with) is first_host + h.  The tb_*
 * host arrays follow shd_tb_setup's rules (all three parameters 0: no bucket).  The discipline
 * is FIFO. */
shd_status shd_outbound_setup(shd_ctx* ctx, uint32_t n_hosts, uint32_t first_host, uint32_t capacity,
                              const uint64_t* tb_capacity, const uint64_t* tb_refill_increment,
                              const uint64_t* tb_refill_interval_ns, const uint64_t* tb_last_refill);
/* shd_outbound_setup with the discipline named.  qdisc = SHD_QDISC_FIFO: shd_outbound_setup,
 * max_sockets is ignored.  qdisc = SHD_QDISC_ROUND_ROBIN: `capacity` is still the packets a host
 * may have queued, max_sockets the sockets it may have in its rrQueue at once.
 * SHD_QDISC_FIFO_SOCKETS, SHD_QDISC_ROUND_ROBIN_SOCKETS: the same two limits, max_sockets the
 * sockets in the host's heap or rrQueue.  SHD_ERR_INVALID: any other qdisc, or max_sockets == 0
 * under any discipline but SHD_QDISC_FIFO (the stage stays as it was). */
shd_status shd_outbound_setup_qdisc(shd_ctx* ctx, uint32_t n_hosts, uint32_t first_host, uint32_t capacity,
                                    uint32_t qdisc, uint32_t max_sockets, const uint64_t* tb_capacity,
                                    const uint64_t* tb_refill_increment, const uint64_t* tb_refill_interval_ns,
                                    const uint64_t* tb_last_refill);
/*
 * Advance every host over the window ending at window_end.  Device inputs: host h's offers are
 * [d_off[h], d_off[h+1]) of d_time / d_prio (the 64-bit key of the discipline: under FIFO the
 * FifoPacketPriority; under round-robin the offering socket's canonical handle,
 * compatsocket_getCanonicalHandle, compared for equality only, so any value is allowed -- the
 * reference's round-robin never reads a priority and its FIFO never needs the socket) / d_size
 * (total packet size: what the bucket removes) / d_payload (packet_getPayloadSize, passed through to shd_batch.payload) /
 * d_dst (destination HostId) / d_pkt (the caller's packet id, not UINT32_MAX); every pointer may
 * be NULL when n_offers is 0.  Input contract, per host: times non-decreasing, every time
 * < window_end and >= the previous call's window_end; under FIFO priorities unique among the
 * packets queued on the host (round-robin has no priority check); under round-robin at most
 * `capacity` packets and max_sockets sockets queued on a host; for a host with a bucket every non-local size <= the bucket's capacity.
 * Outputs, engine-owned device arrays valid until the next advance:
 *   *d_batch_out   src_off[n_hosts+1], send_time / dst_host / payload of the packets sent, grouped
 *                  by host in send order, n_packets, chance = NULL: it can be passed to
 *                  shd_relay_round_device or shd_relay_round_sharded as it stands (with first_host
 *                  = the rank's shard start it is the sharded call's layout)
 *   *sent_pkt      sent_pkt[i] = the packet id of batch entry i
 *   *loc_off, *loc_pkt, *loc_time   the local deliveries as a second CSR, *n_local in all: host
 *                  h's are [loc_off[h], loc_off[h+1]) in the order they happened
 * *n_stored = packets still queued or cached; *next_task_time = the earliest outstanding forward
 * task over the hosts (UINT64_MAX: none): fold it into shd_round_window's cpu_next_event_time, as
 * the inbound stage's.  Any output pointer may be NULL.  No collective.
 * SHD_ERR_INVALID: the input contract is violated (an offer's time is checked before it is
 * weighed against the task), d_off is not a CSR over n_offers offers, a priority equals one still
 * queued on that host (FIFO), or a queue exceeded its capacity or its max_sockets -- every such input is refused by a check
 * in the kernel, the window has partly run, and every later call returns SHD_ERR_STATE until
 * shd_outbound_setup; also where the reference panics (the bucket's cases of shd_tb_run_device).  A
 * NULL array with n_offers > 0 or a window_end below the previous one is SHD_ERR_INVALID before
 * anything runs.
 *
 * shd_outbound_advance_sockets is the same call with one more column, d_sock[k] = the canonical
 * handle of the socket that offers packet k (compared for equality only); shd_outbound_advance is
 * shd_outbound_advance_sockets with d_sock = NULL.  Under SHD_QDISC_FIFO_SOCKETS and
 * SHD_QDISC_ROUND_ROBIN_SOCKETS d_prio is the packet priority (0: a control packet) and d_sock is
 * needed: NULL with n_offers > 0 is SHD_ERR_INVALID before anything runs.  Their input contract
 * has no priority rule -- any priorities, equal ones included -- and keeps the rest: times, sizes,
 * packet ids, at most `capacity` packets and max_sockets sockets queued on a host, with the same
 * consequences.  Under SHD_QDISC_FIFO and SHD_QDISC_ROUND_ROBIN d_sock is ignored.
 */
shd_status shd_outbound_advance(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time,
                                const uint64_t* d_prio, const uint32_t* d_size, const uint32_t* d_payload,
                                const uint32_t* d_dst, const uint32_t* d_pkt, uint64_t n_offers,
                                uint64_t window_end, uint64_t bootstrap_end,
                                shd_batch* d_batch_out, const uint32_t** sent_pkt,
                                const uint32_t** loc_off, const uint32_t** loc_pkt, const uint64_t** loc_time,
                                uint64_t* n_local, uint64_t* n_stored, uint64_t* next_task_time);
shd_status shd_outbound_advance_sockets(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time,
                                        const uint64_t* d_prio, const uint64_t* d_sock, const uint32_t* d_size,
                                        const uint32_t* d_payload, const uint32_t* d_dst, const uint32_t* d_pkt,
                                        uint64_t n_offers, uint64_t window_end, uint64_t bootstrap_end,
                                        shd_batch* d_batch_out, const uint32_t** sent_pkt,
                                        const uint32_t** loc_off, const uint32_t** loc_pkt,
                                        const uint64_t** loc_time, uint64_t* n_local, uint64_t* n_stored,
                                        uint64_t* next_task_time);
/* The total sizes of the last advance's batch (device, engine-owned, valid until the next advance):
 * d_size[i] = the size the offer of batch entry i carried -- with *sent_pkt what shd_ledger_record
 * keeps for the destination side.  NULL before the first advance.  SHD_ERR_STATE wherever
 * shd_outbound_get_state returns it. */
shd_status shd_outbound_sent_sizes(shd_ctx* ctx, const uint32_t** d_size);
/* One host's state (any pointer may be NULL): *task_time UINT64_MAX = Idle; the cached packet;
 * the packets queued and the one the next pop takes (FIFO: the lowest priority; round-robin: the
 * head socket's first; the socket disciplines: the head packet, control first, of the heap's root
 * or the rrQueue's head socket; UINT32_MAX: empty); the
 * bucket in the struct of shd_tb_get_state (pending_until = the task time, 0 when Idle).
 * SHD_ERR_STATE while the stage is not ready -- before shd_outbound_setup, or after a contract
 * error until the next setup, as the advance; SHD_ERR_INVALID: host >= n_hosts. */
shd_status shd_outbound_get_state(shd_ctx* ctx, uint32_t host, uint64_t* task_time, uint32_t* has_cached,
                                  uint32_t* cached_pkt, uint32_t* cached_size, uint32_t* queue_len,
                                  uint32_t* head_pkt, shd_tb_state* bucket);
/* One host's rrQueue in order: handles[i] / counts[i] = the i-th socket's canonical handle and
 * its queued packets (control plus data), at most `cap` entries written (host arrays; NULL with
 * cap = 0); *n_sockets = the sockets queued.  Under SHD_QDISC_FIFO_SOCKETS the sockets come as
 * the heap array in index order -- the state the send order is a function of.  The cached packet's
 * socket is listed only if it has further packets.  SHD_ERR_STATE under SHD_QDISC_FIFO, and
 * wherever shd_outbound_get_state returns it; SHD_ERR_INVALID: host >= n_hosts. */
shd_status shd_outbound_get_sockets(shd_ctx* ctx, uint32_t host, uint64_t* handles, uint32_t* counts, uint32_t cap,
                                    uint32_t* n_sockets);

/* ---------------------------------------------------------------------------------------
 * Packet ledger: what joins the event queues to the inbound stage on the device.  A popped event
 * carries its tag, (batch number << 32) | index in that batch; shd_inbound_advance wants the
 * packet's total size and the caller's packet id.  The ledger keeps each batch's (size, id) per
 * packet on the device from the relay round that sent it until its last event has popped, and
 * gathers a window's popped tags into the two arrays the inbound stage takes.  No reference
 * counterpart: the reference's events own their packets.
 *
 * One arena of 8-byte entries, a batch one contiguous slice; space comes back in batch order: a
 * batch that drains before an older one stays held until the older one is gone.  The batches held
 * span at most max_live_batches consecutive batch numbers (numbers never recorded in between
 * count).  The arena grows with its contents kept, in a record only.
 * ------------------------------------------------------------------------------------- */

/* (Re)create an empty ledger.  max_live_batches 0 = 1024; above 4096: SHD_ERR_INVALID.  Also starts
 * the window calls below over (the next one is an open, no relay output is pending). */
shd_status shd_ledger_setup(shd_ctx* ctx, uint32_t max_live_batches);
/* Keep (d_size[i], d_pkt[i]), i < n_packets (device arrays), under batch number `batch`
 * (shd_equeue_next_batch before the batch's advance); n_live of them will pop
 * (shd_relay_out.n_sent).  Batch numbers strictly increase.  n_live == 0 stores nothing.  No host
 * synchronisation: the two arrays are read on the context's stream and must stay as they are until
 * work queued behind the call has finished (engine-owned arrays such as shd_outbound_advance's do:
 * the call that replaces them is queued on the same stream).  SHD_ERR_INVALID before anything runs, the ledger as it was: a NULL array with
 * n_packets > 0, a batch number not above the last one recorded, n_live > n_packets, or a batch
 * max_live_batches or more numbers above the oldest one held. */
shd_status shd_ledger_record(shd_ctx* ctx, uint64_t batch, const uint32_t* d_size, const uint32_t* d_pkt,
                             uint64_t n_packets, uint64_t n_live);
/* The record after a committed shd_relay_round_sharded, a collective: every rank of the
 * communicator calls it.  A sharded round hands a rank the events of its own destination hosts,
 * and their ev_pkt is the packet's index in its SENDER rank's batch, which the receiver does not
 * hold.  d_size / d_pkt / d_dst_host / d_status [n_packets]: this rank's batch entries as
 * shd_ledger_record takes them, with the batch's destinations and the round's SHD_PKT_* statuses
 * (device arrays); d_out: this rank's shd_relay_round_sharded output.  Each SHD_PKT_SENT entry's
 * (size, id) goes to the rank that owns its destination host (shd_shard_range).  On return this
 * rank's ledger holds, under `batch` (ITS OWN shd_equeue_next_batch: batch numbers are per rank),
 * one entry per event it received -- d_out->n_events of them, all live; the senders' entries in
 * rank order, each sender's in its batch order -- and d_out->ev_pkt[e] has been rewritten in place
 * to the index in that slice, so shd_equeue_advance and shd_ledger_gather work unchanged (tag =
 * batch << 32 | index).  A rank that received nothing records nothing and passes no batch to its
 * queues.  Packet ids travel unchanged: the inbound records of a rank carry ids chosen by the
 * sender rank's caller, so a sharded caller picks ids that name a packet across the ranks.
 * local: the caller's own status on entry (SHD_OK, or a failure it carries into the call instead
 * of leaving its peers alone in the collective).  Everything that can differ between the ranks --
 * local, a NULL array with n_packets > 0, a ledger or relay not set up, a batch number not above
 * the last one recorded, a ledger that already spans max_live_batches numbers, an allocation
 * failure -- travels with the sizes in the one small all-to-all the call starts with: if any
 * rank's status is not SHD_OK every rank returns the lowest failing rank's status, with its ledger
 * as it was.  Two host synchronisations: that read-back and the remap's status.  (The remap goes
 * through an inverse table of one 4-byte slot per batch entry of every sender, allocated after
 * the exchange; knob LEDGER_REMAP_SEARCH=1, or a table that cannot be had: a binary search of the
 * sender's indices instead, same results.)  SHD_ERR_INVALID
 * after the exchange, on that rank alone: an event whose ev_pkt names a packet its sender did not
 * send has UINT32_MAX there, and every later ledger call of the rank returns SHD_ERR_STATE until
 * shd_ledger_setup, as after a refused gather.  Without a collective: SHD_ERR_STATE without a
 * communicator, SHD_ERR_INVALID for a NULL ctx or d_out or more than 256 ranks.  At one rank the
 * call is shd_ledger_record with n_live = d_out->n_sent. */
shd_status shd_ledger_record_sharded(shd_ctx* ctx, uint64_t batch, const uint32_t* d_size, const uint32_t* d_pkt,
                                     const uint32_t* d_dst_host, const uint8_t* d_status, uint64_t n_packets,
                                     shd_relay_out* d_out, shd_status local);
/* d_tag[n] as shd_equeue_out.tag lies on the device -> engine-owned device arrays (*d_size)[n],
 * (*d_pkt)[n], valid until the next gather: what shd_inbound_advance takes.  Lowers each named
 * batch's live count; a batch at 0 is retired (the call ends with one read-back of the status and
 * the live counts: its one host synchronisation).  SHD_ERR_INVALID, refused by checks in the
 * kernel before any index is used for a load: a tag whose batch is not held or has no live event
 * left, an index >= its batch's n_packets, a batch popped more often than its n_live.  Such an
 * event has UINT32_MAX in both outputs, the other events of the call are right (of an overdrawn
 * batch at least the surplus events are refused; which ones is not defined), and every later
 * ledger call returns SHD_ERR_STATE until shd_ledger_setup.  A NULL d_tag with n > 0 is
 * SHD_ERR_INVALID before anything runs. */
shd_status shd_ledger_gather(shd_ctx* ctx, const uint64_t* d_tag, uint64_t n, const uint32_t** d_size,
                             const uint32_t** d_pkt);
/* Batches with a live event, their live events, the arena entries held (the sum of n_packets from
 * the oldest batch held to the newest) and the oldest batch held (UINT64_MAX: none).  Any pointer
 * may be NULL.  After every shd_window_open live_events equals the queues' n_pending. */
shd_status shd_ledger_stats(shd_ctx* ctx, uint64_t* live_batches, uint64_t* live_events, uint64_t* entries_held,
                            uint64_t* oldest_batch);

/* ---------------------------------------------------------------------------------------
 * The scheduling window in two calls.  The inbound records of window k come first -- a delivered
 * segment makes its socket answer -- and the CPU turns them into offers of the same window, so a
 * window is
 *   shd_window_open    shd_equeue_advance (merging the relay output the last close left in the
 *                      slot shd_equeue_batch_buffers lent; none: NULL) -> shd_ledger_gather on the
 *                      popped tags -> shd_inbound_advance on the popped off / deliver as they lie
 *                      and the gathered arrays
 *   [CPU: sockets, applications; this window's offers]
 *   shd_window_close   shd_outbound_advance -> if anything was sent shd_relay_round_device (device
 *                      draws) into the lent queue buffers and an engine-owned status array ->
 *                      shd_ledger_record(shd_equeue_next_batch, the batch's sizes and ids,
 *                      n_packets, n_sent)
 * with no packet data crossing the host.  Every event of a batch has deliver >= its window_end, so
 * merging it at the next open pops exactly what merging it at once would have.  The relay output
 * is not merged by the close: shd_round_window already counts its earliest deliver time; the
 * caller folds min(*inbound_next_task, *outbound_next_task) into cpu_next_event_time as with the
 * separate calls.  Outputs are the stages' (engine-owned device arrays, any pointer may be NULL):
 * the open's are shd_inbound_advance's plus the queues' n_popped / n_pending / next_time; the
 * close's are shd_outbound_advance's sent_pkt and local deliveries, *sent_status (SHD_PKT_* per
 * batch entry), *n_batch (batch entries), *n_events (of them sent: events for the queues) and
 * *min_deliver (shd_relay_out.min_deliver; UINT64_MAX: none).
 * SHD_ERR_STATE, nothing changed: relay, queues, runahead, both stages and the ledger are not all
 * set up for the same host count with first_host 0; a close without its open, two opens in a
 * row.  SHD_ERR_INVALID before anything runs: a close whose window_end is not its open's, or
 * a close while the ledger already spans max_live_batches batch numbers.  Otherwise the statuses
 * of the stages, as they return them.
 *
 * Under a communicator of N > 1 ranks a window runs on each rank's shard [lo, hi) of the hosts
 * (shd_shard_range): the relay set up under the communicator, the queues holding the shard, both
 * stages set up for hi - lo hosts, the outbound stage with first_host = lo, runahead and ledger on
 * every rank (a rank without hosts needs neither queues nor stages); anything else stays
 * SHD_ERR_STATE.  The open is local, no collective: queues -> gather -> inbound stage on the
 * rank's hosts.  A rank whose open fails must not leave its peers alone in the close: agreeing
 * after the opens is the caller's job (no rank calls the close, or every rank does).  The close
 * is a collective with the same sequence of collectives on every rank, whatever happens locally:
 *   1. the preconditions (the parts ready, the open seen, window_end its open's, room in the
 *      ledger) agreed in one small collective: if any rank fails them every rank returns the
 *      lowest failing rank's status and nothing has run anywhere.  One refusal comes without a
 *      collective: SHD_ERR_STATE when the relay is not set up under this communicator
 *   2. shd_outbound_advance, local; a rank where it fails still enters the round
 *   3. shd_relay_round_sharded, always (an empty batch, a rank without hosts): an outbound
 *      failure rides in the round's own status agreement, so the round commits on no rank and
 *      every rank's close returns that status (the peers' outbound stages have run their window)
 *   4. shd_ledger_record_sharded
 * *n_events is the number of events this rank RECEIVED (what its queues merge at the next open),
 * *n_batch and *sent_status cover its own sends, *min_deliver is the all-rank value.  Packet ids
 * travel unchanged between the ranks (see shd_ledger_record_sharded).
 * ------------------------------------------------------------------------------------- */
shd_status shd_window_open(shd_ctx* ctx, uint64_t window_end, uint64_t bootstrap_end,
                           const uint32_t** out_off, const uint32_t** out_pkt, const uint64_t** out_time,
                           const uint8_t** out_kind, uint64_t* n_out, uint64_t* n_stored,
                           uint64_t* inbound_next_task, uint64_t* n_popped, uint64_t* n_pending,
                           uint64_t* queue_next_time);
shd_status shd_window_close(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time, const uint64_t* d_prio,
                            const uint32_t* d_size, const uint32_t* d_payload, const uint32_t* d_dst,
                            const uint32_t* d_pkt, uint64_t n_offers, uint64_t window_end, uint64_t sim_end,
                            uint64_t bootstrap_end, const uint32_t** sent_pkt, const uint8_t** sent_status,
                            uint64_t* n_batch, uint64_t* n_events, const uint32_t** loc_off,
                            const uint32_t** loc_pkt, const uint64_t** loc_time, uint64_t* n_local,
                            uint64_t* n_stored, uint64_t* outbound_next_task, uint64_t* min_deliver);
/* shd_window_close with the offers' socket column (shd_outbound_advance_sockets); shd_window_close
 * is this call with d_sock = NULL.  Over an outbound stage set up with one of the two socket
 * disciplines a NULL d_sock with n_offers > 0 is SHD_ERR_INVALID before anything runs; under a
 * communicator it is one of the preconditions the ranks agree on, so every rank's close returns
 * it and nothing has run anywhere. */
shd_status shd_window_close_sockets(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time,
                                    const uint64_t* d_prio, const uint64_t* d_sock, const uint32_t* d_size,
                                    const uint32_t* d_payload, const uint32_t* d_dst, const uint32_t* d_pkt,
                                    uint64_t n_offers, uint64_t window_end, uint64_t sim_end,
                                    uint64_t bootstrap_end, const uint32_t** sent_pkt,
                                    const uint8_t** sent_status, uint64_t* n_batch, uint64_t* n_events,
                                    const uint32_t** loc_off, const uint32_t** loc_pkt,
                                    const uint64_t** loc_time, uint64_t* n_local, uint64_t* n_stored,
                                    uint64_t* outbound_next_task, uint64_t* min_deliver);

/* ---------------------------------------------------------------------------------------
 * Staged offers -> the outbound stage's device columns.  The window's offers as the worker threads
 * leave them at the round barrier, grouped by host on the device: no CPU group-by, no split into
 * seven arrays, no copy per array.  The staging site is notify_socket_has_packets -> Relay::notify
 * (relay/mod.rs:110-135): the thread that runs the host appends the packet's offer to its stage.
 *
 * Stages (shd_relay_flush's contract; scheduler/thread_per_core.rs:188-206: a host runs on one
 * thread per round): stage k is one thread's buffer -- stage_runs[k] runs, run r being
 * (run_host[k][r], run_count[k][r]), and stage_offers[k] records in offers[k], run after run.  A
 * host's offers form ONE run of consecutive records in ONE stage, in the order the host made them
 * (time order: what shd_outbound_advance asks of a host's offers).  Stages and runs come in any
 * order; a host without a run has no offers; a run of count 0 is allowed.  run_host holds global
 * host ids; the hosts grouped are the outbound stage's, [first_host, first_host + n_hosts) -- under
 * a communicator a rank stages its own hosts only (unlike shd_relay_flush, where every rank sees
 * every stage).
 *
 * An offer record is offer_words consecutive uint32_t words: 8 under SHD_QDISC_FIFO /
 * SHD_QDISC_ROUND_ROBIN, 10 under the two _SOCKETS disciplines (10 is accepted under the plain
 * ones: the socket column is then ignored, as d_sock is):
 *   word 0     time_off = now - time_base        word 4     pkt (the caller's id)
 *   word 1     dst (destination HostId, global)  word 5     reserved, ignored
 *   word 2     size (total packet size)          word 6, 7  the d_prio key, low then high
 *   word 3     payload                           word 8, 9  d_sock, low then high (width 10 only)
 *
 * Outputs: engine-owned device arrays, valid until the next shd_offers_group, which
 * shd_outbound_advance_sockets / shd_window_close_sockets take as they stand (d_time = time_base +
 * time_off; *d_sock is NULL at width 8); *n_offers their length.  Any output pointer may be NULL.
 * Stages in pinned memory (shd_host_alloc; every array of every stage) are read where they lie,
 * each byte once; otherwise they are copied stage after stage (the FLUSH_COPY knob forces that).
 * Records should be 8-byte aligned (any allocator's are); others are read word by word.
 *
 * Refusals -- nothing the outbound stage or the stages own has changed:
 *   SHD_ERR_STATE    the outbound stage is not set up
 *   SHD_ERR_NO_HOST  a run's host lies outside [first_host, first_host + n_hosts)
 *   SHD_ERR_INVALID  a host with two runs; a stage whose run counts do not add up to its
 *                    stage_offers; offer_words not 8 or 10, or 8 under a _SOCKETS discipline; a NULL
 *                    array where a count is not zero; 2^32 or more offers or runs
 * Nothing else is checked here: times, priorities, sizes and ids reach shd_outbound_advance
 * unchanged and its contract checks apply to them.
 * ------------------------------------------------------------------------------------- */
shd_status shd_offers_group(shd_ctx* ctx, uint32_t n_stages, const uint32_t* stage_runs,
                            const uint32_t** run_host, const uint32_t** run_count,
                            const uint64_t* stage_offers, const uint32_t** offers, uint32_t offer_words,
                            uint64_t time_base, const uint32_t** d_off, const uint64_t** d_time,
                            const uint64_t** d_prio, const uint64_t** d_sock, const uint32_t** d_size,
                            const uint32_t** d_payload, const uint32_t** d_dst, const uint32_t** d_pkt,
                            uint64_t* n_offers);

/* ---------------------------------------------------------------------------------------
 * shd_window_close from staged offers: shd_offers_group, then shd_window_close_sockets on its
 * arrays; the stage arguments are shd_offers_group's, the rest shd_window_close_sockets'.
 * One context: the window's own preconditions come first (parts ready, the open seen, window_end
 * its open's, room in the ledger), then the grouping; a refused grouping returns its status with
 * the window still open and no stage run, so a corrected close may follow.
 * Under a communicator of N > 1 ranks the grouping runs first and locally, without a collective,
 * and its status is the rank's word in the close's precondition agreement (step 1 above): if any
 * rank's stages are refused every rank returns the lowest failing rank's status, nothing has run
 * anywhere and the window is still open on every rank.  The sequence of collectives is
 * shd_window_close's.  A rank without hosts passes n_stages = 0 (a run there is SHD_ERR_NO_HOST).
 * ------------------------------------------------------------------------------------- */
shd_status shd_window_close_staged(shd_ctx* ctx, uint32_t n_stages, const uint32_t* stage_runs,
                                   const uint32_t** run_host, const uint32_t** run_count,
                                   const uint64_t* stage_offers, const uint32_t** offers, uint32_t offer_words,
                                   uint64_t time_base, uint64_t window_end, uint64_t sim_end,
                                   uint64_t bootstrap_end, const uint32_t** sent_pkt,
                                   const uint8_t** sent_status, uint64_t* n_batch, uint64_t* n_events,
                                   const uint32_t** loc_off, const uint32_t** loc_pkt,
                                   const uint64_t** loc_time, uint64_t* n_local, uint64_t* n_stored,
                                   uint64_t* outbound_next_task, uint64_t* min_deliver);

/* ---------------------------------------------------------------------------------------
 * A window's results in host buffers, one call each: asynchronous copies of the arrays the stages
 * own on the context's stream and ONE wait (shd_copy_to_host waits per array).  Host buffers,
 * pinned for the link's full rate; any pointer may be NULL.
 *   shd_window_records_host  the last shd_window_open's records: off[n_hosts + 1]; pkt, time, kind
 *                            of *n_out entries, the buffers holding cap
 *   shd_window_sent_host     the last close's results: sent_pkt, sent_status of *n_batch entries
 *                            (cap_batch); loc_off[n_hosts + 1]; loc_pkt, loc_time of *n_local
 *                            entries (cap_local)
 * n_hosts: the hosts the window runs here (a sharded rank's own).  SHD_ERR_INVALID: a capacity below
 * its count while a buffer of that capacity is given -- the counts are returned and nothing is
 * copied, so the caller sizes its buffers and calls again.  SHD_ERR_STATE: no open (no close) has
 * succeeded yet, or the arrays are no longer the stage's (set up again, or grown by a later call).
 * ------------------------------------------------------------------------------------- */
shd_status shd_window_records_host(shd_ctx* ctx, uint32_t* off, uint32_t* pkt, uint64_t* time, uint8_t* kind,
                                   uint64_t cap, uint64_t* n_out);
shd_status shd_window_sent_host(shd_ctx* ctx, uint32_t* sent_pkt, uint8_t* sent_status, uint64_t cap_batch,
                                uint32_t* loc_off, uint32_t* loc_pkt, uint64_t* loc_time, uint64_t cap_local,
                                uint64_t* n_batch, uint64_t* n_local);

/* ---------------------------------------------------------------------------------------
 * Bandwidth changes on running stages: re-rate the token buckets (ABI 12).  Link capacity is a
 * host's bw_down / bw_up (relay/mod.rs:277-302 builds both relays' buckets from it, once); the
 * setup calls are the only other way to another rate, and they start the stage over.  These
 * calls change the named hosts' buckets and nothing else: queued packets, CoDel state, the cached
 * packet, the outstanding forward task and the sockets stay as they are.
 *
 * The reference has no counterpart; a re-rate of one bucket at emulated time `at_time` to
 * (capacity C, increment I, interval N) is put together from its pieces (token_bucket.rs:37-60,
 * :127-157):
 *   bucket -> bucket     lazy_refill(at_time) under the old parameters -- the old rate holds up to
 *                        at_time -- then new_inner(C, I, N, at_time) whose balance is
 *                        min(refilled balance, C) instead of C.  The new refill grid starts at at_time.
 *   none -> bucket       (none: all three parameters 0) new_inner(C, I, N, at_time), full
 *   bucket -> none       the host is unlimited; last_refill reads back as at_time, the rest as 0
 *   none -> none         nothing changes
 * An outstanding forward task keeps its time (the reference cannot cancel a scheduled task); a
 * cached packet stays cached and is weighed against the new bucket when its task runs.  Some but
 * not all of C, I, N zero is refused, as at setup.  A host named more than once takes its last
 * entry.  n == 0 is SHD_OK and does nothing.  All arrays are host arrays; `host` is the stage's
 * own index (a sharded rank's local one, global id first_host + host).  No collective: each rank
 * re-rates its own hosts.
 *
 * A call is refused whole -- nothing changed on the device or the host:
 *   SHD_ERR_STATE    the stage is not ready: before its setup, and after a contract error until
 *                    the next setup (where the advance returns it)
 *   SHD_ERR_INVALID  before any launch: a NULL array with n > 0; an index >= the stage's hosts;
 *                    some-but-not-all-zero parameters; at_time below the stage's previous window_end;
 *                    an interval above SIMTIME_MAX or an at_time above EMUTIME_MAX: no values of
 *                    the reference's types
 *   SHD_ERR_INVALID  on the device, for any named host, the lowest such index in *err_host (may be
 *                    NULL; untouched otherwise): at_time before the bucket's last_refill or more
 *                    than SIMTIME_MAX after it (the reference's duration_since would panic); a refill to at_time where the
 *                    reference panics (as the advance's); an outstanding forward task earlier than
 *                    at_time (it would run before the new bucket's last_refill); a capacity C > 0
 *                    below the total size of a packet the host stores now, the cached one
 *                    included -- a blocked packet's task must be able to forward it.  An outbound
 *                    packet whose dst is the host itself never meets the bucket and is exempt.
 * After a successful call an event or offer of a re-rated host earlier than at_time is the caller's
 * contract violation: it meets the advance's "a time before the bucket's last refill".
 *
 *   shd_tb_update                 the replay engine's buckets (shd_tb_setup).  A Pending relay stays
 *                                 Pending until its deadline; only the time rules apply.
 *   shd_inbound_update_buckets    the inbound stage's (bw_down)
 *   shd_outbound_update_buckets   the outbound stage's (bw_up), under any discipline
 *   shd_window_update_bandwidth   both stages from rates in bytes per second, each direction by
 *                                 create_token_bucket (relay/mod.rs:291-302: increment =
 *                                 max(1, rate / 1000), capacity = increment + 1500, interval 1 ms);
 *                                 UINT64_MAX leaves that direction as it is.  Only between a close
 *                                 and the next open: SHD_ERR_STATE while a window is open or before
 *                                 the window's parts are set up.  Both stages are checked before
 *                                 either changes, so a refusal by one leaves both untouched.
 * ------------------------------------------------------------------------------------- */
shd_status shd_tb_update(shd_ctx* ctx, uint64_t n, const uint32_t* relay, const uint64_t* capacity,
                         const uint64_t* refill_increment, const uint64_t* refill_interval_ns, uint64_t at_time,
                         uint32_t* err_relay);
shd_status shd_inbound_update_buckets(shd_ctx* ctx, uint64_t n, const uint32_t* host, const uint64_t* capacity,
                                      const uint64_t* refill_increment, const uint64_t* refill_interval_ns,
                                      uint64_t at_time, uint32_t* err_host);
shd_status shd_outbound_update_buckets(shd_ctx* ctx, uint64_t n, const uint32_t* host, const uint64_t* capacity,
                                       const uint64_t* refill_increment, const uint64_t* refill_interval_ns,
                                       uint64_t at_time, uint32_t* err_host);
shd_status shd_window_update_bandwidth(shd_ctx* ctx, uint64_t n, const uint32_t* host, const uint64_t* down_bytes_per_s,
                                       const uint64_t* up_bytes_per_s, uint64_t at_time, uint32_t* err_host);

/* ---------------------------------------------------------------------------------------
 * GML loader (host code, no GPU needed).  Replaces the reference's
 * gml_parser::parse (src/lib/gml-parser/src/lib.rs:52-57) + NetworkGraph::parse
 * (src/main/network/graph/mod.rs:136-183): GML text -> the shd_graph arrays the routing build
 * takes.  Node index = order of the node in the text (petgraph add_node order); a repeated GML
 * id maps to its later node, as the reference's HashMap insert does.  On failure `msg` holds the
 * reference's message (e.g. "Edge 'latency' must not be 0", "Edge source 7 doesn't exist").
 * ------------------------------------------------------------------------------------- */
typedef struct shd_gml shd_gml;

/* Parse `len` bytes of GML.  SHD_ERR_INVALID: grammar or validation error;
 * SHD_ERR_LATENCY_OVERFLOW: an edge latency does not fit u64 ns (the reference panics in
 * convert(Nano).unwrap(), graph/mod.rs:338). */
shd_status shd_gml_parse(const char* text, size_t len, shd_gml** out, char* msg, size_t msg_len);
/* load_network_graph (graph/mod.rs:481-511) for a GML file: read `path` (xz != 0: decompress it
 * as xz, read_xz :482-494 -- through the system liblzma), require strict UTF-8
 * (String::from_utf8), then shd_gml_parse.  File, decompression and UTF-8 failures are
 * SHD_ERR_INVALID with the reference's context message. */
shd_status shd_gml_load(const char* path, int32_t xz, shd_gml** out, char* msg, size_t msg_len);
/* View of the parsed graph; the arrays stay owned by `g` until shd_gml_free. */
shd_status shd_gml_graph(const shd_gml* g, shd_graph* view);
/* host_bandwidth_down / _up per node in bits/s (UINT64_MAX = attribute absent; values beyond
 * u64 saturate at UINT64_MAX - 1).  Either pointer may be NULL; arrays are [n_nodes]. */
shd_status shd_gml_node_bandwidth(const shd_gml* g, uint64_t* down_bps, uint64_t* up_bps);
void shd_gml_free(shd_gml* g);

#ifdef __cplusplus
}
#endif
#endif /* SHD_ACCEL_H */
