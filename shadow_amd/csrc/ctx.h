// Engine context (one per GPU) and grow-only device scratch.
#pragma once
#include <memory>
#include <vector>

#include "comm.h"
#include "common.h"
#include "edge_update.h"
#include "knobs.h"
#include "ledger_book.h"
#include "rate_update.h"

namespace shd {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p; bytes = o.bytes;
            o.p = nullptr; o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    shd_status ensure(size_t need) {
        if (need <= bytes) return SHD_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        size_t want = need + need / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) return SHD_ERR_NOMEM;
        bytes = want;
        return SHD_OK;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct PinBuf {   // grow-only coherent pinned host memory (a kernel's stores reach the host: readback_into)
    void* p = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    shd_status ensure(size_t need) {
        if (need <= bytes) return SHD_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        if (hipHostMalloc(&p, need, hipHostMallocCoherent) != hipSuccess) return SHD_ERR_NOMEM;
        bytes = need;
        return SHD_OK;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

struct ScanScratch {   // look-back states of the hand-written scans (scan.h)
    DevBuf state;       // [tiles][2] u64
    uint32_t epoch = 0;
};

struct CodelState {   // CoDel router queues (codel.hip)
    DevBuf st, flags, ring, status;
    uint32_t n_hosts = 0, cap = 0;
    bool ready = false;
};

// Stored runs of the event queues before they are compacted (the EQ_MAX_RUNS knob may set the
// limit lower, down to 2).  Each advance merges one source per run, each compaction half
// the runs: on C5 (24 rounds at the steady ~41M pending events) the advance averaged 0.370 ms
// at 8 runs, 0.359 at 12 and 0.355 at 15 (a compaction every ~3 / ~6 / ~7 rounds against more
// sources in every pass); 12 keeps the count kernel's lanes to 13 of its 16.
constexpr int kEqMaxRuns = 12;
constexpr int kEqSlots = kEqMaxRuns + 2;   // + the compaction target + a batch slot handed out for adoption

struct EqRunBuf {   // one stored run of the event queues: a CSR of per-host sorted events
    DevBuf off, deliver, src, seq, tag;
    DevBuf pkt;                 // an adopted relay output keeps ev_pkt: tag = batch << 32 | pkt
    bool has_pkt = false;
    bool fresh = false;         // adopted by the running advance: its cursor is its offsets
    uint64_t batch = 0;
    uint64_t n = 0, left = 0;   // events stored / not yet popped
    bool live = false;
};

struct EqState {   // destination event queues (equeue_priv.h): a list of sorted runs (one per batch)
    EqRunBuf run[kEqSlots];         // slots
    int lend = -1;                  // the slot handed out by shd_equeue_batch_buffers (not live yet)
    bool fold_next = false;         // the next pass folds a compaction in (the run limit was reached)
    uint64_t lend_cap = 0;          // events the lent slot holds
    uint64_t cap_hint = 0;          // the largest run capacity grown so far (every later growth takes it)
    DevBuf curs[2];                 // [kEqSlots][n_hosts] u32 cursors (first unpopped), double-buffered
    DevBuf bcut;                    // [n_hosts] the batch's first kept event per host
    DevBuf pd, ps, pq, pt;          // the last call's popped events
    DevBuf pop_cnt, keep_cnt, pop_off, next;
    DevBuf ranges;                  // [n_hosts][kEqMaxRuns + 1] (cursor, cut) pairs of the last count
    int ccur = 0;
    uint32_t n_hosts = 0;           // queues held here: all hosts, or a sharded rank's [host_lo, host_lo + n_hosts)
    uint32_t host_lo = 0, n_total = 0;
    uint64_t n_pending = 0, n_popped = 0, batches = 0;
    uint64_t head = ~0ull;          // earliest pending deliver time after the last advance (local)
    ScanScratch scan;               // the advance's look-back scans (scan.h)
    bool ready = false;
};

// Runahead (src/main/core/scheduler/runahead.rs:12-115) and the round window
// (controller.rs:86-111) for shd_round_window.
struct RoundState {
    bool ready = false;
    bool dynamic = false;
    uint64_t min_possible = 0, cfg = 0;   // Runahead::min_possible_latency, min_runahead_config (0: None)
    uint64_t min_used = ~0ull;            // Runahead::min_used_latency (UINT64_MAX: None)
    uint64_t batch_min_deliver = ~0ull;   // relay output not yet merged into the queues: its earliest deliver
};

struct TbState {   // token-bucket relays (tbucket.hip)
    DevBuf st, err;
    uint32_t n_relays = 0;
    bool ready = false;
};

// The inbound stage (inbound.hip): per host a CoDel queue, the inbound relay's token bucket and
// the relay words -- its own state, apart from CodelState / TbState above.
struct InboundState {
    DevBuf st, flags, ring;        // the queues: CodelHost, flag word, ring of `cap` packets per host
    DevBuf tb;                     // TbRelay per host
    DevBuf rl;                     // InRelay per host: outstanding task time, the cached packet
    DevBuf cnt, nrec;              // [n_hosts + 1] record region bounds -> offsets; records written
    DevBuf r_pkt, r_time, r_kind;  // the records in their per-host regions
    DevBuf o_off, o_pkt, o_time, o_kind;   // the compact output of the last advance
    DevBuf words;                  // status, n_out, n_stored, min task time
    ScanScratch scan;
    uint32_t n_hosts = 0, cap = 0;
    uint64_t n_stored = 0;         // packets queued or cached after the last advance
    uint64_t prev_end = 0;         // the last advance's window_end
    bool ready = false;
};

// The outbound stage (outbound.hip): per host the interface's queue (FIFO or round-robin), the outbound relay's
// token bucket and the relay words -- its own state, apart from InboundState / TbState above.
struct OutboundState {
    DevBuf ring;                   // FIFO: OutPkt ring of `cap` slots per host, sorted by priority: all but the first packet;
                                   // round-robin: the RrSlot pool of `cap` slots per host (rr_queue.h)
    DevBuf socks, rr_words;        // round-robin: RrSock ring of max_sockets entries per host; the pool's bump count and free list
                                   // the socket disciplines (sock_queue.h): ring is the SqSlot pool, socks the SqSock array
    DevBuf tb;                     // TbRelay per host
    DevBuf rl;                     // OutRelay per host: task time, the queue's first packet, ring head / count, the cached packet
    DevBuf cnt, nsent, nloc;       // [n_hosts + 1] record region bounds -> offsets; SENT / LOCAL records written
    DevBuf r_pkt, r_time, r_dst, r_pay, r_size;   // the records in their per-host regions (SENT front, LOCAL back)
    DevBuf src_off, b_time, b_dst, b_pay, b_pkt, b_size;   // the last advance's batch (shd_batch), its packet ids and total sizes
    DevBuf loc_off, l_pkt, l_time;         // the last advance's local deliveries
    DevBuf words;                  // status, n_sent, n_local, n_stored, min task time
    ScanScratch scan;
    uint32_t n_hosts = 0, first_host = 0, cap = 0;
    uint32_t max_sockets = 0;      // round-robin: sockets a host may have queued at once
    uint32_t qdisc = 0;            // the discipline (SHD_QDISC_*) the stage was set up with
    bool with_sockets() const { return (qdisc & 4u) != 0; }   // the two disciplines whose offers carry the socket column
    uint64_t n_stored = 0;         // packets queued or cached after the last advance
    uint64_t prev_end = 0;         // the last advance's window_end
    bool advanced = false;         // an advance has run since the setup (b_* hold its batch)
    bool ready = false;
};

// The bucket re-rate (rate_update.hip), per target -- the replay engine's relays, the inbound
// stage, the outbound stage: the call's records on the device, its two result words (status bits,
// lowest failing host) and the host's last-entry-wins stamps.
enum RateTarget : int { kRateTb = 0, kRateInbound = 1, kRateOutbound = 2, kRateTargets = 3 };
struct RateState {
    DevBuf rec[kRateTargets];
    DevBuf words;                            // [kRateTargets][2] u64: status bits, lowest failing host
    RateStamps stamps[kRateTargets];
    std::vector<RateRec> host_rec[kRateTargets];   // the records as uploaded (they outlive the copy)
    uint32_t n_rec[kRateTargets] = {0, 0, 0};   // records of the running call (between its check and its apply)
};

// The grouping of staged runs by host (stage_group.hip), one per staged entry point: the runs as
// uploaded (or copied out of the pinned stages) and each host's run.
struct StageGroupState {
    DevBuf runh, runc, runo, rstg;   // per run: host, count, first record in stage order, stage (zero-copy)
    DevBuf hrun, hcnt;               // per host: its run (+1), its records
    DevBuf tab;                      // zero-copy: the stage table, and its pinned source
    PinBuf tab_pin;
    DevBuf red;                      // four words: the two checks, then two of the caller's
    ScanScratch scan;
};

// shd_offers_group (offers.hip): the worker threads' staged offers grouped by host into the
// outbound stage's columns -- the grouping, the records (copy path only), and the grouped columns
// handed out (engine-owned, valid until the next group).
struct OffersState {
    StageGroupState grp;
    DevBuf rec;                      // the records of every stage, stage after stage (copy path)
    DevBuf d_off, d_time, d_prio, d_sock, d_size, d_pay, d_dst, d_pkt;
};

// The packet ledger (ledger.hip): each batch's (total size, packet id) per packet, kept on the
// device from the relay round that sent the batch until its last event has popped.
struct LedgerState {
    LedgerBook book;               // the host's bookkeeping (ledger_book.h); exact between calls:
                                   // every gather ends with a read-back of the live counts
    DevBuf arena;                  // uint2 {size, pkt} entries, a batch = one contiguous slice
    DevBuf rows;                   // LedgerRow per slot (batch & mask); read-only to the gather
    DevBuf pops;                   // [slots] u32: the running gather's pops per batch, zero between calls
    DevBuf g_size, g_pkt;          // the last gather's outputs
    DevBuf words;                  // status, then the live count of every batch from oldest to newest
    PinBuf pin;                    // their host copy
    // shd_ledger_record_sharded: the batch's SENT entries packed per destination rank (index in the
    // batch, {size, pkt}), what the senders' ranks sent here, the per-(rank, workgroup) counts
    // and their scan, the remap's status word
    DevBuf x_sidx, x_sent, x_ridx, x_rent, x_cnt, x_st, x_inv;
    ScanScratch x_scan;
    bool ready = false;
};

// The two-call scheduling window (window.cpp): what shd_window_close leaves for the next open.
struct WindowState {
    bool opened = false;           // an open without its close
    uint64_t window_end = 0;       // the open's
    bool has_out = false;          // `out` is a relay output in the event queues' lent slot, not merged yet
    shd_relay_out out{};
    DevBuf status;                 // the last close's per-packet SHD_PKT_* (engine-owned)
    // under a communicator of > 1 ranks `out` is the sharded round's engine-owned output (valid
    // until the next round) and out_batch the number its events were recorded under
    uint64_t out_batch = 0;
    DevBuf no_off;                 // a zero: the batch offsets of a rank without hosts
    // what shd_window_records_host / shd_window_sent_host fetch: the last open's records and the
    // last close's results as the stages handed them out (the arrays are the stages' own)
    struct Records {
        bool valid = false;
        const uint32_t *off = nullptr, *pkt = nullptr;
        const uint64_t* time = nullptr;
        const uint8_t* kind = nullptr;
        uint64_t n = 0;
        uint32_t n_hosts = 0;
    } rec;
    struct Sent {
        bool valid = false;
        const uint32_t *pkt = nullptr, *loc_off = nullptr, *loc_pkt = nullptr;
        const uint8_t* status = nullptr;
        const uint64_t* loc_time = nullptr;
        uint64_t n_batch = 0, n_local = 0;
        uint32_t n_hosts = 0;
    } sent;
};

struct RelayState {
    bool ready = false;
    // shd_relay_setup has succeeded under the present communicator: shd_relay_retable may revive
    // the relay after a resident run stopped it (a change of communicator clears both flags)
    bool set_up = false;
    uint32_t n_hosts = 0;
    // source hosts this context stamps: all hosts, or (set up under a communicator of > 1
    // ranks) the rank's shard [src_lo, src_lo + n_src), which is also its destination shard
    uint32_t src_lo = 0, n_src = 0;
    bool sharded = false;
    uint32_t n_nodes = 0;
    bool own_table = false;   // table copied by shd_relay_setup (else: routing resident table)
    bool table_narrow = false;  // every path latency < 2^32 ns -> 16-byte event records (v2)
    bool force_v1 = false;      // SHD_RELAY_FORCE_V1=1 (testing)
    bool force_v3 = false;      // SHD_RELAY_FORCE_V3=1 (testing): radix pipeline, not v7
    int last_pipe = 0;          // pipeline of the last round: 1, 3, 7 or 8
    bool count_on = true;       // per-path packet counters (RoutingInfo::increment_packet_count)
    bool last_v2 = false;
    uint64_t seq_bound = 0;     // >= every host's next event id
    uint64_t last_recv = 0;     // events this rank received in the last sharded round
    uint32_t hn_bits = 0, hn_words = 0;   // packed host -> node map (0 bits: not used)
    unsigned long long red_host[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // counts: per-path packet counters over all committed rounds; counts_round: the running
    // round's increments, added to counts only when the round commits (a failed or rerun round
    // leaves counts untouched)
    DevBuf host_node, order, hn_packed, lat, loss, path, rng, next_id, rng2, next_id2, counts,
        counts_round;
    // per-round scratch
    DevBuf pk_off, pk_time, pk_dst, pk_pay, pk_chance, st, ev_key, ev_key2, ev_val, ev_val2,
        ev_deliver, ev_seq, ev_src, ev_pkt, ev_off, dst_cnt, red, rec, brec, tmp, draws,
        bin_cnt, bin_base, bin_lb;
    ScanScratch scan;     // pipeline 1's destination offsets (scan.h)
    ScanScratch col_scan; // pipeline 7's bin bases (bin_col_scan's look-back states)
    DevBuf rs_counts;     // pipeline 3's radix sort: per-tile digit counts
    ScanScratch rs_scan;
    // sharded rounds: packed outgoing events, exchange words, per-peer offset blocks, what was
    // received, and the merged events of this rank's destinations (engine-owned outputs)
    DevBuf x_rec, x_words, x_off, x_roff, x_rrec, m_off, m_deliver, m_src, m_seq, m_pkt;
    uint64_t x_cap = 0;   // events x_rrec and m_* hold (grown with a growth agreement, never between collectives)
    // relay_round_sharded_v7: the senders' bin scans, the sizing summary (+ its pinned copy) and
    // the per-sender receive / packet bases
    DevBuf xs_sc, xs_out, xs_b;
    PinBuf xs_pin;
    // the exchange's status part: [0] this rank's status after the sizing gather (0 unless a local
    // failure is carried), [1 + q] the one rank q sent (its own slot stays 0)
    DevBuf xs_st;
    bool xs_st_dirty = false;
    // shd_relay_flush (flush.hip): the round's draws came from the CPU (top 32 bits in `draws`), the
    // grouping of the staged runs (fl_grp), the records as uploaded (fl_send, copy path only), the
    // send permutation (grouped <-> stage order) and the packed outputs
    bool cpu_draws = false;
    // a sharded shd_relay_flush round: event ids leave the device relative to their source host's
    // first id of the round (a receiver does not hold the other ranks' hosts' ids)
    bool rel_ids = false;
    DevBuf fl_goff;   // the flush's grouped offsets over every host (sharded: all ranks' hosts)
    StageGroupState fl_grp;
    // a one-context flush round: pipeline 7's bin sort writes the compact event records here
    // (fl_direct says it did; the other pipelines leave the arrays for fl_events16)
    void* fl_ev_out = nullptr;
    uint32_t fl_b12 = 0;
    bool fl_direct = false;
    DevBuf fl_send, fl_perm, fl_inv, fl_st2, fl_ev16;
};

struct PreparedGraph {
    bool ready = false;
    uint32_t mode = 0, V = 0, n_used = 0;
    bool directed = false, narrow_arcs = false;
    bool dense_rows = false;  // the arc CSR is the complete graph's dense matrix (routing.hip csr_is_dense)
    uint64_t arcs = 0, max_arc_lat = 0, pruned_arcs = 0, tight_arcs = 0;
    uint32_t pruned_pad = 0;   // the pad width of the lists pruned_arcs counted (ArcView::pad)
    uint32_t pruned_path = 0;  // and the prune kernels that made them (ArcView::path)
    uint32_t mean_arc_lat = 1, min_arc_lat = 1;
    bool reordered = false;   // g_offr / g_usedr / g_arc8r / g_aqr hold the locality order
    bool spread = false;      // g_offs / g_useds / g_arc16s hold the wave-spread order (LDS kernel)
    bool used_ident = false;  // used[j] == j for every node (the LDS kernels then skip that gather)
    uint32_t lds_labels = 0;  // how many of the first (highest-degree) nodes keep LDS labels
    std::vector<uint32_t> used, node_ids, es, ed;
    std::vector<uint64_t> el;
    std::vector<float> ep;
    // shd_routing_update_edges (routing_update.hip): the two relabellings (node -> new id) that
    // prepare made, and the edge -> arc-slot map, built at the first update of a prepared graph
    std::vector<uint32_t> pi_r, pi_s;
    EdgeSlots upd;
    std::vector<int32_t> upd_col;   // node -> used index (-1: unused), with the map
    shd_graph view() const {
        shd_graph g{};
        g.n_nodes = V;
        g.n_edges = (uint32_t)es.size();
        g.edge_src = es.data();
        g.edge_dst = ed.data();
        g.edge_latency_ns = el.data();
        g.edge_packet_loss = ep.data();
        g.node_ids = node_ids.data();
        g.directed = directed;
        return g;
    }
};

}  // namespace shd

struct shd_ctx;
namespace shd {
// h_pin words: [0, 3) routing flags, [8, 16) relay reductions, [16, 18) the edge update's min / max arc latency,
// [32, 36) flush checks, [36, 38) offer-group checks,
// [48, 48 + 4 + runs + 1) event-queue counts, [72, 76) inbound-stage words; [80] is the polled marker;
// [81, 86) outbound-stage words, [88, 94) the bucket re-rate's result words
constexpr int kPinWords = 96;
constexpr int kPinMarker = 80;
// Wait until everything enqueued on stream s has finished (see api.cpp)
shd_status wait_stream(shd_ctx* ctx, hipStream_t s);
// n_bytes of device words into h_pin[at ...] and wait for the stream (api.cpp)
shd_status readback(shd_ctx* ctx, hipStream_t s, int at, const void* d_src, size_t n_bytes);
// the same into coherent pinned words of the caller's (PinBuf; n_bytes a multiple of 8, 8-aligned)
shd_status readback_into(shd_ctx* ctx, hipStream_t s, const void* d_src, size_t n_bytes, unsigned long long* h_dst);
// poll the pinned marker h_pin[kPinMarker] (zeroed by the caller) that a kernel sets after writing
// its words into pinned memory; falls back to hipStreamSynchronize after 20 ms
shd_status wait_marker(shd_ctx* ctx, hipStream_t s);
// a committed relay round's (all-rank) reductions: the runahead update (runahead.rs:60-115) and
// the earliest deliver time of the relay output that the queues have not merged yet (rounds.cpp)
void round_note(shd_ctx* ctx, uint64_t min_deliver, uint64_t min_latency);
// the smallest / largest of n device words (rounds.hip); one host synchronisation
shd_status min_u64_device(shd_ctx* ctx, const uint64_t* d, uint64_t n, uint64_t* out);
shd_status max_u64_device(shd_ctx* ctx, const uint64_t* d, uint64_t n, uint64_t* out);
// shd_relay_round_sharded with the caller's own status on entry (relay_shard.hip): a failure is carried
// into the round's status agreement -- the local pipeline is skipped, the round commits nowhere
shd_status relay_round_sharded_local(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o,
                                     shd_status local);
// One small collective under a communicator of > 1 ranks (ledger.hip): every rank passes its own
// status and all return the lowest failing rank's (SHD_OK: none failed); one host synchronisation
shd_status comm_agree(shd_ctx* ctx, shd_status local);
// The bucket re-rate in its parts (rate_update.hip).  rate_stage_check: the host-side rules, the records'
// upload and the check launch; rate_stage_apply: the apply launch, which does nothing where the target's
// check failed on the device; rate_stage_result: the one read-back of the targets in `mask` (bit per
// RateTarget) -- SHD_ERR_INVALID and the lowest failing host of the first target that failed.
// shd_*_update_buckets is check, apply, result; shd_window_update_bandwidth checks both stages
// and reads the result before it applies either.
shd_status rate_stage_check(shd_ctx* ctx, RateTarget t, uint64_t n, const uint32_t* host, const uint64_t* capacity,
                      const uint64_t* increment, const uint64_t* interval, uint64_t at);
shd_status rate_stage_apply(shd_ctx* ctx, RateTarget t, uint64_t at);
shd_status rate_stage_result(shd_ctx* ctx, uint32_t mask, uint32_t* err_host);
shd_status rate_update(shd_ctx* ctx, RateTarget t, uint64_t n, const uint32_t* host, const uint64_t* capacity,
                       const uint64_t* increment, const uint64_t* interval, uint64_t at, uint32_t* err_host);
// free the host mirror of the resident table (it follows the table)
void drop_mirror(shd_ctx* ctx);
}  // namespace shd

struct shd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev[8] = {};
    hipStream_t side = nullptr;        // second stream: work that overlaps the main stream's
    unsigned long long* h_pin = nullptr;   // shd::kPinWords pinned host words: flag / reduction read-backs
    shd::DevBuf g_one;                     // a device word holding 1 (shd::wait_stream's marker)
    bool spin_wait = true;                 // SHD_SPIN_WAIT=0: hipStreamSynchronize instead
    shd::Knobs knobs;                      // tuning / testing knobs (knobs.h), from the env at shd_open
    int n_cu = 0;
    size_t max_lds = 0;

    // resident routing table of the last build: rows [row_begin, row_begin+rows) x cols
    shd::DevBuf t_lat, t_loss;
    uint32_t t_rows = 0, t_cols = 0, t_row_begin = 0;
    bool t_full = false;
    uint64_t* h_mirror_lat = nullptr;   // pinned host copy of the resident table (shd_routing_mirror)
    float* h_mirror_loss = nullptr;
    shd::DevBuf lk_scratch;             // shd_routing_lookup_batch
    shd_routing_info info{};
    uint32_t time_every = 1, time_calls = 0;   // shd_routing_set_timing
    bool time_now = true;                      // this build records ev[2] / ev[3]
    bool stats_on = false;   // SHD_SSSP_STATS=1: count expansions / sweeps (tuning only)

    shd::PreparedGraph prep;
    shd::DevBuf d_es, d_ed, d_el, d_ep, d_col;   // direct mode edge arrays
    // routing scratch
    shd::DevBuf g_off, g_dst, g_lat, g_q, g_lat64, g_used, g_diag_lat, g_diag_loss, g_flags,
        g_dense, g_prune_dst, g_prune_dst2, g_prune_cnt, g_prune_nn, g_labels, g_aux, g_arc16, g_arc8, g_aq, g_fw, g_glab, g_pred,
        g_offr, g_usedr, g_arc8r, g_aqr,   // locality-ordered copies (global-label kernel)
        g_offs, g_useds, g_arc16s,         // wave-spread copies (1024-thread LDS kernel)
        g_umap, g_umap_r, g_umap_s,        // shd_routing_update_edges: per edge the two arc slots (main, copies)
        g_urec, g_ured;                    // its records, and the min / max arc latency words
    shd::DevBuf g_red;                     // min_u64_device / max_u64_device's result word
    // update calls that prepared the graph again (a wide graph); shd_get_knob reads it as UPDATE_REPREPARES
    uint64_t upd_reprepares = 0;
    uint32_t* nh_out = nullptr;   // next-hop rows of the running build (shd_routing_run_next_hops)
    // global-label slots left unlaunched while a sharded build's previous chunk is still being
    // exchanged on the side stream: the persistent kernel fills every CU's LDS, so RCCL's
    // send/recv workgroups would otherwise wait for it to finish (shd_routing_run_sharded)
    uint32_t slot_reserve = 0;

    std::unique_ptr<shd::Comm> comm;   // multi-GPU communicator (shd_comm_init*), or none
    shd::DevBuf comm_scratch;

    shd::RelayState relay;
    shd::EqState eq;
    shd::RoundState rnd;
    shd::CodelState codel;
    shd::TbState tb;
    shd::InboundState inb;
    shd::OutboundState outb;
    shd::OffersState offers;
    shd::LedgerState ledger;
    shd::WindowState win;
    shd::RateState rate;
};
