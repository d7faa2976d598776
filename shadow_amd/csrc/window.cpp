// One scheduling window as two engine calls, no packet data crossing the host:
//   shd_window_open    event queues (merging the relay output the last close left) -> ledger
//                      gather on the popped tags -> inbound stage
//   [the CPU: the inbound records make the sockets answer -- this window's offers]
//   shd_window_close   outbound stage -> relay round into the queues' lent slot -> ledger record
// Under a communicator of more than one rank the window runs on the rank's shard of the hosts: the
// open is local as before, the close a collective -- the sharded round, then the sharded record,
// which brings each sent packet's (size, id) to the rank that owns its destination.
// shd_window_close_staged is the close from the worker threads' staged offers (offers.hip groups
// them by host first); shd_window_records_host / shd_window_sent_host copy a window's results
// into host buffers with one wait each.
// The stages are the ones the separate calls drive (equeue.hip, ledger.hip, inbound.hip,
// outbound.hip, relay*.hip); this file only chains them and keeps what lies between two calls.
#include <vector>

#include "ctx.h"
#include "offer_stage.h"

using namespace shd;

// true under a communicator of more than one rank: the window runs on the rank's shard of the hosts
static bool window_sharded(const shd_ctx* ctx) { return ctx->comm && ctx->comm->size > 1; }

// One context: relay, queues, runahead, both stages and the ledger set up for the same hosts,
// first_host 0.  Under N > 1 ranks: the relay sharded, and for the rank's hosts [lo, hi) the queues
// its shard, both stages hi - lo hosts, the outbound stage's first_host lo; a rank without hosts
// needs neither queues nor stages.
static bool window_ready(const shd_ctx* ctx) {
    if (!ctx->relay.ready || !ctx->rnd.ready || !ctx->ledger.ready) return false;
    const uint32_t H = ctx->relay.n_hosts;
    uint32_t lo = 0, hi = H;
    if (window_sharded(ctx)) {
        if (!ctx->relay.sharded) return false;
        shard_range(H, ctx->comm->size, ctx->comm->rank, &lo, &hi);
        if (hi == lo) return true;
    } else if (ctx->relay.sharded) {
        return false;
    }
    if (!ctx->eq.ready || !ctx->inb.ready || !ctx->outb.ready) return false;
    return ctx->eq.n_hosts == hi - lo && ctx->eq.host_lo == lo && ctx->eq.n_total == H && ctx->inb.n_hosts == hi - lo &&
           ctx->outb.n_hosts == hi - lo && ctx->outb.first_host == lo;
}

static uint32_t window_own_hosts(const shd_ctx* ctx) {
    uint32_t lo = 0, hi = ctx->relay.n_hosts;
    if (window_sharded(ctx)) shard_range(ctx->relay.n_hosts, ctx->comm->size, ctx->comm->rank, &lo, &hi);
    return hi - lo;
}

// a device zero: the batch offsets and the record offsets of a rank without hosts
static shd_status window_no_off(shd_ctx* ctx) {
    WindowState& W = ctx->win;
    if (W.no_off.p) return SHD_OK;
    SHD_TRY(W.no_off.ensure(16));
    SHD_HIP(hipMemsetAsync(W.no_off.p, 0, 16, ctx->stream));
    return SHD_OK;
}

// The close under N > 1 ranks: a collective with the same sequence of collectives on every rank,
// whatever happens locally -- the precondition agreement, the sharded round (its own status
// agreement carries an outbound failure: the round then commits nowhere), the sharded record.
static shd_status window_close_sharded(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time,
                                       const uint64_t* d_prio, const uint64_t* d_sock, const uint32_t* d_size,
                                       const uint32_t* d_payload,
                                       const uint32_t* d_dst, const uint32_t* d_pkt, uint64_t n_offers,
                                       uint64_t window_end, uint64_t sim_end, uint64_t bootstrap_end,
                                       const uint32_t** sent_pkt, const uint8_t** sent_status, uint64_t* n_batch,
                                       uint64_t* n_events, const uint32_t** loc_off, const uint32_t** loc_pkt,
                                       const uint64_t** loc_time, uint64_t* n_local, uint64_t* n_stored,
                                       uint64_t* outbound_next_task, uint64_t* min_deliver,
                                       shd_status local = SHD_OK) {
    WindowState& W = ctx->win;
    SHD_HIP(hipSetDevice(ctx->device));
    const uint32_t n_own = window_own_hosts(ctx);
    // 1. the preconditions, agreed: after this either every rank runs the window or none has.
    //    `local`: what the caller found before the call (the staged close's grouping) -- this
    //    rank's word in the agreement
    shd_status pre = local;
    const LedgerBook& B = ctx->ledger.book;
    if (pre == SHD_OK) {
        if (!window_ready(ctx) || !W.opened) pre = SHD_ERR_STATE;
        else if (window_end != W.window_end) pre = SHD_ERR_INVALID;
        else if (n_own && B.oldest != kLedgerNone && ctx->eq.batches - B.oldest >= B.max_live) pre = SHD_ERR_INVALID;
        else if (n_own && n_offers && ctx->outb.with_sockets() && !d_sock) pre = SHD_ERR_INVALID;   // the socket column
        else if (!n_own) pre = window_no_off(ctx);
    }
    SHD_TRY(comm_agree(ctx, pre));
    W.opened = false;
    W.has_out = false;
    W.sent.valid = false;
    // 2. the outbound stage, local; a rank where it fails still enters the round
    shd_batch batch{};
    const uint32_t *b_pkt = nullptr, *b_size = nullptr;
    shd_status st = SHD_OK;
    if (n_own) {
        st = shd_outbound_advance_sockets(ctx, d_off, d_time, d_prio, d_sock, d_size, d_payload, d_dst, d_pkt, n_offers,
                                          window_end, bootstrap_end, &batch, &b_pkt, loc_off, loc_pkt, loc_time,
                                          n_local, n_stored, outbound_next_task);
        if (st == SHD_OK && batch.n_packets) st = shd_outbound_sent_sizes(ctx, &b_size);
        if (st == SHD_OK && batch.n_packets) st = W.status.ensure(batch.n_packets);
    } else {
        batch.src_off = W.no_off.as<uint32_t>();
        if (loc_off) *loc_off = W.no_off.as<uint32_t>();
        if (loc_pkt) *loc_pkt = nullptr;
        if (loc_time) *loc_time = nullptr;
        if (n_local) *n_local = 0;
        if (n_stored) *n_stored = 0;
        if (outbound_next_task) *outbound_next_task = ~0ull;
    }
    if (st != SHD_OK) batch = shd_batch{};   // (nothing of it is read: the round skips its local pipeline)
    // 3. the round, always: an empty batch and a rank without hosts included
    shd_relay_out out{};
    out.status = batch.n_packets ? W.status.as<uint8_t>() : nullptr;
    const shd_round round{window_end, sim_end, bootstrap_end};
    const shd_status st_round = relay_round_sharded_local(ctx, &batch, &round, &out, st);
    // 4. the record, always: a failed round is every rank's status on entry, so every rank skips alike
    uint64_t number = n_own ? ctx->eq.batches : 0;
    SHD_TRY(shd_ledger_record_sharded(ctx, number, b_size, b_pkt, batch.dst_host, W.status.as<uint8_t>(),
                                      batch.n_packets, &out, st_round));
    W.out = out;
    W.out_batch = number;
    W.has_out = out.n_events > 0;
    // a rank that received nothing passes no batch to its queues: no relay output is pending for them
    if (n_own && !W.has_out) ctx->rnd.batch_min_deliver = ~0ull;
    if (sent_pkt) *sent_pkt = b_pkt;
    if (sent_status) *sent_status = W.status.as<uint8_t>();
    if (n_batch) *n_batch = batch.n_packets;
    if (n_events) *n_events = out.n_events;
    if (min_deliver) *min_deliver = out.min_deliver;
    return SHD_OK;
}

// an async copy of n elements of a stage's device array into the caller's buffer (either may be absent)
template <class T>
static shd_status window_fetch(shd_ctx* ctx, T* dst, const T* d_src, uint64_t n) {
    if (dst && d_src && n) SHD_HIP(hipMemcpyAsync(dst, d_src, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return SHD_OK;
}

// the preconditions of a one-context close, before any stage has run
static shd_status window_close_pre(const shd_ctx* ctx, uint64_t window_end) {
    const WindowState& W = ctx->win;
    if (!window_ready(ctx) || !W.opened) return SHD_ERR_STATE;
    if (window_end != W.window_end) return SHD_ERR_INVALID;
    // the batch this close may send must find a row: refused here, before any stage has run
    const LedgerBook& B = ctx->ledger.book;
    if (B.oldest != kLedgerNone && ctx->eq.batches - B.oldest >= B.max_live) return SHD_ERR_INVALID;
    return SHD_OK;
}

// The close on the offers as device arrays.  `local` (under a communicator): this rank's status
// from before the call, its word in the precondition agreement.
static shd_status window_close_arrays(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time,
                                      const uint64_t* d_prio, const uint64_t* d_sock, const uint32_t* d_size,
                                      const uint32_t* d_payload, const uint32_t* d_dst, const uint32_t* d_pkt,
                                      uint64_t n_offers, uint64_t window_end, uint64_t sim_end, uint64_t bootstrap_end,
                                      const uint32_t** sent_pkt, const uint8_t** sent_status, uint64_t* n_batch,
                                      uint64_t* n_events, const uint32_t** loc_off, const uint32_t** loc_pkt,
                                      const uint64_t** loc_time, uint64_t* n_local, uint64_t* n_stored,
                                      uint64_t* outbound_next_task, uint64_t* min_deliver, shd_status local) {
    WindowState& W = ctx->win;
    // what shd_window_sent_host fetches is kept whichever outputs the caller asked for
    WindowState::Sent k{};
    if (!sent_pkt) sent_pkt = &k.pkt;
    if (!sent_status) sent_status = &k.status;
    if (!n_batch) n_batch = &k.n_batch;
    if (!loc_off) loc_off = &k.loc_off;
    if (!loc_pkt) loc_pkt = &k.loc_pkt;
    if (!loc_time) loc_time = &k.loc_time;
    if (!n_local) n_local = &k.n_local;
    if (window_sharded(ctx)) {
        // the one refusal without a collective: a relay not set up under this communicator (every
        // rank sets it up, or none); everything else is agreed between the ranks first
        if (!ctx->relay.ready || !ctx->relay.sharded) return SHD_ERR_STATE;
        SHD_TRY(window_close_sharded(ctx, d_off, d_time, d_prio, d_sock, d_size, d_payload, d_dst, d_pkt, n_offers,
                                     window_end, sim_end, bootstrap_end, sent_pkt, sent_status, n_batch, n_events, loc_off,
                                     loc_pkt, loc_time, n_local, n_stored, outbound_next_task, min_deliver, local));
        W.sent = WindowState::Sent{true, *sent_pkt, *loc_off, *loc_pkt, *sent_status, *loc_time, *n_batch, *n_local,
                                   window_own_hosts(ctx)};
        return SHD_OK;
    }
    SHD_TRY(window_close_pre(ctx, window_end));
    shd_batch batch{};
    const uint32_t* b_pkt = nullptr;
    SHD_TRY(shd_outbound_advance_sockets(ctx, d_off, d_time, d_prio, d_sock, d_size, d_payload, d_dst, d_pkt, n_offers,
                                         window_end, bootstrap_end, &batch, &b_pkt, loc_off, loc_pkt, loc_time, n_local,
                                         n_stored, outbound_next_task));
    W.opened = false;
    W.has_out = false;
    W.sent.valid = false;
    uint64_t sent = 0, low = ~0ull;
    if (batch.n_packets) {
        shd_relay_out out{};
        SHD_TRY(shd_equeue_batch_buffers(ctx, batch.n_packets, &out));
        SHD_TRY(W.status.ensure(batch.n_packets));
        out.status = W.status.as<uint8_t>();
        const shd_round round{window_end, sim_end, bootstrap_end};
        SHD_TRY(shd_relay_round_device(ctx, &batch, &round, &out));
        uint64_t number = 0;
        const uint32_t* b_size = nullptr;
        SHD_TRY(shd_equeue_next_batch(ctx, &number));
        SHD_TRY(shd_outbound_sent_sizes(ctx, &b_size));
        SHD_TRY(shd_ledger_record(ctx, number, b_size, b_pkt, batch.n_packets, out.n_sent));
        W.out = out;
        W.has_out = true;
        sent = out.n_sent;
        low = out.min_deliver;
    }
    *sent_pkt = b_pkt;
    *sent_status = W.status.as<uint8_t>();
    *n_batch = batch.n_packets;
    if (n_events) *n_events = sent;
    if (min_deliver) *min_deliver = low;
    W.sent = WindowState::Sent{true, b_pkt, *loc_off, *loc_pkt, *sent_status, *loc_time, batch.n_packets, *n_local,
                               ctx->outb.n_hosts};
    return SHD_OK;
}

extern "C" {

shd_status shd_window_open(shd_ctx* ctx, uint64_t window_end, uint64_t bootstrap_end, const uint32_t** out_off,
                           const uint32_t** out_pkt, const uint64_t** out_time, const uint8_t** out_kind,
                           uint64_t* n_out, uint64_t* n_stored, uint64_t* inbound_next_task, uint64_t* n_popped,
                           uint64_t* n_pending, uint64_t* queue_next_time) {
    if (!ctx) return SHD_ERR_INVALID;
    WindowState& W = ctx->win;
    if (!window_ready(ctx) || W.opened) return SHD_ERR_STATE;
    W.rec.valid = false;
    if (window_sharded(ctx)) {
        if (window_own_hosts(ctx) == 0) {   // a rank without hosts: nothing pops, nothing is delivered
            SHD_HIP(hipSetDevice(ctx->device));
            SHD_TRY(window_no_off(ctx));
            W.rec = WindowState::Records{true, W.no_off.as<uint32_t>(), nullptr, nullptr, nullptr, 0, 0};
            if (out_off) *out_off = W.no_off.as<uint32_t>();
            if (out_pkt) *out_pkt = nullptr;
            if (out_time) *out_time = nullptr;
            if (out_kind) *out_kind = nullptr;
            if (n_out) *n_out = 0;
            if (n_stored) *n_stored = 0;
            if (inbound_next_task) *inbound_next_task = ~0ull;
            if (n_popped) *n_popped = 0;
            if (n_pending) *n_pending = 0;
            if (queue_next_time) *queue_next_time = ~0ull;
            W.has_out = false;
            W.opened = true;
            W.window_end = window_end;
            return SHD_OK;
        }
        // (relay or queues set up again since the close: the round's output, or its number, is gone)
        if (W.has_out && (W.out.ev_deliver != ctx->relay.m_deliver.p || ctx->eq.batches != W.out_batch)) W.has_out = false;
    } else if (W.has_out && (ctx->eq.lend < 0 || W.out.ev_deliver != ctx->eq.run[ctx->eq.lend].deliver.p)) {
        W.has_out = false;   // (queues set up again since the close: the slot, and the batch in it, are gone)
    }
    shd_equeue_out eo{};
    SHD_TRY(shd_equeue_advance(ctx, W.has_out ? &W.out : nullptr, window_end, &eo));
    W.has_out = false;
    const uint32_t *d_size = nullptr, *d_pkt = nullptr;
    SHD_TRY(shd_ledger_gather(ctx, eo.tag, eo.n_popped, &d_size, &d_pkt));
    WindowState::Records r{};
    SHD_TRY(shd_inbound_advance(ctx, eo.off, eo.deliver, d_size, d_pkt, eo.n_popped, window_end, bootstrap_end, &r.off,
                                &r.pkt, &r.time, &r.kind, &r.n, n_stored, inbound_next_task));
    r.n_hosts = ctx->inb.n_hosts;
    r.valid = true;
    W.rec = r;
    if (out_off) *out_off = r.off;
    if (out_pkt) *out_pkt = r.pkt;
    if (out_time) *out_time = r.time;
    if (out_kind) *out_kind = r.kind;
    if (n_out) *n_out = r.n;
    if (n_popped) *n_popped = eo.n_popped;
    if (n_pending) *n_pending = eo.n_pending;
    if (queue_next_time) *queue_next_time = eo.next_time;
    W.opened = true;
    W.window_end = window_end;
    return SHD_OK;
}

shd_status shd_window_close_sockets(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time,
                                    const uint64_t* d_prio, const uint64_t* d_sock, const uint32_t* d_size,
                                    const uint32_t* d_payload, const uint32_t* d_dst, const uint32_t* d_pkt,
                                    uint64_t n_offers, uint64_t window_end, uint64_t sim_end, uint64_t bootstrap_end,
                                    const uint32_t** sent_pkt, const uint8_t** sent_status, uint64_t* n_batch,
                                    uint64_t* n_events, const uint32_t** loc_off, const uint32_t** loc_pkt,
                                    const uint64_t** loc_time, uint64_t* n_local, uint64_t* n_stored,
                                    uint64_t* outbound_next_task, uint64_t* min_deliver) {
    if (!ctx) return SHD_ERR_INVALID;
    return window_close_arrays(ctx, d_off, d_time, d_prio, d_sock, d_size, d_payload, d_dst, d_pkt, n_offers, window_end,
                               sim_end, bootstrap_end, sent_pkt, sent_status, n_batch, n_events, loc_off, loc_pkt, loc_time,
                               n_local, n_stored, outbound_next_task, min_deliver, SHD_OK);
}

shd_status shd_window_close_staged(shd_ctx* ctx, uint32_t n_stages, const uint32_t* stage_runs,
                                   const uint32_t** run_host, const uint32_t** run_count, const uint64_t* stage_offers,
                                   const uint32_t** offers, uint32_t offer_words, uint64_t time_base,
                                   uint64_t window_end, uint64_t sim_end, uint64_t bootstrap_end,
                                   const uint32_t** sent_pkt, const uint8_t** sent_status, uint64_t* n_batch,
                                   uint64_t* n_events, const uint32_t** loc_off, const uint32_t** loc_pkt,
                                   const uint64_t** loc_time, uint64_t* n_local, uint64_t* n_stored,
                                   uint64_t* outbound_next_task, uint64_t* min_deliver) {
    if (!ctx) return SHD_ERR_INVALID;
    const uint32_t *d_off = nullptr, *d_size = nullptr, *d_payload = nullptr, *d_dst = nullptr, *d_pkt = nullptr;
    const uint64_t *d_time = nullptr, *d_prio = nullptr, *d_sock = nullptr;
    uint64_t n_offers = 0;
    shd_status local = SHD_OK;
    if (window_sharded(ctx)) {
        if (!ctx->relay.ready || !ctx->relay.sharded) return SHD_ERR_STATE;
        // the grouping first and locally, no collective: its status is this rank's word in the
        // agreement, so a refusal here is every rank's and no rank has run a stage
        if (window_own_hosts(ctx) == 0) {
            // a rank without hosts stages nothing (n_stages = 0): any run names a host it does not have
            uint64_t n_runs = 0;
            if (!offer_stages_ok(n_stages, stage_runs, run_host, run_count, stage_offers, offers, offer_words, false,
                                 &n_runs, nullptr))
                local = SHD_ERR_INVALID;
            else if (n_runs)
                local = SHD_ERR_NO_HOST;
        } else {
            local = shd_offers_group(ctx, n_stages, stage_runs, run_host, run_count, stage_offers, offers, offer_words,
                                     time_base, &d_off, &d_time, &d_prio, &d_sock, &d_size, &d_payload, &d_dst, &d_pkt,
                                     &n_offers);
        }
    } else {
        // the window's own preconditions first; a failed grouping leaves the window open and no
        // stage run, so a corrected close may follow
        SHD_TRY(window_close_pre(ctx, window_end));
        SHD_TRY(shd_offers_group(ctx, n_stages, stage_runs, run_host, run_count, stage_offers, offers, offer_words,
                                 time_base, &d_off, &d_time, &d_prio, &d_sock, &d_size, &d_payload, &d_dst, &d_pkt,
                                 &n_offers));
    }
    return window_close_arrays(ctx, d_off, d_time, d_prio, d_sock, d_size, d_payload, d_dst, d_pkt, n_offers, window_end,
                               sim_end, bootstrap_end, sent_pkt, sent_status, n_batch, n_events, loc_off, loc_pkt, loc_time,
                               n_local, n_stored, outbound_next_task, min_deliver, local);
}

shd_status shd_window_records_host(shd_ctx* ctx, uint32_t* off, uint32_t* pkt, uint64_t* time, uint8_t* kind,
                                   uint64_t cap, uint64_t* n_out) {
    if (!ctx) return SHD_ERR_INVALID;
    const WindowState::Records& R = ctx->win.rec;
    const InboundState& I = ctx->inb;
    // the arrays are the inbound stage's: gone when it was set up again or its buffers grew since
    if (!R.valid) return SHD_ERR_STATE;
    if (R.n_hosts && (!I.ready || I.n_hosts != R.n_hosts || R.off != I.o_off.p || R.pkt != I.o_pkt.p ||
                      R.time != I.o_time.p || R.kind != I.o_kind.p))
        return SHD_ERR_STATE;
    if (n_out) *n_out = R.n;
    if ((pkt || time || kind) && cap < R.n) return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    SHD_TRY(window_fetch(ctx, off, R.off, (uint64_t)R.n_hosts + 1));
    SHD_TRY(window_fetch(ctx, pkt, R.pkt, R.n));
    SHD_TRY(window_fetch(ctx, time, R.time, R.n));
    SHD_TRY(window_fetch(ctx, kind, R.kind, R.n));
    return wait_stream(ctx, ctx->stream);
}

shd_status shd_window_sent_host(shd_ctx* ctx, uint32_t* sent_pkt, uint8_t* sent_status, uint64_t cap_batch,
                                uint32_t* loc_off, uint32_t* loc_pkt, uint64_t* loc_time, uint64_t cap_local,
                                uint64_t* n_batch, uint64_t* n_local) {
    if (!ctx) return SHD_ERR_INVALID;
    const WindowState::Sent& S = ctx->win.sent;
    const OutboundState& O = ctx->outb;
    // the arrays are the outbound stage's and the window's status array
    if (!S.valid) return SHD_ERR_STATE;
    if (S.n_hosts && (!O.ready || O.n_hosts != S.n_hosts || S.pkt != O.b_pkt.p || S.loc_off != O.loc_off.p ||
                      S.loc_pkt != O.l_pkt.p || S.loc_time != O.l_time.p || S.status != ctx->win.status.p))
        return SHD_ERR_STATE;
    if (n_batch) *n_batch = S.n_batch;
    if (n_local) *n_local = S.n_local;
    if (((sent_pkt || sent_status) && cap_batch < S.n_batch) || ((loc_pkt || loc_time) && cap_local < S.n_local))
        return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    SHD_TRY(window_fetch(ctx, sent_pkt, S.pkt, S.n_batch));
    SHD_TRY(window_fetch(ctx, sent_status, S.status, S.n_batch));
    SHD_TRY(window_fetch(ctx, loc_off, S.loc_off, (uint64_t)S.n_hosts + 1));
    SHD_TRY(window_fetch(ctx, loc_pkt, S.loc_pkt, S.n_local));
    SHD_TRY(window_fetch(ctx, loc_time, S.loc_time, S.n_local));
    return wait_stream(ctx, ctx->stream);
}

shd_status shd_window_close(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time, const uint64_t* d_prio,
                            const uint32_t* d_size, const uint32_t* d_payload, const uint32_t* d_dst,
                            const uint32_t* d_pkt, uint64_t n_offers, uint64_t window_end, uint64_t sim_end,
                            uint64_t bootstrap_end, const uint32_t** sent_pkt, const uint8_t** sent_status,
                            uint64_t* n_batch, uint64_t* n_events, const uint32_t** loc_off, const uint32_t** loc_pkt,
                            const uint64_t** loc_time, uint64_t* n_local, uint64_t* n_stored,
                            uint64_t* outbound_next_task, uint64_t* min_deliver) {
    return shd_window_close_sockets(ctx, d_off, d_time, d_prio, nullptr, d_size, d_payload, d_dst, d_pkt, n_offers,
                                    window_end, sim_end, bootstrap_end, sent_pkt, sent_status, n_batch, n_events, loc_off,
                                    loc_pkt, loc_time, n_local, n_stored, outbound_next_task, min_deliver);
}

// Both stages' buckets from new link rates, between a close and the next open.  create_token_bucket
// (relay/mod.rs:291-302) per direction; UINT64_MAX leaves a direction as it is.  Both stages are
// checked before either changes: a refusal by one leaves both untouched.
shd_status shd_window_update_bandwidth(shd_ctx* ctx, uint64_t n, const uint32_t* host, const uint64_t* down_bytes_per_s,
                                       const uint64_t* up_bytes_per_s, uint64_t at_time, uint32_t* err_host) {
    if (!ctx) return SHD_ERR_INVALID;
    if (!window_ready(ctx) || ctx->win.opened) return SHD_ERR_STATE;
    if (n && (!host || !down_bytes_per_s || !up_bytes_per_s)) return SHD_ERR_INVALID;
    if (n == 0) return SHD_OK;
    if (window_own_hosts(ctx) == 0) return SHD_ERR_INVALID;   // (a rank without hosts has no stage: any index is past it)
    std::vector<uint32_t> hs[2];
    std::vector<uint64_t> cap[2], inc[2], itv[2];
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t bps[2] = {down_bytes_per_s[i], up_bytes_per_s[i]};
        for (int d = 0; d < 2; ++d) {
            if (bps[d] == ~0ull) continue;
            uint64_t c, k, t;
            rate_from_bandwidth(bps[d], c, k, t);
            hs[d].push_back(host[i]);
            cap[d].push_back(c);
            inc[d].push_back(k);
            itv[d].push_back(t);
        }
    }
    // (an index past the stage in a direction that UINT64_MAX skips is still refused)
    for (uint64_t i = 0; i < n; ++i)
        if (host[i] >= ctx->inb.n_hosts) return SHD_ERR_INVALID;
    const RateTarget tg[2] = {kRateInbound, kRateOutbound};
    shd_status st = SHD_OK;
    for (int d = 0; d < 2 && st == SHD_OK; ++d)
        st = rate_stage_check(ctx, tg[d], hs[d].size(), hs[d].data(), cap[d].data(), inc[d].data(), itv[d].data(), at_time);
    if (st == SHD_OK) st = rate_stage_result(ctx, 1u << kRateInbound | 1u << kRateOutbound, err_host);
    for (int d = 0; d < 2 && st == SHD_OK; ++d) st = rate_stage_apply(ctx, tg[d], at_time);
    if (st == SHD_OK) st = wait_stream(ctx, ctx->stream);
    ctx->rate.n_rec[kRateInbound] = ctx->rate.n_rec[kRateOutbound] = 0;
    return st;
}

}  // extern "C"
