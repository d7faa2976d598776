// One scheduling window as two engine calls, no packet data crossing the host:
//   shd_window_open    event queues (merging the relay output the last close left) -> ledger
//                      gather on the popped tags -> inbound stage
//   [the CPU: the inbound records make the sockets answer -- this window's offers]
//   shd_window_close   outbound stage -> relay round into the queues' lent slot -> ledger record
// The stages are the ones the separate calls drive (equeue.hip, ledger.hip, inbound.hip,
// outbound.hip, relay.hip); this file only chains them and keeps what lies between two calls.
#include "ctx.h"

using namespace shd;

// relay, queues, runahead, both stages and the ledger set up for the same hosts, first_host 0, no
// communicator of more than one rank (a received event's index would name the sender rank's batch)
static bool window_ready(const shd_ctx* ctx) {
    if (ctx->comm && ctx->comm->size > 1) return false;
    if (!ctx->relay.ready || ctx->relay.sharded || !ctx->eq.ready || !ctx->rnd.ready || !ctx->inb.ready ||
        !ctx->outb.ready || !ctx->ledger.ready)
        return false;
    const uint32_t H = ctx->relay.n_hosts;
    return ctx->eq.n_hosts == H && ctx->eq.n_total == H && ctx->inb.n_hosts == H && ctx->outb.n_hosts == H &&
           ctx->outb.first_host == 0;
}

extern "C" {

shd_status shd_window_open(shd_ctx* ctx, uint64_t window_end, uint64_t bootstrap_end, const uint32_t** out_off,
                           const uint32_t** out_pkt, const uint64_t** out_time, const uint8_t** out_kind,
                           uint64_t* n_out, uint64_t* n_stored, uint64_t* inbound_next_task, uint64_t* n_popped,
                           uint64_t* n_pending, uint64_t* queue_next_time) {
    if (!ctx) return SHD_ERR_INVALID;
    WindowState& W = ctx->win;
    if (!window_ready(ctx) || W.opened) return SHD_ERR_STATE;
    // (queues set up again since the close: the slot, and the batch in it, are gone)
    if (W.has_out && (ctx->eq.lend < 0 || W.out.ev_deliver != ctx->eq.run[ctx->eq.lend].deliver.p)) W.has_out = false;
    shd_equeue_out eo{};
    SHD_TRY(shd_equeue_advance(ctx, W.has_out ? &W.out : nullptr, window_end, &eo));
    W.has_out = false;
    const uint32_t *d_size = nullptr, *d_pkt = nullptr;
    SHD_TRY(shd_ledger_gather(ctx, eo.tag, eo.n_popped, &d_size, &d_pkt));
    SHD_TRY(shd_inbound_advance(ctx, eo.off, eo.deliver, d_size, d_pkt, eo.n_popped, window_end, bootstrap_end, out_off,
                                out_pkt, out_time, out_kind, n_out, n_stored, inbound_next_task));
    if (n_popped) *n_popped = eo.n_popped;
    if (n_pending) *n_pending = eo.n_pending;
    if (queue_next_time) *queue_next_time = eo.next_time;
    W.opened = true;
    W.window_end = window_end;
    return SHD_OK;
}

shd_status shd_window_close(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time, const uint64_t* d_prio,
                            const uint32_t* d_size, const uint32_t* d_payload, const uint32_t* d_dst,
                            const uint32_t* d_pkt, uint64_t n_offers, uint64_t window_end, uint64_t sim_end,
                            uint64_t bootstrap_end, const uint32_t** sent_pkt, const uint8_t** sent_status,
                            uint64_t* n_batch, uint64_t* n_events, const uint32_t** loc_off, const uint32_t** loc_pkt,
                            const uint64_t** loc_time, uint64_t* n_local, uint64_t* n_stored,
                            uint64_t* outbound_next_task, uint64_t* min_deliver) {
    if (!ctx) return SHD_ERR_INVALID;
    WindowState& W = ctx->win;
    if (!window_ready(ctx) || !W.opened) return SHD_ERR_STATE;
    if (window_end != W.window_end) return SHD_ERR_INVALID;
    // the batch this close may send must find a row: refused here, before any stage has run
    const LedgerBook& B = ctx->ledger.book;
    if (B.oldest != kLedgerNone && ctx->eq.batches - B.oldest >= B.max_live) return SHD_ERR_INVALID;
    shd_batch batch{};
    const uint32_t* b_pkt = nullptr;
    SHD_TRY(shd_outbound_advance(ctx, d_off, d_time, d_prio, d_size, d_payload, d_dst, d_pkt, n_offers, window_end,
                                 bootstrap_end, &batch, &b_pkt, loc_off, loc_pkt, loc_time, n_local, n_stored,
                                 outbound_next_task));
    W.opened = false;
    W.has_out = false;
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
    if (sent_pkt) *sent_pkt = b_pkt;
    if (sent_status) *sent_status = W.status.as<uint8_t>();
    if (n_batch) *n_batch = batch.n_packets;
    if (n_events) *n_events = sent;
    if (min_deliver) *min_deliver = low;
    return SHD_OK;
}

}  // extern "C"
