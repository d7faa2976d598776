// The relay round's frame (overview and the list of units: relay_priv.h): the narrow pipelines'
// arguments, the ladder over the pipelines, the commit, and the relay's C entry points with the
// setup's two packing kernels.  The pipelines themselves live in the other relay units.
#include <algorithm>
#include <cstring>
#include <vector>

#include "relay_bins.h"

namespace shd {

RelayArgs3 relay_args3(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o) {
    RelayState& R = ctx->relay;
    const uint64_t n = b->n_packets;
    const uint32_t H = R.n_hosts;
    RelayArgs3 a{};
    a.gs = kS5Hosts;
    a.n_hosts = H;
    a.n_nodes = R.n_nodes;
    a.src_lo = R.src_lo;
    a.n_src = R.n_src;
    a.src_off = b->src_off;
    a.send_time = b->send_time;
    a.dst_host = b->dst_host;
    a.payload = b->payload;
    a.chance = b->chance;
    a.keep_rng = R.cpu_draws ? 1u : 0u;
    a.host_node = R.host_node.as<uint32_t>();
    a.path = R.path.as<uint2>();
    a.order = R.order.as<uint32_t>();
    a.rng = R.rng.as<uint64_t>();
    a.next_id = R.next_id.as<uint64_t>();
    a.rng_out = R.rng2.as<uint64_t>();
    a.next_id_out = R.next_id2.as<uint64_t>();
    a.counts = R.count_on ? R.counts_round.as<unsigned long long>() : nullptr;
    a.round_end = rd->round_end;
    a.sim_end = rd->sim_end;
    a.bootstrap_end = rd->bootstrap_end;
    // event ids below 2^32 for the whole round: records carry absolute ids, no per-event gather
    // (rel_ids: records keep the id relative to the host's first of the round)
    a.abs_seq = !R.rel_ids && R.seq_bound + n < (1ull << 32) ? 1u : 0u;
    a.status = o->status;
    a.rec = R.rec.as<uint4>();
    a.key = R.ev_val.as<uint32_t>();
    a.red = R.red.as<unsigned long long>();
    return a;
}

shd_status relay_read_red(shd_ctx* ctx) {
    RelayState& R = ctx->relay;
    SHD_HIP(hipGetLastError());
    SHD_TRY(readback(ctx, ctx->stream, 8, R.red.p, 8 * sizeof(unsigned long long)));
    std::memcpy(R.red_host, ctx->h_pin + 8, sizeof(R.red_host));
    return SHD_OK;
}

// One round: the new host state (RNG streams, event ids) is written to the second buffer and
// committed only when the round succeeds, so a failed round leaves the hosts untouched.
__global__ __launch_bounds__(256) void counts_commit(unsigned long long* __restrict__ counts,
                                                     const unsigned long long* __restrict__ delta,
                                                     uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && delta[i]) {   // RoutingInfo::increment_packet_count saturates (graph/mod.rs:451-458)
        const unsigned long long c = counts[i], d = delta[i];
        counts[i] = c + d < c ? ~0ull : c + d;
    }
}

// The round's pipelines and checks; nothing of the hosts' state is committed yet.  A ladder: the
// bins (7), else the radix sort (3) when a bin overflowed or the bins do not apply, else the
// 64-bit records (1) when the table or a deliver offset of this round is wide.
shd_status relay_run(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o) {
    RelayState& R = ctx->relay;
    const uint32_t H = R.n_hosts;
    const uint64_t nn = (uint64_t)R.n_nodes * R.n_nodes;
    SHD_TRY(R.red.ensure(64));
    SHD_TRY(R.dst_cnt.ensure((size_t)(H + 1) * 4));
    if (R.count_on) SHD_TRY(R.counts_round.ensure(nn * 8));
    // every rung counts into a zeroed per-round buffer; only the committed attempt reaches the
    // counters (a rerun or a failed round must not count)
    auto rung = [&](int pipe) -> shd_status {
        if (R.count_on) SHD_HIP(hipMemsetAsync(R.counts_round.p, 0, nn * 8, ctx->stream));
        R.last_pipe = pipe;
        return SHD_OK;
    };
    bool narrow = R.table_narrow && !R.force_v1;
    bool sorted = false;
    if (narrow && relay_v7_ok(ctx, b->n_packets, div_up(H, kBinDst))) {
        SHD_TRY(rung(7));
        SHD_TRY(relay_device_v7(ctx, b, rd, o));
        sorted = !R.red_host[6];   // else a bin overflowed: redo with the radix pipeline
    }
    if (narrow && !sorted) {
        SHD_TRY(rung(3));
        SHD_TRY(relay_device_v3(ctx, b, rd, o));
    }
    if (narrow && R.red_host[4]) narrow = false;   // a deliver offset needs 64 bits: redo with v1
    if (!narrow) {
        SHD_TRY(rung(1));
        SHD_TRY(relay_device_v1(ctx, b, rd, o));
    }
    if (R.red_host[3] != ~0ull) return SHD_ERR_NO_HOST;
    if (narrow && R.red_host[5]) return SHD_ERR_INVALID;   // a host's send times went backwards
    R.last_v2 = narrow;
    return SHD_OK;
}

// Commit a successful round: the per-path counters, the new RNG streams and event ids.
shd_status relay_commit(shd_ctx* ctx, shd_relay_out* o) {
    RelayState& R = ctx->relay;
    const uint64_t nn = (uint64_t)R.n_nodes * R.n_nodes;
    if (R.count_on && nn) {
        counts_commit<<<div_up(nn, 256), 256, 0, ctx->stream>>>(
            R.counts.as<unsigned long long>(), R.counts_round.as<unsigned long long>(), nn);
        SHD_HIP(hipGetLastError());
    }
    std::swap(R.rng, R.rng2);
    std::swap(R.next_id, R.next_id2);
    R.seq_bound += R.red_host[2];
    o->min_deliver = R.red_host[0];
    o->min_latency = R.red_host[1];
    o->n_sent = R.red_host[2];
    return SHD_OK;
}

static shd_status relay_device(shd_ctx* ctx, const shd_batch* b, const shd_round* rd,
                               shd_relay_out* o) {
    SHD_TRY(relay_run(ctx, b, rd, o));
    SHD_TRY(relay_commit(ctx, o));
    o->n_dst = ctx->relay.n_hosts;
    o->n_events = (uint32_t)o->n_sent;
    round_note(ctx, o->min_deliver, o->min_latency);
    return SHD_OK;
}

// shd_relay_flush (flush.hip): one round on the batch it grouped on the device
shd_status relay_flush_round(shd_ctx* ctx, const shd_batch* b, const shd_round* rd, shd_relay_out* o) {
    return relay_device(ctx, b, rd, o);
}

// the bit-packed host -> node map for relay_stamp_v6 (built at setup)
__global__ __launch_bounds__(256) void pack_host_node(const uint32_t* __restrict__ host_node,
                                                      uint32_t n_hosts, uint32_t bits,
                                                      uint32_t n_words, uint32_t* __restrict__ out) {
    const uint32_t wi = blockIdx.x * 256 + threadIdx.x;
    if (wi >= n_words) return;
    // word wi holds bits [32 wi, 32 wi + 32) of the concatenated entries
    const uint64_t b0 = (uint64_t)wi * 32;
    uint32_t word = 0;
    for (uint64_t j = b0 / bits; j < n_hosts && j * bits < b0 + 32; ++j) {
        const int64_t sh = (int64_t)(j * bits) - (int64_t)b0;
        const uint64_t v = host_node[j];
        word |= sh >= 0 ? (uint32_t)(v << sh) : (uint32_t)(v >> -sh);
    }
    out[wi] = word;
}

// pack the routing table for the narrow pipeline: one 8-byte gather per packet
__global__ __launch_bounds__(256) void pack_path(const uint64_t* __restrict__ lat,
                                                 const float* __restrict__ loss, uint64_t nn,
                                                 uint2* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nn) out[i] = make_uint2((uint32_t)lat[i], __float_as_uint(loss[i]));
}

}  // namespace shd

using namespace shd;

extern "C" {

shd_status shd_relay_setup(shd_ctx* ctx, uint32_t n_hosts, const uint32_t* host_node,
                           uint32_t n_nodes, const uint64_t* lat, const float* loss,
                           const uint64_t* rng_state, const uint64_t* next_event_id) {
    if (!ctx || n_hosts == 0 || !host_node || !rng_state || !next_event_id || n_nodes == 0)
        return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    RelayState& R = ctx->relay;
    hipStream_t s = ctx->stream;
    for (uint32_t h = 0; h < n_hosts; h++)
        if (host_node[h] >= n_nodes) return SHD_ERR_INVALID;
    if ((lat == nullptr) != (loss == nullptr)) return SHD_ERR_INVALID;
    if (!lat) {
        if (!ctx->t_full || ctx->t_cols != n_nodes) return SHD_ERR_STATE;
        R.own_table = false;
    } else {
        const size_t nn = (size_t)n_nodes * n_nodes;
        SHD_TRY(R.lat.ensure(nn * 8));
        SHD_TRY(R.loss.ensure(nn * 4));
        SHD_HIP(hipMemcpyAsync(R.lat.p, lat, nn * 8, hipMemcpyHostToDevice, s));
        SHD_HIP(hipMemcpyAsync(R.loss.p, loss, nn * 4, hipMemcpyHostToDevice, s));
        R.own_table = true;
    }
    SHD_TRY(R.host_node.ensure((size_t)n_hosts * 4));
    SHD_TRY(R.rng.ensure((size_t)n_hosts * 32));
    SHD_TRY(R.next_id.ensure((size_t)n_hosts * 8));
    SHD_TRY(R.rng2.ensure((size_t)n_hosts * 32));
    SHD_TRY(R.next_id2.ensure((size_t)n_hosts * 8));
    SHD_TRY(R.counts.ensure((size_t)n_nodes * n_nodes * 8));
    SHD_HIP(hipMemcpyAsync(R.host_node.p, host_node, (size_t)n_hosts * 4, hipMemcpyHostToDevice, s));
    // under a communicator of > 1 ranks this context stamps only its shard of the hosts
    R.sharded = ctx->comm && ctx->comm->size > 1;
    uint32_t src_lo = 0, src_hi = n_hosts;
    if (R.sharded) shard_range(n_hosts, ctx->comm->size, ctx->comm->rank, &src_lo, &src_hi);
    R.src_lo = src_lo;
    R.n_src = src_hi - src_lo;
    {   // stamp workgroups take hosts in source-node order: their path gathers share table rows
        std::vector<uint32_t> ord(R.n_src);
        for (uint32_t h = 0; h < R.n_src; h++) ord[h] = src_lo + h;
        std::stable_sort(ord.begin(), ord.end(),
                         [&](uint32_t x, uint32_t y) { return host_node[x] < host_node[y]; });
        SHD_TRY(R.order.ensure(std::max<size_t>(ord.size(), 1) * 4));
        if (!ord.empty())
            SHD_HIP(hipMemcpyAsync(R.order.p, ord.data(), ord.size() * 4, hipMemcpyHostToDevice, s));
        SHD_HIP(hipStreamSynchronize(s));
    }
    // both state buffers hold every host: a round writes only its source hosts' entries into the
    // second buffer, so the others keep their values across the swap
    SHD_HIP(hipMemcpyAsync(R.rng.p, rng_state, (size_t)n_hosts * 32, hipMemcpyHostToDevice, s));
    SHD_HIP(hipMemcpyAsync(R.next_id.p, next_event_id, (size_t)n_hosts * 8, hipMemcpyHostToDevice, s));
    SHD_HIP(hipMemcpyAsync(R.rng2.p, rng_state, (size_t)n_hosts * 32, hipMemcpyHostToDevice, s));
    SHD_HIP(hipMemcpyAsync(R.next_id2.p, next_event_id, (size_t)n_hosts * 8, hipMemcpyHostToDevice, s));
    R.seq_bound = 0;   // upper bound of every next event id (grows by n_sent per round)
    for (uint32_t h = 0; h < n_hosts; h++) R.seq_bound = std::max<uint64_t>(R.seq_bound, next_event_id[h]);
    SHD_HIP(hipMemsetAsync(R.counts.p, 0, (size_t)n_nodes * n_nodes * 8, s));
    SHD_HIP(hipStreamSynchronize(s));
    R.n_hosts = n_hosts;
    R.n_nodes = n_nodes;
    if (ctx->comm) SHD_TRY(relay_shard_alloc(ctx));   // shd_relay_round_sharded at any rank count
    {   // v2 needs every path latency < 2^32 ns (max over the table)
        const uint64_t* tl = R.own_table ? R.lat.as<uint64_t>() : ctx->t_lat.as<uint64_t>();
        const uint64_t nn = (uint64_t)n_nodes * n_nodes;
        uint64_t mx = 0;
        SHD_TRY(max_u64_device(ctx, tl, nn, &mx));
        R.table_narrow = (mx >> 32) == 0;
        if (R.table_narrow) {   // packed {lat32, loss} table: one 8-byte gather per packet
            const float* tp = R.own_table ? R.loss.as<float>() : ctx->t_loss.as<float>();
            SHD_TRY(R.path.ensure(nn * 8));
            pack_path<<<div_up(nn, 256), 256, 0, s>>>(tl, tp, nn, R.path.as<uint2>());
            SHD_HIP(hipGetLastError());
            SHD_HIP(hipStreamSynchronize(s));
        }
    }
    R.force_v1 = ctx->knobs.on(K_RELAY_FORCE_V1);
    R.force_v3 = ctx->knobs.on(K_RELAY_FORCE_V3);   // testing: radix pipeline instead of v7
    {   // bit-packed host -> node map for the LDS-resident stamp, when it fits
        uint32_t bits = 1;
        while (bits < 32 && (n_nodes - 1) >> bits) ++bits;
        const uint64_t words = ((uint64_t)n_hosts * bits + 31) / 32 + 1;
        R.hn_bits = 0;   // (SHD_RELAY_NO_LDS_MAP=1, testing: force the gather path)
        if (words * 4 + relay_stamp_fixed_lds() <= ctx->max_lds && !ctx->knobs.on(K_RELAY_NO_LDS_MAP)) {
            SHD_TRY(R.hn_packed.ensure(words * 4));
            pack_host_node<<<div_up(words, 256), 256, 0, s>>>(R.host_node.as<uint32_t>(), n_hosts, bits,
                                                              (uint32_t)words, R.hn_packed.as<uint32_t>());
            SHD_HIP(hipGetLastError());
            SHD_HIP(hipStreamSynchronize(s));
            R.hn_bits = bits;
            R.hn_words = (uint32_t)words;
        }
    }
    R.ready = true;
    R.set_up = true;
    return SHD_OK;
}

// A new table under a relay that keeps everything else: the host -> node map, the stamp order,
// the hosts' RNG streams and event ids, seq_bound, the path counters, the sharding and the knobs
// read at setup.  Everything is checked (and the table's extremes are known) before anything changes.
shd_status shd_relay_retable(shd_ctx* ctx, uint32_t n_nodes, const uint64_t* lat, const float* loss) {
    if (!ctx) return SHD_ERR_INVALID;
    RelayState& R = ctx->relay;
    if (!R.set_up) return SHD_ERR_STATE;
    if (n_nodes != R.n_nodes || (lat == nullptr) != (loss == nullptr)) return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t nn = (uint64_t)n_nodes * n_nodes;
    RoundState& W = ctx->rnd;
    uint64_t mx = 0, mn = ~0ull;
    if (!lat) {
        if (!ctx->t_full || ctx->t_cols != n_nodes) return SHD_ERR_STATE;
        SHD_TRY(max_u64_device(ctx, ctx->t_lat.as<uint64_t>(), nn, &mx));
        if (W.ready) SHD_TRY(min_u64_device(ctx, ctx->t_lat.as<uint64_t>(), nn, &mn));
    } else {
        for (uint64_t i = 0; i < nn; ++i) {
            mx = std::max(mx, lat[i]);
            mn = std::min(mn, lat[i]);
        }
    }
    if (W.ready && mn == 0) return SHD_ERR_INVALID;   // Runahead::new asserts a non-zero minimum latency
    if ((mx >> 32) == 0) SHD_TRY(R.path.ensure(nn * 8));
    if (lat) {
        SHD_TRY(R.lat.ensure(nn * 8));
        SHD_TRY(R.loss.ensure(nn * 4));
        SHD_HIP(hipMemcpyAsync(R.lat.p, lat, nn * 8, hipMemcpyHostToDevice, s));
        SHD_HIP(hipMemcpyAsync(R.loss.p, loss, nn * 4, hipMemcpyHostToDevice, s));
    }
    R.own_table = lat != nullptr;
    R.table_narrow = (mx >> 32) == 0;
    if (R.table_narrow) {
        const uint64_t* tl = R.own_table ? R.lat.as<uint64_t>() : ctx->t_lat.as<uint64_t>();
        const float* tp = R.own_table ? R.loss.as<float>() : ctx->t_loss.as<float>();
        pack_path<<<div_up(nn, 256), 256, 0, s>>>(tl, tp, nn, R.path.as<uint2>());
        SHD_HIP(hipGetLastError());
    }
    SHD_HIP(hipStreamSynchronize(s));   // the caller's arrays are free again
    R.ready = true;
    if (W.ready) {
        // manager.rs:246-251 takes min_possible from RoutingInfo; a latency observed on the old
        // network says nothing about the new one.  batch_min_deliver stays: the pending relay
        // output is still to be merged (the reason this call exists beside shd_runahead_setup)
        W.min_possible = mn;
        W.min_used = ~0ull;
    }
    return SHD_OK;
}

shd_status shd_relay_round_device(shd_ctx* ctx, const shd_batch* d_batch, const shd_round* round,
                                  shd_relay_out* d_out) {
    if (!ctx || !d_batch || !round || !d_out) return SHD_ERR_INVALID;
    if (!ctx->relay.ready || ctx->relay.sharded) return SHD_ERR_STATE;
    if (!d_batch->src_off || (d_batch->n_packets && (!d_batch->send_time || !d_batch->dst_host ||
                                                     !d_batch->payload)))
        return SHD_ERR_INVALID;
    if (!d_out->status || !d_out->ev_off || !d_out->ev_deliver || !d_out->ev_src ||
        !d_out->ev_seq || !d_out->ev_pkt)
        return SHD_ERR_INVALID;
    // an output slot lent by shd_equeue_batch_buffers holds lend_cap events: a round that could
    // send more would write past it, so it is refused before any kernel runs
    const EqState& Q = ctx->eq;
    if (Q.ready && Q.lend >= 0 && d_out->ev_deliver == Q.run[Q.lend].deliver.p &&
        d_batch->n_packets > Q.lend_cap)
        return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    return relay_device(ctx, d_batch, round, d_out);
}

shd_status shd_relay_round(shd_ctx* ctx, const shd_batch* batch, const shd_round* round,
                           shd_relay_out* out) {
    if (!ctx || !batch || !round || !out || !batch->src_off) return SHD_ERR_INVALID;
    RelayState& R = ctx->relay;
    if (!R.ready || R.sharded) return SHD_ERR_STATE;
    SHD_HIP(hipSetDevice(ctx->device));
    const uint64_t n = batch->n_packets;
    const uint32_t H = R.n_hosts;
    if (batch->src_off[0] != 0 || batch->src_off[H] != n) return SHD_ERR_INVALID;
    for (uint32_t h = 0; h < H; h++)
        if (batch->src_off[h + 1] < batch->src_off[h]) return SHD_ERR_INVALID;
    hipStream_t s = ctx->stream;
    const size_t nn = std::max<uint64_t>(n, 1);
    SHD_TRY(R.pk_off.ensure((size_t)(H + 1) * 4));
    SHD_TRY(R.pk_time.ensure(nn * 8));
    SHD_TRY(R.pk_dst.ensure(nn * 4));
    SHD_TRY(R.pk_pay.ensure(nn * 4));
    SHD_TRY(R.st.ensure(nn));
    SHD_TRY(R.ev_off.ensure((size_t)(H + 1) * 4));
    SHD_TRY(R.ev_deliver.ensure(nn * 8));
    SHD_TRY(R.ev_src.ensure(nn * 4));
    SHD_TRY(R.ev_seq.ensure(nn * 8));
    SHD_TRY(R.ev_pkt.ensure(nn * 4));
    SHD_HIP(hipMemcpyAsync(R.pk_off.p, batch->src_off, (size_t)(H + 1) * 4, hipMemcpyHostToDevice, s));
    if (n) {
        SHD_HIP(hipMemcpyAsync(R.pk_time.p, batch->send_time, n * 8, hipMemcpyHostToDevice, s));
        SHD_HIP(hipMemcpyAsync(R.pk_dst.p, batch->dst_host, n * 4, hipMemcpyHostToDevice, s));
        SHD_HIP(hipMemcpyAsync(R.pk_pay.p, batch->payload, n * 4, hipMemcpyHostToDevice, s));
    }
    const double* d_chance = nullptr;
    if (batch->chance && n) {
        SHD_TRY(R.pk_chance.ensure(n * 8));
        SHD_HIP(hipMemcpyAsync(R.pk_chance.p, batch->chance, n * 8, hipMemcpyHostToDevice, s));
        d_chance = R.pk_chance.as<double>();
    }
    shd_batch db{n, R.pk_off.as<uint32_t>(), R.pk_time.as<uint64_t>(), R.pk_dst.as<uint32_t>(),
                 R.pk_pay.as<uint32_t>(), d_chance};
    shd_relay_out dout{};
    dout.status = R.st.as<uint8_t>();
    dout.ev_off = R.ev_off.as<uint32_t>();
    dout.ev_deliver = R.ev_deliver.as<uint64_t>();
    dout.ev_src = R.ev_src.as<uint32_t>();
    dout.ev_seq = R.ev_seq.as<uint64_t>();
    dout.ev_pkt = R.ev_pkt.as<uint32_t>();
    SHD_TRY(relay_device(ctx, &db, round, &dout));
    const uint64_t ns = dout.n_sent;
    if (out->status && n) SHD_HIP(hipMemcpyAsync(out->status, dout.status, n, hipMemcpyDeviceToHost, s));
    if (out->ev_off) SHD_HIP(hipMemcpyAsync(out->ev_off, dout.ev_off, (size_t)(H + 1) * 4, hipMemcpyDeviceToHost, s));
    if (ns) {
        if (out->ev_deliver) SHD_HIP(hipMemcpyAsync(out->ev_deliver, dout.ev_deliver, ns * 8, hipMemcpyDeviceToHost, s));
        if (out->ev_src) SHD_HIP(hipMemcpyAsync(out->ev_src, dout.ev_src, ns * 4, hipMemcpyDeviceToHost, s));
        if (out->ev_seq) SHD_HIP(hipMemcpyAsync(out->ev_seq, dout.ev_seq, ns * 8, hipMemcpyDeviceToHost, s));
        if (out->ev_pkt) SHD_HIP(hipMemcpyAsync(out->ev_pkt, dout.ev_pkt, ns * 4, hipMemcpyDeviceToHost, s));
    }
    SHD_HIP(hipStreamSynchronize(s));
    out->min_deliver = dout.min_deliver;
    out->min_latency = dout.min_latency;
    out->n_sent = ns;
    out->n_dst = H;
    out->n_events = (uint32_t)ns;
    return SHD_OK;
}

shd_status shd_relay_round_sharded(shd_ctx* ctx, const shd_batch* d_batch, const shd_round* round,
                                   shd_relay_out* d_out) {
    if (!ctx || !d_batch || !round || !d_out) return SHD_ERR_INVALID;
    if (!ctx->comm || !ctx->relay.ready || ctx->relay.sharded != (ctx->comm->size > 1))
        return SHD_ERR_STATE;
    if (!d_batch->src_off || (d_batch->n_packets && (!d_batch->send_time || !d_batch->dst_host ||
                                                     !d_batch->payload)))
        return SHD_ERR_INVALID;
    if (d_batch->n_packets && !d_out->status) return SHD_ERR_INVALID;
    if (!ctx->relay.x_words.p || !ctx->relay.x_roff.p) return SHD_ERR_STATE;   // set up before the communicator
    SHD_HIP(hipSetDevice(ctx->device));
    return relay_round_sharded_local(ctx, d_batch, round, d_out, SHD_OK);
}

shd_status shd_relay_get_host_state(shd_ctx* ctx, uint64_t* rng_state, uint64_t* next_event_id) {
    if (!ctx) return SHD_ERR_INVALID;
    RelayState& R = ctx->relay;
    if (!R.ready) return SHD_ERR_STATE;
    SHD_HIP(hipSetDevice(ctx->device));
    if (rng_state)
        SHD_HIP(hipMemcpyAsync(rng_state, R.rng.p, (size_t)R.n_hosts * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (next_event_id)
        SHD_HIP(hipMemcpyAsync(next_event_id, R.next_id.p, (size_t)R.n_hosts * 8, hipMemcpyDeviceToHost, ctx->stream));
    SHD_HIP(hipStreamSynchronize(ctx->stream));
    return SHD_OK;
}

shd_status shd_relay_last_pipeline(const shd_ctx* ctx, int32_t* pipeline) {
    if (!ctx || !pipeline) return SHD_ERR_INVALID;
    *pipeline = ctx->relay.last_pipe;
    return SHD_OK;
}

shd_status shd_relay_set_counters(shd_ctx* ctx, int32_t enabled) {
    if (!ctx) return SHD_ERR_INVALID;
    ctx->relay.count_on = enabled != 0;
    return SHD_OK;
}

shd_status shd_path_packet_counts(shd_ctx* ctx, uint64_t* counts) {
    if (!ctx || !counts) return SHD_ERR_INVALID;
    RelayState& R = ctx->relay;
    if (!R.ready) return SHD_ERR_STATE;
    SHD_HIP(hipSetDevice(ctx->device));
    SHD_HIP(hipMemcpyAsync(counts, R.counts.p, (size_t)R.n_nodes * R.n_nodes * 8, hipMemcpyDeviceToHost, ctx->stream));
    SHD_HIP(hipStreamSynchronize(ctx->stream));
    return SHD_OK;
}

}  // extern "C"
