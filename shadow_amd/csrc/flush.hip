// shd_relay_flush: the drop-in form of the relay round -- the worker threads' staging buffers as
// they stand at the round barrier, grouped by source host on the device, with the CPU-drawn loss
// draws, and compact outputs for the trip back over PCIe.
//
// Reference: Worker::send_packet (src/main/core/worker.rs:328-413) runs on every worker thread;
// each host runs on one thread per round (scheduler/thread_per_core.rs:188-206), so a host's sends
// are ONE contiguous run in ONE thread's buffer, in send order.  The round's sends reach the device
// as those buffers (stage = thread), each a list of runs (host, count) and 12-byte send records:
//   time_off = now - time_base, dst | SHD_SEND_PAYLOAD (payload_size > 0 is all the drop rule reads,
//   worker.rs:370), draw_hi = the source host's next_u64() >> 32 at send time.  gen::<f64>() is
//   (next_u64 >> 11) * 2^-53 and consumes exactly one next_u64, so the CPU stream advances as in
//   the reference; the top 32 bits decide `chance >= reliability` exactly for every reliability
//   1f32 - loss (relay_priv.h draw_drops).
// The device turns the runs into the grouped layout the pipelines take (src_off, one contiguous
// range per host in host order; the grouping is stage_group.h's, shared with shd_offers_group, the
// gather this unit's), runs the round with those draws (the device streams are left
// untouched), and writes back per send a 2-bit status in stage order, and per event a 16-byte
// record {deliver - round_end, src host, event id - the host's first id of the round, send index
// in stage order} grouped by destination in EventQueue order (event.rs:84-155).
#include <algorithm>

#include "pin_view.h"
#include "relay_priv.h"
#include "stage_group.h"

namespace shd {

struct Send12 {
    uint32_t time_off, dst, draw_hi;
};
static_assert(sizeof(Send12) == sizeof(shd_send12), "12-byte staged send");
constexpr uint32_t kSendWords = sizeof(Send12) / 4;

// one wave per host: its run's records (stage_run) into the grouped arrays the pipelines read, the
// permutation both ways (grouped position <-> send index in stage order).  Under a communicator
// every rank groups every host's sends (the permutation covers all of them) but writes the arrays
// of its own hosts [lo, hi) only, from position src_off[lo] on.
__global__ __launch_bounds__(256) void fl_gather(StageRuns g, uint32_t n_hosts, const uint32_t* __restrict__ src_off,
                                                 uint64_t time_base, uint64_t* __restrict__ send_time,
                                                 uint32_t* __restrict__ dst_host, uint32_t* __restrict__ payload,
                                                 uint32_t* __restrict__ draws, uint32_t* __restrict__ perm,
                                                 uint32_t* __restrict__ inv, uint32_t lo, uint32_t hi) {
    const uint32_t h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (h >= n_hosts) return;
    RunRecords run;
    if (!stage_run(g, src_off, h, lane, run)) return;
    const uint32_t from = run.from, to = run.to, cnt = run.cnt;
    const bool own = h >= lo && h < hi;
    const uint32_t base = src_off[lo];
    const Send12* rs = reinterpret_cast<const Send12*>(run.rec);
    for (uint32_t k = lane; k < cnt; k += 64) {
        const uint32_t p = to + k;
        perm[p] = from + k;
        inv[from + k] = p;
        if (!own) continue;
        const Send12 x = rs[k];
        const uint32_t q = p - base;
        send_time[q] = time_base + x.time_off;
        dst_host[q] = x.dst & ~SHD_SEND_PAYLOAD;
        payload[q] = x.dst >> 31;
        draws[q] = x.draw_hi;
    }
}

// a sharded flush: this rank's hosts' offsets from 0 (the batch of the sharded round), and its
// grouped range [src_off[lo], src_off[hi]) in red[2], red[3] for the host
__global__ __launch_bounds__(256) void fl_rebase(const uint32_t* __restrict__ goff, uint32_t lo, uint32_t n_own,
                                                 uint32_t* __restrict__ off, unsigned long long* __restrict__ red) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k <= n_own) off[k] = goff[lo + k] - goff[lo];
    if (k == 0) {
        red[2] = goff[lo];
        red[3] = goff[lo + n_own];
    }
}

// an event record: 16 bytes {deliver - round_end, src, seq_off, send}, or (shd_flush_out.event_bytes
// = 12) 12 bytes without the source host, which the caller's packet (send index) already names
__device__ __forceinline__ void fl_put_event(void* out, bool b12, uint64_t e, uint32_t d, uint32_t s, uint32_t q,
                                             uint32_t send) {
    if (b12) {
        uint32_t* o = static_cast<uint32_t*>(out) + 3 * e;
        o[0] = d;
        o[1] = q;
        o[2] = send;
    } else {
        static_cast<uint4*>(out)[e] = make_uint4(d, s, q, send);
    }
}

// 2-bit statuses in stage order: byte j holds sends 4j .. 4j+3 (send 4j + k in bits 2k, 2k+1);
// sharded: the statuses of grouped positions [base, base + n_own) (this rank's hosts), 0 elsewhere
__global__ __launch_bounds__(256) void fl_status2(uint64_t n, const uint32_t* __restrict__ inv,
                                                  const uint8_t* __restrict__ st, uint8_t* __restrict__ out,
                                                  uint32_t base, uint32_t n_own) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j * 4 >= n) return;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (j * 4 + k < n) {
            const uint32_t p = inv[j * 4 + k] - base;
            if (p < n_own) v |= (uint32_t)(st[p] & 3u) << (2 * k);
        }
    out[j] = (uint8_t)v;
}

// 16-byte event records of a sharded flush: the ids are already relative (RelayState::rel_ids);
// ev_pkt indexes its sender rank's grouped sends, which start at goff[first host of that rank]
__global__ __launch_bounds__(256) void fl_events16x(uint64_t n, uint64_t round_end, const uint64_t* __restrict__ deliver,
                                                    const uint32_t* __restrict__ src, const uint64_t* __restrict__ seq,
                                                    const uint32_t* __restrict__ pkt, const uint32_t* __restrict__ goff,
                                                    uint32_t per, const uint32_t* __restrict__ perm,
                                                    void* __restrict__ out, uint32_t b12) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint32_t s = src[e], first = (s / per) * per;
    fl_put_event(out, b12 != 0, e, (uint32_t)(deliver[e] - round_end), s, (uint32_t)seq[e], perm[goff[first] + pkt[e]]);
}

// event records (already grouped by destination in EventQueue order)
__global__ __launch_bounds__(256) void fl_events16(uint64_t n, uint64_t round_end, const uint64_t* __restrict__ deliver,
                                                   const uint32_t* __restrict__ src, const uint64_t* __restrict__ seq,
                                                   const uint32_t* __restrict__ pkt, const uint64_t* __restrict__ seq_base,
                                                   const uint32_t* __restrict__ perm, void* __restrict__ out, uint32_t b12) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint32_t s = src[e];
    fl_put_event(out, b12 != 0, e, (uint32_t)(deliver[e] - round_end), s, (uint32_t)(seq[e] - seq_base[s]), perm[pkt[e]]);
}

}  // namespace shd

using namespace shd;

extern "C" {

void* shd_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void shd_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

shd_status shd_relay_flush(shd_ctx* ctx, const shd_stage* stages, uint32_t n_stages, uint64_t time_base,
                           const shd_round* round, shd_flush_out* out) {
    if (!ctx || !round || !out || (n_stages && !stages)) return SHD_ERR_INVALID;
    if (out->struct_size != sizeof(shd_flush_out)) return SHD_ERR_INVALID;   // another header's layout
    if (out->event_bytes != 0 && out->event_bytes != 12 && out->event_bytes != 16) return SHD_ERR_INVALID;
    const uint32_t eb = out->event_bytes == 12 ? 12u : 16u;
    RelayState& R = ctx->relay;
    if (!R.ready) return SHD_ERR_STATE;
    if (R.sharded && (!R.x_words.p || !R.xs_pin.p)) return SHD_ERR_STATE;   // set up before the communicator
    // host-side shape checks (each stage's runs cover exactly its records)
    std::vector<StageView> views(n_stages);
    for (uint32_t k = 0; k < n_stages; ++k)
        views[k] = StageView{stages[k].n_runs, stages[k].run_host, stages[k].run_count, stages[k].n_sends, stages[k].sends};
    uint64_t n = 0;
    if (!stages_ok(views.data(), n_stages, nullptr, &n)) return SHD_ERR_INVALID;
    const uint32_t H = R.n_hosts;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nn = std::max<uint64_t>(n, 1);
    SHD_TRY(R.fl_perm.ensure(nn * 4));
    SHD_TRY(R.fl_inv.ensure(nn * 4));
    SHD_TRY(R.fl_st2.ensure(nn / 4 + 1));
    SHD_TRY(R.fl_ev16.ensure(nn * 16));
    SHD_TRY(R.pk_off.ensure((size_t)(H + 1) * 4));
    SHD_TRY(R.pk_time.ensure(nn * 8));
    SHD_TRY(R.pk_dst.ensure(nn * 4));
    SHD_TRY(R.pk_pay.ensure(nn * 4));
    SHD_TRY(R.draws.ensure(nn * 4));
    SHD_TRY(R.st.ensure(nn));
    SHD_TRY(R.ev_off.ensure((size_t)(H + 1) * 4));
    SHD_TRY(R.ev_deliver.ensure(nn * 8));
    SHD_TRY(R.ev_src.ensure(nn * 4));
    SHD_TRY(R.ev_seq.ensure(nn * 8));
    SHD_TRY(R.ev_pkt.ensure(nn * 4));
    SHD_TRY(R.red.ensure(64));
    SHD_TRY(R.fl_goff.ensure((size_t)(H + 1) * 4));
    // under a communicator: this rank's hosts [lo, hi) (the stages hold every rank's hosts)
    uint32_t lo = 0, hi = H;
    if (R.sharded) shard_range(H, ctx->comm->size, ctx->comm->rank, &lo, &hi);
    // 1. the grouping over every host (stage_group.h; the FLUSH_COPY knob forces the copies)
    uint32_t* goff = R.sharded ? R.fl_goff.as<uint32_t>() : R.pk_off.as<uint32_t>();   // grouped offsets, all hosts
    StageRuns g;
    SHD_TRY(stage_group(R.fl_grp, views.data(), n_stages, kSendWords, 0, H, ctx->knobs.on(K_FLUSH_COPY), R.fl_send, goff,
                        s, &g));
    // 2. the gather
    if (n)
        fl_gather<<<div_up(H, 4), 256, 0, s>>>(g, H, goff, time_base, R.pk_time.as<uint64_t>(), R.pk_dst.as<uint32_t>(),
                                                R.pk_pay.as<uint32_t>(), R.draws.as<uint32_t>(),
                                                R.fl_perm.as<uint32_t>(), R.fl_inv.as<uint32_t>(), lo, hi);
    if (R.sharded)
        fl_rebase<<<div_up((uint64_t)(hi - lo) + 1, 256), 256, 0, s>>>(goff, lo, hi - lo, R.pk_off.as<uint32_t>(), g.red);
    SHD_HIP(hipGetLastError());
    // h_pin words 32-35: the checks (and, sharded, this rank's grouped range).  Under a communicator a
    // failed check is this rank's alone: the flush returns before the round's collectives, as a call
    // with invalid arguments would, on whichever ranks see the bad runs (every rank sees the same
    // stages, so all of them do).
    SHD_TRY(readback(ctx, s, 32, g.red, R.sharded ? 32 : 16));
    if (ctx->h_pin[33] != ~0ull) return SHD_ERR_NO_HOST;   // a run of a host the relay does not have
    if (ctx->h_pin[32] != ~0ull) return SHD_ERR_INVALID;   // a host with two runs (two threads, or split)
    const uint64_t base = R.sharded ? ctx->h_pin[34] : 0, n_own = R.sharded ? ctx->h_pin[35] - ctx->h_pin[34] : n;
    // 3. the round on the grouped batch with the CPU's draws (the device streams stay as they are)
    shd_batch db{n_own, R.pk_off.as<uint32_t>(), R.pk_time.as<uint64_t>(), R.pk_dst.as<uint32_t>(),
                 R.pk_pay.as<uint32_t>(), nullptr};
    shd_relay_out dout{};
    dout.status = R.st.as<uint8_t>();
    dout.ev_off = R.ev_off.as<uint32_t>();
    dout.ev_deliver = R.ev_deliver.as<uint64_t>();
    dout.ev_src = R.ev_src.as<uint32_t>();
    dout.ev_seq = R.ev_seq.as<uint64_t>();
    dout.ev_pkt = R.ev_pkt.as<uint32_t>();
    // zero-copy outputs: the events and the 2-bit statuses written by the kernels straight into the
    // caller's pinned buffers, so no copy follows the round (the writes cross the link as they go)
    const bool zo = !ctx->knobs.on(K_FLUSH_COPY);
    void* ev_host = zo && out->events ? const_cast<void*>(dev_view(out->events)) : nullptr;
    uint8_t* st2_host = zo && out->status2 ? static_cast<uint8_t*>(const_cast<void*>(dev_view(out->status2))) : nullptr;
    void* ev_dst = ev_host ? ev_host : R.fl_ev16.p;
    uint8_t* st2_dst = st2_host ? st2_host : R.fl_st2.as<uint8_t>();
    R.cpu_draws = true;
    R.rel_ids = true;   // records carry ids relative to the source's first of the round
    R.fl_ev_out = R.sharded ? nullptr : ev_dst;
    R.fl_b12 = eb == 12 ? 1u : 0u;
    R.fl_direct = false;
    const shd_status st = R.sharded ? relay_flush_round_sharded(ctx, &db, round, &dout)
                                    : relay_flush_round(ctx, &db, round, &dout);
    R.cpu_draws = false;
    R.rel_ids = false;
    R.fl_ev_out = nullptr;
    const bool direct = R.fl_direct && R.last_pipe == 7;   // (a rerun on pipeline 3 / 1 wrote the arrays)
    R.fl_direct = false;
    SHD_TRY(st);
    // 4. compact outputs (the round committed: next_id2 holds every own host's first id of the round)
    const uint64_t ns = dout.n_sent, n_ev = R.sharded ? dout.n_events : ns;
    const uint64_t* seq_base = R.next_id2.as<uint64_t>();
    if (n) fl_status2<<<div_up((n + 3) / 4, 256), 256, 0, s>>>(n, R.fl_inv.as<uint32_t>(), R.st.as<uint8_t>(),
                                                              st2_dst, (uint32_t)base, (uint32_t)n_own);
    if (n_ev && R.sharded)
        fl_events16x<<<div_up(n_ev, 256), 256, 0, s>>>(n_ev, round->round_end, dout.ev_deliver, dout.ev_src,
                                                       dout.ev_seq, dout.ev_pkt, goff,
                                                       (uint32_t)div_up((uint64_t)H, (uint64_t)ctx->comm->size),
                                                       R.fl_perm.as<uint32_t>(), ev_dst, eb == 12 ? 1u : 0u);
    else if (n_ev && !direct)
        fl_events16<<<div_up(ns, 256), 256, 0, s>>>(ns, round->round_end, R.ev_deliver.as<uint64_t>(),
                                                    R.ev_src.as<uint32_t>(), R.ev_seq.as<uint64_t>(),
                                                    R.ev_pkt.as<uint32_t>(), seq_base, R.fl_perm.as<uint32_t>(),
                                                    ev_dst, eb == 12 ? 1u : 0u);
    SHD_HIP(hipGetLastError());
    if (out->status2 && n && !st2_host)
        SHD_HIP(hipMemcpyAsync(out->status2, R.fl_st2.p, (n + 3) / 4, hipMemcpyDeviceToHost, s));
    if (out->ev_off)
        SHD_HIP(hipMemcpyAsync(out->ev_off, dout.ev_off, (size_t)(hi - lo + 1) * 4, hipMemcpyDeviceToHost, s));
    if (out->events && n_ev && !ev_host)
        SHD_HIP(hipMemcpyAsync(out->events, R.fl_ev16.p, n_ev * eb, hipMemcpyDeviceToHost, s));
    if (out->seq_base && hi > lo)
        SHD_HIP(hipMemcpyAsync(out->seq_base + lo, seq_base + lo, (size_t)(hi - lo) * 8, hipMemcpyDeviceToHost, s));
    SHD_TRY(wait_stream(ctx, s));
    out->min_deliver = dout.min_deliver;
    out->min_latency = dout.min_latency;
    out->n_sent = ns;
    out->n_events = n_ev;
    return SHD_OK;
}

}  // extern "C"
