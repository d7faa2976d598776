// shd_offers_group: the front door of the window's close -- the worker threads' staged offers as
// they stand at the round barrier, grouped by host on the device into the columns the outbound
// stage takes (d_off and seven columns), so that the caller neither groups ~10M offers on the CPU
// nor splits them into seven arrays with a copy each.
//
// Reference: a socket with packets to send reaches notify_socket_has_packets -> Relay::notify
// (relay/mod.rs:110-135) on the worker thread that runs its host; each host runs on one thread per
// round (scheduler/thread_per_core.rs:188-206), so a host's offers are ONE contiguous run in ONE
// thread's buffer, in the order the host made them -- time order, the outbound stage's contract.
// The stage (= thread) contract is shd_relay_flush's (flush.hip); the record is offer_stage.h's.
// stage_group (stage_group.h) maps the runs to hosts over the outbound stage's range and scans the
// per-host counts into d_off; the gather here moves a wave per host.
#include <algorithm>

#include "offer_stage.h"
#include "stage_group.h"

namespace shd {

constexpr int kOffersPinWord = 36;   // h_pin words 36, 37: the two checks

// one record into registers: 8-byte loads where every record is 8-aligned (A8), else word by word
template <bool A8>
__device__ __forceinline__ void of_load(const uint32_t* __restrict__ p, uint32_t words, uint32_t (&w)[kOfferWordsSock]) {
    if (A8) {
        const uint2* q = reinterpret_cast<const uint2*>(p);
#pragma unroll
        for (uint32_t i = 0; i < kOfferWords / 2; ++i) {
            const uint2 v = q[i];
            w[2 * i] = v.x;
            w[2 * i + 1] = v.y;
        }
        const uint2 v = words == kOfferWordsSock ? q[kOfferWords / 2] : make_uint2(0, 0);
        w[kOfferSock] = v.x;
        w[kOfferSock + 1] = v.y;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kOfferWords; ++i) w[i] = p[i];
        w[kOfferSock] = words == kOfferWordsSock ? p[kOfferSock] : 0u;
        w[kOfferSock + 1] = words == kOfferWordsSock ? p[kOfferSock + 1] : 0u;
    }
}

// one wave per host: its run's records (stage_run), a record per lane, into the grouped columns
template <bool A8>
__global__ __launch_bounds__(256) void of_gather(StageRuns g, uint32_t n_hosts, const uint32_t* __restrict__ d_off,
                                                 uint64_t time_base, uint64_t* __restrict__ d_time,
                                                 uint64_t* __restrict__ d_prio, uint64_t* __restrict__ d_sock,
                                                 uint32_t* __restrict__ d_size, uint32_t* __restrict__ d_pay,
                                                 uint32_t* __restrict__ d_dst, uint32_t* __restrict__ d_pkt) {
    const uint32_t h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, words = g.rec_words;
    if (h >= n_hosts) return;
    RunRecords run;
    if (!stage_run(g, d_off, h, lane, run)) return;
    for (uint32_t k = lane; k < run.cnt; k += 64) {
        uint32_t w[kOfferWordsSock];
        of_load<A8>(run.rec + (size_t)k * words, words, w);
        const Offer o = offer_decode(w, words, time_base);
        const uint32_t p = run.to + k;
        d_time[p] = o.time;
        d_prio[p] = o.prio;
        if (words == kOfferWordsSock) d_sock[p] = o.sock;
        d_size[p] = o.size;
        d_pay[p] = o.payload;
        d_dst[p] = o.dst;
        d_pkt[p] = o.pkt;
    }
}

}  // namespace shd

using namespace shd;

extern "C" {

shd_status shd_offers_group(shd_ctx* ctx, uint32_t n_stages, const uint32_t* stage_runs, const uint32_t** run_host,
                            const uint32_t** run_count, const uint64_t* stage_offers, const uint32_t** offers,
                            uint32_t offer_words, uint64_t time_base, const uint32_t** d_off, const uint64_t** d_time,
                            const uint64_t** d_prio, const uint64_t** d_sock, const uint32_t** d_size,
                            const uint32_t** d_payload, const uint32_t** d_dst, const uint32_t** d_pkt,
                            uint64_t* n_offers) {
    if (!ctx) return SHD_ERR_INVALID;
    const OutboundState& O = ctx->outb;
    if (!O.ready) return SHD_ERR_STATE;
    uint64_t n = 0;
    if (!offer_stages_ok(n_stages, stage_runs, run_host, run_count, stage_offers, offers, offer_words, O.with_sockets(),
                         nullptr, &n))
        return SHD_ERR_INVALID;
    OffersState& F = ctx->offers;
    const uint32_t H = O.n_hosts;
    const bool sock = offer_words == kOfferWordsSock;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nn = std::max<uint64_t>(n, 1);
    SHD_TRY(F.d_off.ensure((size_t)(H + 1) * 4));
    SHD_TRY(F.d_time.ensure(nn * 8));
    SHD_TRY(F.d_prio.ensure(nn * 8));
    if (sock) SHD_TRY(F.d_sock.ensure(nn * 8));
    SHD_TRY(F.d_size.ensure(nn * 4));
    SHD_TRY(F.d_pay.ensure(nn * 4));
    SHD_TRY(F.d_dst.ensure(nn * 4));
    SHD_TRY(F.d_pkt.ensure(nn * 4));
    // 1. the grouping (the FLUSH_COPY knob forces the copies, as it does for the flush)
    const std::vector<StageView> views = offer_stage_views(n_stages, stage_runs, run_host, run_count, stage_offers, offers);
    StageRuns g;
    SHD_TRY(stage_group(F.grp, views.data(), n_stages, offer_words, O.first_host, H, ctx->knobs.on(K_FLUSH_COPY), F.rec,
                        F.d_off.as<uint32_t>(), s, &g));
    // 2. the gather: 8-byte loads where every record is 8-aligned (both widths are multiples of 8
    //    bytes; the copies lie in the engine's own 256-aligned buffer)
    bool a8 = true;
    for (uint32_t k = 0; g.tab && k < n_stages; ++k)
        if (reinterpret_cast<uintptr_t>(F.grp.tab_pin.as<StageTab>()[k].rec) & 7u) a8 = false;
    if (n && H) {
        auto gather = a8 ? of_gather<true> : of_gather<false>;
        gather<<<div_up(H, 4), 256, 0, s>>>(g, H, F.d_off.as<uint32_t>(), time_base, F.d_time.as<uint64_t>(),
                                            F.d_prio.as<uint64_t>(), F.d_sock.as<uint64_t>(), F.d_size.as<uint32_t>(),
                                            F.d_pay.as<uint32_t>(), F.d_dst.as<uint32_t>(), F.d_pkt.as<uint32_t>());
    }
    SHD_HIP(hipGetLastError());
    SHD_TRY(readback(ctx, s, kOffersPinWord, g.red, 16));
    if (ctx->h_pin[kOffersPinWord + 1] != ~0ull) return SHD_ERR_NO_HOST;   // a run of a host the stage does not have
    if (ctx->h_pin[kOffersPinWord] != ~0ull) return SHD_ERR_INVALID;       // a host with two runs (two threads, or split)
    if (d_off) *d_off = F.d_off.as<uint32_t>();
    if (d_time) *d_time = F.d_time.as<uint64_t>();
    if (d_prio) *d_prio = F.d_prio.as<uint64_t>();
    if (d_sock) *d_sock = sock ? F.d_sock.as<uint64_t>() : nullptr;
    if (d_size) *d_size = F.d_size.as<uint32_t>();
    if (d_payload) *d_payload = F.d_pay.as<uint32_t>();
    if (d_dst) *d_dst = F.d_dst.as<uint32_t>();
    if (d_pkt) *d_pkt = F.d_pkt.as<uint32_t>();
    if (n_offers) *n_offers = n;
    return SHD_OK;
}

}  // extern "C"
