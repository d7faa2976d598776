// Bandwidth changes on the running stages: re-rate the token buckets of named hosts between two
// windows, with everything else a stage holds -- queues, CoDel state, the cached packet, the
// outstanding forward task, the socket arrays -- left as it is.  One unit for the three places a
// TbRelay per host lives: the replay engine (tbucket.hip), the inbound stage (inbound.hip) and the
// outbound stage under each of its four disciplines (outbound.hip).
//
// The reference builds a relay's bucket once (relay/mod.rs:277-302) and has no counterpart; the
// operation is put together from its own pieces (token_bucket.rs:37-60 new_inner, :127-157
// lazy_refill): rate_update.h states it, tb_rerate (tbucket_ops.h) is the arithmetic.
//
// A call is two launches and one read-back of two words (status bits, the lowest failing host):
//   rate_check   a lane per record (one record per named host after the last-entry-wins pass).  It
//                re-rates a copy of the host's bucket for the time rules, reads the host's relay
//                words for the task rule, and walks the host's stored packets for the largest
//                non-local size -- only where the capacity shrinks (or there was no bucket): every
//                stored packet is at most the present capacity, checked when it was taken in.  A
//                host that stores at most the packet in its relay words never touches its ring.
//   rate_apply   a lane per record; leaves at once where the check set a status bit, so a refused
//                call changes no host.  No two lanes share a host.
// Why a re-rate may be refused on the device: `at` before the bucket's last refill (duration_since
// would panic), a refill that panics in the reference, an outstanding forward task before `at`
// (it would later run before the new bucket's last_refill), or a new capacity below a stored
// packet's size -- the stages' loops end because a blocked packet's task always forwards it, and
// a re-rate keeps that true.  A packet whose destination is the host itself never meets the
// outbound bucket and is exempt.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "codel_lane.h"
#include "ctx.h"
#include "inbound_relay.h"
#include "outbound_queue.h"
#include "tbucket_ops.h"

namespace shd {

constexpr int kRatePinWord = 88;   // ctx->h_pin words [88, 94)
static_assert(kRatePinWord > kPinMarker && kRatePinWord + 2 * kRateTargets <= kPinWords,
              "the re-rate's words above the polled marker");
// status bits (word 0 of a target); any of them is SHD_ERR_INVALID
constexpr uint32_t kRateBefore = 1u;   // `at` before the bucket's last refill
constexpr uint32_t kRatePanic = 2u;    // where the reference panics in the refill (token_bucket.rs unwraps)
constexpr uint32_t kRateTask = 4u;     // the outstanding forward task is earlier than `at`
constexpr uint32_t kRateSize = 8u;     // the new capacity is below a stored packet's size
constexpr uint64_t kRateIdle = ~0ull;

// What rate_check reads of a host beside its bucket: look(h, walk, task, largest) gives the
// outstanding task's time (kRateIdle: none) and, where `walk`, the largest size among the stored
// packets that meet the bucket.

struct RateTbView {   // the replay engine: no stored packets; a Pending relay stays Pending
    __device__ __forceinline__ void look(uint32_t, bool, uint64_t& task, uint32_t& largest) const {
        task = kRateIdle;
        largest = 0;
    }
};

struct RateInView {   // the inbound stage: the CoDel ring and the cached packet; nothing is local
    const CodelHost* st;
    const uint4* ring;
    const InRelay* rl;
    uint32_t cap;
    __device__ __forceinline__ void look(uint32_t h, bool walk, uint64_t& task, uint32_t& largest) const {
        const InRelay R = rl[h];
        task = R.task;
        largest = 0;
        if (!walk) return;
        if (R.has_cached) largest = R.cached_size;
        const CodelHost s = st[h];
        if (s.count == 0 || s.head >= cap) return;
        codel_visit(s, ring + (size_t)h * cap, cap, [&](uint32_t size) { largest = size > largest ? size : largest; });
    }
};

template <class Q>
struct RateOutView {   // the outbound stage under discipline Q: its queue and the cached packet
    typename Q::Args qa;
    const OutRelay* rl;
    uint32_t first_host;
    __device__ __forceinline__ void look(uint32_t h, bool walk, uint64_t& task, uint32_t& largest) const {
        const OutRelay R = rl[h];
        task = R.task;
        largest = 0;
        if (!walk) return;
        const uint32_t self = first_host + h;   // a packet to the host itself is local: relay/mod.rs:222-230
        auto see = [&](uint32_t size, uint32_t dst) {
            if (dst != self && size > largest) largest = size;
        };
        if (R.has_cached) see(R.cached_size, R.cached_dst);
        Q::visit(qa, h, R, see);
    }
};

template <class View>
__global__ __launch_bounds__(256) void rate_check(uint32_t n, const RateRec* __restrict__ rec,
                                                  const TbRelay* __restrict__ tb, const View view, uint64_t at,
                                                  unsigned long long* words) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const RateRec r = rec[i];
    TbRelay B = tb[r.host];   // a copy: nothing is written here
    const uint64_t old_cap = B.capacity;
    uint32_t err = 0;
    if (old_cap && at < B.last_refill) err |= kRateBefore;
    bool bad = false;
    tb_rerate(B, at, r.capacity, r.increment, r.interval, bad);
    if (bad) err |= kRatePanic;
    // stored packets are at most the present capacity (checked as they were taken in): only a
    // smaller capacity, or the first one of a host that had none, can be below one of them
    const bool walk = r.capacity && (old_cap == 0 || r.capacity < old_cap);
    uint64_t task;
    uint32_t largest;
    view.look(r.host, walk, task, largest);
    if (task != kRateIdle && task < at) err |= kRateTask;
    if (walk && largest > r.capacity) err |= kRateSize;
    if (err) {
        atomicOr(words, (unsigned long long)err);
        atomicMin(words + 1, (unsigned long long)r.host);
    }
}

__global__ __launch_bounds__(256) void rate_apply(uint32_t n, const RateRec* __restrict__ rec, TbRelay* tb,
                                                  uint64_t at, const unsigned long long* __restrict__ words) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || words[0] != 0) return;   // a refused call changes no host
    const RateRec r = rec[i];
    TbRelay B = tb[r.host];
    bool bad = false;   // (the check ran the same arithmetic and found it clean)
    tb_rerate(B, at, r.capacity, r.increment, r.interval, bad);
    tb[r.host] = B;
}

struct RateInfo {   // a target as the re-rate sees it
    bool ready;
    uint32_t n_hosts;
    uint64_t prev_end;
    TbRelay* tb;
};

static RateInfo rate_info(shd_ctx* ctx, RateTarget t) {
    switch (t) {
    case kRateTb: return RateInfo{ctx->tb.ready, ctx->tb.n_relays, 0, ctx->tb.st.as<TbRelay>()};
    case kRateInbound: return RateInfo{ctx->inb.ready, ctx->inb.n_hosts, ctx->inb.prev_end, ctx->inb.tb.as<TbRelay>()};
    default: return RateInfo{ctx->outb.ready, ctx->outb.n_hosts, ctx->outb.prev_end, ctx->outb.tb.as<TbRelay>()};
    }
}

shd_status rate_stage_check(shd_ctx* ctx, RateTarget t, uint64_t n, const uint32_t* host, const uint64_t* capacity,
                      const uint64_t* increment, const uint64_t* interval, uint64_t at) {
    RateState& S = ctx->rate;
    S.n_rec[t] = 0;
    const RateInfo T = rate_info(ctx, t);
    if (!T.ready) return SHD_ERR_STATE;   // not set up, or a contract error since: as the advance
    if (!rate_updates_valid(n, T.n_hosts, host, capacity, increment, interval, at, T.prev_end)) return SHD_ERR_INVALID;
    if (n == 0) return SHD_OK;
    // (the records stay in the context until the next call: the upload reads them)
    S.host_rec[t] = rate_updates_records(S.stamps[t], T.n_hosts, n, host, capacity, increment, interval);
    const uint32_t m = (uint32_t)S.host_rec[t].size();   // <= n_hosts
    hipStream_t s = ctx->stream;
    SHD_HIP(hipSetDevice(ctx->device));
    SHD_TRY(S.rec[t].ensure((size_t)m * sizeof(RateRec)));
    if (!S.words.p) {
        SHD_TRY(S.words.ensure(2 * kRateTargets * 8));
        SHD_HIP(hipMemsetAsync(S.words.p, 0, 2 * kRateTargets * 8, s));
    }
    unsigned long long* words = S.words.as<unsigned long long>() + 2 * t;
    SHD_HIP(hipMemsetAsync(words, 0, 8, s));
    SHD_HIP(hipMemsetAsync(words + 1, 0xFF, 8, s));
    SHD_HIP(hipMemcpyAsync(S.rec[t].p, S.host_rec[t].data(), (size_t)m * sizeof(RateRec), hipMemcpyHostToDevice, s));
    const RateRec* rec = S.rec[t].as<RateRec>();
    const dim3 grid(div_up(m, 256)), block(256);
    if (t == kRateTb) {
        rate_check<<<grid, block, 0, s>>>(m, rec, T.tb, RateTbView{}, at, words);
    } else if (t == kRateInbound) {
        const InboundState& I = ctx->inb;
        rate_check<<<grid, block, 0, s>>>(m, rec, T.tb, RateInView{I.st.as<CodelHost>(), I.ring.as<uint4>(),
                                                                    I.rl.as<InRelay>(), I.cap}, at, words);
    } else {
        const OutboundState& O = ctx->outb;
        const OutRelay* rl = O.rl.as<OutRelay>();
        if (O.qdisc == SHD_QDISC_FIFO_SOCKETS)
            rate_check<<<grid, block, 0, s>>>(
                m, rec, T.tb, RateOutView<OutFifoSock>{{O.ring.as<SqSlot>(), O.socks.as<SqSock>(), nullptr, O.cap,
                                                        O.max_sockets}, rl, O.first_host}, at, words);
        else if (O.qdisc == SHD_QDISC_ROUND_ROBIN_SOCKETS)
            rate_check<<<grid, block, 0, s>>>(
                m, rec, T.tb, RateOutView<OutRrSock>{{O.ring.as<SqSlot>(), O.socks.as<SqSock>(), nullptr, O.cap,
                                                      O.max_sockets}, rl, O.first_host}, at, words);
        else if (O.qdisc == SHD_QDISC_ROUND_ROBIN)
            rate_check<<<grid, block, 0, s>>>(
                m, rec, T.tb, RateOutView<OutRr>{{O.ring.as<RrSlot>(), O.socks.as<RrSock>(), O.rr_words.as<uint2>(),
                                                  O.cap, O.max_sockets}, rl, O.first_host}, at, words);
        else
            rate_check<<<grid, block, 0, s>>>(m, rec, T.tb, RateOutView<OutFifo>{{O.ring.as<OutPkt>(), O.cap}, rl,
                                                                                 O.first_host}, at, words);
    }
    SHD_HIP(hipGetLastError());
    S.n_rec[t] = m;
    return SHD_OK;
}

shd_status rate_stage_apply(shd_ctx* ctx, RateTarget t, uint64_t at) {
    RateState& S = ctx->rate;
    const uint32_t m = S.n_rec[t];
    if (m == 0) return SHD_OK;
    SHD_HIP(hipSetDevice(ctx->device));
    rate_apply<<<div_up(m, 256), 256, 0, ctx->stream>>>(m, S.rec[t].as<RateRec>(), rate_info(ctx, t).tb, at,
                                                        S.words.as<unsigned long long>() + 2 * t);
    SHD_HIP(hipGetLastError());
    return SHD_OK;
}

shd_status rate_stage_result(shd_ctx* ctx, uint32_t mask, uint32_t* err_host) {
    RateState& S = ctx->rate;
    bool any = false;
    for (int t = 0; t < kRateTargets; ++t) any |= (mask >> t & 1u) && S.n_rec[t];
    if (!any) return SHD_OK;   // an empty call: nothing was launched
    SHD_HIP(hipSetDevice(ctx->device));
    SHD_TRY(readback(ctx, ctx->stream, kRatePinWord, S.words.p, 2 * kRateTargets * 8));
    for (int t = 0; t < kRateTargets; ++t) {
        if (!(mask >> t & 1u) || S.n_rec[t] == 0) continue;
        const unsigned long long* w = ctx->h_pin + kRatePinWord + 2 * t;
        if ((uint32_t)w[0]) {
            if (err_host) *err_host = (uint32_t)w[1];
            return SHD_ERR_INVALID;
        }
    }
    return SHD_OK;
}

shd_status rate_update(shd_ctx* ctx, RateTarget t, uint64_t n, const uint32_t* host, const uint64_t* capacity,
                       const uint64_t* increment, const uint64_t* interval, uint64_t at, uint32_t* err_host) {
    if (!ctx) return SHD_ERR_INVALID;
    SHD_TRY(rate_stage_check(ctx, t, n, host, capacity, increment, interval, at));
    SHD_TRY(rate_stage_apply(ctx, t, at));
    const shd_status st = rate_stage_result(ctx, 1u << t, err_host);
    ctx->rate.n_rec[t] = 0;
    return st;
}

}  // namespace shd
