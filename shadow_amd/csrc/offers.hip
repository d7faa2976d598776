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
// The device maps runs to hosts (a host with two runs and a host outside the outbound stage's
// range are the two device-side checks), scans the per-host counts into d_off and gathers a wave
// per host.  Pinned stages are read where they lie, once: the run arrays by of_runs_zc (which
// copies them to the device arrays the scans read), the records by the gather.
#include <algorithm>
#include <cstring>
#include <vector>

#include "offer_stage.h"
#include "pin_view.h"
#include "scan.h"

namespace shd {

constexpr int kOffersPinWord = 36;   // h_pin words 36, 37: the two checks

struct OfStage {
    const uint32_t* rh;    // device views of the stage's run_host / run_count / offers
    const uint32_t* rc;
    const uint32_t* rec;
    uint64_t offer_base;   // the stage's first offer in stage order
    uint64_t n_offers;
    uint32_t run_base, n_runs;
};

// per run: its host's run index (+1).  red[0]: a host with a second run (the lowest such host),
// red[1]: a run of a host outside [first_host, first_host + n_hosts) (the lowest such run)
__device__ __forceinline__ void of_map_run(uint32_t r, uint32_t host, uint32_t first_host, uint32_t n_hosts,
                                           uint32_t* __restrict__ hrun, unsigned long long* __restrict__ red) {
    const uint32_t h = host - first_host;   // (a host below first_host wraps past n_hosts)
    if (host < first_host || h >= n_hosts) {
        atomicMin(&red[1], (unsigned long long)r);
        return;
    }
    if (atomicExch(&hrun[h], r + 1) != 0) atomicMin(&red[0], (unsigned long long)h);
}

__global__ __launch_bounds__(256) void of_runs(uint32_t n_runs, const uint32_t* __restrict__ run_host,
                                               uint32_t first_host, uint32_t n_hosts, uint32_t* __restrict__ hrun,
                                               unsigned long long* __restrict__ red) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_runs) return;
    of_map_run(r, run_host[r], first_host, n_hosts, hrun, red);
}

// of_runs on the pinned stages themselves: each run's host and count (read once, copied to the
// device arrays the scans read) and its stage
__global__ __launch_bounds__(256) void of_runs_zc(uint32_t n_runs, const OfStage* __restrict__ st, uint32_t n_stages,
                                                  uint32_t first_host, uint32_t n_hosts, uint32_t* __restrict__ runh,
                                                  uint32_t* __restrict__ runc, uint32_t* __restrict__ rstage,
                                                  uint32_t* __restrict__ hrun, unsigned long long* __restrict__ red) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_runs) return;
    uint32_t lo = 0, hi = n_stages;   // the last stage whose first run is <= r (stages without runs skipped)
    while (hi - lo > 1) {
        const uint32_t m = (lo + hi) >> 1;
        if (st[m].run_base <= r) lo = m; else hi = m;
    }
    while (lo + 1 < n_stages && (st[lo].n_runs == 0 || r - st[lo].run_base >= st[lo].n_runs)) ++lo;
    const uint32_t i = r - st[lo].run_base;   // (< n_runs of the stage: r < the total of the stages' runs)
    const uint32_t host = st[lo].rh[i];
    runh[r] = host;
    runc[r] = st[lo].rc[i];
    rstage[r] = lo;
    of_map_run(r, host, first_host, n_hosts, hrun, red);
}

// per host: its offer count (0 without a run); entry n_hosts is 0 so one scan gives d_off[0..H]
__global__ __launch_bounds__(256) void of_host_counts(uint32_t n_hosts, const uint32_t* __restrict__ hrun,
                                                      const uint32_t* __restrict__ run_count,
                                                      uint32_t* __restrict__ hcnt) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h > n_hosts) return;
    const uint32_t r = h < n_hosts ? hrun[h] : 0u;
    hcnt[h] = r ? run_count[r - 1] : 0u;
}

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

// one wave per host: its run's records, a record per lane, into the grouped columns.  The run
// lies in the uploaded copy (st == nullptr) or in its stage's pinned buffer; a run that would
// leave its stage (the pinned counts changed under the call) is not read: red[0].
template <bool A8>
__global__ __launch_bounds__(256) void of_gather(uint32_t n_hosts, const uint32_t* __restrict__ hrun,
                                                 const uint32_t* __restrict__ run_off,
                                                 const uint32_t* __restrict__ d_off, const uint32_t* __restrict__ rec,
                                                 uint32_t words, uint64_t time_base, uint64_t* __restrict__ d_time,
                                                 uint64_t* __restrict__ d_prio, uint64_t* __restrict__ d_sock,
                                                 uint32_t* __restrict__ d_size, uint32_t* __restrict__ d_pay,
                                                 uint32_t* __restrict__ d_dst, uint32_t* __restrict__ d_pkt,
                                                 const OfStage* __restrict__ st, const uint32_t* __restrict__ rstage,
                                                 unsigned long long* __restrict__ red) {
    const uint32_t h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (h >= n_hosts) return;
    const uint32_t r = hrun[h];
    if (!r) return;
    const uint32_t from = run_off[r - 1], to = d_off[h], cnt = d_off[h + 1] - to;
    const uint32_t* rs = rec + (size_t)from * words;
    if (st) {
        const OfStage& S = st[rstage[r - 1]];
        const uint64_t at = from - S.offer_base;
        if (at + cnt > S.n_offers) {
            if (lane == 0) atomicMin(&red[0], (unsigned long long)h);
            return;
        }
        rs = S.rec + at * words;
    }
    for (uint32_t k = lane; k < cnt; k += 64) {
        uint32_t w[kOfferWordsSock];
        of_load<A8>(rs + (size_t)k * words, words, w);
        const Offer o = offer_decode(w, words, time_base);
        const uint32_t p = to + k;
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
    uint64_t n = 0, n_runs = 0;
    if (!offer_stages_ok(n_stages, stage_runs, run_host, run_count, stage_offers, offers, offer_words, O.with_sockets(),
                         &n_runs, &n))
        return SHD_ERR_INVALID;
    OffersState& F = ctx->offers;
    const uint32_t H = O.n_hosts, words = offer_words;
    const bool sock = words == kOfferWordsSock;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nn = std::max<uint64_t>(n, 1), nr = std::max<uint64_t>(n_runs, 1);
    SHD_TRY(F.runh.ensure(nr * 4));
    SHD_TRY(F.runc.ensure(nr * 4));
    SHD_TRY(F.runo.ensure(nr * 4));
    SHD_TRY(F.hrun.ensure((size_t)(H + 1) * 4));
    SHD_TRY(F.hcnt.ensure((size_t)(H + 1) * 4));
    SHD_TRY(F.red.ensure(16));
    SHD_TRY(F.d_off.ensure((size_t)(H + 1) * 4));
    SHD_TRY(F.d_time.ensure(nn * 8));
    SHD_TRY(F.d_prio.ensure(nn * 8));
    if (sock) SHD_TRY(F.d_sock.ensure(nn * 8));
    SHD_TRY(F.d_size.ensure(nn * 4));
    SHD_TRY(F.d_pay.ensure(nn * 4));
    SHD_TRY(F.d_dst.ensure(nn * 4));
    SHD_TRY(F.d_pkt.ensure(nn * 4));
    // 1. the stages: read where they lie when every array is pinned (zero-copy), else copied stage
    //    after stage (the FLUSH_COPY knob forces the copies, as it does for the flush)
    std::vector<OfStage> tab(n_stages);
    bool zc = n_stages > 0 && !ctx->knobs.on(K_FLUSH_COPY);
    bool a8 = true;   // every record 8-aligned: both widths are multiples of 8 bytes
    {
        uint64_t at = 0;
        uint32_t ar = 0;
        for (uint32_t k = 0; k < n_stages; ++k) {
            OfStage& T = tab[k];
            if (zc) {
                T.rh = static_cast<const uint32_t*>(stage_runs[k] ? dev_view(run_host[k]) : nullptr);
                T.rc = static_cast<const uint32_t*>(stage_runs[k] ? dev_view(run_count[k]) : nullptr);
                T.rec = static_cast<const uint32_t*>(stage_offers[k] ? dev_view(offers[k]) : nullptr);
                if ((stage_runs[k] && (!T.rh || !T.rc)) || (stage_offers[k] && !T.rec)) zc = false;
                if (reinterpret_cast<uintptr_t>(T.rec) & 7u) a8 = false;
            }
            T.offer_base = at;
            T.n_offers = stage_offers[k];
            T.run_base = ar;
            T.n_runs = stage_runs[k];
            at += stage_offers[k];
            ar += stage_runs[k];
        }
    }
    if (zc) {
        SHD_TRY(F.tab.ensure((size_t)n_stages * sizeof(OfStage)));
        SHD_TRY(F.tab_pin.ensure((size_t)n_stages * sizeof(OfStage)));
        SHD_TRY(F.rstg.ensure(nr * 4));
        std::memcpy(F.tab_pin.p, tab.data(), (size_t)n_stages * sizeof(OfStage));
        SHD_HIP(hipMemcpyAsync(F.tab.p, F.tab_pin.p, (size_t)n_stages * sizeof(OfStage), hipMemcpyHostToDevice, s));
    } else {
        a8 = true;   // (the copies lie in the engine's own 256-aligned buffer)
        SHD_TRY(F.rec.ensure(nn * words * 4));
        for (uint32_t k = 0; k < n_stages; ++k) {
            const OfStage& T = tab[k];
            if (T.n_runs) {
                SHD_HIP(hipMemcpyAsync(F.runh.as<uint32_t>() + T.run_base, run_host[k], (size_t)T.n_runs * 4,
                                       hipMemcpyHostToDevice, s));
                SHD_HIP(hipMemcpyAsync(F.runc.as<uint32_t>() + T.run_base, run_count[k], (size_t)T.n_runs * 4,
                                       hipMemcpyHostToDevice, s));
            }
            if (T.n_offers)
                SHD_HIP(hipMemcpyAsync(F.rec.as<uint32_t>() + T.offer_base * words, offers[k], T.n_offers * words * 4,
                                       hipMemcpyHostToDevice, s));
        }
    }
    // 2. runs -> hosts, per-host counts, d_off, the gather
    unsigned long long* red = F.red.as<unsigned long long>();
    SHD_HIP(hipMemsetAsync(F.hrun.p, 0, (size_t)(H + 1) * 4, s));
    SHD_HIP(hipMemsetAsync(red, 0xFF, 16, s));
    if (n_runs) {
        if (zc)
            of_runs_zc<<<div_up(n_runs, 256), 256, 0, s>>>((uint32_t)n_runs, F.tab.as<OfStage>(), n_stages, O.first_host, H,
                                                            F.runh.as<uint32_t>(), F.runc.as<uint32_t>(),
                                                            F.rstg.as<uint32_t>(), F.hrun.as<uint32_t>(), red);
        else
            of_runs<<<div_up(n_runs, 256), 256, 0, s>>>((uint32_t)n_runs, F.runh.as<uint32_t>(), O.first_host, H,
                                                         F.hrun.as<uint32_t>(), red);
        SHD_TRY(scan_excl2(F.scan, F.runc.as<uint32_t>(), F.runo.as<uint32_t>(), nullptr, nullptr, n_runs, s));
    }
    of_host_counts<<<div_up((uint64_t)H + 1, 256), 256, 0, s>>>(H, F.hrun.as<uint32_t>(), F.runc.as<uint32_t>(),
                                                                F.hcnt.as<uint32_t>());
    SHD_TRY(scan_excl2(F.scan, F.hcnt.as<uint32_t>(), F.d_off.as<uint32_t>(), nullptr, nullptr, (uint64_t)H + 1, s));
    if (n && H) {
        auto gather = a8 ? of_gather<true> : of_gather<false>;
        gather<<<div_up(H, 4), 256, 0, s>>>(H, F.hrun.as<uint32_t>(), F.runo.as<uint32_t>(), F.d_off.as<uint32_t>(),
                                            F.rec.as<uint32_t>(), words, time_base, F.d_time.as<uint64_t>(),
                                            F.d_prio.as<uint64_t>(), F.d_sock.as<uint64_t>(), F.d_size.as<uint32_t>(),
                                            F.d_pay.as<uint32_t>(), F.d_dst.as<uint32_t>(), F.d_pkt.as<uint32_t>(),
                                            zc ? F.tab.as<OfStage>() : nullptr, zc ? F.rstg.as<uint32_t>() : nullptr, red);
    }
    SHD_HIP(hipGetLastError());
    SHD_TRY(readback(ctx, s, kOffersPinWord, red, 16));
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
