// CoDel inbound router queues on the GPU: one queue per destination host,
// device-resident across calls; a call replays every host's push/pop operations of a batch in
// order, lane per host.
//
// Reference semantics: src/main/network/router/codel_queue.rs (FlyearthR/shadow), restated line
// by line in codel_lane.h (CodelLane: push, pop and the two drop paths), which the inbound stage
// (inbound.hip) compiles too.
// The host's packets in the queue live in a per-host ring of `capacity` entries; a push beyond it
// is reported (SHD_ERR_INVALID) instead of growing, the one deviation from the unbounded VecDeque.
// The per-host work is a short sequential state machine, so the lane-per-host kernel is
// latency-bound by design; it keeps the queues resident next to the relay output they consume.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "codel_lane.h"
#include "ctx.h"

namespace shd {

constexpr uint32_t kOpBatch = 16;   // ops per lane loaded ahead of the state machine

struct CodelFate {   // CodelLane's sink: fate[id] = (op << 2) | kind; an id >= n_ids is reported
    uint64_t* fate;
    uint32_t n_ids;
    uint32_t* status;
    __device__ void mark(uint32_t pkt, uint32_t op, uint32_t kind) {
        if (pkt < n_ids) fate[pkt] = ((uint64_t)op << 2) | kind;
        else atomicOr(status, 2u);
    }
};

__global__ __launch_bounds__(256) void codel_run(uint32_t n_hosts, const uint32_t* __restrict__ off,
                                                 const uint64_t* __restrict__ time,
                                                 const uint32_t* __restrict__ size,
                                                 const uint32_t* __restrict__ pkt, CodelHost* st,
                                                 uint32_t* flags_arr, uint4* ring, uint32_t cap,
                                                 uint32_t* __restrict__ pop_out,
                                                 uint64_t* __restrict__ fate, uint32_t n_ids,
                                                 uint32_t* status) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h >= n_hosts) return;
    CodelLane<CodelFate> L;
    L.s = st[h];
    L.flags = flags_arr[h];
    L.ring = ring + (size_t)h * cap;
    L.cap = cap;
    L.sink = CodelFate{fate, n_ids, status};
    // The host's ops are read kOpBatch at a time into registers (loads clamped into the range,
    // all issued before the state machine runs), so a lane waits for one memory latency per
    // batch instead of one per op, and its consecutive 8-byte times share cache lines.
    const uint32_t kb = off[h], ke = off[h + 1];
    for (uint32_t k0 = kb; k0 < ke; k0 += kOpBatch) {
        uint64_t tm[kOpBatch];
        uint32_t sz[kOpBatch], pk[kOpBatch];
#pragma unroll
        for (uint32_t i = 0; i < kOpBatch; ++i) {
            const uint32_t k = min(k0 + i, ke - 1);
            tm[i] = time[k];
            sz[i] = size[k];
            pk[i] = pkt[k];
        }
#pragma unroll
        for (uint32_t i = 0; i < kOpBatch; ++i) {
            const uint32_t k = k0 + i;
            if (k >= ke) break;
            const uint64_t now = tm[i];
            if (sz[i] == kPop) {
                uint32_t got_size;
                const uint32_t got = L.pop(now, k, &got_size);
                pop_out[k] = got;
                if (got != kPop) L.sink.mark(got, k, 1);
            } else {
                pop_out[k] = kPop;
                // the reference's queue never fills (LIMIT = usize::MAX)
                if (!L.push(pk[i], sz[i], now)) atomicOr(status, 1u);
            }
        }
    }
    st[h] = L.s;
    flags_arr[h] = L.flags & ~kCodelPanic;
    if (L.flags & kCodelPanic) atomicOr(status, 4u);   // where the reference panics (the control law)
}

}  // namespace shd

using namespace shd;

extern "C" {

shd_status shd_codel_setup(shd_ctx* ctx, uint32_t n_hosts, uint32_t capacity) {
    if (!ctx || capacity == 0) return SHD_ERR_INVALID;
    CodelState& C = ctx->codel;
    SHD_HIP(hipSetDevice(ctx->device));
    SHD_TRY(C.st.ensure(std::max<size_t>(n_hosts, 1) * sizeof(CodelHost)));
    SHD_TRY(C.flags.ensure(std::max<size_t>(n_hosts, 1) * 4));
    SHD_TRY(C.ring.ensure(std::max<size_t>((size_t)n_hosts * capacity, 1) * 16));
    SHD_TRY(C.status.ensure(16));
    SHD_HIP(hipMemsetAsync(C.st.p, 0, (size_t)n_hosts * sizeof(CodelHost), ctx->stream));
    SHD_HIP(hipMemsetAsync(C.flags.p, 0, (size_t)n_hosts * 4, ctx->stream));
    SHD_HIP(hipStreamSynchronize(ctx->stream));
    C.n_hosts = n_hosts;
    C.cap = capacity;
    C.ready = true;
    return SHD_OK;
}

shd_status shd_codel_run_device(shd_ctx* ctx, const shd_codel_ops* ops, uint32_t* pop_out,
                                uint64_t* fate, uint32_t n_ids) {
    if (!ctx || !ops) return SHD_ERR_INVALID;
    CodelState& C = ctx->codel;
    if (!C.ready) return SHD_ERR_STATE;
    hipStream_t s = ctx->stream;
    SHD_HIP(hipSetDevice(ctx->device));
    SHD_HIP(hipMemsetAsync(C.status.p, 0, 4, s));
    if (C.n_hosts)
        codel_run<<<div_up(C.n_hosts, 256), 256, 0, s>>>(
            C.n_hosts, ops->host_off, ops->time, ops->size, ops->pkt, C.st.as<CodelHost>(),
            C.flags.as<uint32_t>(), C.ring.as<uint4>(), C.cap, pop_out, fate, n_ids,
            C.status.as<uint32_t>());
    SHD_HIP(hipGetLastError());
    SHD_HIP(hipMemcpyAsync(ctx->h_pin + 24, C.status.p, 4, hipMemcpyDeviceToHost, s));
    SHD_HIP(hipStreamSynchronize(s));
    const uint32_t st = (uint32_t)ctx->h_pin[24];
    if (st) {
        // the batch ran with the offending pushes / marks skipped, or past a point where the
        // reference panics: the queues now hold a state the reference never reaches (and a ring slot freed by a pop may have been reused), so
        // they cannot be rolled back -- shd_codel_setup must run again before the next batch
        C.ready = false;
        return SHD_ERR_INVALID;
    }
    return SHD_OK;
}

shd_status shd_codel_get_state(shd_ctx* ctx, uint32_t host, shd_codel_state* out) {
    if (!ctx || !out) return SHD_ERR_INVALID;
    CodelState& C = ctx->codel;
    if (!C.ready || host >= C.n_hosts) return SHD_ERR_INVALID;
    CodelHost hs;
    uint32_t fl = 0;
    SHD_HIP(hipMemcpy(&hs, C.st.as<CodelHost>() + host, sizeof(hs), hipMemcpyDeviceToHost));
    SHD_HIP(hipMemcpy(&fl, C.flags.as<uint32_t>() + host, 4, hipMemcpyDeviceToHost));
    out->len = hs.count;
    out->mode = (fl & kModeDrop) ? 1 : 0;
    out->has_interval_end = (fl & kHasIntervalEnd) ? 1 : 0;
    out->has_drop_next = (fl & kHasDropNext) ? 1 : 0;
    out->interval_end = hs.interval_end;
    out->drop_next = hs.drop_next;
    out->current_drop_count = hs.cur;
    out->previous_drop_count = hs.prev;
    out->total_bytes_stored = hs.total;
    return SHD_OK;
}

}  // extern "C"
