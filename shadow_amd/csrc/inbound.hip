// The inbound stage on the GPU: per destination host a CoDel router queue, the inbound relay's
// token bucket and the relay's own state, device-resident across calls.  One call advances every
// host over one scheduling window, lane per host, straight from the popped packet events the
// event queues (equeue.hip) leave on the device: send_packet -> event queues -> router -> relay
// -> "packet reaches the interface at time t" without a CPU round trip per blocked packet.
//
// Reference semantics (FlyearthR/shadow):
//   src/main/host/host.rs
//     :742-746 Host::execute's packet branch: Router::route_incoming_packet, i.e. CoDelQueue::push
//              at the event's time, then Relay::notify
//     :281-292 the router's address is UNSPECIFIED: an inbound packet is never "local"
//     :634-640 push_local_event discards tasks at or after the simulation end (no window ends
//              after it, so "a task at T >= window_end stays outstanding" covers it)
//   src/main/core/work/event.rs
//     :102-110 at equal time a Packet event orders before a Local one (the forward task)
//   src/main/network/relay/mod.rs
//     :110-135 notify: Idle -> forward_later(ZERO), a task at the event's time; Pending -> nothing
//     :165-177 run_forward_task: the relay is Idle again, then the forwarding loop
//     :200-272 forward_until_blocked: is_bootstrapping once per task (worker.rs:492-494); take
//              the cached packet or pop the source (CoDelQueue::pop at the task's time, which may
//              drop first and may return none: Idle); unless bootstrapping or unlimited,
//              conforming_remove(total size); Err(d): cache the packet, forward_later(d) -- the
//              task runs at now + d, EmulatedTime saturating -- else forward at the task's time
// The queue is codel_lane.h's CodelLane, the bucket tbucket_ops.h's tb_conforming_remove: the
// functions the replay kernels (codel.hip, tbucket.hip) compile.
//
// Per host the lane merges its events (times non-decreasing, all inside the window) with its own
// forward task:
//     t_ev <= task            push the event, notify
//     else task < window_end  run the task
//     else                    done: the task stays outstanding for a later call
// Each packet leaves the stage at most once, as one record (FORWARDED or DROPPED, pkt, time), so
// host h writes into a region of (its events + stored + cached) records, bounded by a scan
// (scan.h); a second scan of the records written gives the exact offsets they are compacted to.
// The loop ends because a blocked packet's task always forwards it (size <= the bucket's
// capacity, checked at the push): a host runs at most one task per event (notify), one per
// forwarded packet (a block) -- counted down, so no input can spin a lane.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "codel_lane.h"
#include "ctx.h"
#include "inbound_relay.h"
#include "scan.h"
#include "tbucket_ops.h"

namespace shd {

// (kInIdle and the relay words InRelay: inbound_relay.h)
constexpr uint32_t kInBatch = 8;       // events per lane loaded ahead of the state machine
constexpr int kInPinWord = 72;         // ctx->h_pin words [72, 76)
static_assert(kInPinWord + 4 <= kPinMarker, "inbound words below the polled marker");
// status bits (words[0]); any of them is SHD_ERR_INVALID
constexpr uint32_t kInBadOff = 1u;     // offsets not monotone / not covering n_events
constexpr uint32_t kInBadTime = 2u;    // an event before its predecessor (or the last window), or >= window_end
constexpr uint32_t kInBadPkt = 4u;     // a size above the bucket's capacity, or packet id UINT32_MAX
constexpr uint32_t kInRingFull = 8u;
constexpr uint32_t kInPanic = 16u;     // where the reference panics (token_bucket.rs / codel_queue.rs unwraps)
constexpr uint32_t kInSpin = 32u;      // the task budget ran out (unreachable under the input contract)
constexpr uint32_t kInRegion = 64u;    // a record past the host's region (unreachable: one record per packet)

struct InRecords {   // CodelLane's sink: kind 1 FORWARDED, 2 DROPPED, at the running task's time
    uint32_t* pkt;
    uint64_t* time;
    uint8_t* kind;
    uint32_t w, end;
    uint64_t now;
    bool over;
    __device__ void mark(uint32_t p, uint32_t, uint32_t k) {
        if (w < end) {
            pkt[w] = p;
            time[w] = now;
            kind[w] = (uint8_t)k;
            ++w;
        } else {
            over = true;
        }
    }
};

// cnt[h] = the records host h can write: its events + stored + cached; cnt[n_hosts] = 0 (the scan's
// total).  Offsets that are not a CSR over n_events events are reported and count as no events.
__global__ __launch_bounds__(256) void inb_count(uint32_t n_hosts, const uint32_t* __restrict__ off,
                                                 uint64_t n_events, const CodelHost* __restrict__ st,
                                                 const InRelay* __restrict__ rl, uint32_t* __restrict__ cnt,
                                                 uint32_t* __restrict__ nrec, uint32_t* status) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h > n_hosts) return;
    if (h == n_hosts) {
        cnt[h] = 0;
        nrec[h] = 0;
        return;
    }
    uint32_t ne = 0;
    if (off) {
        const uint32_t a = off[h], b = off[h + 1];
        const bool ok = a <= b && b <= n_events && (h != 0 || a == 0) && (h + 1 != n_hosts || b == n_events);
        if (ok) ne = b - a;
        else atomicOr(status, kInBadOff);
    }
    cnt[h] = ne + st[h].count + rl[h].has_cached;
}

__global__ __launch_bounds__(256) void inb_run(uint32_t n_hosts, const uint32_t* __restrict__ off,
                                               const uint64_t* __restrict__ time,
                                               const uint32_t* __restrict__ size,
                                               const uint32_t* __restrict__ pkt, CodelHost* st,
                                               uint32_t* flags_arr, uint4* ring, uint32_t cap, TbRelay* tb,
                                               InRelay* rl, const uint32_t* __restrict__ reg_off,
                                               uint32_t* __restrict__ nrec, uint32_t* r_pkt, uint64_t* r_time,
                                               uint8_t* r_kind, uint64_t prev_end, uint64_t window_end,
                                               uint64_t bootstrap_end, unsigned long long* words) {
    __shared__ uint64_t s_tm[kInBatch][256];
    __shared__ uint32_t s_sz[kInBatch][256], s_pk[kInBatch][256];
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    uint32_t* status = reinterpret_cast<uint32_t*>(words);
    bool live = h < n_hosts;
    // bad offsets (inb_count): no lane reads an event, nothing is written
    if (live && (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kInBadOff)) {
        nrec[h] = 0;
        live = false;
    }
    uint32_t n_out = 0, stored = 0;
    uint64_t task_min = kInIdle;
    if (live) {
        CodelLane<InRecords> L;
        L.s = st[h];
        L.flags = flags_arr[h];
        L.ring = ring + (size_t)h * cap;
        L.cap = cap;
        L.sink = InRecords{r_pkt, r_time, r_kind, reg_off[h], reg_off[h + 1], 0, false};
        const uint32_t base = L.sink.w;
        TbRelay B = tb[h];
        InRelay R = rl[h];
        uint32_t k = off ? off[h] : 0u;
        const uint32_t ke = off ? off[h + 1] : 0u;
        // one task per event (notify) and one per packet that can leave (a block), + slack
        uint64_t budget = 2ull * (ke - k) + L.s.count + R.has_cached + 2u;
        // The host's events are read kInBatch at a time (loads clamped into the range, all issued
        // together): one memory latency per batch instead of one per event.  The state machine
        // below is one loop whose body holds the push and the task once, so the batch is indexed
        // at run time: it is parked in the lane's own LDS column (registers indexed at run time
        // end up in scratch memory; a column is read and written by its lane alone, no barrier).
        uint32_t bi = kInBatch;
        uint64_t last_t = prev_end;
        uint32_t err = 0;
        bool bad = false;
        for (;;) {
            const bool have = k < ke;
            if (have && bi == kInBatch) {
                uint64_t tm[kInBatch];
                uint32_t sz[kInBatch], pk[kInBatch];
#pragma unroll
                for (uint32_t i = 0; i < kInBatch; ++i) {
                    const uint32_t kk = min(k + i, ke - 1);
                    tm[i] = time[kk];
                    sz[i] = size[kk];
                    pk[i] = pkt[kk];
                }
#pragma unroll
                for (uint32_t i = 0; i < kInBatch; ++i) {
                    s_tm[i][threadIdx.x] = tm[i];
                    s_sz[i][threadIdx.x] = sz[i];
                    s_pk[i][threadIdx.x] = pk[i];
                }
                bi = 0;
            }
            const uint64_t t_ev = have ? s_tm[bi][threadIdx.x] : kInIdle;
            // the time contract, checked before the event is weighed against the task: an event at
            // or past window_end behind a task carried past it would otherwise end the loop unread
            if (have && (t_ev < last_t || t_ev >= window_end)) {
                err |= kInBadTime;
                break;
            }
            if (have && t_ev <= R.task) {   // Packet before Local at equal time (event.rs:102-110)
                const uint32_t s_ = s_sz[bi][threadIdx.x], p_ = s_pk[bi][threadIdx.x];
                if ((B.capacity && s_ > B.capacity) || p_ == kPop) {
                    err |= kInBadPkt;
                    break;
                }
                if (!L.push(p_, s_, t_ev)) {   // route_incoming_packet (host.rs:742-746)
                    err |= kInRingFull;
                    break;
                }
                last_t = t_ev;
                if (R.task == kInIdle) R.task = t_ev;   // Relay::notify: forward_later(ZERO)
                ++k;
                ++bi;
            } else if (R.task < window_end) {   // run_forward_task (relay/mod.rs:165-177)
                if (budget-- == 0) {
                    err |= kInSpin;
                    break;
                }
                const uint64_t T = R.task;
                R.task = kInIdle;
                const bool boot = T < bootstrap_end;   // Worker::is_bootstrapping, once per task
                L.sink.now = T;
                for (;;) {   // forward_until_blocked (relay/mod.rs:200-272); each pass takes a packet
                    uint32_t p_, s_;
                    if (R.has_cached) {
                        p_ = R.cached_pkt;
                        s_ = R.cached_size;
                        R.has_cached = 0;
                    } else {
                        p_ = L.pop(T, 0, &s_);
                        if (p_ == kPop) break;   // ran out of packets: Idle
                    }
                    if (!boot && B.capacity) {
                        uint64_t d;
                        if (!tb_conforming_remove(B, T, s_, d, bad)) {
                            R.has_cached = 1;
                            R.cached_pkt = p_;
                            R.cached_size = s_;
                            R.task = emutime_sat_add(T, d);   // forward_later(blocking_dur)
                            break;
                        }
                    }
                    L.sink.mark(p_, 0, 1);
                }
            } else {
                break;
            }
        }
        if (bad || (L.flags & kCodelPanic)) err |= kInPanic;
        if (L.sink.over) err |= kInRegion;
        if (err) atomicOr(status, err);
        st[h] = L.s;
        flags_arr[h] = L.flags & ~kCodelPanic;
        tb[h] = B;
        rl[h] = R;
        n_out = L.sink.w - base;
        nrec[h] = n_out;
        stored = L.s.count + R.has_cached;
        task_min = R.task;
    }
    // the call's totals: one atomic per wave and word
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_out += (uint32_t)__shfl_xor((int)n_out, o);
        stored += (uint32_t)__shfl_xor((int)stored, o);
        const uint64_t t = ((uint64_t)(uint32_t)__shfl_xor((int)(task_min >> 32), o) << 32) |
                           (uint32_t)__shfl_xor((int)(uint32_t)task_min, o);
        task_min = t < task_min ? t : task_min;
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_out) atomicAdd(words + 1, (unsigned long long)n_out);
        if (stored) atomicAdd(words + 2, (unsigned long long)stored);
        if (task_min != kInIdle) atomicMin(words + 3, (unsigned long long)task_min);
    }
}

// output position d -> its host (the last h with out_off[h] <= d: the one whose records hold d)
// -> the record's slot in the host's region.  The work follows the records written, not the
// slots bounded: positions at or past out_off[n_hosts] have nothing to do.
__global__ __launch_bounds__(256) void inb_compact(uint64_t n_slots, uint32_t n_hosts,
                                                   const uint32_t* __restrict__ reg_off,
                                                   const uint32_t* __restrict__ out_off,
                                                   const uint32_t* __restrict__ r_pkt,
                                                   const uint64_t* __restrict__ r_time,
                                                   const uint8_t* __restrict__ r_kind, uint32_t* __restrict__ o_pkt,
                                                   uint64_t* __restrict__ o_time, uint8_t* __restrict__ o_kind) {
    const uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= min((uint64_t)out_off[n_hosts], n_slots)) return;
    uint32_t lo = 0, hi = n_hosts;   // out_off[lo] <= d < out_off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (out_off[mid] <= d) lo = mid;
        else hi = mid;
    }
    // (inside host lo's region: d - out_off[lo] < the records it wrote <= the region's size)
    const uint64_t i = (uint64_t)reg_off[lo] + (d - out_off[lo]);
    o_pkt[d] = r_pkt[i];
    o_time[d] = r_time[i];
    o_kind[d] = r_kind[i];
}

}  // namespace shd

using namespace shd;

extern "C" {

shd_status shd_inbound_setup(shd_ctx* ctx, uint32_t n_hosts, uint32_t capacity, const uint64_t* tb_capacity,
                             const uint64_t* tb_refill_increment, const uint64_t* tb_refill_interval_ns,
                             const uint64_t* tb_last_refill) {
    if (!ctx || capacity == 0) return SHD_ERR_INVALID;
    std::vector<TbRelay> hb;
    SHD_TRY(tb_rows(n_hosts, tb_capacity, tb_refill_increment, tb_refill_interval_ns, tb_last_refill, hb));
    InboundState& I = ctx->inb;
    I.ready = false;
    hipStream_t s = ctx->stream;
    SHD_HIP(hipSetDevice(ctx->device));
    const size_t n1 = std::max<size_t>(n_hosts, 1);
    SHD_TRY(I.st.ensure(n1 * sizeof(CodelHost)));
    SHD_TRY(I.flags.ensure(n1 * 4));
    SHD_TRY(I.ring.ensure(std::max<size_t>((size_t)n_hosts * capacity, 1) * 16));
    SHD_TRY(I.tb.ensure(n1 * sizeof(TbRelay)));
    SHD_TRY(I.rl.ensure(n1 * sizeof(InRelay)));
    SHD_TRY(I.cnt.ensure(((size_t)n_hosts + 1) * 4));
    SHD_TRY(I.nrec.ensure(((size_t)n_hosts + 1) * 4));
    SHD_TRY(I.o_off.ensure(((size_t)n_hosts + 1) * 4));
    SHD_TRY(I.words.ensure(32));
    SHD_HIP(hipMemsetAsync(I.st.p, 0, (size_t)n_hosts * sizeof(CodelHost), s));
    SHD_HIP(hipMemsetAsync(I.flags.p, 0, (size_t)n_hosts * 4, s));
    SHD_HIP(hipMemsetAsync(I.o_off.p, 0, ((size_t)n_hosts + 1) * 4, s));
    const std::vector<InRelay> hr(n_hosts, InRelay{kInIdle, 0, 0, 0, 0});
    if (n_hosts) {
        SHD_HIP(hipMemcpyAsync(I.tb.p, hb.data(), (size_t)n_hosts * sizeof(TbRelay), hipMemcpyHostToDevice, s));
        SHD_HIP(hipMemcpyAsync(I.rl.p, hr.data(), (size_t)n_hosts * sizeof(InRelay), hipMemcpyHostToDevice, s));
    }
    SHD_HIP(hipStreamSynchronize(s));
    I.n_hosts = n_hosts;
    I.cap = capacity;
    I.n_stored = 0;
    I.prev_end = 0;
    I.ready = true;
    return SHD_OK;
}

shd_status shd_inbound_advance(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time,
                               const uint32_t* d_size, const uint32_t* d_pkt, uint64_t n_events,
                               uint64_t window_end, uint64_t bootstrap_end, const uint32_t** out_off,
                               const uint32_t** out_pkt, const uint64_t** out_time, const uint8_t** out_kind,
                               uint64_t* n_out, uint64_t* n_stored, uint64_t* next_task_time) {
    if (!ctx) return SHD_ERR_INVALID;
    InboundState& I = ctx->inb;
    if (!I.ready) return SHD_ERR_STATE;
    // argument errors: nothing has run, the stage stays as it was
    if (n_events && (!d_off || !d_time || !d_size || !d_pkt)) return SHD_ERR_INVALID;
    if (n_events && I.n_hosts == 0) return SHD_ERR_INVALID;
    if (window_end < I.prev_end) return SHD_ERR_INVALID;
    const uint64_t n_slots = n_events + I.n_stored;   // every packet leaves at most once
    if (n_slots >= 0xFFFFFFFFull) return SHD_ERR_INVALID;
    hipStream_t s = ctx->stream;
    SHD_HIP(hipSetDevice(ctx->device));
    const size_t r1 = std::max<size_t>(n_slots, 1);
    SHD_TRY(I.r_pkt.ensure(r1 * 4));
    SHD_TRY(I.r_time.ensure(r1 * 8));
    SHD_TRY(I.r_kind.ensure(r1));
    SHD_TRY(I.o_pkt.ensure(r1 * 4));
    SHD_TRY(I.o_time.ensure(r1 * 8));
    SHD_TRY(I.o_kind.ensure(r1));
    unsigned long long* words = I.words.as<unsigned long long>();
    SHD_HIP(hipMemsetAsync(words, 0, 24, s));
    SHD_HIP(hipMemsetAsync(words + 3, 0xFF, 8, s));
    const uint32_t H = I.n_hosts;
    if (H) {
        uint32_t* cnt = I.cnt.as<uint32_t>();
        uint32_t* nrec = I.nrec.as<uint32_t>();
        inb_count<<<div_up((uint64_t)H + 1, 256), 256, 0, s>>>(H, d_off, n_events, I.st.as<CodelHost>(),
                                                               I.rl.as<InRelay>(), cnt, nrec,
                                                               reinterpret_cast<uint32_t*>(words));
        SHD_HIP(hipGetLastError());
        SHD_TRY(scan_excl2(I.scan, cnt, cnt, nullptr, nullptr, (uint64_t)H + 1, s));   // -> region offsets
        inb_run<<<div_up(H, 256), 256, 0, s>>>(H, d_off, d_time, d_size, d_pkt, I.st.as<CodelHost>(),
                                               I.flags.as<uint32_t>(), I.ring.as<uint4>(), I.cap,
                                               I.tb.as<TbRelay>(), I.rl.as<InRelay>(), cnt, nrec,
                                               I.r_pkt.as<uint32_t>(), I.r_time.as<uint64_t>(),
                                               I.r_kind.as<uint8_t>(), I.prev_end, window_end, bootstrap_end, words);
        SHD_HIP(hipGetLastError());
        SHD_TRY(scan_excl2(I.scan, nrec, I.o_off.as<uint32_t>(), nullptr, nullptr, (uint64_t)H + 1, s));
        if (n_slots) {
            // (a thread per slot: n_out is known on the device only; the surplus threads leave at once)
            inb_compact<<<div_up(n_slots, 256), 256, 0, s>>>(
                n_slots, H, cnt, I.o_off.as<uint32_t>(), I.r_pkt.as<uint32_t>(), I.r_time.as<uint64_t>(),
                I.r_kind.as<uint8_t>(), I.o_pkt.as<uint32_t>(), I.o_time.as<uint64_t>(), I.o_kind.as<uint8_t>());
            SHD_HIP(hipGetLastError());
        }
    }
    // status, the record count, the stored total and the earliest task in one pinned read
    SHD_TRY(readback(ctx, s, kInPinWord, words, 32));
    const unsigned long long* w = ctx->h_pin + kInPinWord;
    if ((uint32_t)w[0]) {
        // the window ran up to the offending event on its host and in full elsewhere: the stage
        // now holds a state the reference never reaches -- shd_inbound_setup must run again
        I.ready = false;
        return SHD_ERR_INVALID;
    }
    I.n_stored = w[2];
    I.prev_end = window_end;
    if (out_off) *out_off = I.o_off.as<uint32_t>();
    if (out_pkt) *out_pkt = I.o_pkt.as<uint32_t>();
    if (out_time) *out_time = I.o_time.as<uint64_t>();
    if (out_kind) *out_kind = I.o_kind.as<uint8_t>();
    if (n_out) *n_out = w[1];
    if (n_stored) *n_stored = w[2];
    if (next_task_time) *next_task_time = w[3];
    return SHD_OK;
}

shd_status shd_inbound_get_state(shd_ctx* ctx, uint32_t host, uint64_t* task_time, uint32_t* has_cached,
                                 uint32_t* cached_pkt, uint32_t* cached_size, shd_codel_state* codel,
                                 shd_tb_state* bucket) {
    if (!ctx) return SHD_ERR_INVALID;
    InboundState& I = ctx->inb;
    if (!I.ready) return SHD_ERR_STATE;   // not set up, or a contract error since: as the advance
    if (host >= I.n_hosts) return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    InRelay r;
    SHD_HIP(hipMemcpy(&r, I.rl.as<InRelay>() + host, sizeof(r), hipMemcpyDeviceToHost));
    if (task_time) *task_time = r.task;
    if (has_cached) *has_cached = r.has_cached;
    if (cached_pkt) *cached_pkt = r.has_cached ? r.cached_pkt : 0;
    if (cached_size) *cached_size = r.has_cached ? r.cached_size : 0;
    if (codel) {
        CodelHost hs;
        uint32_t fl = 0;
        SHD_HIP(hipMemcpy(&hs, I.st.as<CodelHost>() + host, sizeof(hs), hipMemcpyDeviceToHost));
        SHD_HIP(hipMemcpy(&fl, I.flags.as<uint32_t>() + host, 4, hipMemcpyDeviceToHost));
        codel->len = hs.count;
        codel->mode = (fl & kModeDrop) ? 1 : 0;
        codel->has_interval_end = (fl & kHasIntervalEnd) ? 1 : 0;
        codel->has_drop_next = (fl & kHasDropNext) ? 1 : 0;
        codel->interval_end = hs.interval_end;
        codel->drop_next = hs.drop_next;
        codel->current_drop_count = hs.cur;
        codel->previous_drop_count = hs.prev;
        codel->total_bytes_stored = hs.total;
    }
    if (bucket) {
        TbRelay b;
        SHD_HIP(hipMemcpy(&b, I.tb.as<TbRelay>() + host, sizeof(b), hipMemcpyDeviceToHost));
        bucket->capacity = b.capacity;
        bucket->balance = b.balance;
        bucket->refill_increment = b.increment;
        bucket->refill_interval = b.interval;
        bucket->last_refill = b.last_refill;
        bucket->pending_until = r.task == kInIdle ? 0 : r.task;   // the relay's task, as shd_tb_state names it
    }
    return SHD_OK;
}

// the hosts' bw_down buckets re-rated at `at_time` (rate_update.hip): queues, CoDel state, the
// cached packet and the outstanding task stay
shd_status shd_inbound_update_buckets(shd_ctx* ctx, uint64_t n, const uint32_t* host, const uint64_t* capacity,
                                      const uint64_t* refill_increment, const uint64_t* refill_interval_ns,
                                      uint64_t at_time, uint32_t* err_host) {
    return rate_update(ctx, kRateInbound, n, host, capacity, refill_increment, refill_interval_ns, at_time, err_host);
}

}  // extern "C"
