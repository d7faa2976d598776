// The outbound stage on the GPU: per source host the network interface's queuing discipline (FIFO
// or round-robin: interface_qdisc, configuration.rs:396-397), the outbound relay's token bucket and the relay's own state, device-resident across calls.  One
// call advances every host over one scheduling window, lane per host, from the window's offers
// ("socket data became sendable") to the instant each packet enters Worker::send_packet: the
// shd_batch a relay round (relay.hip) takes, with no CPU step in between.
//
// Reference semantics (FlyearthR/shadow):
//   src/main/host/host.rs
//     :285-288, :871-880 relay_inet_out: the interface is the source, the router the sink;
//              notify_socket_has_packets ends in Relay::notify
//     :604-610 get_next_packet_priority: one counter per host, so priorities are unique per host
//   src/main/host/network/network_interface.c
//     :276-316 _networkinterface_selectFifo: the socket whose head packet has the lowest priority
//     :235-273 _networkinterface_selectRoundRobin, :366-392 networkinterface_wantsSend: the
//              rrQueue (rr_queue.h restates both)
//   src/main/host/network/network_queuing_disciplines.c
//     :90-102  the FIFO comparison of two sockets' head priorities (never equal under OutFifo's
//              contract; a tie is "smaller" both ways: OutFifoSock)
//   src/main/network/relay/mod.rs
//     :110-135 notify: Idle -> forward_later(ZERO), a task at the offer's time ("allow packets to
//              accumulate", :124-126); Pending -> nothing
//     :165-177 run_forward_task: the relay is Idle again, then the forwarding loop
//     :200-272 forward_until_blocked: is_bootstrapping once per task; take the cached packet or
//              pop the source (none: Idle); a packet whose destination is the source device is
//              local (:222-230): it is forwarded without the bucket and pushed back to the
//              interface (:262-265); otherwise, unless bootstrapping or unlimited,
//              conforming_remove(total size); Err(d): cache the packet, forward_later(d) -- the
//              task runs at now + d, EmulatedTime saturating -- else the packet goes to the router
//   src/main/network/router/mod.rs
//     :49-55   Router::push of an outbound packet calls Worker::send_packet at the task's time
// Each socket offers its packets in increasing priority, so "lowest head priority over the
// sockets" is "lowest priority over all queued packets": one priority queue per host is exact.
// The bucket is tbucket_ops.h's tb_conforming_remove, the function tbucket.hip and inbound.hip
// compile.
//
// Per host the lane merges its offers (times non-decreasing, all inside the window) with its own
// forward task:
//     t_offer <= task         insert the packet by priority, notify
//     else task < window_end  run the task
//     else                    done: the task stays outstanding for a later call
// An offer at the task's own time is inserted before the task runs (the sends of one event
// accumulate).  Exactness: the merge is exact whenever a host's offers at one instant arrive in
// increasing priority -- everything but a same-instant retransmission -- and also when the bucket
// does not block at that instant; otherwise a later offer of the same instant and a lower
// priority, which the reference's task would not have seen yet, goes first here.  The cached
// packet is never overtaken, not by a local packet and not by a lower priority (head-of-line
// blocking, as the reference).
//
// Under round-robin (OutRr below) "insert by priority" reads "offer to the socket's packets" and
// the 64-bit key is the socket's canonical handle; the merge is then exact whenever a host's
// offers at one instant belong to one event (one accumulation under relay/mod.rs:124-126) or to
// one socket.  Two events on one host at the same nanosecond that offer on different sockets are
// rotated together here; in the reference the first event's task may already have drained its
// packets.  Within a socket packets leave in offer order under OutFifo and OutRr, which see a
// socket as one list.  OutFifoSock and OutRrSock (below, sock_queue.h) keep the sockets with the
// control and the data buffer of socket.c:432-437 -- every TCP control packet has priority 0 and
// leaves before its socket's data -- and, for FIFO, the reference's array heap of sockets
// (priority_queue.c), whose send order is a function of the array: a control packet offered to a
// queued socket changes its key in place.  Under OutFifoSock a same-instant retransmission is
// exact too (order within a socket is offer order); two events of one host at one nanosecond
// stay inexact as under round-robin.
//
// Not covered: the loopback relay (unlimited, every packet local), the pcap and tracker side
// effects of networkinterface_pop, and the CPU-delay model (as the inbound stage).
//
// Each packet leaves the stage at most once, as one record: SENT (pkt, time, dst, payload, size) or
// LOCAL (pkt, time).  Host h owns a region of (its offers + queued + cached) records, bounded by a
// scan (scan.h); the record's kind picks the end it is written at -- SENT from the front, LOCAL
// from the back -- so the two kinds never meet and each keeps its order.  Two more scans (sent
// and local per host, one launch) give the offsets both are compacted to.  The loop ends because
// a blocked packet's task always forwards it (size <= the bucket's capacity, checked at the
// insert): a host runs at most one task per offer (notify) and one per packet that leaves (a
// block) -- counted down, so no input can spin a lane.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "ctx.h"
#include "outbound_queue.h"
#include "scan.h"
#include "tbucket_ops.h"

namespace shd {

// Offers per lane loaded ahead, and hosts per workgroup of outb_run.  An offer is 32 bytes, so the
// batch's LDS columns take kOutBatch * 32 * kOutLanes bytes: 16 KB.  One wave per workgroup: a
// finished wave frees its slot at once, and 100k hosts make 1563 workgroups for the 256 CUs.
// Measured in one session on a 100k-host, 10M-offer window: 8 x 64 1.45 ms,
// 8 x 128 1.53 ms, 4 x 128 1.56 ms, 4 x 256 1.58 ms.
constexpr uint32_t kOutBatch = 8;
constexpr uint32_t kOutLanes = 64;
static_assert(kOutBatch * 32 * kOutLanes <= 65536 && kOutLanes % 64 == 0, "outb_run's static LDS");
// (the socket disciplines park one more 8-byte column, the offering socket: 40 bytes an offer, 20 KB)
static_assert(kOutBatch * 40 * kOutLanes <= 65536, "outb_run's static LDS with the socket column");
constexpr int kOutPinWord = 81;        // ctx->h_pin words [81, 86)
constexpr int kOutWords = 5;           // status, n_sent, n_local, n_stored, min task time
static_assert(kOutPinWord > kPinMarker && kOutPinWord + kOutWords <= kPinWords,
              "outbound words above the polled marker");

// (the relay words, the status bits and the queuing disciplines OutFifo, OutRr, OutFifoSock and
// OutRrSock: outbound_queue.h)

// the socket column of the offer batch: LDS only in the instances that call this
__device__ __forceinline__ uint64_t (*outb_sock_col())[kOutLanes] {
    __shared__ uint64_t s_sk[kOutBatch][kOutLanes];
    return s_sk;
}

// cnt[h] = the records host h can write: its offers + queued + cached; cnt[n_hosts] = 0 (the scan's
// total).  Offsets that are not a CSR over n_offers offers are reported and count as no offers.
__global__ __launch_bounds__(256) void outb_count(uint32_t n_hosts, const uint32_t* __restrict__ off,
                                                  uint64_t n_offers, const OutRelay* __restrict__ rl,
                                                  uint32_t* __restrict__ cnt, uint32_t* __restrict__ nsent,
                                                  uint32_t* __restrict__ nloc, uint32_t* status) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h > n_hosts) return;
    if (h == n_hosts) {
        cnt[h] = 0;
        nsent[h] = 0;
        nloc[h] = 0;
        return;
    }
    uint32_t no = 0;
    if (off) {
        const uint32_t a = off[h], b = off[h + 1];
        const bool ok = a <= b && b <= n_offers && (h != 0 || a == 0) && (h + 1 != n_hosts || b == n_offers);
        if (ok) no = b - a;
        else atomicOr(status, kOutBadOff);
    }
    cnt[h] = no + rl[h].count + rl[h].has_cached;
}

template <class Q>
__global__ __launch_bounds__(kOutLanes) void outb_run(
    uint32_t n_hosts, uint32_t first_host, const uint32_t* __restrict__ off, const uint64_t* __restrict__ time,
    const uint64_t* __restrict__ prio, const uint32_t* __restrict__ size, const uint32_t* __restrict__ payload,
    const uint32_t* __restrict__ dst, const uint32_t* __restrict__ pkt, const typename Q::Args qa, TbRelay* tb,
    OutRelay* rl, const uint32_t* __restrict__ reg_off, uint32_t* __restrict__ nsent, uint32_t* __restrict__ nloc,
    uint32_t* r_pkt, uint64_t* r_time, uint32_t* r_dst, uint32_t* r_pay, uint32_t* r_size, uint64_t prev_end,
    uint64_t window_end,
    uint64_t bootstrap_end, unsigned long long* words) {
    __shared__ uint64_t s_tm[kOutBatch][kOutLanes], s_pr[kOutBatch][kOutLanes];
    __shared__ uint32_t s_sz[kOutBatch][kOutLanes], s_pl[kOutBatch][kOutLanes], s_ds[kOutBatch][kOutLanes],
        s_pk[kOutBatch][kOutLanes];
    constexpr bool kSock = OutHasSock<Q>::value;
    uint64_t(*s_sk)[kOutLanes] = nullptr;
    if constexpr (kSock) s_sk = outb_sock_col();
    const uint32_t h = blockIdx.x * kOutLanes + threadIdx.x;
    uint32_t* status = reinterpret_cast<uint32_t*>(words);
    bool live = h < n_hosts;
    // bad offsets (outb_count): no lane reads an offer, nothing is written
    if (live && (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kOutBadOff)) {
        nsent[h] = 0;
        nloc[h] = 0;
        live = false;
    }
    uint32_t n_s = 0, n_l = 0, stored = 0;
    uint64_t task_min = kOutIdle;
    if (live) {
        TbRelay B = tb[h];
        OutRelay R = rl[h];
        Q q(qa, h, R);   // the discipline's queue: its part of R, its arrays
        const uint32_t self = first_host + h;   // the host's global id: what "local" compares with
        const uint32_t r_lo = reg_off[h], r_hi = reg_off[h + 1];
        uint32_t k = off ? off[h] : 0u;
        const uint32_t ke = off ? off[h + 1] : 0u;
        // one task per offer (notify) and one per packet that can leave (a block), + slack
        uint64_t budget = 2ull * (ke - k) + R.count + R.has_cached + 2u;
        // The host's offers are read kOutBatch at a time (loads clamped into the range, all issued
        // together): one memory latency per batch instead of one per offer.  The state machine
        // below is one loop whose body holds the insert and the task once, so the batch is indexed
        // at run time: it is parked in the lane's own LDS column (registers indexed at run time
        // end up in scratch memory; a column is read and written by its lane alone, no barrier).
        uint32_t bi = kOutBatch;
        uint64_t last_t = prev_end;
        uint32_t err = 0;
        bool bad = false;
        for (;;) {
            const bool have = k < ke;
            if (have && bi == kOutBatch) {
                uint64_t tm[kOutBatch], pr[kOutBatch];
                uint32_t sz[kOutBatch], pl[kOutBatch], ds[kOutBatch], pk[kOutBatch];
                [[maybe_unused]] uint64_t sk[kSock ? kOutBatch : 1];
#pragma unroll
                for (uint32_t i = 0; i < kOutBatch; ++i) {
                    const uint32_t kk = min(k + i, ke - 1);
                    tm[i] = time[kk];
                    pr[i] = prio[kk];
                    if constexpr (kSock) sk[i] = qa.sock[kk];
                    sz[i] = size[kk];
                    pl[i] = payload[kk];
                    ds[i] = dst[kk];
                    pk[i] = pkt[kk];
                }
#pragma unroll
                for (uint32_t i = 0; i < kOutBatch; ++i) {
                    s_tm[i][threadIdx.x] = tm[i];
                    s_pr[i][threadIdx.x] = pr[i];
                    s_sz[i][threadIdx.x] = sz[i];
                    s_pl[i][threadIdx.x] = pl[i];
                    s_ds[i][threadIdx.x] = ds[i];
                    s_pk[i][threadIdx.x] = pk[i];
                    if constexpr (kSock) s_sk[i][threadIdx.x] = sk[i];
                }
                bi = 0;
            }
            const uint64_t t_of = have ? s_tm[bi][threadIdx.x] : kOutIdle;
            // the time contract, checked before the offer is weighed against the task: an offer at
            // or past window_end behind a task carried past it would otherwise end the loop unread
            if (have && (t_of < last_t || t_of >= window_end)) {
                err |= kOutBadTime;
                break;
            }
            if (have && t_of <= R.task) {   // notify_socket_has_packets, then Relay::notify
                OutPkt e;
                e.prio = s_pr[bi][threadIdx.x];
                e.pkt = s_pk[bi][threadIdx.x];
                e.size = s_sz[bi][threadIdx.x];
                e.payload = s_pl[bi][threadIdx.x];
                e.dst = s_ds[bi][threadIdx.x];
                if (e.pkt == kOutNoPkt || (e.dst != self && B.capacity && e.size > B.capacity)) {
                    err |= kOutBadPkt;
                    break;
                }
                if constexpr (kSock) {
                    if (const uint32_t refused = q.insert(R, e, s_sk[bi][threadIdx.x])) {
                        err |= refused;
                        break;
                    }
                } else {
                    if (const uint32_t refused = q.insert(R, e)) {
                        err |= refused;
                        break;
                    }
                }
                last_t = t_of;
                if (R.task == kOutIdle) R.task = t_of;   // Relay::notify: forward_later(ZERO)
                ++k;
                ++bi;
            } else if (R.task < window_end) {   // run_forward_task (relay/mod.rs:165-177)
                if (budget-- == 0) {
                    err |= kOutSpin;
                    break;
                }
                const uint64_t T = R.task;
                R.task = kOutIdle;
                const bool boot = T < bootstrap_end;   // Worker::is_bootstrapping, once per task
                for (;;) {   // forward_until_blocked (relay/mod.rs:200-272); each pass takes a packet
                    uint32_t p_, s_, pl_, d_;
                    if (R.has_cached) {
                        p_ = R.cached_pkt;
                        s_ = R.cached_size;
                        pl_ = R.cached_payload;
                        d_ = R.cached_dst;
                        R.has_cached = 0;
                    } else {
                        if (R.count == 0) break;   // ran out of packets: Idle
                        q.pop(R, p_, s_, pl_, d_);   // networkinterface_pop
                    }
                    const bool local = d_ == self;   // relay/mod.rs:222-230
                    if (!boot && !local && B.capacity) {
                        uint64_t d;
                        if (!tb_conforming_remove(B, T, s_, d, bad)) {
                            R.has_cached = 1;
                            R.cached_pkt = p_;
                            R.cached_size = s_;
                            R.cached_payload = pl_;
                            R.cached_dst = d_;
                            R.task = emutime_sat_add(T, d);   // forward_later(blocking_dur)
                            break;
                        }
                    }
                    if (n_s + n_l >= r_hi - r_lo) {
                        err |= kOutRegion;
                        break;
                    }
                    if (local) {   // back to the interface (relay/mod.rs:262-265): not sent
                        const uint32_t w = r_hi - 1 - n_l;
                        r_pkt[w] = p_;
                        r_time[w] = T;
                        ++n_l;
                    } else {       // Router::push -> Worker::send_packet at T (router/mod.rs:49-55)
                        const uint32_t w = r_lo + n_s;
                        r_pkt[w] = p_;
                        r_time[w] = T;
                        r_dst[w] = d_;
                        r_pay[w] = pl_;
                        r_size[w] = s_;   // the total size: what the destination's bucket removes (the ledger)
                        ++n_s;
                    }
                }
                if (err) break;
            } else {
                break;
            }
        }
        if (bad) err |= kOutPanic;
        if (err) atomicOr(status, err);
        q.store(R);
        tb[h] = B;
        rl[h] = R;
        nsent[h] = n_s;
        nloc[h] = n_l;
        stored = R.count + R.has_cached;
        task_min = R.task;
    }
    // the call's totals: one atomic per wave and word
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_s += (uint32_t)__shfl_xor((int)n_s, o);
        n_l += (uint32_t)__shfl_xor((int)n_l, o);
        stored += (uint32_t)__shfl_xor((int)stored, o);
        const uint64_t t = ((uint64_t)(uint32_t)__shfl_xor((int)(task_min >> 32), o) << 32) |
                           (uint32_t)__shfl_xor((int)(uint32_t)task_min, o);
        task_min = t < task_min ? t : task_min;
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_s) atomicAdd(words + 1, (unsigned long long)n_s);
        if (n_l) atomicAdd(words + 2, (unsigned long long)n_l);
        if (stored) atomicAdd(words + 3, (unsigned long long)stored);
        if (task_min != kOutIdle) atomicMin(words + 4, (unsigned long long)task_min);
    }
}

// the last h with o[h] <= d: the host whose records hold output position d (d < o[n_hosts])
__device__ __forceinline__ uint32_t outb_host_of(const uint32_t* __restrict__ o, uint32_t n_hosts, uint64_t d) {
    uint32_t lo = 0, hi = n_hosts;   // o[lo] <= d < o[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (o[mid] <= d) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Output position d of either kind -> its host -> the record's slot in the host's region: the
// i-th SENT record is the region's i-th slot, the i-th LOCAL one its i-th slot from the end.  The
// work follows the records written, not the slots bounded: positions at or past the totals have
// nothing to do.
__global__ __launch_bounds__(256) void outb_compact(
    uint64_t n_slots, uint32_t n_hosts, const uint32_t* __restrict__ reg_off, const uint32_t* __restrict__ src_off,
    const uint32_t* __restrict__ loc_off, const uint32_t* __restrict__ r_pkt, const uint64_t* __restrict__ r_time,
    const uint32_t* __restrict__ r_dst, const uint32_t* __restrict__ r_pay, const uint32_t* __restrict__ r_size,
    uint64_t* __restrict__ b_time, uint32_t* __restrict__ b_dst, uint32_t* __restrict__ b_pay,
    uint32_t* __restrict__ b_pkt, uint32_t* __restrict__ b_size,
    uint32_t* __restrict__ l_pkt, uint64_t* __restrict__ l_time) {
    const uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (d < min((uint64_t)src_off[n_hosts], n_slots)) {
        const uint32_t h = outb_host_of(src_off, n_hosts, d);
        // (inside host h's region: d - src_off[h] < the records it sent <= the region's size)
        const uint64_t i = (uint64_t)reg_off[h] + (d - src_off[h]);
        b_time[d] = r_time[i];
        b_dst[d] = r_dst[i];
        b_pay[d] = r_pay[i];
        b_pkt[d] = r_pkt[i];
        b_size[d] = r_size[i];
    }
    if (d < min((uint64_t)loc_off[n_hosts], n_slots)) {
        const uint32_t h = outb_host_of(loc_off, n_hosts, d);
        const uint64_t i = (uint64_t)reg_off[h + 1] - 1 - (d - loc_off[h]);
        l_pkt[d] = r_pkt[i];
        l_time[d] = r_time[i];
    }
}

}  // namespace shd

using namespace shd;

extern "C" {

shd_status shd_outbound_setup_qdisc(shd_ctx* ctx, uint32_t n_hosts, uint32_t first_host, uint32_t capacity,
                                    uint32_t qdisc, uint32_t max_sockets, const uint64_t* tb_capacity,
                                    const uint64_t* tb_refill_increment, const uint64_t* tb_refill_interval_ns,
                                    const uint64_t* tb_last_refill) {
    if (!ctx || capacity == 0) return SHD_ERR_INVALID;
    if (qdisc != SHD_QDISC_FIFO && qdisc != SHD_QDISC_ROUND_ROBIN && qdisc != SHD_QDISC_FIFO_SOCKETS &&
        qdisc != SHD_QDISC_ROUND_ROBIN_SOCKETS)
        return SHD_ERR_INVALID;
    const bool rr = qdisc == SHD_QDISC_ROUND_ROBIN;
    const bool sq = qdisc == SHD_QDISC_FIFO_SOCKETS || qdisc == SHD_QDISC_ROUND_ROBIN_SOCKETS;
    // (slot and ring indices are summed in 32 bits before they wrap)
    if ((rr || sq) && (max_sockets == 0 || max_sockets > 0x7FFFFFFFu || capacity > 0x7FFFFFFFu)) return SHD_ERR_INVALID;
    if ((uint64_t)first_host + n_hosts > 0xFFFFFFFFull) return SHD_ERR_INVALID;   // global ids are u32
    std::vector<TbRelay> hb;
    SHD_TRY(tb_rows(n_hosts, tb_capacity, tb_refill_increment, tb_refill_interval_ns, tb_last_refill, hb));
    OutboundState& O = ctx->outb;
    O.ready = false;
    hipStream_t s = ctx->stream;
    SHD_HIP(hipSetDevice(ctx->device));
    const size_t n1 = std::max<size_t>(n_hosts, 1);
    SHD_TRY(O.ring.ensure(std::max<size_t>((size_t)n_hosts * capacity, 1) *
                          (sq ? sizeof(SqSlot) : rr ? sizeof(RrSlot) : sizeof(OutPkt))));
    // (the socket disciplines' pool words lie in the relay words: neither array needs a first write)
    if (sq) SHD_TRY(O.socks.ensure(std::max<size_t>((size_t)n_hosts * max_sockets, 1) * sizeof(SqSock)));
    if (rr) {
        SHD_TRY(O.socks.ensure(std::max<size_t>((size_t)n_hosts * max_sockets, 1) * sizeof(RrSock)));
        SHD_TRY(O.rr_words.ensure(n1 * sizeof(uint2)));
    }
    SHD_TRY(O.tb.ensure(n1 * sizeof(TbRelay)));
    SHD_TRY(O.rl.ensure(n1 * sizeof(OutRelay)));
    SHD_TRY(O.cnt.ensure(((size_t)n_hosts + 1) * 4));
    SHD_TRY(O.nsent.ensure(((size_t)n_hosts + 1) * 4));
    SHD_TRY(O.nloc.ensure(((size_t)n_hosts + 1) * 4));
    SHD_TRY(O.src_off.ensure(((size_t)n_hosts + 1) * 4));
    SHD_TRY(O.loc_off.ensure(((size_t)n_hosts + 1) * 4));
    SHD_TRY(O.words.ensure(kOutWords * 8));
    SHD_HIP(hipMemsetAsync(O.src_off.p, 0, ((size_t)n_hosts + 1) * 4, s));
    SHD_HIP(hipMemsetAsync(O.loc_off.p, 0, ((size_t)n_hosts + 1) * 4, s));
    OutRelay idle{};
    idle.task = kOutIdle;
    const std::vector<OutRelay> hr(n_hosts, idle);
    // an empty pool: nothing bumped, no free slot; its links are written as slots are freed
    const std::vector<uint2> hw(rr ? n_hosts : 0, make_uint2(0, kRrNil));
    if (!hw.empty())
        SHD_HIP(hipMemcpyAsync(O.rr_words.p, hw.data(), hw.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
    if (n_hosts) {
        SHD_HIP(hipMemcpyAsync(O.tb.p, hb.data(), (size_t)n_hosts * sizeof(TbRelay), hipMemcpyHostToDevice, s));
        SHD_HIP(hipMemcpyAsync(O.rl.p, hr.data(), (size_t)n_hosts * sizeof(OutRelay), hipMemcpyHostToDevice, s));
    }
    SHD_HIP(hipStreamSynchronize(s));
    O.n_hosts = n_hosts;
    O.first_host = first_host;
    O.cap = capacity;
    O.qdisc = qdisc;
    O.max_sockets = rr || sq ? max_sockets : 0;
    O.n_stored = 0;
    O.prev_end = 0;
    O.advanced = false;
    O.ready = true;
    return SHD_OK;
}

shd_status shd_outbound_setup(shd_ctx* ctx, uint32_t n_hosts, uint32_t first_host, uint32_t capacity,
                              const uint64_t* tb_capacity, const uint64_t* tb_refill_increment,
                              const uint64_t* tb_refill_interval_ns, const uint64_t* tb_last_refill) {
    return shd_outbound_setup_qdisc(ctx, n_hosts, first_host, capacity, SHD_QDISC_FIFO, 0, tb_capacity,
                                    tb_refill_increment, tb_refill_interval_ns, tb_last_refill);
}

shd_status shd_outbound_advance_sockets(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time,
                                        const uint64_t* d_prio, const uint64_t* d_sock, const uint32_t* d_size,
                                        const uint32_t* d_payload, const uint32_t* d_dst, const uint32_t* d_pkt,
                                        uint64_t n_offers, uint64_t window_end, uint64_t bootstrap_end,
                                        shd_batch* d_batch_out, const uint32_t** sent_pkt, const uint32_t** loc_off,
                                        const uint32_t** loc_pkt, const uint64_t** loc_time, uint64_t* n_local,
                                        uint64_t* n_stored, uint64_t* next_task_time) {
    if (!ctx) return SHD_ERR_INVALID;
    OutboundState& O = ctx->outb;
    if (!O.ready) return SHD_ERR_STATE;
    // argument errors: nothing has run, the stage stays as it was
    if (n_offers && (!d_off || !d_time || !d_prio || !d_size || !d_payload || !d_dst || !d_pkt)) return SHD_ERR_INVALID;
    if (n_offers && O.with_sockets() && !d_sock) return SHD_ERR_INVALID;   // (the plain disciplines never read it)
    if (n_offers && O.n_hosts == 0) return SHD_ERR_INVALID;
    if (window_end < O.prev_end) return SHD_ERR_INVALID;
    const uint64_t n_slots = n_offers + O.n_stored;   // every packet leaves at most once
    if (n_slots >= 0xFFFFFFFFull) return SHD_ERR_INVALID;
    hipStream_t s = ctx->stream;
    SHD_HIP(hipSetDevice(ctx->device));
    const size_t r1 = std::max<size_t>(n_slots, 1);
    SHD_TRY(O.r_pkt.ensure(r1 * 4));
    SHD_TRY(O.r_time.ensure(r1 * 8));
    SHD_TRY(O.r_dst.ensure(r1 * 4));
    SHD_TRY(O.r_pay.ensure(r1 * 4));
    SHD_TRY(O.r_size.ensure(r1 * 4));
    SHD_TRY(O.b_time.ensure(r1 * 8));
    SHD_TRY(O.b_dst.ensure(r1 * 4));
    SHD_TRY(O.b_pay.ensure(r1 * 4));
    SHD_TRY(O.b_pkt.ensure(r1 * 4));
    SHD_TRY(O.b_size.ensure(r1 * 4));
    SHD_TRY(O.l_pkt.ensure(r1 * 4));
    SHD_TRY(O.l_time.ensure(r1 * 8));
    unsigned long long* words = O.words.as<unsigned long long>();
    SHD_HIP(hipMemsetAsync(words, 0, 32, s));
    SHD_HIP(hipMemsetAsync(words + 4, 0xFF, 8, s));
    const uint32_t H = O.n_hosts;
    if (H) {
        uint32_t* cnt = O.cnt.as<uint32_t>();
        uint32_t* nsent = O.nsent.as<uint32_t>();
        uint32_t* nloc = O.nloc.as<uint32_t>();
        const uint32_t* off = d_off;   // (NULL: no offers; given with n_offers = 0 it must be all zero)
        outb_count<<<div_up((uint64_t)H + 1, 256), 256, 0, s>>>(H, off, n_offers, O.rl.as<OutRelay>(), cnt, nsent,
                                                                nloc, reinterpret_cast<uint32_t*>(words));
        SHD_HIP(hipGetLastError());
        SHD_TRY(scan_excl2(O.scan, cnt, cnt, nullptr, nullptr, (uint64_t)H + 1, s));   // -> region offsets
        // one kernel, two instances: the discipline is the queue policy alone
        auto run = [&](auto kernel, auto qa) {
            kernel<<<div_up(H, kOutLanes), kOutLanes, 0, s>>>(
                H, O.first_host, off, d_time, d_prio, d_size, d_payload, d_dst, d_pkt, qa, O.tb.as<TbRelay>(),
                O.rl.as<OutRelay>(), cnt, nsent, nloc, O.r_pkt.as<uint32_t>(), O.r_time.as<uint64_t>(),
                O.r_dst.as<uint32_t>(), O.r_pay.as<uint32_t>(), O.r_size.as<uint32_t>(), O.prev_end, window_end,
                bootstrap_end, words);
        };
        if (O.with_sockets()) {
            const OutFifoSock::Args qa{O.ring.as<SqSlot>(), O.socks.as<SqSock>(), d_sock, O.cap, O.max_sockets};
            if (O.qdisc == SHD_QDISC_FIFO_SOCKETS) run(outb_run<OutFifoSock>, qa);
            else run(outb_run<OutRrSock>, OutRrSock::Args{qa.pool_all, qa.socks_all, qa.sock, qa.cap, qa.max_sockets});
        } else if (O.qdisc == SHD_QDISC_ROUND_ROBIN)
            run(outb_run<OutRr>, OutRr::Args{O.ring.as<RrSlot>(), O.socks.as<RrSock>(), O.rr_words.as<uint2>(), O.cap,
                                             O.max_sockets});
        else
            run(outb_run<OutFifo>, OutFifo::Args{O.ring.as<OutPkt>(), O.cap});
        SHD_HIP(hipGetLastError());
        // the sent and the local counts per host, both in one launch -> src_off, loc_off
        SHD_TRY(scan_excl2(O.scan, nsent, O.src_off.as<uint32_t>(), nloc, O.loc_off.as<uint32_t>(), (uint64_t)H + 1, s));
        if (n_slots) {
            // (a thread per slot: the totals are known on the device only; the surplus threads leave at once)
            outb_compact<<<div_up(n_slots, 256), 256, 0, s>>>(
                n_slots, H, cnt, O.src_off.as<uint32_t>(), O.loc_off.as<uint32_t>(), O.r_pkt.as<uint32_t>(),
                O.r_time.as<uint64_t>(), O.r_dst.as<uint32_t>(), O.r_pay.as<uint32_t>(), O.r_size.as<uint32_t>(),
                O.b_time.as<uint64_t>(), O.b_dst.as<uint32_t>(), O.b_pay.as<uint32_t>(), O.b_pkt.as<uint32_t>(),
                O.b_size.as<uint32_t>(), O.l_pkt.as<uint32_t>(),
                O.l_time.as<uint64_t>());
            SHD_HIP(hipGetLastError());
        }
    }
    // status, the two record counts, the stored total and the earliest task in one pinned read
    SHD_TRY(readback(ctx, s, kOutPinWord, words, kOutWords * 8));
    const unsigned long long* w = ctx->h_pin + kOutPinWord;
    if ((uint32_t)w[0]) {
        // the window ran up to the offending offer on its host and in full elsewhere: the stage
        // now holds a state the reference never reaches -- shd_outbound_setup must run again
        O.ready = false;
        return SHD_ERR_INVALID;
    }
    O.n_stored = w[3];
    O.prev_end = window_end;
    O.advanced = true;
    if (d_batch_out) {
        d_batch_out->n_packets = w[1];
        d_batch_out->src_off = O.src_off.as<uint32_t>();
        d_batch_out->send_time = O.b_time.as<uint64_t>();
        d_batch_out->dst_host = O.b_dst.as<uint32_t>();
        d_batch_out->payload = O.b_pay.as<uint32_t>();
        d_batch_out->chance = nullptr;
    }
    if (sent_pkt) *sent_pkt = O.b_pkt.as<uint32_t>();
    if (loc_off) *loc_off = O.loc_off.as<uint32_t>();
    if (loc_pkt) *loc_pkt = O.l_pkt.as<uint32_t>();
    if (loc_time) *loc_time = O.l_time.as<uint64_t>();
    if (n_local) *n_local = w[2];
    if (n_stored) *n_stored = w[3];
    if (next_task_time) *next_task_time = w[4];
    return SHD_OK;
}

shd_status shd_outbound_advance(shd_ctx* ctx, const uint32_t* d_off, const uint64_t* d_time,
                                const uint64_t* d_prio, const uint32_t* d_size, const uint32_t* d_payload,
                                const uint32_t* d_dst, const uint32_t* d_pkt, uint64_t n_offers,
                                uint64_t window_end, uint64_t bootstrap_end, shd_batch* d_batch_out,
                                const uint32_t** sent_pkt, const uint32_t** loc_off, const uint32_t** loc_pkt,
                                const uint64_t** loc_time, uint64_t* n_local, uint64_t* n_stored,
                                uint64_t* next_task_time) {
    return shd_outbound_advance_sockets(ctx, d_off, d_time, d_prio, nullptr, d_size, d_payload, d_dst, d_pkt, n_offers,
                                        window_end, bootstrap_end, d_batch_out, sent_pkt, loc_off, loc_pkt, loc_time,
                                        n_local, n_stored, next_task_time);
}

shd_status shd_outbound_sent_sizes(shd_ctx* ctx, const uint32_t** d_size) {
    if (!ctx || !d_size) return SHD_ERR_INVALID;
    OutboundState& O = ctx->outb;
    if (!O.ready) return SHD_ERR_STATE;   // not set up, or a contract error since: as shd_outbound_get_state
    // (before the first advance the array is empty: the batch it belongs to has no entry)
    *d_size = O.advanced ? O.b_size.as<uint32_t>() : nullptr;
    return SHD_OK;
}

shd_status shd_outbound_get_state(shd_ctx* ctx, uint32_t host, uint64_t* task_time, uint32_t* has_cached,
                                  uint32_t* cached_pkt, uint32_t* cached_size, uint32_t* queue_len,
                                  uint32_t* head_pkt, shd_tb_state* bucket) {
    if (!ctx) return SHD_ERR_INVALID;
    OutboundState& O = ctx->outb;
    if (!O.ready) return SHD_ERR_STATE;   // not set up, or a contract error since: as the advance
    if (host >= O.n_hosts) return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    OutRelay r;
    SHD_HIP(hipMemcpy(&r, O.rl.as<OutRelay>() + host, sizeof(r), hipMemcpyDeviceToHost));
    if (task_time) *task_time = r.task;
    if (has_cached) *has_cached = r.has_cached;
    if (cached_pkt) *cached_pkt = r.has_cached ? r.cached_pkt : 0;
    if (cached_size) *cached_size = r.has_cached ? r.cached_size : 0;
    if (queue_len) *queue_len = r.count;
    if (head_pkt) {
        *head_pkt = r.count ? r.head_pkt : kOutNoPkt;
        if (O.with_sockets() && r.count && r.pad) {   // the head socket's entry, then its head packet's slot
            const bool fifo = O.qdisc == SHD_QDISC_FIFO_SOCKETS;
            SqQueue q;
            OutFifoSock::unpack(r, q);
            SqSock e;
            SqSlot p;
            SHD_HIP(hipMemcpy(&e, O.socks.as<SqSock>() + (size_t)host * O.max_sockets + sq_at(q, 0, O.max_sockets, fifo),
                              sizeof(e), hipMemcpyDeviceToHost));
            const uint32_t slot = e.cfirst != kSqNil ? e.cfirst : e.dfirst;
            if (slot >= O.cap) return SHD_ERR_STATE;   // (never after a window that returned SHD_OK)
            SHD_HIP(hipMemcpy(&p, O.ring.as<SqSlot>() + (size_t)host * O.cap + slot, sizeof(p), hipMemcpyDeviceToHost));
            *head_pkt = p.pkt;
        }
    }
    if (bucket) {
        TbRelay b;
        SHD_HIP(hipMemcpy(&b, O.tb.as<TbRelay>() + host, sizeof(b), hipMemcpyDeviceToHost));
        bucket->capacity = b.capacity;
        bucket->balance = b.balance;
        bucket->refill_increment = b.increment;
        bucket->refill_interval = b.interval;
        bucket->last_refill = b.last_refill;
        bucket->pending_until = r.task == kOutIdle ? 0 : r.task;   // the relay's task, as shd_tb_state names it
    }
    return SHD_OK;
}

shd_status shd_outbound_get_sockets(shd_ctx* ctx, uint32_t host, uint64_t* handles, uint32_t* counts, uint32_t cap,
                                    uint32_t* n_sockets) {
    if (!ctx) return SHD_ERR_INVALID;
    OutboundState& O = ctx->outb;
    if (!O.ready || O.qdisc == SHD_QDISC_FIFO) return SHD_ERR_STATE;   // (a plain FIFO stage keeps no sockets)
    if (host >= O.n_hosts || (cap && (!handles || !counts))) return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    if (O.with_sockets()) {   // the host's words, its pool and its socket array, listed by sock_queue.h
        OutRelay r;
        std::vector<SqSlot> pool(O.cap);
        std::vector<SqSock> socks(O.max_sockets);
        SHD_HIP(hipMemcpy(&r, O.rl.as<OutRelay>() + host, sizeof(r), hipMemcpyDeviceToHost));
        SHD_HIP(hipMemcpy(pool.data(), O.ring.as<SqSlot>() + (size_t)host * O.cap, pool.size() * sizeof(SqSlot),
                          hipMemcpyDeviceToHost));
        SHD_HIP(hipMemcpy(socks.data(), O.socks.as<SqSock>() + (size_t)host * O.max_sockets,
                          socks.size() * sizeof(SqSock), hipMemcpyDeviceToHost));
        SqQueue q;
        OutFifoSock::unpack(r, q);
        if (q.n_socks > O.max_sockets) return SHD_ERR_STATE;   // (never after a window that returned SHD_OK)
        const uint32_t n = sq_counts(q, pool.data(), O.cap, socks.data(), O.max_sockets,
                                     O.qdisc == SHD_QDISC_FIFO_SOCKETS, handles, counts, cap);
        if (n_sockets) *n_sockets = n;
        return SHD_OK;
    }
    // the host's words, its pool and its socket ring; the chains are walked here by rr_queue.h
    OutRelay r;
    uint2 w;
    std::vector<RrSlot> pool(O.cap);
    std::vector<RrSock> socks(O.max_sockets);
    SHD_HIP(hipMemcpy(&r, O.rl.as<OutRelay>() + host, sizeof(r), hipMemcpyDeviceToHost));
    SHD_HIP(hipMemcpy(&w, O.rr_words.as<uint2>() + host, sizeof(w), hipMemcpyDeviceToHost));
    SHD_HIP(hipMemcpy(pool.data(), O.ring.as<RrSlot>() + (size_t)host * O.cap, pool.size() * sizeof(RrSlot),
                      hipMemcpyDeviceToHost));
    SHD_HIP(hipMemcpy(socks.data(), O.socks.as<RrSock>() + (size_t)host * O.max_sockets,
                      socks.size() * sizeof(RrSock), hipMemcpyDeviceToHost));
    RrQueue q;
    OutRr::unpack(r, w, q);
    const uint32_t n = rr_counts(q, pool.data(), O.cap, socks.data(), O.max_sockets, handles, counts, cap);
    if (n_sockets) *n_sockets = n;
    return SHD_OK;
}

// the hosts' bw_up buckets re-rated at `at_time` (rate_update.hip): queues, sockets, the cached
// packet and the outstanding task stay
shd_status shd_outbound_update_buckets(shd_ctx* ctx, uint64_t n, const uint32_t* host, const uint64_t* capacity,
                                       const uint64_t* refill_increment, const uint64_t* refill_interval_ns,
                                       uint64_t at_time, uint32_t* err_host) {
    return rate_update(ctx, kRateOutbound, n, host, capacity, refill_increment, refill_interval_ns, at_time, err_host);
}

}  // extern "C"
