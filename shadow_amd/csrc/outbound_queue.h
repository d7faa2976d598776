// The outbound stage's per-host words and its queuing disciplines: what outbound.hip (the advance)
// and rate_update.hip (the re-rate's walk over the stored packets) both compile.
#pragma once
#include <cstdint>

#include "common.h"
#include "rr_queue.h"
#include "sock_queue.h"

namespace shd {

constexpr uint64_t kOutIdle = ~0ull;   // no outstanding forward task
constexpr uint32_t kOutNoPkt = ~0u;    // not a packet id
// status bits (words[0]); any of them is SHD_ERR_INVALID
constexpr uint32_t kOutBadOff = 1u;     // offsets not monotone / not covering n_offers
constexpr uint32_t kOutBadTime = 2u;    // an offer before its predecessor (or the last window), or >= window_end
constexpr uint32_t kOutBadPkt = 4u;     // a non-local size above the bucket's capacity, or packet id UINT32_MAX
constexpr uint32_t kOutRingFull = 8u;
constexpr uint32_t kOutPanic = 16u;     // where the reference panics (token_bucket.rs unwraps)
constexpr uint32_t kOutSpin = 32u;      // the task budget ran out (unreachable under the input contract)
constexpr uint32_t kOutRegion = 64u;    // a record past the host's region (unreachable: one record per packet)
constexpr uint32_t kOutBadPrio = 128u;  // a priority equal to one still queued on the host (FIFO)
constexpr uint32_t kOutSockFull = 256u; // one socket more than max_sockets in a host's rrQueue (round-robin) or heap

struct OutPkt {   // 24 bytes: a queued packet
    uint64_t prio;
    uint32_t pkt, size, payload, dst;
};

struct OutRelay {   // 72 bytes per host
    uint64_t task;         // time of the outstanding forward task (RelayState::Pending), kOutIdle: Idle
    // The queue, `count` packets in increasing priority: the first (the one the next pop takes)
    // lies here, the other count - 1 in ring[head ...).  A host whose queue goes 0 -> 1 -> 0 --
    // every host that is not held back -- never touches its ring.
    uint64_t head_prio;
    uint64_t tail_prio;    // the largest priority queued (count >= 1): an offer above it is appended unread
    uint32_t head, count;
    uint32_t head_pkt, head_size, head_payload, head_dst;
    uint32_t has_cached, cached_pkt, cached_size, cached_payload, cached_dst, pad;   // RelayInternal::next_packet
};
static_assert(sizeof(OutRelay) == 72, "OutRelay layout");

// The queuing discipline behind outb_run (configuration.rs:396-397, QDiscMode): what an offer
// does to the host's queue and which packet a pop takes.  Everything else -- the merge with the
// forward task, the cached packet, the bucket, the records -- is the kernel's, once.  A policy is
// built per lane from the kernel's arguments and the host's relay words; insert returns status
// bits (0: taken), pop needs R.count >= 1, store puts the policy's own words back.  Both keep
// R.count (packets queued) and R.head_* (the packet the next pop takes) current:
// shd_outbound_get_state and outb_count read them for either discipline.  visit (read-only, the
// re-rate's: rate_update.hip) calls f(size, dst) for every packet queued, in no promised order.

// FIFO (network_interface.c:276-316): the lowest priority queued, a sorted ring per host.
struct OutFifo {
    struct Args {
        OutPkt* ring_all;
        uint32_t cap;
    };
    OutPkt* ring;
    uint32_t cap;
    __device__ __forceinline__ OutFifo(const Args& a, uint32_t h, const OutRelay&)
        : ring(a.ring_all + (size_t)h * a.cap), cap(a.cap) {}
    __device__ __forceinline__ uint32_t insert(OutRelay& R, const OutPkt& e) {
        if (R.count == cap) return kOutRingFull;
        if (R.count == 0) {
            R.head_prio = e.prio;
            R.head_pkt = e.pkt;
            R.head_size = e.size;
            R.head_payload = e.payload;
            R.head_dst = e.dst;
            R.tail_prio = e.prio;
        } else if (e.prio == R.head_prio || e.prio == R.tail_prio) {
            return kOutBadPrio;
        } else if (e.prio < R.head_prio) {   // the new first packet: the old one goes in front of the ring
            R.head = R.head == 0 ? cap - 1 : R.head - 1;
            ring[R.head] = OutPkt{R.head_prio, R.head_pkt, R.head_size, R.head_payload, R.head_dst};
            R.head_prio = e.prio;
            R.head_pkt = e.pkt;
            R.head_size = e.size;
            R.head_payload = e.payload;
            R.head_dst = e.dst;
        } else {
            // behind the ring's last packet; the priorities in arrival order (e.prio above
            // tail_prio) append without a read, any other shifts the larger ones up.  The
            // shift stops inside the ring at the latest at its start: e.prio > head_prio.
            uint32_t pos = R.count - 1;   // packets in the ring
            if (e.prio > R.tail_prio) {
                R.tail_prio = e.prio;
            } else {
                bool dup = false;
                while (pos > 0) {
                    uint32_t j = R.head + pos - 1;
                    if (j >= cap) j -= cap;
                    const OutPkt q = ring[j];
                    if (q.prio <= e.prio) {
                        dup = q.prio == e.prio;   // where the shift stopped
                        break;
                    }
                    uint32_t j1 = j + 1;
                    if (j1 == cap) j1 = 0;
                    ring[j1] = q;
                    --pos;
                }
                if (dup) return kOutBadPrio;
            }
            uint32_t j = R.head + pos;
            if (j >= cap) j -= cap;
            ring[j] = e;
        }
        ++R.count;
        return 0;
    }
    __device__ __forceinline__ void pop(OutRelay& R, uint32_t& p_, uint32_t& s_, uint32_t& pl_, uint32_t& d_) {
        p_ = R.head_pkt;           // the lowest priority queued
        s_ = R.head_size;
        pl_ = R.head_payload;
        d_ = R.head_dst;
        if (--R.count) {           // the next one moves up from the ring
            const OutPkt q = ring[R.head];
            R.head = R.head + 1 == cap ? 0 : R.head + 1;
            R.head_prio = q.prio;
            R.head_pkt = q.pkt;
            R.head_size = q.size;
            R.head_payload = q.payload;
            R.head_dst = q.dst;
        }
    }
    __device__ __forceinline__ void store(OutRelay&) {}
    // the head packet in the relay words, then the count - 1 packets of the ring
    template <class F>
    static __device__ __forceinline__ void visit(const Args& a, uint32_t h, const OutRelay& R, F&& f) {
        if (R.count == 0) return;
        f(R.head_size, R.head_dst);
        const OutPkt* ring = a.ring_all + (size_t)h * a.cap;
        const uint32_t n = min(R.count, a.cap) - 1;
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t j = R.head + i;
            if (j >= a.cap) j -= a.cap;
            const OutPkt q = ring[j];
            f(q.size, q.dst);
        }
    }
};

// Round-robin (network_interface.c:235-273): rr_queue.h's queue, the functions
// tests/rr_queue_main.cpp compiles.  The offer's 64-bit key is the socket's canonical handle.  The
// queue's words live in the relay words the FIFO form uses for its own -- head_prio: the head
// socket's handle; head_*: its first packet; tail_prio: the first and last slot of its further
// packets; head, pad: the socket ring's start and length -- so outb_count and
// shd_outbound_get_state serve both; the pool's two words (bump count, free list) lie in an array
// of their own.
struct OutRr {
    struct Args {
        RrSlot* pool_all;
        RrSock* socks_all;
        uint2* words_all;
        uint32_t cap, max_sockets;
    };
    RrQueue q;
    RrSlot* pool;
    RrSock* socks;
    uint2* pw;
    uint32_t cap, max_sockets;
    static __host__ __device__ __forceinline__ void unpack(const OutRelay& R, uint2 w, RrQueue& q) {
        q.handle = R.head_prio;
        q.pkt = R.head_pkt;
        q.size = R.head_size;
        q.payload = R.head_payload;
        q.dst = R.head_dst;
        q.first = (uint32_t)R.tail_prio;
        q.last = (uint32_t)(R.tail_prio >> 32);
        q.count = R.count;
        q.ring_head = R.head;
        q.ring_count = R.pad;
        q.bump = w.x;
        q.free = w.y;
    }
    __device__ __forceinline__ OutRr(const Args& a, uint32_t h, const OutRelay& R)
        : pool(a.pool_all + (size_t)h * a.cap), socks(a.socks_all + (size_t)h * a.max_sockets),
          pw(a.words_all + h), cap(a.cap), max_sockets(a.max_sockets) {
        unpack(R, *pw, q);
    }
    __device__ __forceinline__ uint32_t insert(OutRelay& R, const OutPkt& e) {
        const RrOffer o = rr_offer(q, pool, cap, socks, max_sockets, e.prio, e.pkt, e.size, e.payload, e.dst);
        if (o != kRrOk) return o == kRrPoolFull ? kOutRingFull : kOutSockFull;
        R.count = q.count;   // (the one word the kernel's own code reads between the calls)
        return 0;
    }
    __device__ __forceinline__ void pop(OutRelay& R, uint32_t& p_, uint32_t& s_, uint32_t& pl_, uint32_t& d_) {
        rr_pop(q, pool, socks, max_sockets, p_, s_, pl_, d_);
        R.count = q.count;
    }
    __device__ __forceinline__ void store(OutRelay& R) {
        R.count = q.count;
        R.head_pkt = q.pkt;
        R.head_size = q.size;
        R.head_payload = q.payload;
        R.head_dst = q.dst;
        R.head_prio = q.handle;
        R.tail_prio = (uint64_t)q.first | ((uint64_t)q.last << 32);
        R.head = q.ring_head;
        R.pad = q.ring_count;
        *pw = make_uint2(q.bump, q.free);
    }
    // rr_visit over the host's words, pool and socket ring (the pool's two words are not needed)
    template <class F>
    static __device__ __forceinline__ void visit(const Args& a, uint32_t h, const OutRelay& R, F&& f) {
        if (R.count == 0) return;
        RrQueue q;
        unpack(R, make_uint2(0, kRrNil), q);
        rr_visit(q, a.pool_all + (size_t)h * a.cap, a.cap, a.socks_all + (size_t)h * a.max_sockets, a.max_sockets, f);
    }
};

// The two disciplines over sockets with both buffers of socket.c (SHD_QDISC_FIFO_SOCKETS,
// SHD_QDISC_ROUND_ROBIN_SOCKETS): sock_queue.h's queue, the functions tests/sock_queue_main.cpp
// compiles.  An offer has two keys, the packet's priority (0: a control packet) and the offering
// socket's canonical handle, a column of its own (Args::sock); priorities need not be unique.  The
// queue's words live in the relay words -- count: the packets queued; pad: the entries in the
// socket array (0 with count 1: the one packet lies in head_prio (its socket), tail_prio (its
// priority) and head_*); otherwise head: the rrQueue's start, tail_prio: the pool's bump count and
// free list -- so outb_count serves all four.  R.head_pkt is current only for a queue of one:
// shd_outbound_get_state reads the arrays.
template <bool kFifo>
struct OutSock {
    struct Args {
        SqSlot* pool_all;
        SqSock* socks_all;
        const uint64_t* sock;   // the offers' socket column
        uint32_t cap, max_sockets;
    };
    SqQueue q;
    SqSlot* pool;
    SqSock* socks;
    uint32_t cap, max_sockets;
    static __host__ __device__ __forceinline__ void unpack(const OutRelay& R, SqQueue& q) {
        q.count = R.count;
        q.n_socks = R.pad;
        q.ring_head = R.head;
        q.pkt = R.head_pkt;
        q.size = R.head_size;
        q.payload = R.head_payload;
        q.dst = R.head_dst;
        if (R.pad) {
            q.handle = q.prio = 0;
            q.bump = (uint32_t)R.tail_prio;
            q.free = (uint32_t)(R.tail_prio >> 32);
        } else {
            q.handle = R.head_prio;
            q.prio = R.tail_prio;
            q.bump = 0;
            q.free = kSqNil;
        }
    }
    __device__ __forceinline__ OutSock(const Args& a, uint32_t h, const OutRelay& R)
        : pool(a.pool_all + (size_t)h * a.cap), socks(a.socks_all + (size_t)h * a.max_sockets), cap(a.cap),
          max_sockets(a.max_sockets) {
        unpack(R, q);
    }
    __device__ __forceinline__ uint32_t insert(OutRelay& R, const OutPkt& e, uint64_t handle) {
        const SqOffer o = sq_offer(q, pool, cap, socks, max_sockets, kFifo, handle, e.prio, e.pkt, e.size, e.payload, e.dst);
        if (o != kSqOk) return o == kSqPoolFull ? kOutRingFull : kOutSockFull;
        R.count = q.count;   // (the one word the kernel's own code reads between the calls)
        return 0;
    }
    __device__ __forceinline__ void pop(OutRelay& R, uint32_t& p_, uint32_t& s_, uint32_t& pl_, uint32_t& d_) {
        sq_pop(q, pool, socks, max_sockets, kFifo, p_, s_, pl_, d_);
        R.count = q.count;
    }
    __device__ __forceinline__ void store(OutRelay& R) {
        R.count = q.count;
        R.pad = q.n_socks;
        R.head = q.ring_head;
        R.head_pkt = q.pkt;
        R.head_size = q.size;
        R.head_payload = q.payload;
        R.head_dst = q.dst;
        if (q.n_socks) {
            R.head_prio = 0;
            R.tail_prio = (uint64_t)q.bump | ((uint64_t)q.free << 32);
        } else {
            R.head_prio = q.handle;
            R.tail_prio = q.prio;
        }
    }
    // sq_visit over the host's words, pool and socket array
    template <class F>
    static __device__ __forceinline__ void visit(const Args& a, uint32_t h, const OutRelay& R, F&& f) {
        if (R.count == 0) return;
        SqQueue q;
        unpack(R, q);
        sq_visit(q, a.pool_all + (size_t)h * a.cap, a.cap, a.socks_all + (size_t)h * a.max_sockets, a.max_sockets,
                 kFifo, f);
    }
};
using OutFifoSock = OutSock<true>;
using OutRrSock = OutSock<false>;

// a discipline whose offers carry the socket column beside the priority
template <class Q> struct OutHasSock { static constexpr bool value = false; };
template <bool kFifo> struct OutHasSock<OutSock<kFifo>> { static constexpr bool value = true; };

}  // namespace shd
