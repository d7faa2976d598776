// One host's round-robin queuing discipline (network_interface.c:235-273, :366-392;
// network_queuing_disciplines.c:29-88): the rrQueue, an ordered list of distinct sockets, each
// with the packets it has offered in offer order (socket.c:434-467; the separate control buffer of
// socket.c:467 is sock_queue.h's, for SHD_QDISC_ROUND_ROBIN_SOCKETS).  One set of functions for the kernel (outbound.hip) and for a
// program of its own (tests/rr_queue_main.cpp, built with the sanitizers): free of HIP.
//
//   offer   the packet goes behind its socket's packets; a socket that is not queued is pushed at
//           the tail (networkinterface_wantsSend: find, else push)
//   pop     the head socket's first packet; the socket goes to the tail if it has more, else it
//           leaves (_networkinterface_selectRoundRobin)
//
// Layout.  The head socket and its first packet -- what the next pop takes -- lie in the RrQueue
// words themselves, so a host whose queue goes 0 -> 1 -> 0 touches neither array.  Every other
// packet lies in a pool of `cap` slots per host, a socket's packets chained through `next`; free
// slots come from a bump count first and from a list threaded through `next` after that, so a
// setup writes no links.  The sockets behind the head one lie in a ring of `max_sockets` entries,
// in rrQueue order, each with the first and the last slot of its chain.  The pool never runs out
// before `cap` packets are queued (the head packet takes no slot) and the ring holds at most
// max_sockets - 1 sockets, so the socket that rotates always finds its entry free.
#pragma once
#include <stdint.h>

#include "shard.h"   // SHD_HOST_DEVICE

namespace shd {

constexpr uint32_t kRrNil = ~0u;   // no slot

struct RrSlot {   // 20 bytes: a queued packet behind its socket's first
    uint32_t pkt, size, payload, dst, next;
};

struct RrSock {   // 16 bytes: a queued socket behind the head one
    uint64_t handle;
    uint32_t first, last;   // its chain in the pool (never empty)
};

struct RrQueue {
    uint64_t handle;                    // the head socket (count >= 1)
    uint32_t pkt, size, payload, dst;   // its first packet
    uint32_t first, last;               // its further packets in the pool, kRrNil: none
    uint32_t count;                     // packets queued, this one included
    uint32_t ring_head, ring_count;     // the sockets behind the head one: ring[ring_head ...)
    uint32_t bump, free;                // the pool: slots never used yet start at bump; the free list
};

enum RrOffer : uint32_t { kRrOk = 0, kRrPoolFull = 1, kRrSocketsFull = 2 };

SHD_HOST_DEVICE inline void rr_init(RrQueue& q) {
    q.handle = 0;
    q.pkt = q.size = q.payload = q.dst = 0;
    q.first = q.last = kRrNil;
    q.count = q.ring_head = q.ring_count = q.bump = 0;
    q.free = kRrNil;
}

// sockets in the rrQueue
SHD_HOST_DEVICE inline uint32_t rr_sockets(const RrQueue& q) { return q.count ? 1u + q.ring_count : 0u; }

SHD_HOST_DEVICE inline uint32_t rr_wrap(uint32_t i, uint32_t n) { return i >= n ? i - n : i; }

// a slot for one more packet (the caller has checked count < cap: one is left)
SHD_HOST_DEVICE inline uint32_t rr_alloc(RrQueue& q, const RrSlot* pool) {
    if (q.free != kRrNil) {
        const uint32_t s = q.free;
        q.free = pool[s].next;
        return s;
    }
    return q.bump++;
}

// The ring entry that holds `handle`, kRrNil: none.  The handles are loaded four at a time
// (indices clamped into the live entries): one memory latency per four sockets, not one each.
SHD_HOST_DEVICE inline uint32_t rr_find(const RrQueue& q, const RrSock* ring, uint32_t max_sockets, uint64_t handle) {
    for (uint32_t i = 0; i < q.ring_count; i += 4) {
        uint32_t at[4];
        uint64_t hd[4];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t k = i + j < q.ring_count ? i + j : q.ring_count - 1;
            at[j] = rr_wrap(q.ring_head + k, max_sockets);
            hd[j] = ring[at[j]].handle;
        }
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < 4; ++j)
            if (hd[j] == handle) return at[j];   // (a clamped repeat names the same entry)
    }
    return kRrNil;
}

// networkinterface_wantsSend after the socket has taken the packet into its buffer.  Refused
// (nothing changed): `cap` packets are queued, or the socket would be the max_sockets + 1st.
SHD_HOST_DEVICE inline RrOffer rr_offer(RrQueue& q, RrSlot* pool, uint32_t cap, RrSock* ring, uint32_t max_sockets,
                                        uint64_t handle, uint32_t pkt, uint32_t size, uint32_t payload,
                                        uint32_t dst) {
    if (q.count >= cap) return kRrPoolFull;
    if (q.count == 0) {   // the socket becomes the head, its packet the next pop's
        q.handle = handle;
        q.pkt = pkt;
        q.size = size;
        q.payload = payload;
        q.dst = dst;
        q.first = q.last = kRrNil;
        q.count = 1;
        return kRrOk;
    }
    if (handle == q.handle) {   // find: the head socket
        const uint32_t s = rr_alloc(q, pool);
        pool[s] = RrSlot{pkt, size, payload, dst, kRrNil};
        if (q.first == kRrNil) q.first = s;
        else pool[q.last].next = s;
        q.last = s;
        ++q.count;
        return kRrOk;
    }
    const uint32_t at = rr_find(q, ring, max_sockets, handle);
    if (at == kRrNil && q.ring_count + 1 >= max_sockets) return kRrSocketsFull;
    const uint32_t s = rr_alloc(q, pool);
    pool[s] = RrSlot{pkt, size, payload, dst, kRrNil};
    if (at != kRrNil) {   // find: queued already
        pool[ring[at].last].next = s;
        ring[at].last = s;
    } else {              // push at the tail
        ring[rr_wrap(q.ring_head + q.ring_count, max_sockets)] = RrSock{handle, s, s};
        ++q.ring_count;
    }
    ++q.count;
    return kRrOk;
}

// the socket at ring_head becomes the head socket; its first packet moves into the words
SHD_HOST_DEVICE inline void rr_take_head(RrQueue& q, RrSlot* pool, const RrSock* ring, uint32_t max_sockets) {
    const RrSock s = ring[q.ring_head];
    q.ring_head = rr_wrap(q.ring_head + 1, max_sockets);
    const RrSlot p = pool[s.first];
    pool[s.first].next = q.free;
    q.free = s.first;
    q.handle = s.handle;
    q.pkt = p.pkt;
    q.size = p.size;
    q.payload = p.payload;
    q.dst = p.dst;
    q.first = p.next;
    q.last = p.next == kRrNil ? kRrNil : s.last;
}

// _networkinterface_selectRoundRobin (count >= 1): the head socket's first packet; the socket is
// pushed back at the tail if it has more to send, before the caller knows what becomes of the packet.
SHD_HOST_DEVICE inline void rr_pop(RrQueue& q, RrSlot* pool, RrSock* ring, uint32_t max_sockets, uint32_t& pkt,
                                   uint32_t& size, uint32_t& payload, uint32_t& dst) {
    pkt = q.pkt;
    size = q.size;
    payload = q.payload;
    dst = q.dst;
    --q.count;
    if (q.first != kRrNil) {
        if (q.ring_count == 0) {   // alone in the rrQueue: popped and pushed, the head again
            const RrSlot p = pool[q.first];
            pool[q.first].next = q.free;
            q.free = q.first;
            q.pkt = p.pkt;
            q.size = p.size;
            q.payload = p.payload;
            q.dst = p.dst;
            q.first = p.next;
            if (p.next == kRrNil) q.last = kRrNil;
        } else {                   // to the tail; the next socket moves up
            ring[rr_wrap(q.ring_head + q.ring_count, max_sockets)] = RrSock{q.handle, q.first, q.last};
            rr_take_head(q, pool, ring, max_sockets);
        }
    } else if (q.ring_count) {     // the socket leaves the rrQueue
        --q.ring_count;
        rr_take_head(q, pool, ring, max_sockets);
    }
}

// The rrQueue in order with each socket's queued packets, at most out_cap entries written;
// returns the sockets queued.  (A chain is walked for at most `cap` steps: a state the functions
// above left never needs more.)
SHD_HOST_DEVICE inline uint32_t rr_counts(const RrQueue& q, const RrSlot* pool, uint32_t cap, const RrSock* ring,
                                          uint32_t max_sockets, uint64_t* handles, uint32_t* counts,
                                          uint32_t out_cap) {
    const uint32_t n = rr_sockets(q);
    for (uint32_t i = 0; i < n && i < out_cap; ++i) {
        uint64_t hd = q.handle;
        uint32_t s = q.first, c = 1;
        if (i) {
            const RrSock& e = ring[rr_wrap(q.ring_head + (i - 1), max_sockets)];
            hd = e.handle;
            s = e.first;
            c = 0;
        }
        for (uint32_t steps = 0; s != kRrNil && s < cap && steps < cap; ++steps, ++c) s = pool[s].next;
        handles[i] = hd;
        counts[i] = c;
    }
    return n;
}

// Every queued packet, read-only: f(size, dst) for the head socket's first packet (the words), its
// further packets, then each socket of the ring with its chain.  Free slots lie on no chain and
// are not visited.  (At most `cap` slots are followed in all: a state the functions above left
// never needs more.)
template <class F>
SHD_HOST_DEVICE inline void rr_visit(const RrQueue& q, const RrSlot* pool, uint32_t cap, const RrSock* ring,
                                     uint32_t max_sockets, F&& f) {
    if (q.count == 0) return;
    f(q.size, q.dst);
    uint32_t steps = 0;
    for (uint32_t s = q.first; s != kRrNil && s < cap && steps < cap; ++steps) {
        f(pool[s].size, pool[s].dst);
        s = pool[s].next;
    }
    for (uint32_t i = 0; i < q.ring_count && i < max_sockets; ++i) {
        const RrSock& e = ring[rr_wrap(q.ring_head + i, max_sockets)];
        for (uint32_t s = e.first; s != kRrNil && s < cap && steps < cap; ++steps) {
            f(pool[s].size, pool[s].dst);
            s = pool[s].next;
        }
    }
}

}  // namespace shd
