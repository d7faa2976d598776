// One host's sockets as the reference's interface sees them, with both output buffers of
// socket.c, under either queuing discipline.  One set of functions for the kernel (outbound.hip,
// OutFifoSock and OutRrSock) and for a program of its own (tests/sock_queue_main.cpp, built with
// the sanitizers): free of HIP.
//
//   socket.c:432-437   a packet of priority 0 goes to the socket's outputControlBuffer, every
//                      other one to its outputBuffer; tcp.c:947-963 gives priority 0 to every
//                      control packet (pure ACK, SYN, FIN), and the host's counter starts at 1
//   socket.c:182-189, :466-467   peek and pull take the control buffer first
//   network_interface.c:366-392  wantsSend, after the socket has taken the packet: a socket that
//                      is not queued is pushed
//   FIFO (fifo = true)   network_interface.c:276-316 over the array heap of priority_queue.c
//                      :87-140, :189-208, compared by network_queuing_disciplines.c:90-102:
//                      smaller(i, j) = !(key(i) > key(j)), key = the socket's head priority NOW, a
//                      tie "smaller" both ways.  Push appends and sifts up; pop swaps the root with
//                      the last entry, shrinks, sifts down from 0 (the right child when
//                      smaller(right, left)), pulls the root socket's head packet and pushes the
//                      socket again if it still has data.  A control packet offered to a socket
//                      that is in the heap changes its key where it stands: nothing is re-heapified,
//                      so the send order is a function of the array, not "lowest priority first".
//   round-robin (fifo = false)   network_interface.c:235-273: rr_queue.h's rotation, the pull
//                      taking the control buffer first.
//
// Layout.  `socks` holds the queued sockets -- exactly those with a packet -- as 32-byte entries:
// under FIFO the heap array itself, entry i at socks[i]; under round-robin a ring of max_sockets
// entries that starts at ring_head.  An entry has the handle, the first and last slot of its
// control and of its data list, and its key: 0 while the control list is non-empty, else the data
// head's priority.  The only key change outside a pop is "control offered to a socket whose
// control list was empty".  Packets lie in a pool of `cap` 32-byte slots per host, chained through
// `next`; free slots come from a bump count first and from a list threaded through `next` after
// that, and an empty queue starts its pool over.  A queue of one packet keeps it in the SqQueue
// words (n_socks = 0, count = 1): a host whose queue goes 0 -> 1 -> 0 touches neither array; a
// second offer moves that packet into slot 0 and its socket into entry 0 first.  Every loop is
// bounded by max_sockets (the find), log2(max_sockets) (the sifts) or cap (the listing).
#pragma once
#include <stdint.h>

#include "shard.h"   // SHD_HOST_DEVICE

namespace shd {

constexpr uint32_t kSqNil = ~0u;   // no slot, no entry

struct SqSlot {   // 32 bytes: a queued packet
    uint64_t prio;
    uint32_t pkt, size, payload, dst, next, pad;
};

struct SqSock {   // 32 bytes: a queued socket
    uint64_t handle;
    uint64_t key;                              // what the heap compares: its head priority
    uint32_t cfirst, clast, dfirst, dlast;     // control list, data list; kSqNil: empty
};

struct SqQueue {
    uint64_t handle, prio;              // the one packet of a queue that holds one (n_socks == 0)
    uint32_t pkt, size, payload, dst;
    uint32_t count;                     // packets queued
    uint32_t n_socks;                   // entries in socks
    uint32_t ring_head;                 // round-robin: the head socket's entry
    uint32_t bump, free;                // the pool: slots never used yet start at bump; the free list
};

enum SqOffer : uint32_t { kSqOk = 0, kSqPoolFull = 1, kSqSocketsFull = 2 };

SHD_HOST_DEVICE inline void sq_init(SqQueue& q) {
    q.handle = q.prio = 0;
    q.pkt = q.size = q.payload = q.dst = 0;
    q.count = q.n_socks = q.ring_head = q.bump = 0;
    q.free = kSqNil;
}

// sockets queued
SHD_HOST_DEVICE inline uint32_t sq_sockets(const SqQueue& q) { return q.n_socks ? q.n_socks : (q.count ? 1u : 0u); }

// where the i-th socket (heap index, or place in the rotation) lies, i < n_socks <= max_sockets
SHD_HOST_DEVICE inline uint32_t sq_at(const SqQueue& q, uint32_t i, uint32_t max_sockets, bool fifo) {
    if (fifo) return i;
    const uint32_t j = q.ring_head + i;
    return j >= max_sockets ? j - max_sockets : j;
}

// a slot for one more packet (the caller has checked count < cap: one is left)
SHD_HOST_DEVICE inline uint32_t sq_alloc(SqQueue& q, const SqSlot* pool) {
    if (q.free != kSqNil) {
        const uint32_t s = q.free;
        q.free = pool[s].next;
        return s;
    }
    return q.bump++;
}

// the entry that holds `handle`, kSqNil: none
SHD_HOST_DEVICE inline uint32_t sq_find(const SqQueue& q, const SqSock* socks, uint32_t max_sockets, bool fifo,
                                        uint64_t handle) {
    for (uint32_t i = 0; i < q.n_socks; ++i) {
        const uint32_t at = sq_at(q, i, max_sockets, fifo);
        if (socks[at].handle == handle) return at;
    }
    return kSqNil;
}

// priorityqueue_push of a socket that is not queued (FIFO: append, sift up while
// smaller(index, parent)), rrsocketqueue_push (round-robin: the tail)
SHD_HOST_DEVICE inline void sq_push(SqQueue& q, SqSock* socks, uint32_t max_sockets, bool fifo, const SqSock& e) {
    uint32_t idx = q.n_socks++;
    if (!fifo) {
        socks[sq_at(q, idx, max_sockets, false)] = e;
        return;
    }
    while (idx > 0) {
        const uint32_t par = (idx - 1) / 2;
        const SqSock p = socks[par];
        if (e.key > p.key) break;   // not smaller(index, parent)
        socks[idx] = p;
        idx = par;
    }
    socks[idx] = e;
}

// priorityqueue_pop (FIFO) / rrsocketqueue_pop: the socket leaves, n_socks >= 1
SHD_HOST_DEVICE inline SqSock sq_pop_sock(SqQueue& q, SqSock* socks, uint32_t max_sockets, bool fifo) {
    if (!fifo) {
        const SqSock r = socks[q.ring_head];
        q.ring_head = q.ring_head + 1 >= max_sockets ? 0 : q.ring_head + 1;
        --q.n_socks;
        return r;
    }
    const SqSock r = socks[0];
    const uint32_t n = --q.n_socks;
    if (n) {   // the last entry takes the root's place and sifts down over the n left
        // (entry n stays where it is until its place is known: only its key is held over the loop)
        const uint64_t last_key = socks[n].key;
        uint32_t idx = 0;
        for (;;) {
            uint32_t child = 2 * idx + 1;
            if (child >= n) break;
            uint64_t key = socks[child].key;
            if (child + 1 < n) {
                const uint64_t right = socks[child + 1].key;
                if (!(right > key)) {   // smaller(right, left)
                    key = right;
                    ++child;
                }
            }
            if (key > last_key) break;   // not smaller(child, index)
            socks[idx] = socks[child];
            idx = child;
        }
        socks[idx] = socks[n];
    }
    return r;
}

// networkinterface_wantsSend after the socket has taken the packet into the buffer its priority
// names.  Refused (nothing changed): `cap` packets are queued, or the socket would be the
// max_sockets + 1st.
SHD_HOST_DEVICE inline SqOffer sq_offer(SqQueue& q, SqSlot* pool, uint32_t cap, SqSock* socks, uint32_t max_sockets,
                                        bool fifo, uint64_t handle, uint64_t prio, uint32_t pkt, uint32_t size,
                                        uint32_t payload, uint32_t dst) {
    if (q.count >= cap) return kSqPoolFull;
    if (q.count == 0) {   // the one packet of the queue: in the words
        q.handle = handle;
        q.prio = prio;
        q.pkt = pkt;
        q.size = size;
        q.payload = payload;
        q.dst = dst;
        q.count = 1;
        q.n_socks = 0;
        return kSqOk;
    }
    if (q.n_socks == 0) {   // a second packet: the first moves into the arrays (the pool is unused: slot 0)
        if (handle != q.handle && max_sockets < 2) return kSqSocketsFull;
        q.bump = 1;
        q.free = kSqNil;
        pool[0] = SqSlot{q.prio, q.pkt, q.size, q.payload, q.dst, kSqNil, 0};
        const bool c0 = q.prio == 0;
        socks[0] = SqSock{q.handle, q.prio, c0 ? 0u : kSqNil, c0 ? 0u : kSqNil, c0 ? kSqNil : 0u, c0 ? kSqNil : 0u};
        q.ring_head = 0;
        q.n_socks = 1;
    }
    const uint32_t at = sq_find(q, socks, max_sockets, fifo, handle);
    if (at == kSqNil && q.n_socks >= max_sockets) return kSqSocketsFull;
    const uint32_t s = sq_alloc(q, pool);
    pool[s] = SqSlot{prio, pkt, size, payload, dst, kSqNil, 0};
    const bool control = prio == 0;
    if (at != kSqNil) {   // queued already: the packet goes behind its list, the entry stays where it is
        SqSock e = socks[at];
        if (control) {
            if (e.cfirst == kSqNil) {
                e.cfirst = s;
                e.key = 0;   // the head is a control packet now: the key changes in place
            } else {
                pool[e.clast].next = s;
            }
            e.clast = s;
        } else {
            if (e.dfirst == kSqNil) e.dfirst = s;   // (the control list is non-empty: the key stays 0)
            else pool[e.dlast].next = s;
            e.dlast = s;
        }
        socks[at] = e;
    } else {
        sq_push(q, socks, max_sockets, fifo,
                SqSock{handle, prio, control ? s : kSqNil, control ? s : kSqNil, control ? kSqNil : s,
                       control ? kSqNil : s});
    }
    ++q.count;
    return kSqOk;
}

// _networkinterface_selectFirstInFirstOut / _networkinterface_selectRoundRobin (count >= 1): pop the
// socket, pull its head packet (control first), push the socket again if it still has data --
// before the caller knows what becomes of the packet.
SHD_HOST_DEVICE inline void sq_pop(SqQueue& q, SqSlot* pool, SqSock* socks, uint32_t max_sockets, bool fifo,
                                   uint32_t& pkt, uint32_t& size, uint32_t& payload, uint32_t& dst) {
    if (q.n_socks == 0) {   // the one packet in the words
        pkt = q.pkt;
        size = q.size;
        payload = q.payload;
        dst = q.dst;
        q.count = 0;
        return;
    }
    SqSock r = sq_pop_sock(q, socks, max_sockets, fifo);
    const bool control = r.cfirst != kSqNil;
    const uint32_t s = control ? r.cfirst : r.dfirst;
    const SqSlot p = pool[s];
    if (control) {
        r.cfirst = p.next;
        if (p.next == kSqNil) r.clast = kSqNil;
    } else {
        r.dfirst = p.next;
        if (p.next == kSqNil) r.dlast = kSqNil;
    }
    pkt = p.pkt;
    size = p.size;
    payload = p.payload;
    dst = p.dst;
    pool[s].next = q.free;
    q.free = s;
    if (--q.count == 0) {   // (the socket has left: n_socks is 0) the pool starts over
        q.bump = 0;
        q.free = kSqNil;
        return;
    }
    if (r.cfirst != kSqNil) {
        r.key = 0;
        sq_push(q, socks, max_sockets, fifo, r);
    } else if (r.dfirst != kSqNil) {
        r.key = pool[r.dfirst].prio;
        sq_push(q, socks, max_sockets, fifo, r);
    }
}

// the packet the next pop takes (count >= 1)
SHD_HOST_DEVICE inline uint32_t sq_head_pkt(const SqQueue& q, const SqSlot* pool, const SqSock* socks,
                                            uint32_t max_sockets, bool fifo) {
    if (q.n_socks == 0) return q.pkt;
    const SqSock& r = socks[sq_at(q, 0, max_sockets, fifo)];
    return pool[r.cfirst != kSqNil ? r.cfirst : r.dfirst].pkt;
}

// The queued sockets -- FIFO: the heap array in index order; round-robin: rrQueue order -- each
// with its queued packets, control plus data; at most out_cap entries written; returns the sockets
// queued.  (A list is walked for at most `cap` steps: a state the functions above left never
// needs more.)
SHD_HOST_DEVICE inline uint32_t sq_counts(const SqQueue& q, const SqSlot* pool, uint32_t cap, const SqSock* socks,
                                          uint32_t max_sockets, bool fifo, uint64_t* handles, uint32_t* counts,
                                          uint32_t out_cap) {
    const uint32_t n = sq_sockets(q);
    if (q.n_socks == 0) {
        if (n && out_cap) {
            handles[0] = q.handle;
            counts[0] = 1;
        }
        return n;
    }
    for (uint32_t i = 0; i < n && i < out_cap; ++i) {
        const SqSock& e = socks[sq_at(q, i, max_sockets, fifo)];
        uint32_t c = 0, steps = 0;
        for (uint32_t s = e.cfirst; s != kSqNil && s < cap && steps < cap; ++steps, ++c) s = pool[s].next;
        for (uint32_t s = e.dfirst; s != kSqNil && s < cap && steps < cap; ++steps, ++c) s = pool[s].next;
        handles[i] = e.handle;
        counts[i] = c;
    }
    return n;
}

// Every queued packet, read-only: f(size, dst) for the one packet in the words (n_socks == 0), else
// for each queued socket's control list and data list.  Free slots lie on no list and are not
// visited.  (At most `cap` slots are followed in all: a state the functions above left never needs
// more.)
template <class F>
SHD_HOST_DEVICE inline void sq_visit(const SqQueue& q, const SqSlot* pool, uint32_t cap, const SqSock* socks,
                                     uint32_t max_sockets, bool fifo, F&& f) {
    if (q.count == 0) return;
    if (q.n_socks == 0) {
        f(q.size, q.dst);
        return;
    }
    uint32_t steps = 0;
    for (uint32_t i = 0; i < q.n_socks && i < max_sockets; ++i) {
        const SqSock& e = socks[sq_at(q, i, max_sockets, fifo)];
        for (uint32_t s = e.cfirst; s != kSqNil && s < cap && steps < cap; ++steps) {
            f(pool[s].size, pool[s].dst);
            s = pool[s].next;
        }
        for (uint32_t s = e.dfirst; s != kSqNil && s < cap && steps < cap; ++steps) {
            f(pool[s].size, pool[s].dst);
            s = pool[s].next;
        }
    }
}

}  // namespace shd
