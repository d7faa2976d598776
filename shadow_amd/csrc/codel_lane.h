// One host's CoDel queue as a lane's state machine: the device code codel.hip (operation replay)
// and inbound.hip (the inbound stage) both compile.
//
// Reference semantics: src/main/network/router/codel_queue.rs (FlyearthR/shadow)
//   :19-33   TARGET 10 ms, INTERVAL 100 ms, LIMIT usize::MAX; CONFIG_MTU 1500 (definitions.h:124)
//   :125-147 pop: codel_pop, then store mode / drop_from_store_mode / drop_from_drop_mode
//   :149-198 the two drop paths (control law reset with delta, repeated drops)
//   :201-255 codel_pop (RFC 8289 dodequeue) and process_standing_delay (interval_end)
//   :258-300 should_drop, was_dropping_recently (16 intervals), apply_control_law
//            time + round(INTERVAL / sqrt(count)) in f64 (round half away from zero)
// Time types (emulated_time.rs, simulation_time.rs): interval_end = now.saturating_add(INTERVAL)
// is EmulatedTime's and stops at EMUTIME_MAX; the standing delay and was_dropping_recently are
// saturating_duration_since, 0 when the earlier time is later and when the difference is above
// SIMTIME_MAX.  The control law goes through to_abs_simtime (a panic for a time before
// SIMULATION_START) and SimulationTime::saturating_add, whose u64 sum cannot overflow here, so a
// sum above SIMTIME_MAX -- a drop time past EMUTIME_MAX -- meets its unwrap: a panic, not a
// saturation.  Both set kCodelPanic in the lane's flags (a bit of a word the lane holds in a vector
// register anyway: a flag of its own is a lane mask in scalar registers, and inb_run had none to
// spare); the caller reports it and keeps it out of the stored flags.
//   :291-306 push (never full: LIMIT is unbounded)
// The host's packets in the queue live in a per-host ring of `cap` entries; a push beyond it is
// refused (the caller reports it) instead of growing, the one deviation from the unbounded VecDeque.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.h"
#include "time_limits.h"

namespace shd {

constexpr uint64_t kTarget = 10000000ull;
constexpr uint64_t kInterval = 100000000ull;
constexpr uint64_t kMtu = 1500;
constexpr uint32_t kPop = 0xFFFFFFFFu;
constexpr uint32_t kHasIntervalEnd = 1u, kHasDropNext = 2u, kModeDrop = 4u;
constexpr uint32_t kCodelPanic = 8u;   // lane-local: where the reference panics (never stored)

struct CodelHost {   // 48 bytes per host
    uint64_t interval_end, drop_next, cur, prev, total;
    uint32_t head, count;
};

// usize::saturating_sub (the byte total, the drop counts); no time goes through it
__device__ __forceinline__ uint64_t sat_sub(uint64_t a, uint64_t b) { return a > b ? a - b : 0ull; }
// EmulatedTime::saturating_add of INTERVAL (emulated_time.rs:95-108)
__device__ __forceinline__ uint64_t codel_interval_end(uint64_t now) {
    return now > kEmutimeMax - kInterval ? kEmutimeMax : now + kInterval;   // (one compare: u64 overflow included)
}
// EmulatedTime::saturating_duration_since (emulated_time.rs:84-93)
__device__ __forceinline__ uint64_t sat_duration_since(uint64_t later, uint64_t earlier) {
    const uint64_t d = later < earlier ? 0ull : later - earlier;
    return d > kSimtimeMax ? 0ull : d;   // (two selects in a row: no lane mask is kept)
}

__device__ __forceinline__ uint64_t control_law(uint64_t t, uint64_t count, uint32_t& flags) {
    // IEEE f64 sqrt and division (correctly rounded on gfx950), as Rust's f64 ops
    const double sq = count == 0 ? 1.0 : sqrt((double)count);
    const double div = (double)kInterval / sq;
    const uint64_t inc = (uint64_t)round(div);   // Rust f64::round: half away from zero; <= 1e8
    // to_abs_simtime's and SimulationTime::saturating_add's unwraps (codel_queue.rs:297-299)
    // one compare for both: t - kSimStart wraps to at least kSimtimeMax + 2 for a t before the start
    flags |= t - kSimStart > kSimtimeMax - inc ? kCodelPanic : 0u;
    return t + inc;
}

// Sink: where a packet that leaves the queue is recorded -- mark(pkt, op, kind), kind 1 dequeued
// (the caller's), 2 dropped (pop's own, in drop order, before the packet the pop returns).
template <class Sink>
struct CodelLane {
    CodelHost s;
    uint32_t flags;
    uint4* ring;   // {pkt, size, ts lo, ts hi}
    uint32_t cap;
    Sink sink;

    // push (codel_queue.rs:291-306); false when the ring is full (nothing is stored)
    __device__ bool push(uint32_t pkt, uint32_t size, uint64_t now) {
        if (s.count == cap) return false;
        uint32_t tail = s.head + s.count;
        if (tail >= cap) tail -= cap;
        ring[tail] = make_uint4(pkt, size, (uint32_t)now, (uint32_t)(now >> 32));
        ++s.count;
        s.total += size;
        return true;
    }
    // codel_pop (dodequeue): returns false when the queue is empty
    __device__ bool codel_pop(uint64_t now, uint32_t* pkt, uint32_t* size, bool* ok_to_drop) {
        if (s.count == 0) {
            flags &= ~kHasIntervalEnd;
            return false;
        }
        const uint4 e = ring[s.head];
        s.head = s.head + 1 == cap ? 0 : s.head + 1;
        --s.count;
        s.total = sat_sub(s.total, e.y);
        const uint64_t ts = ((uint64_t)e.w << 32) | e.z;
        const uint64_t standing = sat_duration_since(now, ts);
        *pkt = e.x;
        *size = e.y;
        if (standing < kTarget || s.total <= kMtu) {   // process_standing_delay
            flags &= ~kHasIntervalEnd;
            *ok_to_drop = false;
        } else if (flags & kHasIntervalEnd) {
            *ok_to_drop = now >= s.interval_end;
        } else {
            s.interval_end = codel_interval_end(now);
            flags |= kHasIntervalEnd;
            *ok_to_drop = false;
        }
        return true;
    }
    __device__ bool should_drop(uint64_t now) const { return (flags & kHasDropNext) && now >= s.drop_next; }
    __device__ bool dropping_recently(uint64_t now) const {
        return (flags & kHasDropNext) && sat_duration_since(now, s.drop_next) < kInterval * 16;
    }
    // pop (codel_queue.rs:125-198); returns the dequeued packet (its size in *size) or kPop
    __device__ uint32_t pop(uint64_t now, uint32_t op, uint32_t* size) {
        uint32_t pkt = 0;
        bool drop = false;
        if (!codel_pop(now, &pkt, size, &drop)) {
            flags &= ~kModeDrop;
            return kPop;
        }
        if (!drop) {
            flags &= ~kModeDrop;
            return pkt;
        }
        if (!(flags & kModeDrop)) {   // drop_from_store_mode
            sink.mark(pkt, op, 2);
            uint32_t nxt = 0;
            bool nd = false;
            const bool have = codel_pop(now, &nxt, size, &nd);
            flags |= kModeDrop;
            const uint64_t delta = sat_sub(s.cur, s.prev);
            s.cur = dropping_recently(now) && delta > 1 ? delta : 1;
            s.drop_next = control_law(now, s.cur, flags);
            flags |= kHasDropNext;
            s.prev = s.cur;
            return have ? nxt : kPop;
        }
        // drop_from_drop_mode
        bool have = true;
        bool item_drop = true;
        while (have && (flags & kModeDrop) && should_drop(now)) {
            sink.mark(pkt, op, 2);
            ++s.cur;
            have = codel_pop(now, &pkt, size, &item_drop);
            if (have && item_drop) s.drop_next = control_law(s.drop_next, s.cur, flags);
            else flags &= ~kModeDrop;
        }
        return have ? pkt : kPop;
    }
};

// Every packet of a host's queue, read-only: f(size) over ring[head ... head + count), wrapping.
template <class F>
__device__ __forceinline__ void codel_visit(const CodelHost& s, const uint4* ring, uint32_t cap, F&& f) {
    const uint32_t n = s.count < cap ? s.count : cap;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t j = s.head + i;
        if (j >= cap) j -= cap;
        f(ring[j].y);
    }
}

}  // namespace shd
