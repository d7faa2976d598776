// One relay's token bucket: the arithmetic tbucket.hip (attempt replay) and inbound.hip (the
// inbound stage) both compile.
//
// Reference semantics: src/main/network/relay/token_bucket.rs (FlyearthR/shadow)
//   :37-60   new_inner: a bucket only when capacity, increment and interval are all non-zero;
//            it starts full
//   :75-86   conforming_remove: lazy refill, then balance.checked_sub(decrement) or the
//            conforming duration
//   :94-120  compute_conforming_duration: ceil(missing / increment) refills; 0 -> ZERO,
//            1 -> the span to the next refill, n -> span + interval * (n - 1), saturating
//   :127-157 lazy_refill: n = elapsed / interval whole refills, balance + increment * n
//            (u64 saturating) clamped to the capacity, last_refill += interval * n; both spans
//            are duration_since (emulated_time.rs:79-87): now before last_refill panics, and so
//            does a difference above SIMTIME_MAX
// Times: EmulatedTime ns (u64); SimulationTime saturates at SIMTIME_MAX, EmulatedTime at
// EMUTIME_MAX.  A product, sum or span beyond SIMTIME_MAX that does not overflow u64 is where the
// reference panics (from_c_simtime(..).unwrap()); `bad` records it.
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"
#include "time_limits.h"

namespace shd {

struct TbRelay {   // 48 bytes per relay; capacity 0 = no bucket (unlimited)
    uint64_t capacity, balance, increment, interval, last_refill, pending;
};

// SimulationTime::saturating_mul / saturating_add (simulation_time.rs:135-148)
__device__ __forceinline__ uint64_t simtime_sat_mul(uint64_t t, uint64_t k, bool& bad) {
    const uint64_t hi = __umul64hi(t, k);
    if (hi) return kSimtimeMax;
    const uint64_t p = t * k;
    bad |= p > kSimtimeMax;
    return p;
}
__device__ __forceinline__ uint64_t simtime_sat_add(uint64_t a, uint64_t b, bool& bad) {
    const uint64_t s = a + b;
    if (s < a) return kSimtimeMax;
    bad |= s > kSimtimeMax;
    return s;
}
// EmulatedTime::saturating_add (emulated_time.rs:95-108)
__device__ __forceinline__ uint64_t emutime_sat_add(uint64_t t, uint64_t d) {
    const uint64_t s = t + d;
    return (s < t || s > kEmutimeMax) ? kEmutimeMax : s;
}

// conforming_remove(dec) at `now` (token_bucket.rs:75-86) on a relay that has a bucket: true and
// v = the balance after the removal, or false and v = the duration until it would conform
__device__ __forceinline__ bool tb_conforming_remove(TbRelay& s, uint64_t now, uint64_t dec, uint64_t& v,
                                                     bool& bad) {
    // lazy_refill (token_bucket.rs:127-157)
    // duration_since(..).unwrap() panics: now is earlier, or the span is no SimulationTime (one
    // compare for both: an earlier now counts as the largest span)
    uint64_t span = now < s.last_refill ? ~0ull : now - s.last_refill;
    const bool before = span > kSimtimeMax;
    bad |= before;
    span = before ? 0ull : span;
    if (span >= s.interval) {
        const uint64_t n = span / s.interval;
        const uint64_t tok = __umul64hi(s.increment, n) ? ~0ull : s.increment * n;
        const uint64_t sum = s.balance + tok < s.balance ? ~0ull : s.balance + tok;
        s.balance = sum < s.capacity ? sum : s.capacity;
        s.last_refill = emutime_sat_add(s.last_refill, simtime_sat_mul(s.interval, n, bad));
        span = now < s.last_refill ? ~0ull : now - s.last_refill;
        const bool before2 = span > kSimtimeMax;
        bad |= before2;
        span = before2 ? 0ull : span;
    }
    const uint64_t next_span = s.interval - span;
    if (s.balance >= dec) {
        s.balance -= dec;
        v = s.balance;
        return true;
    }
    // compute_conforming_duration (token_bucket.rs:94-120)
    const uint64_t req = dec - s.balance;
    const uint64_t nr = req / s.increment + (req % s.increment ? 1u : 0u);
    v = nr == 0 ? 0ull
      : nr == 1 ? next_span
                : simtime_sat_add(next_span, simtime_sat_mul(s.interval, nr - 1, bad), bad);
    return false;
}

// A re-rate of the relay's bucket at `at` to (capacity C, increment I, interval N), all three 0: no
// bucket (rate_update.h states the rules).  The old rate holds up to `at`: lazy_refill(at) under
// the old parameters -- tb_conforming_remove of nothing, with its `bad` conditions -- then
// new_inner(C, I, N, at) with the balance min(refilled balance, C); a relay without a bucket gets
// a full one, as every new bucket.  The relay's pending deadline is not touched.
__device__ __forceinline__ void tb_rerate(TbRelay& s, uint64_t at, uint64_t C, uint64_t I, uint64_t N, bool& bad) {
    uint64_t balance = C;
    if (s.capacity) {
        uint64_t v;
        (void)tb_conforming_remove(s, at, 0, v, bad);
        balance = v < C ? v : C;
    } else if (C == 0) {
        return;   // no bucket before or after: nothing changes
    }
    s.capacity = C;
    s.balance = balance;
    s.increment = I;
    s.interval = N;
    s.last_refill = at;
}

// Host rows of a setup call: all three parameters 0 = no bucket; some but not all 0 is
// SHD_ERR_INVALID (TokenBucket::new -> None, which the reference unwraps), and so is a bucket
// whose interval is no SimulationTime (above SIMTIME_MAX) or whose last_refill is no EmulatedTime
// (above EMUTIME_MAX): from_c_simtime / from_c_emutime give None.  Buckets start full.
inline shd_status tb_rows(uint32_t n, const uint64_t* capacity, const uint64_t* refill_increment,
                          const uint64_t* refill_interval_ns, const uint64_t* last_refill,
                          std::vector<TbRelay>& h) {
    if (n && (!capacity || !refill_increment || !refill_interval_ns || !last_refill)) return SHD_ERR_INVALID;
    h.resize(n);
    for (uint32_t r = 0; r < n; ++r) {
        const bool any = capacity[r] || refill_increment[r] || refill_interval_ns[r];
        const bool all = capacity[r] && refill_increment[r] && refill_interval_ns[r];
        if (any && !all) return SHD_ERR_INVALID;
        if (all && (refill_interval_ns[r] > kSimtimeMax || last_refill[r] > kEmutimeMax)) return SHD_ERR_INVALID;
        h[r] = TbRelay{capacity[r], capacity[r], refill_increment[r], refill_interval_ns[r], last_refill[r], 0};
    }
    return SHD_OK;
}

}  // namespace shd
