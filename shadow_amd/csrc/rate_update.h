// The host side of the bucket re-rate (rate_update.hip: shd_tb_update, shd_inbound_update_buckets,
// shd_outbound_update_buckets, shd_window_update_bandwidth): the call's validation, the
// last-entry-wins pass over its entries and the records that are uploaded, one per host that the
// call names.  No HIP type in here: tests/rate_update_main.cpp compiles this header alone, with the
// address and undefined-behaviour sanitizers, and tests/test_rate_update.py runs it.
//
// A re-rate of one bucket at emulated time `at` to (capacity C, increment I, interval N):
// lazy_refill(at) under the old parameters (token_bucket.rs:127-157), then
// TokenBucket::new_inner(C, I, N, at) (:37-60) whose balance is min(refilled balance, C) instead
// of C.  All three 0: the host becomes unlimited; some but not all 0 is refused, as at setup
// (tb_rows, tbucket_ops.h), and so is an interval above SIMTIME_MAX (no SimulationTime) or an `at`
// above EMUTIME_MAX (no EmulatedTime: `at` is the refill's `now` and the new last_refill).  The device side (tb_rerate, tbucket_ops.h) does the arithmetic.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "time_limits.h"

namespace shd {

struct RateRec {   // 32 bytes: one named host and its new parameters
    uint64_t capacity, increment, interval;
    uint32_t host, pad;
};

struct RateStamps {   // per host: the call that named it last (rate_updates_records)
    std::vector<uint32_t> stamp;
    uint32_t call = 0;
};

// create_token_bucket (relay/mod.rs:291-302) of a rate in bytes per second
inline void rate_from_bandwidth(uint64_t bytes_per_s, uint64_t& capacity, uint64_t& increment, uint64_t& interval) {
    increment = std::max<uint64_t>(1, bytes_per_s / 1000);
    capacity = increment + 1500;   // CONFIG_MTU (definitions.h:124)
    interval = 1000000;            // 1 ms
}

// The host-side rules of one call; nothing is changed by it.  prev_end: the stage's previous
// window_end (0 where there is none): a re-rate inside a window that has run is refused.
inline bool rate_updates_valid(uint64_t n, uint32_t n_hosts, const uint32_t* host, const uint64_t* capacity,
                               const uint64_t* increment, const uint64_t* interval, uint64_t at, uint64_t prev_end) {
    if (n == 0) return true;   // an empty call does nothing, whatever its time
    if (!host || !capacity || !increment || !interval) return false;
    if (at < prev_end || at > kEmutimeMax) return false;
    for (uint64_t i = 0; i < n; ++i) {
        if (host[i] >= n_hosts) return false;
        const bool any = capacity[i] || increment[i] || interval[i];
        const bool all = capacity[i] && increment[i] && interval[i];
        if (any && !all) return false;
        if (interval[i] > kSimtimeMax) return false;   // new_inner(C, I, N, at): N is a SimulationTime
    }
    return true;
}

// The entries that count, as records: a host named more than once takes its last entry.  The
// records stand in the order of those entries, last to first; O(n) (the stamps are per host, one
// word).  The call's entries have passed rate_updates_valid.
inline std::vector<RateRec> rate_updates_records(RateStamps& S, uint32_t n_hosts, uint64_t n, const uint32_t* host,
                                                 const uint64_t* capacity, const uint64_t* increment,
                                                 const uint64_t* interval) {
    if (S.stamp.size() != n_hosts) {
        S.stamp.assign(n_hosts, 0u);
        S.call = 0;
    }
    if (++S.call == 0) {   // the stamp wrapped: start over
        std::fill(S.stamp.begin(), S.stamp.end(), 0u);
        S.call = 1;
    }
    std::vector<RateRec> rec;
    rec.reserve(std::min<uint64_t>(n, n_hosts));
    for (uint64_t i = n; i-- > 0;) {
        uint32_t& s = S.stamp[host[i]];
        if (s == S.call) continue;
        s = S.call;
        rec.push_back(RateRec{capacity[i], increment[i], interval[i], host[i], 0});
    }
    return rec;
}

}  // namespace shd
