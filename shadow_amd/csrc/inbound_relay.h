// The inbound stage's relay words per host: what inbound.hip (the advance) and rate_update.hip (the
// re-rate's walk over the stored packets) both compile.
#pragma once
#include <cstdint>

namespace shd {

constexpr uint64_t kInIdle = ~0ull;    // no outstanding forward task

struct InRelay {   // 24 bytes per host
    uint64_t task;   // time of the outstanding forward task (RelayState::Pending), kInIdle: Idle
    uint32_t has_cached, cached_pkt, cached_size, pad;   // RelayInternal::next_packet
};

}  // namespace shd
