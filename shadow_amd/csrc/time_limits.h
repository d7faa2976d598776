// The limits of the reference's two time types (FlyearthR/shadow, src/lib/shadow-shim-helper-rs):
// SimulationTime, a duration in ns, and EmulatedTime, an instant in ns since the Unix epoch.  Plain
// constants, no HIP type: the device headers (tbucket_ops.h, codel_lane.h) and the host-only
// rate_update.h all read them.  DESIGN.md ("The time seam") lists what saturates where.
#pragma once
#include <stdint.h>

namespace shd {

constexpr uint64_t kSimtimeMax = 17500059273709551614ull;   // simulation_time.rs:377
constexpr uint64_t kEmutimeMax = ~0ull - 1ull;               // emulated_time.rs:27 (2^64 - 1 is EMUTIME_INVALID)
constexpr uint64_t kSimStart = 946684800ull * 1000000000ull; // EmulatedTime::SIMULATION_START (emulated_time.rs:34)
static_assert(kSimtimeMax == kEmutimeMax - kSimStart, "simulation_time.rs:378-379");

}  // namespace shd
