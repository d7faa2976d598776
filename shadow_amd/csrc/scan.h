// The hand-written scan every pipeline shares (no library kernels on any path); the kernel and
// its launch live in scan.hip.
//
// scan_excl2: exclusive scans of one or two u32 arrays in ONE launch: a tile of 8192 entries per
// 1024-thread workgroup (8 per thread, two 16-byte loads), a block scan, then a decoupled
// look-back over the earlier tiles' published sums (a workgroup's tile comes from a ticket
// counter, so a tile waits only on tiles whose workgroups already run).  Each tile's state word is epoch << 34 | flag << 32 | value (flag 1:
// the tile's own sum, 2: the inclusive prefix); the epoch changes every launch, so the states are
// never cleared between launches.
#pragma once
#include "ctx.h"

namespace shd {

constexpr uint32_t kScanV = 8;   // entries per thread

// exclusive scans of n entries of a (and b; b_in / b_out may be null); in-place is allowed
// (a_out == a_in)
shd_status scan_excl2(ScanScratch& S, const uint32_t* a_in, uint32_t* a_out, const uint32_t* b_in, uint32_t* b_out,
                      uint64_t n, hipStream_t s);

}  // namespace shd
