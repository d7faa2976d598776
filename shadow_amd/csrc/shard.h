// The rank that owns a host (or a routing row): shard_range's inverse (comm.h), one function for
// the host code and the kernels.  Free of HIP: tests/test_ledger_owner.py compiles it into a
// program of its own (tests/ledger_owner_main.cpp) and holds it against shd_shard_range.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHD_HOST_DEVICE __host__ __device__
#else
#define SHD_HOST_DEVICE
#endif

namespace shd {

// Shards are contiguous blocks of ceil(total / n); the ranks past the last block own nothing, so
// an index past `total` (no host) falls to the last rank like the last block's.
SHD_HOST_DEVICE inline uint32_t shard_owner(uint32_t total, uint32_t n, uint32_t index) {
    const uint64_t per = ((uint64_t)total + n - 1) / n;
    if (per == 0) return 0;
    const uint64_t q = index / per;
    return (uint32_t)(q < n - 1 ? q : n - 1);
}

}  // namespace shd
