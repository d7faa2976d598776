// The limits and the destination-bin arithmetic that more than one relay unit compiles (overview
// and the list of units: relay_priv.h).  A constant only one unit reads stays next to its kernel.
#pragma once
#include "relay_priv.h"

namespace shd {

// source hosts per stamp workgroup / host group (relay_stamp_v5, relay_stamp_v6, relay_bin_hist)
constexpr uint32_t kS5Hosts = 64;

// Pipeline 7's destination bins: kBinDst consecutive destinations each (relay_stamp_v6<BIN>)
constexpr uint32_t kBinShift = 5;
constexpr uint32_t kBinDst = 1u << kBinShift;

// the bin of a destination and its place dl in the bin (RelayArgs3::sh_per)
__device__ __forceinline__ uint32_t dst_bin(const RelayArgs3& a, uint32_t dst, uint32_t& dl) {
    if (a.sh_per == 0) {
        dl = dst & (kBinDst - 1);
        return dst >> kBinShift;
    }
    // dst / sh_per: exact for dst, sh_per < 2^18 (the error of the rounded-up reciprocal stays
    // below 2^-22, under the smallest distance 1 / sh_per of a fraction from the next integer)
    const uint32_t r = (uint32_t)(((uint64_t)dst * a.sh_mul) >> 40);
    const uint32_t x = dst - r * a.sh_per;
    dl = x & (kBinDst - 1);
    return r * a.sh_bpr + (x >> kBinShift);
}
constexpr uint32_t kHistSplit = 2;   // histogram rows per stamp workgroup (relay_bin_hist)

constexpr uint32_t kV7MaxHosts = 1u << 18;      // src host bits in the record
constexpr uint32_t kV7MaxPackets = 1u << 24;    // packet-index bits in bin_sort_v7's key
constexpr uint32_t kB7Cap = 3584;               // records per bin staged in LDS (C5: ~3200)

}  // namespace shd
