// Zero-copy staging (stage_group.hip) and zero-copy outputs (flush.hip): the device's view of a
// caller's pinned host buffer.
#pragma once
#include "common.h"

namespace shd {

// a device view of host memory p when it is pinned (hipHostMalloc / registered), else nullptr
inline const void* dev_view(const void* p) {
    if (!p) return nullptr;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();   // pageable memory: not an error of the call
        return nullptr;
    }
    if (at.type != hipMemoryTypeHost || !at.devicePointer || !at.hostPointer) return nullptr;
    return static_cast<const char*>(at.devicePointer) + (static_cast<const char*>(p) - static_cast<const char*>(at.hostPointer));
}

}  // namespace shd
