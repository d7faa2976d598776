// The grouping of staged runs by host (stage_group.h): the three kernels before a caller's gather
// and the host-side entry that launches them.
#include "stage_group.h"

#include <algorithm>
#include <cstring>

#include "pin_view.h"
#include "scan.h"

namespace shd {

// per run: its host's run index (+1).  red[0]: a host with a second run (the lowest such host),
// red[1]: a run of a host outside [first_host, first_host + n_hosts) (the lowest such run)
__device__ __forceinline__ void sg_map_run(uint32_t r, uint32_t host, uint32_t first_host, uint32_t n_hosts,
                                           uint32_t* __restrict__ hrun, unsigned long long* __restrict__ red) {
    const uint32_t h = host - first_host;   // (a host below first_host wraps past n_hosts)
    if (host < first_host || h >= n_hosts) {
        atomicMin(&red[1], (unsigned long long)r);
        return;
    }
    if (atomicExch(&hrun[h], r + 1) != 0) atomicMin(&red[0], (unsigned long long)h);
}

__global__ __launch_bounds__(256) void sg_runs(uint32_t n_runs, const uint32_t* __restrict__ run_host,
                                               uint32_t first_host, uint32_t n_hosts, uint32_t* __restrict__ hrun,
                                               unsigned long long* __restrict__ red) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_runs) return;
    sg_map_run(r, run_host[r], first_host, n_hosts, hrun, red);
}

// sg_runs on the pinned stages themselves: each run's host and count (read once, copied to the
// device arrays the scans read) and its stage
__global__ __launch_bounds__(256) void sg_runs_zc(uint32_t n_runs, const StageTab* __restrict__ st, uint32_t n_stages,
                                                  uint32_t first_host, uint32_t n_hosts, uint32_t* __restrict__ runh,
                                                  uint32_t* __restrict__ runc, uint32_t* __restrict__ rstage,
                                                  uint32_t* __restrict__ hrun, unsigned long long* __restrict__ red) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_runs) return;
    uint32_t lo = 0, hi = n_stages;   // the last stage whose first run is <= r (stages without runs skipped)
    while (hi - lo > 1) {
        const uint32_t m = (lo + hi) >> 1;
        if (st[m].run_base <= r) lo = m; else hi = m;
    }
    while (lo + 1 < n_stages && (st[lo].n_runs == 0 || r - st[lo].run_base >= st[lo].n_runs)) ++lo;
    const uint32_t i = r - st[lo].run_base;   // (< n_runs of the stage: r < the total of the stages' runs)
    const uint32_t host = st[lo].rh[i];
    runh[r] = host;
    runc[r] = st[lo].rc[i];
    rstage[r] = lo;
    sg_map_run(r, host, first_host, n_hosts, hrun, red);
}

// per host: its record count (0 without a run); entry n_hosts is 0 so one scan gives off[0..H]
__global__ __launch_bounds__(256) void sg_host_counts(uint32_t n_hosts, const uint32_t* __restrict__ hrun,
                                                      const uint32_t* __restrict__ run_count,
                                                      uint32_t* __restrict__ hcnt) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h > n_hosts) return;
    const uint32_t r = h < n_hosts ? hrun[h] : 0u;
    hcnt[h] = r ? run_count[r - 1] : 0u;
}

shd_status stage_group(StageGroupState& G, const StageView* stages, uint32_t n_stages, uint32_t rec_words,
                       uint32_t first_host, uint32_t n_hosts, bool force_copy, DevBuf& rec_copy, uint32_t* off,
                       hipStream_t s, StageRuns* out) {
    const uint32_t H = n_hosts;
    // 1. the stages: read where they lie when every array is pinned (zero-copy), else copied stage
    //    after stage (pinned host memory -- shd_host_alloc -- moves at the link's rate; pageable
    //    memory is staged by the runtime)
    std::vector<StageTab> tab(n_stages);
    bool zc = n_stages > 0 && !force_copy;
    uint64_t n = 0, n_runs = 0;
    for (uint32_t k = 0; k < n_stages; ++k) {
        const StageView& S = stages[k];
        StageTab& T = tab[k];
        if (zc) {
            T.rh = static_cast<const uint32_t*>(S.n_runs ? dev_view(S.run_host) : nullptr);
            T.rc = static_cast<const uint32_t*>(S.n_runs ? dev_view(S.run_count) : nullptr);
            T.rec = static_cast<const uint32_t*>(S.n_records ? dev_view(S.records) : nullptr);
            if ((S.n_runs && (!T.rh || !T.rc)) || (S.n_records && !T.rec)) zc = false;
        }
        T.rec_base = n;
        T.n_rec = S.n_records;
        T.run_base = (uint32_t)n_runs;
        T.n_runs = S.n_runs;
        n += S.n_records;
        n_runs += S.n_runs;
    }
    const size_t nr = std::max<uint64_t>(n_runs, 1);
    SHD_TRY(G.runh.ensure(nr * 4));
    SHD_TRY(G.runc.ensure(nr * 4));
    SHD_TRY(G.runo.ensure(nr * 4));
    SHD_TRY(G.hrun.ensure((size_t)(H + 1) * 4));
    SHD_TRY(G.hcnt.ensure((size_t)(H + 1) * 4));
    SHD_TRY(G.red.ensure(32));
    if (zc) {
        SHD_TRY(G.tab.ensure((size_t)n_stages * sizeof(StageTab)));
        SHD_TRY(G.tab_pin.ensure((size_t)n_stages * sizeof(StageTab)));
        SHD_TRY(G.rstg.ensure(nr * 4));
        std::memcpy(G.tab_pin.p, tab.data(), (size_t)n_stages * sizeof(StageTab));
        SHD_HIP(hipMemcpyAsync(G.tab.p, G.tab_pin.p, (size_t)n_stages * sizeof(StageTab), hipMemcpyHostToDevice, s));
    } else {
        SHD_TRY(rec_copy.ensure(std::max<uint64_t>(n, 1) * rec_words * 4));
        for (uint32_t k = 0; k < n_stages; ++k) {
            const StageView& S = stages[k];
            const StageTab& T = tab[k];
            if (T.n_runs) {
                SHD_HIP(hipMemcpyAsync(G.runh.as<uint32_t>() + T.run_base, S.run_host, (size_t)T.n_runs * 4,
                                       hipMemcpyHostToDevice, s));
                SHD_HIP(hipMemcpyAsync(G.runc.as<uint32_t>() + T.run_base, S.run_count, (size_t)T.n_runs * 4,
                                       hipMemcpyHostToDevice, s));
            }
            if (T.n_rec)
                SHD_HIP(hipMemcpyAsync(rec_copy.as<uint32_t>() + T.rec_base * rec_words, S.records,
                                       T.n_rec * rec_words * 4, hipMemcpyHostToDevice, s));
        }
    }
    // 2. runs -> hosts, per-host counts, the grouped offsets
    unsigned long long* red = G.red.as<unsigned long long>();
    SHD_HIP(hipMemsetAsync(G.hrun.p, 0, (size_t)(H + 1) * 4, s));
    SHD_HIP(hipMemsetAsync(red, 0xFF, 16, s));
    if (n_runs) {
        if (zc)
            sg_runs_zc<<<div_up(n_runs, 256), 256, 0, s>>>((uint32_t)n_runs, G.tab.as<StageTab>(), n_stages, first_host, H,
                                                            G.runh.as<uint32_t>(), G.runc.as<uint32_t>(),
                                                            G.rstg.as<uint32_t>(), G.hrun.as<uint32_t>(), red);
        else
            sg_runs<<<div_up(n_runs, 256), 256, 0, s>>>((uint32_t)n_runs, G.runh.as<uint32_t>(), first_host, H,
                                                         G.hrun.as<uint32_t>(), red);
        SHD_TRY(scan_excl2(G.scan, G.runc.as<uint32_t>(), G.runo.as<uint32_t>(), nullptr, nullptr, n_runs, s));
    }
    sg_host_counts<<<div_up((uint64_t)H + 1, 256), 256, 0, s>>>(H, G.hrun.as<uint32_t>(), G.runc.as<uint32_t>(),
                                                                G.hcnt.as<uint32_t>());
    SHD_TRY(scan_excl2(G.scan, G.hcnt.as<uint32_t>(), off, nullptr, nullptr, (uint64_t)H + 1, s));
    *out = StageRuns{G.hrun.as<uint32_t>(), G.runo.as<uint32_t>(), zc ? nullptr : rec_copy.as<uint32_t>(),
                     zc ? G.tab.as<StageTab>() : nullptr, zc ? G.rstg.as<uint32_t>() : nullptr, red, rec_words};
    return SHD_OK;
}

}  // namespace shd
