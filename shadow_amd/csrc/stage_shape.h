// A stage as both staged entry points see it (shd_relay_flush, shd_offers_group) and the host-side
// check of the stages' shape.  No HIP type in here: offer_stage.h includes this header, and
// tests/offer_stage_main.cpp compiles the two alone under the address and undefined-behaviour
// sanitizers.
//
// A stage is one worker thread's buffer at the round barrier: runs (host, count) and, run after
// run, the hosts' records in the order each host made them.
#pragma once
#include <stdint.h>

namespace shd {

struct StageView {
    uint32_t n_runs;
    const uint32_t* run_host;    // [n_runs]
    const uint32_t* run_count;   // [n_runs] the run's records, consecutive in `records`
    uint64_t n_records;
    const void* records;         // [n_records] of the caller's record size
};

// The stages' shape, checked on the host before anything is uploaded: fewer than 2^32 runs and
// records in all, no NULL array where a count is not zero, every stage's run counts adding up to
// its n_records.  The totals come first, so no array is read for a call too large; of the arrays
// the run counts only are read.  false: refused, the totals are not written.
inline bool stages_ok(const StageView* st, uint32_t n_stages, uint64_t* n_runs, uint64_t* n_records) {
    if (n_stages && !st) return false;
    uint64_t nr = 0, nn = 0;
    for (uint32_t k = 0; k < n_stages; ++k) {
        if (st[k].n_records >= (1ull << 32)) return false;
        nr += st[k].n_runs;
        nn += st[k].n_records;
        if (nr >= (1ull << 32) || nn >= (1ull << 32)) return false;
    }
    for (uint32_t k = 0; k < n_stages; ++k) {
        const StageView& S = st[k];
        if (S.n_runs && (!S.run_host || !S.run_count)) return false;
        if (S.n_records && !S.records) return false;
        uint64_t c = 0;
        for (uint32_t r = 0; r < S.n_runs; ++r) c += S.run_count[r];
        if (c != S.n_records) return false;
    }
    if (n_runs) *n_runs = nr;
    if (n_records) *n_records = nn;
    return true;
}

}  // namespace shd
