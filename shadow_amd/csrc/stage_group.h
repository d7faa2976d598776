// The grouping of staged runs by host, shared by the staged entry points (shd_relay_flush,
// shd_offers_group).  Each takes the worker threads' buffers as they stand at the round barrier
// (stage_shape.h): the device maps every run to its host (a host with two runs and a host outside
// the range are the two device-side checks), scans the run counts and the per-host counts, and the
// caller's gather then moves a wave per host.  Pinned stages are read where they lie, once -- the
// run arrays by the run mapper (which copies them to the device arrays the scans read), the records
// by the gather -- instead of one copy per buffer (three per worker thread, each with ~11 us of
// launch gap, plus the re-read of the uploaded records); pageable stages, or any stage under the
// FLUSH_COPY knob, are copied stage after stage.  The kernels and stage_group live in
// stage_group.hip; a caller keeps its record format, its gather's loop and its read-back.
#pragma once
#include "ctx.h"
#include "stage_shape.h"

namespace shd {

struct StageTab {          // zero-copy: one stage of the table the kernels read
    const uint32_t* rh;    // device views of the stage's run_host / run_count / records
    const uint32_t* rc;
    const uint32_t* rec;
    uint64_t rec_base;     // the stage's first record in stage order
    uint64_t n_rec;
    uint32_t run_base, n_runs;
};

struct StageRuns {         // what a gather needs (a kernel argument): device pointers, valid until the state's next grouping
    const uint32_t* hrun;      // per host: its run (+1), 0 without one
    const uint32_t* run_off;   // per run: its first record in stage order
    const uint32_t* copy;      // the records of every stage, stage after stage (copy path)
    const StageTab* tab;       // read in place: the stage table and each run's stage; else null
    const uint32_t* rstage;
    unsigned long long* red;   // [0] a host with two runs, or whose run would leave its stage (the lowest such
                               // host); [1] a run of a host outside the range (the lowest such run); ~0: none
    uint32_t rec_words;
};

// Group `stages` (which have passed stages_ok; records of rec_words u32 words) by host over
// [first_host, first_host + n_hosts) on stream s: the table or the copies (force_copy, or a stage
// that is not pinned: the records into rec_copy), hrun and the check words cleared, runs -> hosts,
// the run counts scanned, the per-host counts scanned into off[0 .. n_hosts].  No read-back: the
// check words are the caller's to fetch after its gather.
shd_status stage_group(StageGroupState& G, const StageView* stages, uint32_t n_stages, uint32_t rec_words,
                       uint32_t first_host, uint32_t n_hosts, bool force_copy, DevBuf& rec_copy, uint32_t* off,
                       hipStream_t s, StageRuns* out);

struct RunRecords {
    const uint32_t* rec;     // the run's first record: in the uploaded copy, or in its stage's pinned buffer
    uint32_t from, to, cnt;  // its first record in stage order, its grouped offset, its records
};

// Host h's run for the wave that gathers it; false: nothing to gather.  A run that would leave its
// stage (the pinned counts changed under the call) is not read: red[0].
__device__ __forceinline__ bool stage_run(const StageRuns& g, const uint32_t* __restrict__ off, uint32_t h,
                                          uint32_t lane, RunRecords& out) {
    const uint32_t r = g.hrun[h];
    if (!r) return false;
    out.from = g.run_off[r - 1];
    out.to = off[h];
    out.cnt = off[h + 1] - out.to;
    if (!g.tab) {
        out.rec = g.copy + (size_t)out.from * g.rec_words;
        return true;
    }
    const StageTab& S = g.tab[g.rstage[r - 1]];
    const uint64_t at = out.from - S.rec_base;
    if (at + out.cnt > S.n_rec) {
        if (lane == 0) atomicMin(&g.red[0], (unsigned long long)h);
        return false;
    }
    out.rec = S.rec + at * g.rec_words;
    return true;
}

}  // namespace shd
