// Device-resident destination event queues.
//
// Reference: every sent packet becomes Event::new_packet(deliver, src_host, src_event_id) pushed
// into the destination host's Mutex<EventQueue> (src/main/core/worker.rs:619-629), a
// BinaryHeap<Reverse<..>> ordered by (time, Packet before Local, src host id, src event id)
// (src/main/core/work/event.rs:84-155, event_queue.rs:28-48).  At the next round the host pops
// every event with time < window_end (src/main/host/host.rs:697-706), in that order; what
// remains waits for a later round (a latency longer than one window keeps an event pending for
// several rounds).  next_event_time() is the head's time (event_queue.rs:43-45).
//
// Here the pending packet events of all destinations of this GPU are a short list of RUNS, one
// per batch (the relay output of a round: per destination already in that order), each a CSR
// of per-host sorted events with a per-host cursor (its first unpopped event).  An advance
// (shd_equeue_advance) never rewrites the pending events: per host it finds every run's prefix
// below window_end (a binary search from the cursor), merges those prefixes and the batch's into
// the popped output -- the host's popped events staged in LDS and ranked by a wave sort of their
// deliver times (equal times: by searches, an event's rank being its index in its own run plus
// the number of smaller (time, src, seq) keys in each other run); no atomics, deterministic
// (keys are unique: (src, seq) never repeats) -- moves the cursors, and stores the
// batch's remainder as a new run.  A run whose events are all popped is dropped; when
// the run limit is reached (kEqMaxRuns, or the EQ_MAX_RUNS knob), half of them -- those holding
// the fewest pending events -- are compacted into one by the next advance's own pass (the same
// merge, every event of those runs).
// Traffic per advance ~ the batch (read + its remainder written) + the popped events (read +
// written), instead of every pending event read and written each round.
//
// equeue.hip: the run slots, their growth, the sources of a pass, the full compaction and the C
// entry points.  equeue_pass.hip: the kernels and eq_pass, the one place that launches them.
#pragma once
#include "ctx.h"

namespace shd {

constexpr uint32_t kEqSrcMax = kEqMaxRuns + 1;   // the stored runs + the incoming batch

struct EqSrc {   // one source of an advance: a stored run (from its cursor) or the batch
    const uint32_t* off;       // [n_hosts + 1]
    const uint32_t* lo;        // stored run: per-host cursor; batch: nullptr (= off)
    uint32_t* cut;             // per host: first event not popped (eqr_count writes, eqr_merge reads)
    const uint64_t* deliver;
    const uint32_t* src;
    const uint64_t* seq;
    const uint64_t* tag;       // stored run
    const uint32_t* pkt;       // batch: tag = batch << 32 | pkt
    uint64_t batch;
};

struct EqSrcs {
    EqSrc s[kEqSrcMax];
    uint32_t n;
    int32_t b;   // index of the batch source, -1 without one
    // sources whose remainders [cut, end) are merged into the new run together with the batch's
    // (a compaction folded into the advance: those runs are dropped after it)
    uint32_t fold = 0;
};

struct EqOut {
    uint64_t* deliver;
    uint32_t* src;
    uint64_t* seq;
    uint64_t* tag;
};

inline EqOut eq_run_out(EqRunBuf& r) {
    return EqOut{r.deliver.as<uint64_t>(), r.src.as<uint32_t>(), r.seq.as<uint64_t>(), r.tag.as<uint64_t>()};
}

// Q.next layout (one read-back per call): [0] unused, [1] popped, [2] kept batch events, [3] head
// time, [4 + k] events of source k left after the pop; then eqr_count's per-block partials
constexpr uint32_t kEqWords = 4 + kEqSrcMax;
constexpr uint32_t kEqCountBlocks = 2048;   // eqr_count's grid: per-block partials, no hot atomics
                                            // (full occupancy for its latency-bound searches: 1024 blocks 64 us, 2048 55)
constexpr uint32_t kEqPart = 1 + kEqSrcMax;  // partial words per block: head time, left per source

constexpr int kEqPinWord = 48;   // ctx->h_pin words [48, 48 + kEqWords)
static_assert(kEqPinWord + (int)kEqWords <= kPinMarker, "queue counts below the polled marker");

// One pass: per-host cuts at window_end, scans, the merge of every source's popped prefix into
// `out` at offsets out_off, and (nrun) the batch's remainder and the folded runs' (S.fold) into a
// new run whose cursor goes to nrun_cur.  Returns with the counts in ctx->h_pin + kEqPinWord.
shd_status eq_pass(shd_ctx* ctx, const EqSrcs& S, uint64_t window_end, uint32_t* out_off, EqOut out, EqRunBuf* nrun,
                   uint32_t* nrun_cur, uint64_t n_in);

}  // namespace shd
