// The event queues' run bookkeeping and C entry points (overview: equeue_priv.h): run slots and
// their growth, the sources of a pass, the full compaction.  Every kernel is in equeue_pass.hip.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "equeue_priv.h"

namespace shd {

// a stored run's event arrays for n events (the ensure keeps growth headroom: slots are reused
// round after round)
// hint = false (shd_equeue_pending's full compaction, the whole pending set in one run): the
// growth neither takes nor raises the slots' shared capacity -- a hint raised to 1.5x every pending
// event would make every later slot growth that large (advisor, round 5: ~14x the largest run)
static shd_status eq_run_alloc(EqState& Q, EqRunBuf& r, uint32_t n_hosts, uint64_t n, bool hint = true) {
    // room for half as many again: the runs' sizes wander from round to round, and a regrowth
    // (hipFree + hipMalloc of ~0.5 GB of arrays) inside an advance cost ~0.3 ms (C5: 0.78 ms rounds);
    // and at least the largest capacity any slot has grown to, so the slots reach their steady
    // size in one growth each instead of several (the slots take turns as batch, remainder and
    // compaction runs of different sizes)
    const size_t m = std::max<uint64_t>(n, 1);
    if (r.deliver.bytes < m * 8 || r.src.bytes < m * 4 || r.seq.bytes < m * 8 || r.tag.bytes < m * 8) {
        const size_t g = hint ? std::max<size_t>(m + m / 2, Q.cap_hint) : m + m / 2;
        if (hint) Q.cap_hint = g;
        SHD_TRY(r.deliver.ensure(g * 8));
        SHD_TRY(r.src.ensure(g * 4));
        SHD_TRY(r.seq.ensure(g * 8));
        SHD_TRY(r.tag.ensure(g * 8));
    }
    SHD_TRY(r.off.ensure((size_t)(n_hosts + 1) * 4));
    SHD_TRY(r.deliver.ensure(m * 8));
    SHD_TRY(r.src.ensure(m * 4));
    SHD_TRY(r.seq.ensure(m * 8));
    SHD_TRY(r.tag.ensure(m * 8));
    r.has_pkt = false;
    r.fresh = false;
    return SHD_OK;
}

static uint32_t* eq_cursor(EqState& Q, int buf, int slot) {
    return Q.curs[buf].as<uint32_t>() + (size_t)slot * Q.n_hosts;
}

// the live runs as sources, from their cursors; cuts into the other cursor buffer
static EqSrcs eq_sources(EqState& Q, int* slots) {
    EqSrcs S{};
    S.b = -1;
    for (int r = 0; r < kEqSlots; ++r) {
        EqRunBuf& R = Q.run[r];
        if (!R.live) continue;
        slots[S.n] = r;
        // a run adopted by this call has no cursor yet: it starts at its offsets (lo = null)
        S.s[S.n++] = EqSrc{R.off.as<uint32_t>(), R.fresh ? nullptr : eq_cursor(Q, Q.ccur, r), eq_cursor(Q, 1 - Q.ccur, r),
                           R.deliver.as<uint64_t>(), R.src.as<uint32_t>(), R.seq.as<uint64_t>(),
                           R.has_pkt ? nullptr : R.tag.as<uint64_t>(), R.has_pkt ? R.pkt.as<uint32_t>() : nullptr,
                           R.batch};
    }
    return S;
}

static int eq_free_slot(const EqState& Q) {
    for (int r = 0; r < kEqSlots; ++r)
        if (!Q.run[r].live && r != Q.lend) return r;
    return -1;
}

// The full compaction (shd_equeue_pending): the pending events of every live run into one fresh
// run (cursor at its start); those runs are dropped.  (The compaction the run limit forces is not
// this one: it takes half the runs and rides the advance's own pass, shd_equeue_advance.)
static shd_status eq_compact(shd_ctx* ctx) {
    EqState& Q = ctx->eq;
    int slots[kEqSrcMax];
    EqSrcs S = eq_sources(Q, slots);
    if (S.n == 0) return SHD_OK;
    uint64_t n = 0;
    for (uint32_t k = 0; k < S.n; ++k) n += Q.run[slots[k]].left;
    const int t = eq_free_slot(Q);
    EqRunBuf& T = Q.run[t];
    SHD_TRY(eq_run_alloc(Q, T, Q.n_hosts, n, false));
    // every pending event moves (window ~0); not hot, so the totals read back are checked: exactly
    // the n events the runs' counts promise were moved
    SHD_TRY(eq_pass(ctx, S, ~0ull, T.off.as<uint32_t>(), eq_run_out(T), nullptr, nullptr, n));
    if (ctx->h_pin[kEqPinWord + 1] != n) return SHD_ERR_STATE;
    // the new run's cursor goes to the CURRENT cursor buffer
    SHD_HIP(hipMemcpyAsync(eq_cursor(Q, Q.ccur, t), T.off.p, (size_t)Q.n_hosts * 4, hipMemcpyDeviceToDevice,
                           ctx->stream));
    for (uint32_t k = 0; k < S.n; ++k) Q.run[slots[k]].live = false;
    T.live = n > 0;
    T.n = T.left = n;
    return SHD_OK;
}

}  // namespace shd

using namespace shd;

extern "C" {

shd_status shd_equeue_setup(shd_ctx* ctx, uint32_t n_total) {
    if (!ctx || n_total == 0) return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    EqState& Q = ctx->eq;
    Q.ready = false;
    // under a communicator of > 1 ranks: this rank's destination shard (shd_relay_round_sharded's)
    uint32_t lo = 0, hi = n_total;
    if (ctx->comm && ctx->comm->size > 1) shard_range(n_total, ctx->comm->size, ctx->comm->rank, &lo, &hi);
    const uint32_t n_hosts = hi - lo;
    if (n_hosts == 0) return SHD_ERR_INVALID;
    for (int r = 0; r < kEqSlots; ++r) {
        Q.run[r].live = false;
        Q.run[r].n = Q.run[r].left = 0;
    }
    for (int k = 0; k < 2; ++k) SHD_TRY(Q.curs[k].ensure((size_t)kEqSlots * n_hosts * 4));
    Q.lend = -1;
    SHD_TRY(Q.bcut.ensure((size_t)n_hosts * 4));
    SHD_TRY(Q.pop_cnt.ensure((size_t)(n_hosts + 1) * 4));
    SHD_TRY(Q.keep_cnt.ensure((size_t)(n_hosts + 1) * 4));
    SHD_TRY(Q.pop_off.ensure((size_t)(n_hosts + 1) * 4));
    SHD_TRY(Q.next.ensure((kEqWords + (size_t)kEqCountBlocks * kEqPart) * 8));
    SHD_HIP(hipMemsetAsync(Q.pop_off.p, 0, (size_t)(n_hosts + 1) * 4, ctx->stream));
    SHD_HIP(hipStreamSynchronize(ctx->stream));
    Q.ccur = 0;
    Q.n_hosts = n_hosts;
    Q.host_lo = lo;
    Q.n_total = n_total;
    Q.head = ~0ull;
    Q.n_pending = 0;
    Q.n_popped = 0;
    Q.batches = 0;
    ctx->rnd.batch_min_deliver = ~0ull;   // new queues: no relay output is pending for them
    Q.ready = true;
    return SHD_OK;
}

shd_status shd_equeue_advance(shd_ctx* ctx, const shd_relay_out* d_batch, uint64_t window_end,
                              shd_equeue_out* out);

// the pending runs alone (an adopted batch is one of them by now)
static shd_status advance_runs(shd_ctx* ctx, uint64_t window_end, shd_equeue_out* out) {
    return shd_equeue_advance(ctx, nullptr, window_end, out);
}

shd_status shd_equeue_batch_buffers(shd_ctx* ctx, uint64_t max_events, shd_relay_out* out) {
    if (!ctx || !out) return SHD_ERR_INVALID;
    EqState& Q = ctx->eq;
    if (!Q.ready) return SHD_ERR_STATE;
    SHD_HIP(hipSetDevice(ctx->device));
    Q.lend = -1;
    const int t = eq_free_slot(Q);
    if (t < 0) return SHD_ERR_STATE;
    EqRunBuf& R = Q.run[t];
    const size_t m = std::max<uint64_t>(max_events, 1);
    SHD_TRY(R.off.ensure((size_t)(Q.n_hosts + 1) * 4));
    if (R.deliver.bytes < m * 8) {   // a growth takes the slots' largest capacity (eq_run_alloc)
        const size_t g = std::max<size_t>(m, Q.cap_hint);
        Q.cap_hint = g;
        SHD_TRY(R.deliver.ensure(g * 8));
        SHD_TRY(R.src.ensure(g * 4));
        SHD_TRY(R.seq.ensure(g * 8));
    }
    SHD_TRY(R.pkt.ensure(std::max<size_t>(m, R.deliver.bytes / 8) * 4));
    Q.lend = t;
    Q.lend_cap = m;   // the relay refuses a round of more events than this into the slot
    out->ev_off = R.off.as<uint32_t>();
    out->ev_deliver = R.deliver.as<uint64_t>();
    out->ev_src = R.src.as<uint32_t>();
    out->ev_seq = R.seq.as<uint64_t>();
    out->ev_pkt = R.pkt.as<uint32_t>();
    out->n_dst = Q.n_hosts;
    out->n_events = 0;
    return SHD_OK;
}

shd_status shd_equeue_advance(shd_ctx* ctx, const shd_relay_out* d_batch, uint64_t window_end,
                              shd_equeue_out* out) {
    if (!ctx || !out) return SHD_ERR_INVALID;
    EqState& Q = ctx->eq;
    if (!Q.ready) return SHD_ERR_STATE;
    const bool has_b = d_batch != nullptr;
    if (has_b && (!d_batch->ev_off || (d_batch->n_events && (!d_batch->ev_deliver || !d_batch->ev_src ||
                                                            !d_batch->ev_seq || !d_batch->ev_pkt))))
        return SHD_ERR_INVALID;
    if (has_b && Q.batches >= 0xFFFFFFFFull) return SHD_ERR_INVALID;   // tag bits exhausted
    // the batch must cover exactly these queues' hosts (ev_off has n_dst + 1 entries): a sharded
    // rank's relay output (n_dst = its shard) into queues set up for another host count would be
    // read past its end on the device
    if (has_b && d_batch->n_dst != Q.n_hosts) return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    const uint32_t H = Q.n_hosts;
    const uint64_t n_b = has_b ? d_batch->n_events : 0;   // this context's events (a sharded round: received)
    const uint64_t n_in = Q.n_pending + n_b;
    if (n_in >= 0xFFFFFFFFull) return SHD_ERR_INVALID;   // 32-bit positions
    // adoption: a batch written into the slot shd_equeue_batch_buffers handed out becomes a stored
    // run as it is -- its cursor starts at its offsets, nothing of it is copied
    bool adopt = false;
    if (has_b && Q.lend >= 0) {
        EqRunBuf& L = Q.run[Q.lend];
        adopt = d_batch->ev_off == L.off.p && d_batch->ev_deliver == L.deliver.p && d_batch->ev_src == L.src.p &&
                d_batch->ev_seq == L.seq.p && d_batch->ev_pkt == L.pkt.p;
        if (adopt && (n_b * 8 > L.deliver.bytes || n_b * 4 > L.pkt.bytes)) return SHD_ERR_INVALID;
        if (!adopt) Q.lend = -1;   // the lent slot went unused: free again
    }
    int live = 0;
    for (int r = 0; r < kEqSlots; ++r) live += Q.run[r].live ? 1 : 0;
    const int max_runs = (int)std::min<int64_t>(std::max<int64_t>(ctx->knobs.get(K_EQ_MAX_RUNS, kEqMaxRuns), 2),
                                                kEqMaxRuns);
    // room for the batch's run: the compaction rides this advance's pass (the picked runs'
    // remainders merge into the new run, no pass of its own)
    if (has_b && n_b && live >= max_runs) Q.fold_next = true;
    if (adopt) {
        const int t = Q.lend;
        EqRunBuf& R = Q.run[t];
        R.fresh = n_b > 0;   // the pass below reads its cursor from its offsets (no cursor copy)
        R.has_pkt = true;
        R.batch = Q.batches;
        R.n = R.left = n_b;
        R.live = n_b > 0;
        Q.lend = -1;
        ++Q.batches;
        Q.n_pending += n_b;
        ctx->rnd.batch_min_deliver = ~0ull;
        return advance_runs(ctx, window_end, out);
    }
    // the popped events: at most everything (headroom: the pending set creeps up at first)
    if (Q.ps.bytes < std::max<uint64_t>(n_in, 1) * 4) {
        const uint64_t cap = std::max<uint64_t>(n_in, 1) * 3 / 2 + 1;
        SHD_TRY(Q.pd.ensure(cap * 8));
        SHD_TRY(Q.ps.ensure(cap * 4));
        SHD_TRY(Q.pq.ensure(cap * 8));
        SHD_TRY(Q.pt.ensure(cap * 8));
    }
    int slots[kEqSrcMax];
    EqSrcs S = eq_sources(Q, slots);
    const uint32_t n_runs = S.n;
    // a folded compaction: the half of the runs holding the fewest pending events -- the oldest,
    // mostly drained ones -- so it costs what those runs still hold, not every pending event (C5:
    // runs drain over hundreds of rounds, the pending set is many rounds' worth)
    uint64_t n_fold = 0;
    if (Q.fold_next && n_runs >= 2) {
        int ord[kEqSrcMax];
        for (uint32_t k = 0; k < n_runs; ++k) ord[k] = (int)k;
        std::sort(ord, ord + n_runs, [&](int a, int b) { return Q.run[slots[a]].left < Q.run[slots[b]].left; });
        const uint32_t take = std::min<uint32_t>(n_runs, std::max<uint32_t>(2, (n_runs + 1) / 2));
        for (uint32_t i = 0; i < take; ++i) {
            S.fold |= 1u << ord[i];
            n_fold += Q.run[slots[ord[i]]].left;
        }
    }
    Q.fold_next = false;
    EqRunBuf* nrun = nullptr;
    int t = -1;
    if (has_b) {
        S.b = (int32_t)S.n;
        S.s[S.n++] = EqSrc{d_batch->ev_off, nullptr, Q.bcut.as<uint32_t>(), d_batch->ev_deliver, d_batch->ev_src,
                           d_batch->ev_seq, nullptr, d_batch->ev_pkt, Q.batches};
    }
    if (has_b || S.fold) {   // the new run: the batch's remainder and / or the folded runs'
        t = eq_free_slot(Q);
        if (t < 0) return SHD_ERR_STATE;
        nrun = &Q.run[t];
        SHD_TRY(eq_run_alloc(Q, *nrun, H, n_b + n_fold));
    }
    const EqOut popped{Q.pd.as<uint64_t>(), Q.ps.as<uint32_t>(), Q.pq.as<uint64_t>(), Q.pt.as<uint64_t>()};
    SHD_TRY(eq_pass(ctx, S, window_end, Q.pop_off.as<uint32_t>(), popped, nrun,
                    nrun ? eq_cursor(Q, 1 - Q.ccur, t) : nullptr, n_in));
    const unsigned long long* wd = ctx->h_pin + kEqPinWord;
    const uint64_t n_pop = wd[1], n_keep = wd[2];
    uint64_t left = 0, into_new = 0;
    for (uint32_t k = 0; k < S.n; ++k) {
        left += wd[4 + k];
        if ((int32_t)k == S.b || ((S.fold >> k) & 1u)) into_new += wd[4 + k];
    }
    if (n_pop + left != n_in || (nrun && into_new != n_keep)) {   // batch ev_off / n_events disagree
        std::fprintf(stderr, "shd_equeue_advance: counts disagree: popped %llu + left %llu != in %llu "
                     "(pending %llu, batch %llu, runs %u, batch kept %llu vs %llu)\n",
                     (unsigned long long)n_pop, (unsigned long long)left, (unsigned long long)n_in,
                     (unsigned long long)Q.n_pending, (unsigned long long)n_b, n_runs,
                     has_b ? (unsigned long long)wd[4 + S.b] : 0ull, (unsigned long long)n_keep);
        return SHD_ERR_INVALID;
    }
    // commit: cursors moved to the cut buffer; drained runs dropped; the batch's remainder is a run
    for (uint32_t k = 0; k < n_runs; ++k) {
        EqRunBuf& R = Q.run[slots[k]];
        const bool folded = (S.fold >> k) & 1u;   // its remainder moved into the new run
        R.left = folded ? 0 : wd[4 + k];
        R.live = R.left > 0;
        R.fresh = false;   // its cursor is in the cut buffer now
    }
    if (nrun) {
        nrun->n = nrun->left = n_keep;
        nrun->live = n_keep > 0;
    }
    if (has_b) ++Q.batches;
    Q.ccur = 1 - Q.ccur;
    Q.n_pending = left;
    Q.n_popped = n_pop;
    out->off = Q.pop_off.as<uint32_t>();
    out->deliver = Q.pd.as<uint64_t>();
    out->src = Q.ps.as<uint32_t>();
    out->seq = Q.pq.as<uint64_t>();
    out->tag = Q.pt.as<uint64_t>();
    out->n_popped = n_pop;
    out->n_pending = left;
    out->next_time = wd[3];
    Q.head = wd[3];
    if (has_b) ctx->rnd.batch_min_deliver = ~0ull;   // merged: the queue heads carry it from now on
    return SHD_OK;
}

shd_status shd_equeue_next_batch(shd_ctx* ctx, uint64_t* batch) {
    if (!ctx || !batch) return SHD_ERR_INVALID;
    if (!ctx->eq.ready) return SHD_ERR_STATE;
    *batch = ctx->eq.batches;
    return SHD_OK;
}

shd_status shd_equeue_copy_popped(shd_ctx* ctx, uint32_t* off, uint64_t* deliver, uint32_t* src,
                                  uint64_t* seq, uint64_t* tag) {
    if (!ctx) return SHD_ERR_INVALID;
    EqState& Q = ctx->eq;
    if (!Q.ready) return SHD_ERR_STATE;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = Q.n_popped;
    if (off) SHD_HIP(hipMemcpyAsync(off, Q.pop_off.p, (size_t)(Q.n_hosts + 1) * 4, hipMemcpyDeviceToHost, s));
    if (n) {
        if (deliver) SHD_HIP(hipMemcpyAsync(deliver, Q.pd.p, n * 8, hipMemcpyDeviceToHost, s));
        if (src) SHD_HIP(hipMemcpyAsync(src, Q.ps.p, n * 4, hipMemcpyDeviceToHost, s));
        if (seq) SHD_HIP(hipMemcpyAsync(seq, Q.pq.p, n * 8, hipMemcpyDeviceToHost, s));
        if (tag) SHD_HIP(hipMemcpyAsync(tag, Q.pt.p, n * 8, hipMemcpyDeviceToHost, s));
    }
    SHD_HIP(hipStreamSynchronize(s));
    return SHD_OK;
}

// The pending queues as one CSR: the runs are compacted into one first (the queues' content and
// every later result are unchanged by a compaction).
shd_status shd_equeue_pending(shd_ctx* ctx, uint32_t* off, uint64_t* deliver, uint32_t* src,
                              uint64_t* seq, uint64_t* tag, uint64_t* n_pending) {
    if (!ctx) return SHD_ERR_INVALID;
    EqState& Q = ctx->eq;
    if (!Q.ready) return SHD_ERR_STATE;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n = Q.n_pending;
    if (n_pending) *n_pending = n;
    if (!off && !(n && (deliver || src || seq || tag))) return SHD_OK;
    SHD_TRY(eq_compact(ctx));
    int live = -1;
    for (int r = 0; r < kEqSlots; ++r)
        if (Q.run[r].live) live = r;
    if (off) {
        if (live >= 0) SHD_HIP(hipMemcpyAsync(off, Q.run[live].off.p, (size_t)(Q.n_hosts + 1) * 4, hipMemcpyDeviceToHost, s));
        else std::memset(off, 0, (size_t)(Q.n_hosts + 1) * 4);
    }
    if (n && live >= 0) {
        const EqRunBuf& R = Q.run[live];
        if (deliver) SHD_HIP(hipMemcpyAsync(deliver, R.deliver.p, n * 8, hipMemcpyDeviceToHost, s));
        if (src) SHD_HIP(hipMemcpyAsync(src, R.src.p, n * 4, hipMemcpyDeviceToHost, s));
        if (seq) SHD_HIP(hipMemcpyAsync(seq, R.seq.p, n * 8, hipMemcpyDeviceToHost, s));
        if (tag) SHD_HIP(hipMemcpyAsync(tag, R.tag.p, n * 8, hipMemcpyDeviceToHost, s));
    }
    SHD_HIP(hipStreamSynchronize(s));
    return SHD_OK;
}

}  // extern "C"
