// The packet ledger: each relay batch's (total size, packet id) per packet, kept on the device
// from the round that sent the batch until its last event has popped from the destination event
// queues.  A popped event carries only its tag, (batch number << 32) | index in that batch; the
// inbound stage wants the packet's total size and the caller's packet id.  ledger_gather turns a
// window's popped tags into those two arrays without the host seeing a packet.
//
// Storage (the bookkeeping is ledger_book.h's):
//   arena   uint2 {size, pkt} entries; a batch is one contiguous slice, written by ledger_record
//   rows    LedgerRow {batch, base, n_packets, live} per slot = batch & mask; the batches held are
//           the numbers oldest .. oldest + span - 1, row d = batch - oldest.  A gather only reads
//           the rows: `live` is the count at the call's start for every workgroup alike
//   pops    per slot, the running gather's pops; ledger_settle takes them off the rows' live
//           counts, zeroes them and writes every held batch's new count behind the status word,
//           which the call reads back once: that is how the host learns which batches are gone
//
// ledger_gather, a workgroup per 1024 events, four per thread (two 16-byte tag loads):
//   A  the first kLgRows rows of the span -> LDS; per event the row, the checks, the dependent
//      8-byte entry load (issued here, used in C); the pops counted per wave: the lanes that name
//      one batch are found with __ballot and their leader adds the count to the batch's LDS
//      counter -- one LDS add per wave and distinct batch, where a per-event add would put 64
//      lanes on one word (a window's pops come from a handful of batches, often from one)
//   B  one global atomicAdd per workgroup and touched batch onto pops[slot]; a sum past the row's
//      live count marks the batch overdrawn for this workgroup
//   C  two coalesced 8-byte stores per thread and vector (sizes, ids)
// A batch at row kLgRows or beyond (more batches held than the LDS table has rows) takes the same
// path with its row read from global memory and its wave's count added to pops[slot] directly.
//
// Every index is checked before it is used for a load: a tag whose batch is not held or has no
// live event left, an index >= the batch's n_packets (or an entry past the arena, which the
// bookkeeping rules out), a batch popped more often than its live count.  Such an event gets
// UINT32_MAX in both outputs and the call fails; nothing is read for it.  Of an overdrawn batch
// the events of every workgroup (row >= kLgRows: wave) whose count went past the live count are
// refused -- at least the surplus; which ones depends on the order the atomics landed in.
#include <algorithm>
#include <cstdint>

#include "ctx.h"

namespace shd {

constexpr uint32_t kLgThreads = 256;
constexpr uint32_t kLgVec = 2;                            // 16-byte tag loads per thread
constexpr uint32_t kLgTile = kLgThreads * kLgVec * 2;     // events per workgroup
constexpr uint32_t kLgRows = 1024;                        // rows (and counters) in LDS: 16 + 4 KB
constexpr uint32_t kLgMaxBatches = 4096;
constexpr uint64_t kLgArena0 = 65536;                     // the arena's first size, entries
// status bits (words[0]); any of them is SHD_ERR_INVALID
constexpr uint32_t kLgNotLive = 1u;     // the tag's batch is not held, or has no live event left
constexpr uint32_t kLgBadIndex = 2u;    // index >= the batch's n_packets
constexpr uint32_t kLgOverdrawn = 4u;   // a batch popped more often than its live count
static_assert(sizeof(LedgerRow) == 16, "LedgerRow layout");

__global__ __launch_bounds__(256) void ledger_record(const uint32_t* __restrict__ size, const uint32_t* __restrict__ pkt,
                                                     uint64_t n, uint2* __restrict__ slice, LedgerRow* row_slot,
                                                     LedgerRow row) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) slice[i] = make_uint2(size[i], pkt[i]);
    if (i == 0) *row_slot = row;
}

// The lanes with ok set name row d; per distinct d one lane adds the lanes' count: to the LDS
// counter (d < nl), or to the slot's global counter, whose answer decides `over` for those lanes.
__device__ __forceinline__ bool lg_count(bool ok, uint32_t d, uint32_t nl, uint32_t* s_cnt, uint32_t* pop_slot,
                                         uint32_t live) {
    const uint32_t lane = threadIdx.x & 63;
    bool over = false;
    uint64_t todo = __ballot(ok);
    while (todo) {   // (todo is the same in every lane: the loop does not diverge)
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t kd = (uint32_t)__shfl((int)d, leader);
        const bool same = ok && d == kd;
        const uint64_t m = __ballot(same);
        const uint32_t c = (uint32_t)__popcll(m);
        uint32_t ov = 0;
        if (lane == (uint32_t)leader) {
            if (kd < nl) atomicAdd(&s_cnt[kd], c);
            else ov = atomicAdd(pop_slot, c) + c > live ? 1u : 0u;
        }
        ov = (uint32_t)__shfl((int)ov, leader);
        if (same && ov) over = true;
        todo &= ~m;
    }
    return over;
}

__global__ __launch_bounds__(256) void ledger_gather(
    const uint64_t* __restrict__ tag, uint64_t n, int vec_ok, const LedgerRow* __restrict__ rows, uint32_t mask,
    uint64_t oldest, uint32_t span, const uint2* __restrict__ arena, uint64_t arena_cap, uint32_t* pops,
    uint32_t* __restrict__ out_size, uint32_t* __restrict__ out_pkt, uint32_t* status) {
    __shared__ LedgerRow s_row[kLgRows];
    __shared__ uint32_t s_cnt[kLgRows];
    const uint32_t nl = min(span, kLgRows);
    for (uint32_t i = threadIdx.x; i < nl; i += kLgThreads) {
        s_row[i] = rows[(uint32_t)(oldest + i) & mask];
        s_cnt[i] = 0;
    }
    __syncthreads();
    const uint64_t tile = (uint64_t)blockIdx.x * kLgTile;
    uint32_t d[kLgVec][2];
    bool ok[kLgVec][2], over[kLgVec][2];
    uint2 ent[kLgVec][2];
    uint32_t err = 0;
#pragma unroll
    for (uint32_t v = 0; v < kLgVec; ++v) {
        const uint64_t i0 = tile + (uint64_t)v * (kLgThreads * 2) + threadIdx.x * 2;
        uint64_t t[2] = {0, 0};
        if (vec_ok && i0 + 1 < n) {
            const ulonglong2 q = *reinterpret_cast<const ulonglong2*>(tag + i0);
            t[0] = q.x;
            t[1] = q.y;
        } else {
            if (i0 < n) t[0] = tag[i0];
            if (i0 + 1 < n) t[1] = tag[i0 + 1];
        }
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {
            const bool valid = i0 + k < n;
            const uint64_t b = t[k] >> 32;
            const uint32_t ix = (uint32_t)t[k];
            const uint64_t dd = b - oldest;           // (b < oldest: wraps far past span)
            const bool inspan = valid && dd < span;
            d[v][k] = inspan ? (uint32_t)dd : 0u;
            LedgerRow r{kLedgerNoBatch, 0, 0, 0};
            if (inspan) r = d[v][k] < nl ? s_row[d[v][k]] : rows[(uint32_t)b & mask];
            const bool held = inspan && r.batch == (uint32_t)b && r.live > 0;
            const uint64_t at = (uint64_t)r.base + ix;
            const bool good = held && ix < r.n_packets && at < arena_cap;
            if (valid && !held) err |= kLgNotLive;
            else if (valid && !good) err |= kLgBadIndex;
            ok[v][k] = good;
            ent[v][k] = make_uint2(~0u, ~0u);
            if (good) ent[v][k] = arena[at];
            over[v][k] = lg_count(good, d[v][k], nl, s_cnt, pops + ((uint32_t)b & mask), r.live);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nl; i += kLgThreads) {
        const uint32_t c = s_cnt[i];
        if (c) {
            const uint32_t old = atomicAdd(pops + ((uint32_t)(oldest + i) & mask), c);
            s_cnt[i] = old + c > s_row[i].live ? 1u : 0u;   // from here on: the batch is overdrawn
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t v = 0; v < kLgVec; ++v) {
        const uint64_t i0 = tile + (uint64_t)v * (kLgThreads * 2) + threadIdx.x * 2;
        uint2 o[2];
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {
            const bool ov = ok[v][k] && (d[v][k] < nl ? s_cnt[d[v][k]] != 0 : over[v][k]);
            if (ov) err |= kLgOverdrawn;
            o[k] = ok[v][k] && !ov ? ent[v][k] : make_uint2(~0u, ~0u);
        }
        if (i0 + 1 < n) {   // (engine-owned outputs: 8-byte aligned at every even index)
            *reinterpret_cast<uint2*>(out_size + i0) = make_uint2(o[0].x, o[1].x);
            *reinterpret_cast<uint2*>(out_pkt + i0) = make_uint2(o[0].y, o[1].y);
        } else if (i0 < n) {
            out_size[i0] = o[0].x;
            out_pkt[i0] = o[0].y;
        }
    }
    if (err) atomicOr(status, err);
}

// Row d of the span: its pops come off its live count (an overdrawn batch keeps its count and
// fails the call), the slot's counter is zero again, the new count goes behind the status word.
__global__ __launch_bounds__(256) void ledger_settle(LedgerRow* rows, uint32_t mask, uint64_t oldest, uint32_t span,
                                                     uint32_t* pops, unsigned long long* words) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= span) return;
    const uint32_t slot = (uint32_t)(oldest + i) & mask;
    const uint32_t p = pops[slot];
    pops[slot] = 0;
    LedgerRow r = rows[slot];
    unsigned long long live = ~0ull;   // no batch of this number is held
    if (r.batch == (uint32_t)(oldest + i)) {
        if (p > r.live) atomicOr(reinterpret_cast<uint32_t*>(words), kLgOverdrawn);
        else r.live -= p;
        rows[slot].live = r.live;
        live = r.live;
    }
    words[1 + i] = live;
}

static shd_status ledger_live(shd_ctx* ctx, LedgerState** out) {
    if (!ctx) return SHD_ERR_INVALID;
    if (!ctx->ledger.ready) return SHD_ERR_STATE;   // not set up, or a refused event since
    *out = &ctx->ledger;
    return SHD_OK;
}

// the arena takes n more entries: its contents move to the front of a larger one, the rows follow
static shd_status ledger_grow(shd_ctx* ctx, LedgerState& L, uint64_t n) {
    hipStream_t s = ctx->stream;
    const LedgerMove m = L.book.plan_grow(n);
    if (m.new_cap >= 0xFFFFFFFFull) return SHD_ERR_NOMEM;   // bases are 32-bit
    DevBuf bigger;
    SHD_TRY(bigger.ensure(m.new_cap * sizeof(uint2)));
    for (int k = 0; k < 2; ++k)
        if (m.len[k])
            SHD_HIP(hipMemcpyAsync(bigger.as<uint2>() + m.dst[k], L.arena.as<uint2>() + m.src[k], m.len[k] * sizeof(uint2),
                                   hipMemcpyDeviceToDevice, s));
    L.book.apply_grow(m);
    SHD_HIP(hipMemcpyAsync(L.rows.p, L.book.rows.data(), L.book.rows.size() * sizeof(LedgerRow), hipMemcpyHostToDevice, s));
    SHD_HIP(hipStreamSynchronize(s));   // the copies have read the old arena before it is freed
    L.arena = std::move(bigger);
    return SHD_OK;
}

}  // namespace shd

using namespace shd;

extern "C" {

shd_status shd_ledger_setup(shd_ctx* ctx, uint32_t max_live_batches) {
    if (!ctx || max_live_batches > kLgMaxBatches) return SHD_ERR_INVALID;
    LedgerState& L = ctx->ledger;
    L.ready = false;
    ctx->win.opened = false;   // a window sequence starts over with its ledger
    ctx->win.has_out = false;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    L.book.setup(max_live_batches ? max_live_batches : 1024, kLgArena0);
    const size_t slots = L.book.rows.size();
    SHD_TRY(L.arena.ensure(kLgArena0 * sizeof(uint2)));
    SHD_TRY(L.rows.ensure(slots * sizeof(LedgerRow)));
    SHD_TRY(L.pops.ensure(slots * 4));
    SHD_TRY(L.words.ensure((1 + (size_t)kLgMaxBatches) * 8));
    SHD_TRY(L.pin.ensure((1 + (size_t)kLgMaxBatches) * 8));
    SHD_TRY(L.g_size.ensure(16));
    SHD_TRY(L.g_pkt.ensure(16));
    SHD_HIP(hipMemsetAsync(L.rows.p, 0xFF, slots * sizeof(LedgerRow), s));   // every slot: no batch
    SHD_HIP(hipMemsetAsync(L.pops.p, 0, slots * 4, s));
    SHD_HIP(hipStreamSynchronize(s));
    L.ready = true;
    return SHD_OK;
}

shd_status shd_ledger_record(shd_ctx* ctx, uint64_t batch, const uint32_t* d_size, const uint32_t* d_pkt,
                             uint64_t n_packets, uint64_t n_live) {
    LedgerState* Lp;
    SHD_TRY(ledger_live(ctx, &Lp));
    LedgerState& L = *Lp;
    // refused before anything runs, the ledger stays as it was
    if (n_packets && (!d_size || !d_pkt)) return SHD_ERR_INVALID;
    const int what = L.book.check_record(batch, n_packets, n_live);
    if (what < 0) return SHD_ERR_INVALID;
    L.book.last = batch;
    if (what == 1) return SHD_OK;   // no event of it will pop: nothing to keep
    SHD_HIP(hipSetDevice(ctx->device));
    uint64_t base = 0;
    if (!L.book.place(n_packets, &base)) {
        SHD_TRY(ledger_grow(ctx, L, n_packets));
        if (!L.book.place(n_packets, &base)) return SHD_ERR_NOMEM;
    }
    L.book.commit_record(batch, base, n_packets, n_live);
    const LedgerRow row = L.book.row(batch);
    ledger_record<<<div_up(n_packets, 256), 256, 0, ctx->stream>>>(d_size, d_pkt, n_packets, L.arena.as<uint2>() + base,
                                                                   L.rows.as<LedgerRow>() + (batch & L.book.mask), row);
    SHD_HIP(hipGetLastError());
    return SHD_OK;
}

shd_status shd_ledger_gather(shd_ctx* ctx, const uint64_t* d_tag, uint64_t n, const uint32_t** d_size,
                             const uint32_t** d_pkt) {
    LedgerState* Lp;
    SHD_TRY(ledger_live(ctx, &Lp));
    LedgerState& L = *Lp;
    if ((n && !d_tag) || n >= 0xFFFFFFFFull) return SHD_ERR_INVALID;
    SHD_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SHD_TRY(L.g_size.ensure((n + 4) * 4));
    SHD_TRY(L.g_pkt.ensure((n + 4) * 4));
    if (d_size) *d_size = L.g_size.as<uint32_t>();
    if (d_pkt) *d_pkt = L.g_pkt.as<uint32_t>();
    if (n == 0) return SHD_OK;
    LedgerBook& B = L.book;
    const uint64_t oldest = B.oldest == kLedgerNone ? 0 : B.oldest;
    const uint32_t span = (uint32_t)B.span();
    unsigned long long* words = L.words.as<unsigned long long>();
    SHD_HIP(hipMemsetAsync(words, 0, 8, s));
    ledger_gather<<<div_up(n, kLgTile), kLgThreads, 0, s>>>(
        d_tag, n, ((uintptr_t)d_tag & 15) == 0 ? 1 : 0, L.rows.as<LedgerRow>(), B.mask, oldest, span, L.arena.as<uint2>(),
        B.cap, L.pops.as<uint32_t>(), L.g_size.as<uint32_t>(), L.g_pkt.as<uint32_t>(), reinterpret_cast<uint32_t*>(words));
    SHD_HIP(hipGetLastError());
    if (span) {
        ledger_settle<<<div_up(span, 256), 256, 0, s>>>(L.rows.as<LedgerRow>(), B.mask, oldest, span, L.pops.as<uint32_t>(),
                                                        words);
        SHD_HIP(hipGetLastError());
    }
    // the status word and every held batch's live count in one read
    unsigned long long* w = L.pin.as<unsigned long long>();
    SHD_TRY(readback_into(ctx, s, words, (1 + (size_t)span) * 8, w));
    if ((uint32_t)w[0]) {
        // the good events' pops are counted, the refused ones' are not: the counts no longer say
        // what is pending -- shd_ledger_setup must run again
        L.ready = false;
        return SHD_ERR_INVALID;
    }
    for (uint32_t i = 0; i < span; ++i)
        if (w[1 + i] != ~0ull && B.holds(oldest + i)) B.set_live(oldest + i, (uint32_t)w[1 + i]);
    B.reclaim();
    return SHD_OK;
}

shd_status shd_ledger_stats(shd_ctx* ctx, uint64_t* live_batches, uint64_t* live_events, uint64_t* entries_held,
                            uint64_t* oldest_batch) {
    LedgerState* Lp;
    SHD_TRY(ledger_live(ctx, &Lp));
    const LedgerBook& B = Lp->book;
    if (live_batches) *live_batches = B.live_batches;
    if (live_events) *live_events = B.live_events;
    if (entries_held) *entries_held = B.entries_held;
    if (oldest_batch) *oldest_batch = B.oldest;
    return SHD_OK;
}

}  // extern "C"
