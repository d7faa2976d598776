// Host bookkeeping of the packet ledger (ledger.hip): where each batch's slice lies in the arena,
// which batches are held, what a growth moves.  Free of HIP: tests/test_ledger.py compiles it
// into a program of its own and runs it under the host sanitizers.
//
// The arena is a ring of entries used in batch order.  A batch is one contiguous slice: one that
// does not fit behind the newest slice starts again at 0 (the entries behind `wrap_end` stay
// unused until the ring has passed them).  Space comes back in batch order only: a batch whose
// events have all popped is held until every older batch is gone.  Rows are addressed by the
// batch number's low bits, so the batches held span at most `max_live` consecutive numbers --
// numbers never recorded (a batch without a live event) in between included.
#pragma once
#include <cstdint>
#include <vector>

namespace shd {

constexpr uint64_t kLedgerNone = ~0ull;
constexpr uint32_t kLedgerNoBatch = ~0u;   // a row that holds no batch (batch numbers stay below it)

struct LedgerRow {   // 16 bytes, the device table's row as well
    uint32_t batch;       // the low 32 bits are the whole number: tags carry no more
    uint32_t base;        // first arena entry
    uint32_t n_packets;
    uint32_t live;        // events not yet popped
};

struct LedgerMove {   // a growth: the held entries move to the front of the new arena
    uint64_t new_cap = 0;
    uint64_t src[2] = {0, 0}, len[2] = {0, 0}, dst[2] = {0, 0};
};

struct LedgerBook {
    uint32_t max_live = 0, mask = 0;
    std::vector<LedgerRow> rows;   // slot = batch & mask
    uint64_t oldest = kLedgerNone, newest = kLedgerNone;   // held batches (kLedgerNone: none)
    uint64_t last = kLedgerNone;                           // the last number passed to a record
    uint64_t cap = 0, head = 0, tail = 0, wrap_end = 0;    // arena entries; used from head to tail
    bool wrapped = false;                                  // the used part runs head .. wrap_end, 0 .. tail
    uint64_t live_batches = 0, live_events = 0, entries_held = 0;

    void setup(uint32_t max_live_batches, uint64_t arena_entries) {
        max_live = max_live_batches;
        uint32_t r = 1;
        while (r < max_live) r <<= 1;
        mask = r - 1;
        rows.assign(r, LedgerRow{kLedgerNoBatch, 0, 0, 0});
        oldest = newest = last = kLedgerNone;
        cap = arena_entries;
        head = tail = wrap_end = 0;
        wrapped = false;
        live_batches = live_events = entries_held = 0;
    }
    LedgerRow& row(uint64_t batch) { return rows[batch & mask]; }
    const LedgerRow& row(uint64_t batch) const { return rows[batch & mask]; }
    bool holds(uint64_t batch) const {
        return oldest != kLedgerNone && batch >= oldest && batch <= newest && row(batch).batch == (uint32_t)batch;
    }
    uint64_t span() const { return oldest == kLedgerNone ? 0 : newest - oldest + 1; }

    // 0: store it; 1: nothing to store (no live event); -1: refused, nothing changes
    int check_record(uint64_t batch, uint64_t n_packets, uint64_t n_live) const {
        if (batch >= kLedgerNoBatch || (last != kLedgerNone && batch <= last)) return -1;
        if (n_packets >= 0xFFFFFFFFull || n_live > n_packets) return -1;
        if (n_live == 0) return 1;
        if (oldest != kLedgerNone && batch - oldest >= max_live) return -1;   // the table is full
        return 0;
    }
    uint64_t used() const { return wrapped ? (wrap_end - head) + tail : tail - head; }

    // the slice of the next batch; false: the arena must grow first (plan_grow / apply_grow)
    bool place(uint64_t n, uint64_t* base) {
        if (oldest == kLedgerNone) {
            head = tail = 0;
            wrapped = false;
        }
        if (!wrapped) {
            if (tail + n <= cap) {
                *base = tail;
                return true;
            }
            if (oldest != kLedgerNone && n <= head) {   // start again at the front
                wrap_end = tail;
                wrapped = true;
                tail = 0;
                *base = 0;
                return true;
            }
            return false;
        }
        if (tail + n <= head) {
            *base = tail;
            return true;
        }
        return false;
    }
    LedgerMove plan_grow(uint64_t n) const {
        LedgerMove m;
        const uint64_t need = used() + n;
        m.new_cap = cap * 2 > need ? cap * 2 : need + need / 4;
        if (oldest == kLedgerNone) return m;
        m.src[0] = head;
        m.len[0] = (wrapped ? wrap_end : tail) - head;
        m.dst[0] = 0;
        if (wrapped) {
            m.src[1] = 0;
            m.len[1] = tail;
            m.dst[1] = m.len[0];
        }
        return m;
    }
    void apply_grow(const LedgerMove& m) {   // every held row gets its new base
        if (oldest != kLedgerNone) {
            for (uint64_t b = oldest; b <= newest; ++b) {
                if (!holds(b)) continue;
                LedgerRow& r = row(b);
                // (wrapped: tail <= head, so a base at or above head lies in the first part)
                r.base = (uint32_t)(r.base >= head ? r.base - head : r.base + m.len[0]);
            }
        }
        tail = m.len[0] + m.len[1];
        head = 0;
        wrapped = false;
        cap = m.new_cap;
    }
    void commit_record(uint64_t batch, uint64_t base, uint64_t n_packets, uint64_t n_live) {
        row(batch) = LedgerRow{(uint32_t)batch, (uint32_t)base, (uint32_t)n_packets, (uint32_t)n_live};
        if (oldest == kLedgerNone) oldest = batch;
        newest = batch;
        tail = base + n_packets;
        ++live_batches;
        live_events += n_live;
        entries_held += n_packets;
    }
    // a gather's read-back: the batch's live count as the device left it
    void set_live(uint64_t batch, uint32_t live) {
        LedgerRow& r = row(batch);
        live_events -= r.live - live;
        if (r.live && !live) --live_batches;
        r.live = live;
    }
    // give back the drained batches at the old end, in batch order
    void reclaim() {
        while (oldest != kLedgerNone && row(oldest).live == 0) {
            LedgerRow& r = row(oldest);
            const uint32_t old_base = r.base;
            entries_held -= r.n_packets;
            r = LedgerRow{kLedgerNoBatch, 0, 0, 0};
            uint64_t b = oldest + 1;
            while (b <= newest && !holds(b)) ++b;
            if (b > newest) {
                oldest = newest = kLedgerNone;
                head = tail = 0;
                wrapped = false;
            } else {
                oldest = b;
                head = row(b).base;
                if (head < old_base) wrapped = false;   // the ring has passed the unused end
            }
        }
    }
};

}  // namespace shd
