// Drives shadow_amd/csrc/ledger_book.h from a script on stdin, with a host array standing in for
// the device arena: tests/test_ledger.py builds this with the address and undefined-behaviour
// sanitizers and holds its answers against tests/ledger_model.py.  An entry is
// (batch << 32) | index, so `verify` finds a slice that another batch has overwritten, and an
// arena of exactly `cap` entries lets the sanitizer find a slice that leaves it.
//
//   setup <max_live> <arena entries>
//   record <batch> <n_packets> <n_live>   -> "stored <base> <grew 0|1>" | "nothing" | "refused"
//   pop <batch> <k>                       -> "ok" | "bad"   (k events of the batch popped, then a reclaim)
//   stats                                 -> live_batches live_events entries_held oldest(-1: none) cap wrapped
//   verify                                -> "ok <batches checked>" | "corrupt <batch>"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

#include "ledger_book.h"

int main() {
    shd::LedgerBook B;
    uint64_t* arena = nullptr;
    std::string op;
    while (std::cin >> op) {
        if (op == "setup") {
            uint32_t m;
            uint64_t cap;
            std::cin >> m >> cap;
            delete[] arena;
            arena = new uint64_t[cap];
            B.setup(m, cap);
        } else if (op == "record") {
            uint64_t b, n, live;
            std::cin >> b >> n >> live;
            const int what = B.check_record(b, n, live);
            if (what < 0) {
                std::puts("refused");
                continue;
            }
            B.last = b;
            if (what == 1) {
                std::puts("nothing");
                continue;
            }
            uint64_t base = 0;
            int grew = 0;
            if (!B.place(n, &base)) {
                const shd::LedgerMove m = B.plan_grow(n);
                uint64_t* bigger = new uint64_t[m.new_cap];
                for (int k = 0; k < 2; ++k)
                    if (m.len[k]) std::memcpy(bigger + m.dst[k], arena + m.src[k], m.len[k] * 8);
                B.apply_grow(m);
                delete[] arena;
                arena = bigger;
                grew = 1;
                if (!B.place(n, &base)) {
                    std::puts("no room after a growth");
                    return 1;
                }
            }
            B.commit_record(b, base, n, live);
            for (uint64_t i = 0; i < n; ++i) arena[base + i] = (b << 32) | i;
            std::printf("stored %llu %d\n", (unsigned long long)base, grew);
        } else if (op == "pop") {
            uint64_t b, k;
            std::cin >> b >> k;
            if (!B.holds(b) || B.row(b).live < k) {
                std::puts("bad");
                continue;
            }
            B.set_live(b, (uint32_t)(B.row(b).live - k));
            B.reclaim();
            std::puts("ok");
        } else if (op == "stats") {
            std::printf("%llu %llu %llu %lld %llu %d\n", (unsigned long long)B.live_batches,
                        (unsigned long long)B.live_events, (unsigned long long)B.entries_held,
                        B.oldest == shd::kLedgerNone ? -1ll : (long long)B.oldest, (unsigned long long)B.cap,
                        B.wrapped ? 1 : 0);
        } else if (op == "verify") {
            uint64_t checked = 0, corrupt = shd::kLedgerNone;
            if (B.oldest != shd::kLedgerNone)
                for (uint64_t b = B.oldest; b <= B.newest && corrupt == shd::kLedgerNone; ++b) {
                    if (!B.holds(b)) continue;
                    const shd::LedgerRow& r = B.row(b);
                    for (uint64_t i = 0; i < r.n_packets; ++i)
                        if (arena[(uint64_t)r.base + i] != ((b << 32) | i)) corrupt = b;
                    ++checked;
                }
            if (corrupt != shd::kLedgerNone) std::printf("corrupt %llu\n", (unsigned long long)corrupt);
            else std::printf("ok %llu\n", (unsigned long long)checked);
        } else {
            std::printf("unknown op %s\n", op.c_str());
            return 2;
        }
    }
    delete[] arena;
    return 0;
}
