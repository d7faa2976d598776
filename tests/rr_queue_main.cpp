// Drives shadow_amd/csrc/rr_queue.h -- the functions outbound.hip's round-robin instance compiles
// -- from a script on stdin: tests/test_outbound_rr.py builds this with the address and
// undefined-behaviour sanitizers and holds its answers against tests/outbound_rr_model.py.  The
// pool has exactly `cap` slots and the socket ring exactly `max_sockets` entries, each an
// allocation of its own, so the sanitizer finds an index that leaves either.
//
//   setup <cap> <max_sockets>
//   offer <handle> <pkt> <size> <payload> <dst>   -> "ok" | "full" | "sockets"
//   pop                                           -> "<pkt> <size> <payload> <dst>" | "empty"
//   state   -> "<packets> <sockets> <head pkt | -1> <bump> :" then " <handle>:<count>" per socket in order
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "rr_queue.h"

int main() {
    shd::RrQueue q;
    shd::rr_init(q);
    shd::RrSlot* pool = nullptr;
    shd::RrSock* ring = nullptr;
    uint32_t cap = 0, ms = 0;
    std::string op;
    while (std::cin >> op) {
        if (op == "setup") {
            std::cin >> cap >> ms;
            delete[] pool;
            delete[] ring;
            pool = new shd::RrSlot[cap];
            ring = new shd::RrSock[ms];
            shd::rr_init(q);
        } else if (op == "offer") {
            uint64_t handle;
            uint32_t pkt, size, payload, dst;
            std::cin >> handle >> pkt >> size >> payload >> dst;
            const shd::RrOffer o = shd::rr_offer(q, pool, cap, ring, ms, handle, pkt, size, payload, dst);
            std::puts(o == shd::kRrOk ? "ok" : o == shd::kRrPoolFull ? "full" : "sockets");
        } else if (op == "pop") {
            if (q.count == 0) {
                std::puts("empty");
                continue;
            }
            uint32_t pkt, size, payload, dst;
            shd::rr_pop(q, pool, ring, ms, pkt, size, payload, dst);
            std::printf("%u %u %u %u\n", pkt, size, payload, dst);
        } else if (op == "state") {
            std::vector<uint64_t> handles(ms);
            std::vector<uint32_t> counts(ms);
            const uint32_t n = shd::rr_counts(q, pool, cap, ring, ms, handles.data(), counts.data(), ms);
            std::printf("%u %u %lld %u :", q.count, n, q.count ? (long long)q.pkt : -1ll, q.bump);
            for (uint32_t i = 0; i < n; ++i) std::printf(" %llu:%u", (unsigned long long)handles[i], counts[i]);
            std::puts("");
        } else {
            std::printf("unknown op %s\n", op.c_str());
            return 2;
        }
    }
    delete[] pool;
    delete[] ring;
    return 0;
}
