// Drives shadow_amd/csrc/sock_queue.h -- the functions outbound.hip's two socket instances compile
// -- from a script on stdin: tests/test_outbound_sock.py builds this with the address and
// undefined-behaviour sanitizers and holds its answers against tests/outbound_sock_model.py.  The
// pool has exactly `cap` slots and the socket array exactly `max_sockets` entries, each an
// allocation of its own, so the sanitizer finds an index that leaves either.
//
//   setup <cap> <max_sockets> <fifo: 1 | 0>
//   offer <handle> <prio> <pkt> <size> <payload> <dst>   -> "ok" | "full" | "sockets"
//   pop                                           -> "<pkt> <size> <payload> <dst>" | "empty"
//   state   -> "<packets> <sockets> <head pkt | -1> <bump> :" then " <handle>:<count>" per socket, the
//              heap array in index order (fifo) or the rrQueue in order
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "sock_queue.h"

int main() {
    shd::SqQueue q;
    shd::sq_init(q);
    shd::SqSlot* pool = nullptr;
    shd::SqSock* socks = nullptr;
    uint32_t cap = 0, ms = 0;
    int fifo = 1;
    std::string op;
    while (std::cin >> op) {
        if (op == "setup") {
            std::cin >> cap >> ms >> fifo;
            delete[] pool;
            delete[] socks;
            pool = new shd::SqSlot[cap];
            socks = new shd::SqSock[ms];
            shd::sq_init(q);
        } else if (op == "offer") {
            uint64_t handle, prio;
            uint32_t pkt, size, payload, dst;
            std::cin >> handle >> prio >> pkt >> size >> payload >> dst;
            const shd::SqOffer o = shd::sq_offer(q, pool, cap, socks, ms, fifo != 0, handle, prio, pkt, size, payload, dst);
            std::puts(o == shd::kSqOk ? "ok" : o == shd::kSqPoolFull ? "full" : "sockets");
        } else if (op == "pop") {
            if (q.count == 0) {
                std::puts("empty");
                continue;
            }
            uint32_t pkt, size, payload, dst;
            shd::sq_pop(q, pool, socks, ms, fifo != 0, pkt, size, payload, dst);
            std::printf("%u %u %u %u\n", pkt, size, payload, dst);
        } else if (op == "state") {
            std::vector<uint64_t> handles(ms);
            std::vector<uint32_t> counts(ms);
            const uint32_t n = shd::sq_counts(q, pool, cap, socks, ms, fifo != 0, handles.data(), counts.data(), ms);
            const long long head = q.count ? (long long)shd::sq_head_pkt(q, pool, socks, ms, fifo != 0) : -1ll;
            std::printf("%u %u %lld %u :", q.count, n, head, q.bump);
            for (uint32_t i = 0; i < n; ++i) std::printf(" %llu:%u", (unsigned long long)handles[i], counts[i]);
            std::puts("");
        } else {
            std::printf("unknown op %s\n", op.c_str());
            return 2;
        }
    }
    delete[] pool;
    delete[] socks;
    return 0;
}
