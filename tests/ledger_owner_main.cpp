// shard_owner (shadow_amd/csrc/shard.h) on its own: for every total 1 .. max_total and world
// 1 .. max_world one line "total world o(0) o(1) ... o(total)" -- every host's owner and, last,
// the owner of the index one past the hosts.  tests/test_ledger_owner.py holds the lines against
// shd_shard_range.
#include <cstdio>
#include <cstdlib>

#include "shard.h"

int main(int argc, char** argv) {
    const unsigned max_total = argc > 1 ? (unsigned)std::atoi(argv[1]) : 200;
    const unsigned max_world = argc > 2 ? (unsigned)std::atoi(argv[2]) : 9;
    for (unsigned total = 1; total <= max_total; ++total)
        for (unsigned world = 1; world <= max_world; ++world) {
            std::printf("%u %u", total, world);
            for (unsigned h = 0; h <= total; ++h) std::printf(" %u", shd::shard_owner(total, world, h));
            std::printf("\n");
        }
    // the widest arguments: no overflow in the block size
    std::printf("max %u %u\n", shd::shard_owner(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu),
                shd::shard_owner(0xFFFFFFFFu, 2, 0xFFFFFFFEu));
    return 0;
}
