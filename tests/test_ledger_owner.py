"""CPU tier of the sharded ledger record: the owner of a host, the one function the pack kernel, the
remap kernel and the host code share (shadow_amd/csrc/shard.h), compiled into a program of its own
(tests/ledger_owner_main.cpp) with the address and undefined-behaviour sanitizers and held against
the library's shd_shard_range for every host of every total 1 .. 200 at worlds 1 .. 9.  The
program stands alone: nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_TOTAL, MAX_WORLD = 200, 9


@pytest.fixture(scope="module")
def owners(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ledger_owner") / "ledger_owner")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "shadow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ledger_owner_main.cpp"), "-o", exe])
    out = subprocess.run([exe, str(MAX_TOTAL), str(MAX_WORLD)], text=True, capture_output=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.splitlines()


def test_owner_is_the_inverse_of_shard_range(owners):
    from shadow_amd.dist import shard_range   # the library's own shd_shard_range (no GPU needed)
    lines = owners[:-1]
    assert len(lines) == MAX_TOTAL * MAX_WORLD
    for line in lines:
        w = [int(x) for x in line.split()]
        total, world, got = w[0], w[1], w[2:]
        assert len(got) == total + 1
        want = [None] * total
        for r in range(world):
            lo, hi = shard_range(total, world, r)
            for h in range(lo, hi):
                assert want[h] is None
                want[h] = r
        assert got[:total] == want, (total, world)
        assert 0 <= got[total] < world   # an index past the hosts still names a rank


def test_owner_takes_the_widest_arguments(owners):
    assert owners[-1].split() == ["max", str(2**32 - 2), "1"]
