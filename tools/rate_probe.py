"""What the bucket re-rate costs (shd_inbound_update_buckets / shd_outbound_update_buckets), next to
the only other way to another rate: setting the stage up again, which also loses its queues.

A 100k-host inbound stage and a 100k-host outbound stage (plain FIFO, then fifo-sockets), every host
on a 1000 B/s bucket with one window's packets stored (four 1500-byte packets a host at the window's
start: one leaves, one is cached, two wait in the ring or pool).  Host-clock times around calls that
end in a device synchronise; medians over REPS repetitions after WARM warm-up ones.  The timed calls
are interleaved within a repetition -- re-rate of 1, 1,000 and all hosts, each to a larger and to a
smaller capacity, then the setup (after which the window is run again, untimed) -- so that drift
in the machine's load falls on every figure alike.  "shrink" calls walk the hosts' stored packets
(the capacity goes down); "grow" calls need no walk.  The first re-rate after a setup is timed apart
(it is not what a caller between two windows makes), and so is a re-rate that follows a window's
advance with no setup before it.

    python tools/rate_probe.py [inbound|fifo|fifo-sockets ...]     (default: all three)
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shadow_amd.inbound import InboundStage  # noqa: E402
from shadow_amd.outbound import OutboundStage  # noqa: E402
from shadow_amd.routing import Engine  # noqa: E402
from shadow_amd.tbucket import SIM_START as S, create_token_bucket  # noqa: E402

H, PER_HOST, REPS, WARM = 100_000, 4, 15, 3
MS = 1_000_000
SMALL, LARGE = create_token_bucket(1000), create_token_bucket(500_000)   # capacities 1501 and 2000


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()


def window_arrays():
    """Four 1500-byte packets per host at the window's start, to another host."""
    n = H * PER_HOST
    host = np.repeat(np.arange(H, dtype=np.uint32), PER_HOST)
    off = np.arange(0, n + 1, PER_HOST, dtype=np.uint32)
    return dict(off=dev(off, np.int32), time=dev(np.full(n, S, np.uint64), np.int64),
                prio=dev(np.arange(1, n + 1, dtype=np.uint64), np.int64), sock=dev(host.astype(np.uint64) + 7, np.int64),
                size=dev(np.full(n, 1500, np.uint32), np.int32), payload=dev(np.full(n, 1448, np.uint32), np.int32),
                dst=dev((host + 1) % H, np.int32), pkt=dev(np.arange(n, dtype=np.uint32), np.int32), n=n)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def probe(name, make, fill, tick):
    """make() -> a fresh stage (the timed setup); fill(stage) runs the window that stores the packets;
    tick(stage, end) runs a window without offers up to `end`."""
    rng = np.random.default_rng(3)
    stage = make()
    stored = fill(stage)
    at = S + 10 * MS   # the window's end: every call re-rates there (at == last_refill afterwards)
    picks = {k: np.sort(rng.permutation(H)[:k]).astype(np.uint32) for k in (1, 1000, H)}
    cols = {(k, which): tuple(np.full(k, v, np.uint64) for v in rows) for k in picks
            for which, rows in (("grow", LARGE), ("shrink", SMALL))}
    ts = {key: [] for key in cols}
    ts["setup"], ts["first"] = [], []
    for rep in range(WARM + REPS):
        # the first call after a setup and a window, apart: it also waits for what they left behind
        t = timed(lambda: stage.update_buckets(picks[1], *cols[(1, "grow")], at))
        stage.update_buckets(picks[1], *cols[(1, "shrink")], at)
        if rep >= WARM:
            ts["first"].append(t)
        for k in picks:
            for which in ("grow", "shrink"):   # 1501 -> 2000 -> 1501: every call changes every named host
                t = timed(lambda: stage.update_buckets(picks[k], *cols[(k, which)], at))
                if rep >= WARM:
                    ts[(k, which)].append(t)
        box = []
        t = timed(lambda: box.append(make()))
        if rep >= WARM:
            ts["setup"].append(t)
        stage = box[0]
        assert fill(stage) == stored
    # what a caller between two windows sees: a window (no setup), then the re-rate at its end
    after = []
    for rep in range(WARM + REPS):
        end = at + (rep + 1) * MS
        tick(stage, end)
        t = timed(lambda: stage.update_buckets(picks[1000], *cols[(1000, "grow" if rep % 2 == 0 else "shrink")], end))
        if rep >= WARM:
            after.append(t)
    print(f"== {name}: {H} hosts, {stored} packets stored ==")
    print(f"{name} re-rate n=  1000 right after a window's advance (no setup before): {np.median(after):7.3f} ms")
    for k in picks:
        g, s = np.median(ts[(k, "grow")]), np.median(ts[(k, "shrink")])
        print(f"{name} re-rate n={k:>6}: grow {g:7.3f} ms | shrink (walks the stored packets) {s:7.3f} ms")
    print(f"{name} the first re-rate (n=1) after a setup and a window: {np.median(ts['first']):7.3f} ms")
    su = np.median(ts["setup"])
    print(f"{name} setup again (loses the {stored} stored packets): {su:7.3f} ms | setup / re-rate of all hosts "
          f"{su / np.median(ts[(H, 'shrink')]):5.1f}x", flush=True)


def main(what):
    rows = tuple(np.full(H, v, np.uint64) for v in SMALL)
    with Engine(0) as eng:
        w = window_arrays()
        torch.cuda.synchronize()
        if "inbound" in what:
            probe("inbound", lambda: InboundStage(eng, *rows, S, ring_capacity=8),
                  lambda st: st.advance_device(w["off"], w["time"], w["size"], w["pkt"], w["n"], S + 10 * MS).n_stored,
                  lambda st, end: st.advance_device(None, None, None, None, 0, end))
        for q in ("fifo", "fifo-sockets"):
            if q in what:
                probe(f"outbound {q}", lambda q=q: OutboundStage(eng, *rows, S, ring_capacity=8, qdisc=q, max_sockets=4),
                      lambda st: st.advance_device(w["off"], w["time"], w["prio"], w["size"], w["payload"], w["dst"],
                                                   w["pkt"], w["n"], S + 10 * MS, d_sock=w["sock"]).n_stored,
                      lambda st, end: st.advance_device(None, None, None, None, None, None, None, 0, end))


if __name__ == "__main__":
    main(sys.argv[1:] or ["inbound", "fifo", "fifo-sockets"])
