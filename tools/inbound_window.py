"""Time the inbound stage on a C5-shaped window, with the two replay kernels for comparison.

    python tools/inbound_window.py [--hosts 100000] [--per-host 100] [--windows 8] [--slow-share 0.5]

Every host gets about --per-host packet events per 1 ms window (sizes 20% 52 B / 60% 1500 B / 20%
uniform, times sorted per host), generated on the device.  --slow-share of the hosts have a
10 MB/s bucket (their packets block, queue up and carry from window to window), the rest the
reference's default 1 Gbit/s (125 MB/s).  Each window is one shd_inbound_advance, timed with the
host clock around the call (it returns after its pinned read-back); the first two windows are
warm-up.  For comparison, on the same number of operations per call: shd_codel_run_device
(alternating push / pop per host) and shd_tb_run_device (one attempt per event, the same buckets).
Prints one JSON line."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS = 10**6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=100_000)
    ap.add_argument("--per-host", type=int, default=100)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--slow-share", type=float, default=0.5)
    ap.add_argument("--ring", type=int, default=1024)
    a = ap.parse_args()

    import numpy as np
    import torch
    from shadow_amd import _native as N
    from shadow_amd.codel import POP, CoDelQueues
    from shadow_amd.inbound import InboundStage
    from shadow_amd.routing import Engine
    from shadow_amd.tbucket import SIM_START, TokenBuckets, create_token_bucket

    H = a.hosts
    g = torch.Generator(device="cuda").manual_seed(5)

    def window(start):
        """(off, time, size) of one window's events on the device, each host's sorted by time."""
        lo, hi = max(a.per_host * 4 // 5, 0), a.per_host * 6 // 5 + 1
        cnt = torch.randint(lo, hi, (H,), generator=g, device="cuda")
        off = torch.zeros(H + 1, dtype=torch.int64, device="cuda")
        off[1:] = torch.cumsum(cnt, 0)
        n = int(off[-1])
        host = torch.repeat_interleave(torch.arange(H, device="cuda"), cnt)
        key, _ = torch.sort(host * MS + torch.randint(0, MS, (n,), generator=g, device="cuda"))
        t = start + (key - host * MS)
        u = torch.rand(n, generator=g, device="cuda")
        size = torch.where(u < 0.2, 52, torch.where(u < 0.8, 1500, torch.randint(1, 1501, (n,), generator=g,
                                                                                   device="cuda")))
        return off.int(), t.contiguous(), size.int(), n

    rates = [10_000_000 if h < a.slow_share * H else 125_000_000 for h in range(H)]
    with Engine(0) as eng:
        stage = InboundStage.from_bandwidth(eng, rates, SIM_START, ring_capacity=a.ring)
        ms, outs, n_ops = [], [], 0
        start = SIM_START
        for w in range(a.windows):
            off, t, size, n = window(start)
            pkt = (torch.arange(n, device="cuda") + w * 50_000_000).int()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = stage.advance_device(off, t, size, pkt, n, start + MS)
            ms.append((time.perf_counter() - t0) * 1e3)
            outs.append((n, r.n_out, r.n_stored))
            n_ops = n
            start += MS
        # the replay kernels on one window's worth of operations
        off, t, size, n = window(SIM_START)
        idx = torch.arange(n, device="cuda")
        first = torch.repeat_interleave(off[:-1].long(), (off[1:] - off[:-1]).long())
        is_pop = ((idx - first) & 1) == 1
        csize = torch.where(is_pop, torch.full_like(size, -1), size)   # -1 = SHD_CODEL_POP as u32
        assert POP == 0xFFFFFFFF
        q = CoDelQueues(eng, H, a.ring)
        pop_out = torch.empty(n, dtype=torch.int32, device="cuda")
        fate = torch.zeros(n, dtype=torch.int64, device="cuda")
        cpkt = idx.int()
        ops = N.CodelOps(n, N.ptr(off).value, N.ptr(t).value, N.ptr(csize).value, N.ptr(cpkt).value)
        cms = []
        for k in range(3):
            if k:   # times must not go back: a fresh set of queues per repeat
                q = CoDelQueues(eng, H, a.ring)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            N.check(eng.lib.shd_codel_run_device(eng.ctx, C.byref(ops), N.ptr(pop_out), N.ptr(fate), n), "codel")
            cms.append((time.perf_counter() - t0) * 1e3)
        rows = [create_token_bucket(b) for b in rates]
        tms = []
        flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        value = torch.empty(n, dtype=torch.int64, device="cuda")
        tops = N.TbOps(n, N.ptr(off).value, N.ptr(t).value, N.ptr(size).value, N.ptr(flags).value)
        for k in range(3):
            TokenBuckets(eng, np.array([r[0] for r in rows], np.uint64), np.array([r[1] for r in rows], np.uint64),
                         np.array([r[2] for r in rows], np.uint64), SIM_START)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            N.check(eng.lib.shd_tb_run_device(eng.ctx, C.byref(tops), N.ptr(status), N.ptr(value)), "tb")
            tms.append((time.perf_counter() - t0) * 1e3)
    timed = ms[2:] if len(ms) > 2 else ms
    print(json.dumps({"hosts": H, "events_per_window": n_ops, "slow_share": a.slow_share,
                      "inbound_ms": [round(x, 3) for x in ms], "inbound_ms_median": round(statistics.median(timed), 3),
                      "inbound_ms_min": round(min(timed), 3),
                      "per_window_events_out_stored": outs,
                      "codel_run_ms": [round(x, 3) for x in cms], "tb_run_ms": [round(x, 3) for x in tms]}))


if __name__ == "__main__":
    main()
