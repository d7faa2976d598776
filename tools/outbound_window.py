"""Time the outbound stage on a C5-shaped window: the counterpart of tools/inbound_window.py, with
the same host and event counts and the same window shape.

    python tools/outbound_window.py [--hosts 100000] [--per-host 100] [--windows 8] [--slow-share 0.5]
                                    [--local-share 0.0] [--swap-share 0.0] [--sockets 4]
                                    [--qdisc fifo|rr|fifo-sockets|rr-sockets] [--control-share 0.2]

Every host gets about --per-host offers per 1 ms window (sizes 20% 52 B / 60% 1500 B / 20% uniform,
times sorted per host, priorities in arrival order, destinations uniform), generated on the device.
--slow-share of the hosts have a 10 MB/s bucket (their packets block, queue up and carry from
window to window), the rest the reference's default 1 Gbit/s (125 MB/s).  --local-share of the
offers go to the offering host itself; --swap-share of the offers trade priorities with their
neighbour (inserts that shift).  --qdisc rr sets the stage up with the round-robin discipline:
each host's offers are spread over --sockets handles (uniformly, the handle in the priority
column), and --ring is still the packets a host may have queued.  --qdisc fifo-sockets and
rr-sockets set up the two disciplines over sockets with a control and a data buffer: the
priorities stay in their column, the handles (again --sockets a host) go to the socket column, and
--control-share of the offers are control packets (priority 0, a bare 52-byte header).  Each
window is one shd_outbound_advance_sockets, timed with the host clock
around the call (it returns after its pinned read-back); the first two windows are warm-up.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS = 10**6
HEADER = 52


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=100_000)
    ap.add_argument("--per-host", type=int, default=100)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--slow-share", type=float, default=0.5)
    ap.add_argument("--local-share", type=float, default=0.0)
    ap.add_argument("--swap-share", type=float, default=0.0)
    ap.add_argument("--ring", type=int, default=1024)
    ap.add_argument("--qdisc", choices=["fifo", "rr", "fifo-sockets", "rr-sockets"], default="fifo")
    ap.add_argument("--sockets", type=int, default=4)
    ap.add_argument("--control-share", type=float, default=0.2)
    a = ap.parse_args()

    import torch
    from shadow_amd.outbound import OutboundStage
    from shadow_amd.routing import Engine
    from shadow_amd.tbucket import SIM_START

    H = a.hosts
    with_sockets = a.qdisc.endswith("-sockets")
    qdisc = {"fifo": "fifo", "rr": "round-robin", "fifo-sockets": "fifo-sockets", "rr-sockets": "round-robin-sockets"}
    g = torch.Generator(device="cuda").manual_seed(5)

    def window(start, w):
        """One window's offers on the device, each host's sorted by time."""
        lo, hi = max(a.per_host * 4 // 5, 0), a.per_host * 6 // 5 + 1
        cnt = torch.randint(lo, hi, (H,), generator=g, device="cuda")
        off = torch.zeros(H + 1, dtype=torch.int64, device="cuda")
        off[1:] = torch.cumsum(cnt, 0)
        n = int(off[-1])
        host = torch.repeat_interleave(torch.arange(H, device="cuda"), cnt)
        key, _ = torch.sort(host * MS + torch.randint(0, MS, (n,), generator=g, device="cuda"))
        t = start + (key - host * MS)
        u = torch.rand(n, generator=g, device="cuda")
        size = torch.where(u < 0.2, 52, torch.where(u < 0.8, 1500, torch.randint(HEADER, 1501, (n,), generator=g,
                                                                                   device="cuda")))
        idx = torch.arange(n, device="cuda")
        prio = idx + (w << 32)               # increasing per host and across windows
        sock = None
        if a.qdisc == "rr":                  # the column is the socket's handle: host << 16 | one of K
            prio = (host << 16) | torch.randint(0, a.sockets, (n,), generator=g, device="cuda")
        if with_sockets:                     # the handle in a column of its own; control packets have priority 0
            sock = ((host << 16) | torch.randint(0, a.sockets, (n,), generator=g, device="cuda")).contiguous()
            control = torch.rand(n, generator=g, device="cuda") < a.control_share
            prio = torch.where(control, 0, prio + 1)   # (the host's counter starts at 1: 0 is the control packets')
            size = torch.where(control, HEADER, size)
        if a.swap_share > 0 and a.qdisc == "fifo":   # neighbours of one host trade priorities
            first = torch.repeat_interleave(off[:-1], cnt)
            even = ((idx - first) & 1) == 0
            last = idx + 1 >= torch.repeat_interleave(off[1:], cnt)
            pick = even & ~last & (torch.rand(n, generator=g, device="cuda") < 2 * a.swap_share)
            up = torch.nonzero(pick).flatten()
            prio[up], prio[up + 1] = prio[up + 1].clone(), prio[up].clone()
        dst = torch.randint(0, H, (n,), generator=g, device="cuda")
        if a.local_share > 0:
            dst = torch.where(torch.rand(n, generator=g, device="cuda") < a.local_share, host, dst)
        pkt = (idx + w * 50_000_000).int()
        return off.int(), t.contiguous(), prio.contiguous(), size.int(), (size - HEADER).int(), dst.int(), pkt, n, sock

    rates = [10_000_000 if h < a.slow_share * H else 125_000_000 for h in range(H)]
    with Engine(0) as eng:
        stage = OutboundStage.from_bandwidth(eng, rates, SIM_START, ring_capacity=a.ring,
                                             qdisc=qdisc[a.qdisc],
                                             max_sockets=max(a.sockets, 1))
        ms, outs, n_ops = [], [], 0
        start = SIM_START
        for w in range(a.windows):
            *arr, n, sock = window(start, w)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = stage.advance_device(*arr, n, start + MS, d_sock=sock)
            ms.append((time.perf_counter() - t0) * 1e3)
            outs.append((n, r.n_sent, r.n_local, r.n_stored))
            n_ops = n
            start += MS
    timed = ms[2:] if len(ms) > 2 else ms
    print(json.dumps({"hosts": H, "offers_per_window": n_ops, "qdisc": a.qdisc,
                      "sockets": a.sockets if a.qdisc != "fifo" else None,
                      "control_share": a.control_share if with_sockets else None, "slow_share": a.slow_share,
                      "local_share": a.local_share, "swap_share": a.swap_share,
                      "outbound_ms": [round(x, 3) for x in ms],
                      "outbound_ms_median": round(statistics.median(timed), 3),
                      "outbound_ms_min": round(min(timed), 3), "outbound_ms_max": round(max(timed), 3),
                      "per_window_offers_sent_local_stored": outs}))


if __name__ == "__main__":
    main()
