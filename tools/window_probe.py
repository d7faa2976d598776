"""Time the two-call scheduling window and the packet ledger on one C5-shaped steady state.

    python tools/window_probe.py [--hosts 100000] [--per-host 100] [--windows 14] [--timed 6] [--nodes 100]
                                 [--lat-windows 6]

Every host offers about --per-host packets per 1 ms window (sizes 20% 52 B / 60% 1500 B / 20%
uniform, times sorted per host, destinations uniform; every host at the reference's default
1 Gbit/s both ways), generated on the device.  Path latencies are spread over 1 .. --lat-windows
windows, so that many batches have events pending at once and every window pops events of all of
them.  The same workload (same seeds, fresh stages) runs twice in one session:

  window    shd_window_open + shd_window_close per window
  separate  the calls the window makes, one by one, each timed: shd_equeue_advance,
            shd_ledger_gather, shd_inbound_advance (the gathered arrays: the sizes already lie on
            the device), shd_outbound_advance, shd_relay_round_device, shd_ledger_record

Host clock around each call.  Every call but the record returns after its own pinned read-back;
the record makes no host synchronisation, so its time is taken to the end of a stream
synchronisation that follows it (the launch alone is printed too).  The last --timed windows
count; the ones before fill the queues.  Prints one JSON line.

    python tools/window_probe.py --ranks N [the same options]

The same workload over N in-process ranks on one GPU (shd_comm_init_local, one host thread per
rank, each rank offering its shard's packets): the sharded open and close per window, then the
close's calls one by one -- shd_outbound_advance, shd_relay_round_sharded,
shd_ledger_record_sharded -- with the ranks entering each timed call together.  Per call the
median over the timed windows of the slowest rank's host clock.  The kernels of the sharded record
(ledger_pack_count, ledger_pack_scatter, the scan, ledger_remap, ledger_record_ent) are read from
a kernel trace of this run; the rest of the call is its sizing all-to-all with its read-back and
the exchange.  --remap-search: the record's remap by binary search instead of its inverse table.

    python tools/window_probe.py --staged THREADS [the same options]

The front door of the close, three ways on the same workload (same seeds, fresh stages each):
  (a) device   shd_window_close on offers that already lie grouped on the device (the yardstick)
  (b) staged   shd_window_close_staged from THREADS pinned per-thread stages (hosts dealt to
               threads, shuffled; 32-byte records)
  (c) host     what a caller did before: the same stages grouped by host on the CPU (numpy's stable
               sort), the seven arrays copied from pinned memory, then shd_window_close -- the
               three parts timed apart
Medians over the last --timed windows; the opens of every mode are printed too."""
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
HEADER = 52


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=100_000)
    ap.add_argument("--per-host", type=int, default=100)
    ap.add_argument("--windows", type=int, default=14)
    ap.add_argument("--timed", type=int, default=6)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--lat-windows", type=int, default=6)
    ap.add_argument("--ring", type=int, default=1024)
    ap.add_argument("--ranks", type=int, default=1)
    ap.add_argument("--remap-search", action="store_true", help="--ranks: knob LEDGER_REMAP_SEARCH=1")
    ap.add_argument("--staged", type=int, default=0, metavar="THREADS",
                    help="the close three ways: device arrays, THREADS pinned stages, host group-by + copies")
    a = ap.parse_args()
    if a.ranks > 1:
        return sharded(a)
    if a.staged:
        return staged(a)

    import numpy as np
    import torch
    from shadow_amd import _native as N
    from shadow_amd import synth
    from shadow_amd.equeue import EventQueues
    from shadow_amd.inbound import InboundStage
    from shadow_amd.ledger import PacketLedger
    from shadow_amd.outbound import OutboundStage
    from shadow_amd.relay import Relay
    from shadow_amd.rounds import Runahead
    from shadow_amd.routing import Engine
    from shadow_amd.tbucket import SIM_START
    from shadow_amd.window import Window

    H, NN = a.hosts, a.nodes
    rs = np.random.default_rng(11)
    lat = rs.integers(MS, a.lat_windows * MS + 1, (NN, NN)).astype(np.uint64)
    lat[0, 0] = MS
    loss = np.full((NN, NN), 0.01, np.float32)
    host_node = synth.c5_host_nodes(H, NN)
    rng0 = synth.host_rng_states(H, 1)
    end_time = SIM_START + 10**12

    def window(g, start, w):
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
        dst = torch.randint(0, H, (n,), generator=g, device="cuda")
        pkt = ((idx + w * 50_000_000) & 0x7FFFFFFF).int()
        return (off.int(), t.contiguous(), (idx + (w << 32)).contiguous(), size.int(), (size - HEADER).int(), dst.int(),
                pkt), n

    def setup(eng):
        parts = [Relay(host_node, rng0, np.zeros(H, np.uint64), lat, loss, engine=eng), EventQueues(eng, H),
                 Runahead(eng, False, MS),
                 OutboundStage.from_bandwidth(eng, [125_000_000] * H, SIM_START, ring_capacity=a.ring),
                 InboundStage.from_bandwidth(eng, [125_000_000] * H, SIM_START, ring_capacity=a.ring),
                 PacketLedger(eng)]
        return parts

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    res = {"hosts": H, "nodes": NN, "lat_windows": a.lat_windows}
    shape = []

    with Engine(0) as eng:   # ---- the window calls
        parts = setup(eng)
        win, led = Window(eng, H), parts[-1]
        g = torch.Generator(device="cuda").manual_seed(5)
        t_open, t_close, start = [], [], SIM_START
        for w in range(a.windows):
            arr, n = window(g, start, w)
            op, ms_o = clock(lambda: win.open(start + MS))
            cl, ms_c = clock(lambda: win.close(*arr, n, start + MS, end_time))
            t_open.append(ms_o)
            t_close.append(ms_c)
            s = led.stats()
            shape.append((n, op.n_popped, op.n_pending, cl.n_batch, cl.n_events, s.live_batches, s.entries_held))
            start += MS
        del parts

    with Engine(0) as eng:   # ---- the same calls one by one
        relay, queues, _, ostage, istage, led = parts = setup(eng)
        g = torch.Generator(device="cuda").manual_seed(5)
        names = ("equeue", "gather", "inbound", "outbound", "relay", "record", "record_launch")
        t = {k: [] for k in names}
        out, status, start = None, None, SIM_START
        for w in range(a.windows):
            arr, n = window(g, start, w)
            we = start + MS
            eq, ms = clock(lambda: queues.advance_device(out, we))
            t["equeue"].append(ms)
            (d_size, d_pkt), ms = clock(lambda: led.gather_device(eq.tag, eq.n_popped))
            t["gather"].append(ms)
            ib, ms = clock(lambda: istage.advance_device(eq.off, eq.deliver, d_size, d_pkt, eq.n_popped, we))
            t["inbound"].append(ms)
            ob, ms = clock(lambda: ostage.advance_device(*arr, n, we))
            t["outbound"].append(ms)
            out = None
            t_relay = t_rec = t_launch = 0.0
            if ob.n_sent:
                out = queues.batch_buffers(ob.n_sent)
                if status is None or len(status) < ob.n_sent:
                    status = torch.empty(ob.n_sent * 5 // 4, dtype=torch.uint8, device="cuda")
                out.status = status.data_ptr()
                rd = N.Round(we, end_time, 0)
                _, t_relay = clock(lambda: N.check(eng.lib.shd_relay_round_device(eng.ctx, C.byref(ob.batch), C.byref(rd),
                                                                                 C.byref(out)), "relay"))
                sizes = C.c_void_p()
                N.check(eng.lib.shd_outbound_sent_sizes(eng.ctx, C.byref(sizes)), "sizes")
                number = led.next_batch()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                led.record(number, sizes.value, ob.sent_pkt, ob.n_sent, out.n_sent)
                t_launch = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
                t_rec = (time.perf_counter() - t0) * 1e3
            t["relay"].append(t_relay)
            t["record"].append(t_rec)
            t["record_launch"].append(t_launch)
            start += MS
        del parts

    k = a.timed
    med = lambda x: round(statistics.median(x[-k:]), 3)  # noqa: E731
    res["per_window_offers_popped_pending_batch_events_livebatches_entries"] = shape[-k:]
    res["open_ms"], res["close_ms"] = med(t_open), med(t_close)
    res["open_plus_close_ms"] = round(res["open_ms"] + res["close_ms"], 3)
    for name in names:
        res[name + "_ms"] = med(t[name])
    res["four_stage_calls_ms"] = round(sum(res[x + "_ms"] for x in ("equeue", "inbound", "outbound", "relay")), 3)
    res["separate_sum_ms"] = round(res["four_stage_calls_ms"] + res["gather_ms"] + res["record_ms"], 3)
    res["open_ms_all"] = [round(x, 3) for x in t_open]
    res["close_ms_all"] = [round(x, 3) for x in t_close]
    res["gather_ms_all"] = [round(x, 3) for x in t["gather"]]
    print(json.dumps(res))


def staged(a):
    import numpy as np
    import torch
    from shadow_amd import synth
    from shadow_amd.equeue import EventQueues
    from shadow_amd.inbound import InboundStage
    from shadow_amd.ledger import PacketLedger
    from shadow_amd.outbound import OfferStages, OutboundStage, group_offers
    from shadow_amd.relay import Relay
    from shadow_amd.rounds import Runahead
    from shadow_amd.routing import Engine
    from shadow_amd.tbucket import SIM_START
    from shadow_amd.window import Window

    H, NN = a.hosts, a.nodes
    rs = np.random.default_rng(11)
    lat = rs.integers(MS, a.lat_windows * MS + 1, (NN, NN)).astype(np.uint64)
    lat[0, 0] = MS
    loss = np.full((NN, NN), 0.01, np.float32)
    host_node = synth.c5_host_nodes(H, NN)
    rng0 = synth.host_rng_states(H, 1)
    end_time = SIM_START + 10**12

    def window(g, start, w):   # main()'s workload
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
        dst = torch.randint(0, H, (n,), generator=g, device="cuda")
        pkt = ((idx + w * 50_000_000) & 0x7FFFFFFF).int()
        return (off.int(), t.contiguous(), (idx + (w << 32)).contiguous(), size.int(), (size - HEADER).int(), dst.int(),
                pkt), n

    def setup(eng):
        return [Relay(host_node, rng0, np.zeros(H, np.uint64), lat, loss, engine=eng), EventQueues(eng, H),
                Runahead(eng, False, MS),
                OutboundStage.from_bandwidth(eng, [125_000_000] * H, SIM_START, ring_capacity=a.ring),
                InboundStage.from_bandwidth(eng, [125_000_000] * H, SIM_START, ring_capacity=a.ring),
                PacketLedger(eng)]

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    def stages_of(arr, start, w):
        """The window's offers as the worker threads would have staged them (host memory)."""
        cols = [x.cpu().numpy() for x in arr]
        cols = [c.view(np.dtype(f"u{c.dtype.itemsize}")) for c in cols]
        return OfferStages.from_grouped(*cols, time_base=start, n_threads=a.staged, seed=w, keep_empty=1.0)

    k = a.timed
    med = lambda x: round(statistics.median(x[-k:]), 3)  # noqa: E731
    res = {"hosts": H, "nodes": NN, "lat_windows": a.lat_windows, "threads": a.staged}
    shapes = {}
    for mode in ("device", "staged", "host"):
        with Engine(0) as eng:
            parts = setup(eng)
            win = Window(eng, H)
            g = torch.Generator(device="cuda").manual_seed(5)
            t = {x: [] for x in ("open", "close", "groupby", "h2d", "bytes")}
            start, shape, pin, dev = SIM_START, [], None, None
            for w in range(a.windows):
                arr, n = window(g, start, w)
                st = stages_of(arr, start, w) if mode != "device" else None
                op, ms = clock(lambda: win.open(start + MS))
                t["open"].append(ms)
                if mode == "device":
                    cl, ms = clock(lambda: win.close(*arr, n, start + MS, end_time))
                elif mode == "staged":
                    held = st.pinned(eng.lib)
                    try:
                        cl, ms = clock(lambda: win.close_staged(held, start, start + MS, end_time))
                    finally:
                        held.free()
                    t["bytes"].append(n * 4 * st.words + 8 * sum(len(h) for h in st.run_host))
                else:
                    if pin is None:   # the caller's seven pinned arrays and their device copies, allocated once
                        room = H * (a.per_host * 6 // 5 + 1)
                        kinds = (torch.int32, torch.int64, torch.int64, torch.int32, torch.int32, torch.int32, torch.int32)
                        pin = [torch.empty(H + 1 if i == 0 else room, dtype=d, pin_memory=True) for i, d in enumerate(kinds)]
                        dev = [torch.empty(p.shape, dtype=p.dtype, device="cuda") for p in pin]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    c = group_offers(st.run_host, st.run_count, st.offers, st.words, start, H)
                    cols = (c[0], c[1], c[2], c[4], c[5], c[6], c[7])
                    t1 = time.perf_counter()
                    for p, d, col in zip(pin, dev, cols):
                        p.numpy()[:len(col)] = col.view(np.dtype(f"i{col.dtype.itemsize}"))
                        d[:len(col)].copy_(p[:len(col)], non_blocking=True)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    cl = win.close(*dev, n, start + MS, end_time)
                    ms = (time.perf_counter() - t2) * 1e3
                    t["groupby"].append((t1 - t0) * 1e3)
                    t["h2d"].append((t2 - t1) * 1e3)
                t["close"].append(ms)
                shape.append((n, op.n_popped, op.n_pending, cl.n_batch, cl.n_events, cl.n_local, cl.n_stored))
                start += MS
            del parts
        shapes[mode] = shape
        print(f"{mode}: close {med(t['close'])} ms", file=sys.stderr, flush=True)
        res[mode + "_open_ms"], res[mode + "_close_ms"] = med(t["open"]), med(t["close"])
        res[mode + "_close_ms_all"] = [round(x, 3) for x in t["close"]]
        if mode == "staged":
            res["staged_bytes"] = int(statistics.median(t["bytes"][-k:]))
        if mode == "host":
            res["host_groupby_ms"], res["host_h2d_ms"] = med(t["groupby"]), med(t["h2d"])
            res["host_total_ms"] = round(res["host_groupby_ms"] + res["host_h2d_ms"] + res["host_close_ms"], 3)
    res["same_results"] = shapes["device"] == shapes["staged"] == shapes["host"]
    res["per_window_offers_popped_pending_batch_events_local_stored"] = shapes["device"][-k:]
    extra = res["staged_close_ms"] - res["device_close_ms"]
    res["staged_minus_device_ms"] = round(extra, 3)
    res["staged_link_GBps"] = round(res["staged_bytes"] / extra / 1e6, 2) if extra > 0 else None
    print(json.dumps(res))


def sharded(a):
    import threading

    import numpy as np
    import torch
    from shadow_amd import _native as N
    from shadow_amd import dist as D
    from shadow_amd import synth
    from shadow_amd.equeue import EventQueues
    from shadow_amd.inbound import InboundStage
    from shadow_amd.ledger import PacketLedger
    from shadow_amd.outbound import OutboundStage
    from shadow_amd.rounds import Runahead
    from shadow_amd.routing import Engine
    from shadow_amd.tbucket import SIM_START
    from shadow_amd.window import Window

    H, NN, W = a.hosts, a.nodes, a.ranks
    rs = np.random.default_rng(11)
    lat = rs.integers(MS, a.lat_windows * MS + 1, (NN, NN)).astype(np.uint64)
    lat[0, 0] = MS
    loss = np.full((NN, NN), 0.01, np.float32)
    host_node = synth.c5_host_nodes(H, NN)
    rng0 = synth.host_rng_states(H, 1)
    end_time = SIM_START + 10**12

    def window(g, start, w, lo, hi):
        """The offers of hosts [lo, hi) (destinations over all hosts; ids distinct across ranks)."""
        n_own = hi - lo
        c_lo, c_hi = max(a.per_host * 4 // 5, 0), a.per_host * 6 // 5 + 1
        cnt = torch.randint(c_lo, c_hi, (n_own,), generator=g, device="cuda")
        off = torch.zeros(n_own + 1, dtype=torch.int64, device="cuda")
        off[1:] = torch.cumsum(cnt, 0)
        n = int(off[-1])
        host = torch.repeat_interleave(torch.arange(n_own, device="cuda"), cnt)
        key, _ = torch.sort(host * MS + torch.randint(0, MS, (n,), generator=g, device="cuda"))
        t = start + (key - host * MS)
        u = torch.rand(n, generator=g, device="cuda")
        size = torch.where(u < 0.2, 52, torch.where(u < 0.8, 1500, torch.randint(HEADER, 1501, (n,), generator=g,
                                                                                   device="cuda")))
        idx = torch.arange(n, device="cuda")
        dst = torch.randint(0, H, (n,), generator=g, device="cuda")
        pkt = ((idx + lo * 2 * a.per_host + w * 50_000_000) & 0x7FFFFFFF).int()
        return (off.int(), t.contiguous(), (idx + (w << 32)).contiguous(), size.int(), (size - HEADER).int(), dst.int(),
                pkt), n

    def setup(eng):
        if a.remap_search:
            eng.set_knob("LEDGER_REMAP_SEARCH", 1)
        relay = D.ShardedRelay(eng, host_node, rng0, np.zeros(H, np.uint64), lat, loss)
        n_own = relay.hi - relay.lo
        return dict(relay=relay, queues=EventQueues(eng, H), ra=Runahead(eng, False, MS),
                    ostage=OutboundStage.from_bandwidth(eng, [125_000_000] * n_own, SIM_START, first_host=relay.lo,
                                                        ring_capacity=a.ring),
                    istage=InboundStage.from_bandwidth(eng, [125_000_000] * n_own, SIM_START, ring_capacity=a.ring),
                    ledger=PacketLedger(eng), win=Window(eng, n_own))

    gate = threading.Barrier(W)

    def clock(fn):
        """The ranks enter the call together; each rank's own host clock around it."""
        torch.cuda.synchronize()
        gate.wait()
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    def run(fns):
        res, errs = [None] * W, []

        def wrap(i):
            try:
                res[i] = fns[i]()
            except BaseException as e:   # noqa: BLE001 -- reported below
                errs.append(e)
                gate.abort()
        ts = [threading.Thread(target=wrap, args=(i,)) for i in range(W)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if errs:
            raise errs[0]
        return res

    def engines_of():
        engines = [Engine(0) for _ in range(W)]
        D.comm_init_local(engines)
        return engines

    def rank_windows(p, rank):
        g = torch.Generator(device="cuda").manual_seed(5 + rank)
        t_open, t_close, shape, start = [], [], [], SIM_START
        lo, hi = p["relay"].lo, p["relay"].hi
        for w in range(a.windows):
            arr, n = window(g, start, w, lo, hi)
            op, ms_o = clock(lambda: p["win"].open(start + MS))
            cl, ms_c = clock(lambda: p["win"].close(*arr, n, start + MS, end_time))
            t_open.append(ms_o)
            t_close.append(ms_c)
            s = p["ledger"].stats()
            shape.append((n, op.n_popped, op.n_pending, cl.n_batch, cl.n_events, s.live_batches, s.entries_held))
            start += MS
        return t_open, t_close, shape

    def rank_calls(p, rank):
        g = torch.Generator(device="cuda").manual_seed(5 + rank)
        t = {k: [] for k in ("outbound", "relay_sharded", "record_sharded")}
        eng, lo, hi, status, out, start = p["relay"].eng, p["relay"].lo, p["relay"].hi, None, None, SIM_START
        for w in range(a.windows):
            arr, n = window(g, start, w, lo, hi)
            we = start + MS
            eq = p["queues"].advance_device(out, we)
            d_size, d_pkt = p["ledger"].gather_device(eq.tag, eq.n_popped)
            p["istage"].advance_device(eq.off, eq.deliver, d_size, d_pkt, eq.n_popped, we)
            ob, ms = clock(lambda: p["ostage"].advance_device(*arr, n, we))
            t["outbound"].append(ms)
            if status is None or len(status) < max(ob.n_sent, 1):
                status = torch.empty(max(ob.n_sent, 1) * 5 // 4, dtype=torch.uint8, device="cuda")
            out = N.RelayOut(status.data_ptr(), None, None, None, None, None, 0, 0, 0, 0, 0)
            rd = N.Round(we, end_time, 0)
            _, ms = clock(lambda: N.check(eng.lib.shd_relay_round_sharded(eng.ctx, C.byref(ob.batch), C.byref(rd),
                                                                          C.byref(out)), "relay"))
            t["relay_sharded"].append(ms)
            sizes = C.c_void_p()
            N.check(eng.lib.shd_outbound_sent_sizes(eng.ctx, C.byref(sizes)), "sizes")
            number = p["ledger"].next_batch()
            _, ms = clock(lambda: p["ledger"].record_sharded(number, sizes.value, ob.sent_pkt, ob.batch.dst_host,
                                                             status, ob.n_sent, out))
            t["record_sharded"].append(ms)
            if not out.n_events:
                out = None
            start += MS
        return t

    k = a.timed
    worst = lambda rows: round(statistics.median([max(x) for x in zip(*rows)][-k:]), 3)  # noqa: E731
    res = {"hosts": H, "nodes": NN, "lat_windows": a.lat_windows, "ranks": W, "remap_search": a.remap_search}
    engines = engines_of()
    try:
        parts = [setup(e) for e in engines]
        out = run([lambda i=i: rank_windows(parts[i], i) for i in range(W)])
        res["open_ms"] = worst([o[0] for o in out])
        res["close_ms"] = worst([o[1] for o in out])
        res["rank0_per_window_offers_popped_pending_batch_events_livebatches_entries"] = out[0][2][-k:]
        res["open_ms_all_rank0"] = [round(x, 3) for x in out[0][0]]
        res["close_ms_all_rank0"] = [round(x, 3) for x in out[0][1]]
        del parts
    finally:
        for e in engines:
            e.close()
    engines = engines_of()
    try:
        parts = [setup(e) for e in engines]
        out = run([lambda i=i: rank_calls(parts[i], i) for i in range(W)])
        for name in ("outbound", "relay_sharded", "record_sharded"):
            res[name + "_ms"] = worst([o[name] for o in out])
            res[name + "_ms_all_rank0"] = [round(x, 3) for x in out[0][name]]
        del parts
    finally:
        for e in engines:
            e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
