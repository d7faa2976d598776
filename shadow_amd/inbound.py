"""Host-side mirror of the inbound stage (``shd_inbound_*``): per destination host the CoDel
router queue, the inbound relay's token bucket and the relay's state, kept on the MI355X engine.

Restates the chain from ``Host::execute``'s packet branch (``src/main/host/host.rs:742-746``)
through ``Router::route_incoming_packet`` and ``Relay::notify`` (``relay/mod.rs:110-135``) to the
forward task (``Relay::forward_until_blocked``, ``relay/mod.rs:200-272``) for every host at once.

``InboundStage(engine, capacity, refill_increment, refill_interval, last_refill)`` -- bucket
parameters per host, all three 0 for a host without a bucket -- or
``InboundStage.from_bandwidth(engine, bytes_per_second, start)``.  ``advance(off, time, size, pkt,
window_end=...)`` consumes one window's packet events grouped by host (host arrays;
``advance_device`` takes them as they lie on the GPU, e.g. the event queues' popped ``off`` and
``deliver``) and returns one record per packet that left the stage: FORWARDED or DROPPED with its
time, grouped by host in the order they happened.  No CPU fallback: without the native library or
a gfx950 GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .tbucket import SIM_START, bandwidth_rows, create_token_bucket, update_buckets

FORWARDED, DROPPED = 1, 2
IDLE = 2**64 - 1


@dataclass
class DeviceRecords:
    """What ``shd_inbound_advance`` returns: engine-owned device arrays (valid until the next
    advance) and the call's totals."""
    off: int               # device pointers
    pkt: int
    time: int
    kind: int
    n_out: int
    n_stored: int          # packets still queued or cached
    next_task_time: int    # earliest outstanding forward task, IDLE when none


@dataclass
class Records:
    off: np.ndarray        # u32 [n_hosts + 1]: host h's records are [off[h], off[h+1])
    pkt: np.ndarray        # u32
    time: np.ndarray       # u64
    kind: np.ndarray       # u8: FORWARDED / DROPPED
    n_stored: int
    next_task_time: int

    def records_for(self, h: int):
        a, b = int(self.off[h]), int(self.off[h + 1])
        return list(zip(self.kind[a:b].tolist(), self.pkt[a:b].tolist(), self.time[a:b].tolist()))


class InboundStage:
    def __init__(self, engine, capacity, refill_increment, refill_interval, last_refill=SIM_START,
                 ring_capacity: int = 4096):
        self.eng = engine
        cap = np.ascontiguousarray(capacity, np.uint64)
        self.n_hosts = len(cap)
        inc = np.ascontiguousarray(np.broadcast_to(np.asarray(refill_increment, np.uint64), cap.shape))
        itv = np.ascontiguousarray(np.broadcast_to(np.asarray(refill_interval, np.uint64), cap.shape))
        last = np.ascontiguousarray(np.broadcast_to(np.asarray(last_refill, np.uint64), cap.shape))
        N.check(engine.lib.shd_inbound_setup(engine.ctx, self.n_hosts, int(ring_capacity), N.ptr(cap), N.ptr(inc),
                                             N.ptr(itv), N.ptr(last)), "shd_inbound_setup")

    @classmethod
    def from_bandwidth(cls, engine, bytes_per_second, start: int = SIM_START, ring_capacity: int = 4096):
        """One ``create_token_bucket`` (relay/mod.rs:291-302) per host, last refilled at ``start``;
        an entry of ``None`` (or a negative one) is a host without a bucket."""
        rows = [(0, 0, 0) if b is None or int(b) < 0 else create_token_bucket(int(b)) for b in bytes_per_second]
        cap, inc, itv = (np.array([r[i] for r in rows], np.uint64) for i in range(3))
        return cls(engine, cap, inc, itv, start, ring_capacity)

    def advance_device(self, d_off, d_time, d_size, d_pkt, n_events: int, window_end: int,
                       bootstrap_end: int = 0) -> DeviceRecords:
        """Device pointers (ints, ctypes pointers or torch tensors; all None for no events)."""
        as_p = lambda a: a if a is None or isinstance(a, (int, C.c_void_p)) else N.ptr(a)  # noqa: E731
        off, pkt, time, kind = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n_out, n_stored, nxt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        N.check(self.eng.lib.shd_inbound_advance(
            self.eng.ctx, as_p(d_off), as_p(d_time), as_p(d_size), as_p(d_pkt), int(n_events), int(window_end),
            int(bootstrap_end), C.byref(off), C.byref(pkt), C.byref(time), C.byref(kind), C.byref(n_out),
            C.byref(n_stored), C.byref(nxt)), "shd_inbound_advance")
        return DeviceRecords(off.value, pkt.value, time.value, kind.value, n_out.value, n_stored.value, nxt.value)

    def advance(self, off=None, time=None, size=None, pkt=None, *, window_end: int, bootstrap_end: int = 0) -> Records:
        """Host arrays of one window's packet events grouped by host (or none) -> the records."""
        keep = [None] * 4
        n = 0
        if off is not None:
            import torch
            n = len(time)
            dev = lambda a, np_dt, dt: torch.from_numpy(np.ascontiguousarray(a, np_dt).view(dt)).cuda()  # noqa: E731
            keep = [dev(off, np.uint32, np.int32), dev(time, np.uint64, np.int64), dev(size, np.uint32, np.int32),
                    dev(pkt, np.uint32, np.int32)]
            assert len(keep[0]) == self.n_hosts + 1 and len(keep[2]) == len(keep[3]) == n
            torch.cuda.synchronize()
        out = self.advance_device(*keep, n, window_end, bootstrap_end)
        del keep
        return self.records(out)

    def records(self, out: DeviceRecords) -> Records:
        """Host copies of an advance's records."""
        n = out.n_out
        off = np.zeros(self.n_hosts + 1, np.uint32)
        pkt = np.zeros(n, np.uint32)
        time = np.zeros(n, np.uint64)
        kind = np.zeros(n, np.uint8)
        for dst, src in ((off, out.off), (pkt, out.pkt), (time, out.time), (kind, out.kind)):
            if dst.nbytes:
                N.check(self.eng.lib.shd_copy_to_host(self.eng.ctx, N.ptr(dst), C.c_void_p(src), dst.nbytes),
                        "shd_copy_to_host")
        return Records(off, pkt, time, kind, out.n_stored, out.next_task_time)

    def update_buckets(self, hosts, capacity, refill_increment, refill_interval, at_time: int):
        """``shd_inbound_update_buckets``: the named hosts' ``bw_down`` buckets re-rated at
        ``at_time`` (>= the last ``window_end``; all three parameters 0: no bucket).  Queues, CoDel
        state, the cached packet and the outstanding task stay as they are.  A refusal (ShdError,
        ``.host`` the lowest failing host) changes nothing."""
        update_buckets(self.eng, "shd_inbound_update_buckets", hosts, capacity, refill_increment, refill_interval,
                       at_time)

    def update_bandwidth(self, hosts, bytes_per_second, at_time: int):
        """``update_buckets`` with ``create_token_bucket`` per entry, as ``from_bandwidth`` (None:
        no bucket)."""
        self.update_buckets(hosts, *bandwidth_rows(bytes_per_second), at_time)

    def state(self, host: int) -> dict:
        """One host: ``task_time`` (None: Idle), ``cached`` ((pkt, size) or None), the queue as
        ``CoDelQueues.state`` and the bucket as ``TokenBuckets.state`` (None: no bucket)."""
        task, has, cp, cs = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        q, b = N.CodelState(), N.TbState()
        N.check(self.eng.lib.shd_inbound_get_state(self.eng.ctx, int(host), C.byref(task), C.byref(has), C.byref(cp),
                                                   C.byref(cs), C.byref(q), C.byref(b)), "shd_inbound_get_state")
        codel = {"len": q.len, "mode": q.mode,
                 "interval_end": q.interval_end if q.has_interval_end else None,
                 "drop_next": q.drop_next if q.has_drop_next else None,
                 "current_drop_count": q.current_drop_count, "previous_drop_count": q.previous_drop_count,
                 "total_bytes_stored": q.total_bytes_stored}
        bucket = {k: int(getattr(b, k)) for k, _ in N.TbState._fields_} if b.capacity else None
        return {"task_time": None if task.value == IDLE else task.value,
                "cached": (cp.value, cs.value) if has.value else None, "codel": codel, "bucket": bucket}
