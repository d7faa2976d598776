"""Host-side mirror of the two-call scheduling window (``shd_window_open`` / ``shd_window_close``).

A window is two engine calls with the CPU in between: ``open`` merges the relay output the last
close left into the event queues, pops the window's events, gathers their sizes and ids from the
packet ledger and runs the inbound stage; the caller's sockets turn the inbound records into this
window's offers; ``close`` runs the outbound stage, the relay round and the ledger record.  No
packet data crosses the host.  ``close_staged`` is the close from the worker threads' staged offers
(``shadow_amd.outbound.OfferStages``), grouped by host on the device; ``records_host`` /
``closed_host`` fetch a window's results with one engine call each.  The relay, the event queues, the runahead, both stages and the
ledger are set up by the caller (``Relay``, ``EventQueues``, ``Runahead``, ``InboundStage``,
``OutboundStage``, ``PacketLedger``) on one engine, for the same hosts.

Under an engine communicator of several ranks (``shadow_amd.dist``) each rank runs the window on its
shard ``[lo, hi)`` of the hosts: ``ShardedRelay``, ``EventQueues`` over all hosts (they keep the
shard), both stages for ``hi - lo`` hosts, the outbound stage with ``first_host=lo``, and
``Window(engine, hi - lo)``.  ``open`` stays local; ``close`` is a collective every rank calls: a
failure on one rank (a wrong ``window_end``, an outbound contract violation) is raised on every
rank.  ``Closed.n_events`` then counts the events this rank received, ``min_deliver`` is the
all-rank value, and packet ids travel unchanged between the ranks, so the caller picks ids that
name a packet across ranks.  No CPU fallback: without the native library or a gfx950 GPU every
call raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .inbound import DeviceRecords, Records

IDLE = 2**64 - 1


@dataclass
class Opened:
    """``shd_window_open``'s outputs: the inbound stage's records (engine-owned device arrays,
    valid until the next open) and the queues' totals."""
    records: DeviceRecords
    n_popped: int
    n_pending: int
    queue_next_time: int   # IDLE when the queues are empty


@dataclass
class Closed:
    """``shd_window_close``'s outputs: device pointers valid until the next close."""
    sent_pkt: int
    sent_status: int
    loc_off: int
    loc_pkt: int
    loc_time: int
    n_batch: int           # batch entries: packets the outbound stage sent
    n_events: int          # of them SENT by the relay: events for the queues
    n_local: int
    n_stored: int
    next_task_time: int    # the outbound stage's, IDLE when none
    min_deliver: int       # the relay output's earliest deliver time, IDLE when none


@dataclass
class ClosedHost:
    sent_pkt: np.ndarray     # u32 [n_batch]
    sent_status: np.ndarray  # u8 [n_batch]: PKT_SKIPPED / PKT_DROPPED / PKT_SENT
    loc_off: np.ndarray      # u32 [n_hosts + 1]
    loc_pkt: np.ndarray      # u32
    loc_time: np.ndarray     # u64


def _as_p(a):
    return a if a is None or isinstance(a, (int, C.c_void_p)) else N.ptr(a)


class Window:
    def __init__(self, engine, n_hosts: int):
        """``n_hosts``: the hosts this engine runs -- all of them, or the rank's ``hi - lo``."""
        self.eng = engine
        self.n_hosts = int(n_hosts)

    def open(self, window_end: int, bootstrap_end: int = 0) -> Opened:
        off, pkt, time, kind = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n_out, n_stored, nxt, n_pop, n_pend, qn = (C.c_uint64(0) for _ in range(6))
        N.check(self.eng.lib.shd_window_open(
            self.eng.ctx, int(window_end), int(bootstrap_end), C.byref(off), C.byref(pkt), C.byref(time),
            C.byref(kind), C.byref(n_out), C.byref(n_stored), C.byref(nxt), C.byref(n_pop), C.byref(n_pend),
            C.byref(qn)), "shd_window_open")
        rec = DeviceRecords(off.value, pkt.value, time.value, kind.value, n_out.value, n_stored.value, nxt.value)
        return Opened(rec, n_pop.value, n_pend.value, qn.value)

    def close(self, d_off, d_time, d_prio, d_size, d_payload, d_dst, d_pkt, n_offers: int, window_end: int,
              sim_end: int, bootstrap_end: int = 0, d_sock=None) -> Closed:
        """The offers as device pointers (ints, ctypes pointers or torch tensors; all None for none).
        ``d_sock``: the offering sockets' canonical handles, the column an outbound stage with
        ``qdisc="fifo-sockets"`` or ``"round-robin-sockets"`` needs beside ``d_prio``."""
        sp, ss, lo, lp, lt = (C.c_void_p() for _ in range(5))
        n_batch, n_ev, n_local, n_stored, nxt, md = (C.c_uint64(0) for _ in range(6))
        N.check(self.eng.lib.shd_window_close_sockets(
            self.eng.ctx, _as_p(d_off), _as_p(d_time), _as_p(d_prio), _as_p(d_sock), _as_p(d_size), _as_p(d_payload),
            _as_p(d_dst), _as_p(d_pkt), int(n_offers), int(window_end), int(sim_end), int(bootstrap_end), C.byref(sp),
            C.byref(ss), C.byref(n_batch), C.byref(n_ev), C.byref(lo), C.byref(lp), C.byref(lt), C.byref(n_local),
            C.byref(n_stored), C.byref(nxt), C.byref(md)), "shd_window_close")
        return Closed(sp.value, ss.value, lo.value, lp.value, lt.value, n_batch.value, n_ev.value, n_local.value,
                      n_stored.value, nxt.value, md.value)

    def close_staged(self, stages, time_base: int, window_end: int, sim_end: int, bootstrap_end: int = 0) -> Closed:
        """``shd_window_close_staged``: the close from the worker threads' staged offers
        (``shadow_amd.outbound.OfferStages``), grouped by host on the device.  A refused staging
        (ShdError) leaves the window open: a corrected close may follow.  A rank without hosts
        passes stages without a thread (``OfferStages([], [], [], 8)``)."""
        sp, ss, lo, lp, lt = (C.c_void_p() for _ in range(5))
        n_batch, n_ev, n_local, n_stored, nxt, md = (C.c_uint64(0) for _ in range(6))
        N.check(self.eng.lib.shd_window_close_staged(
            self.eng.ctx, *stages.args(), int(time_base), int(window_end), int(sim_end), int(bootstrap_end),
            C.byref(sp), C.byref(ss), C.byref(n_batch), C.byref(n_ev), C.byref(lo), C.byref(lp), C.byref(lt),
            C.byref(n_local), C.byref(n_stored), C.byref(nxt), C.byref(md)), "shd_window_close_staged")
        return Closed(sp.value, ss.value, lo.value, lp.value, lt.value, n_batch.value, n_ev.value, n_local.value,
                      n_stored.value, nxt.value, md.value)

    def update_bandwidth(self, hosts, down_bytes_per_second, up_bytes_per_second, at_time: int):
        """``shd_window_update_bandwidth``: between a close and the next open, both stages'
        buckets of the named hosts (the engine's own indices) from new link rates in bytes per
        second, ``create_token_bucket`` per direction; an entry of ``None`` leaves that direction
        as it is.  Both stages are checked before either changes.  A refusal (ShdError, ``.host``
        the lowest failing host of the stage that refused) changes nothing."""
        from .tbucket import UNCHANGED
        h = np.ascontiguousarray(hosts, np.uint32)
        rate = lambda a: np.array([UNCHANGED if b is None else int(b) for b in a], np.uint64)  # noqa: E731
        down, up = rate(down_bytes_per_second), rate(up_bytes_per_second)
        assert len(down) == len(up) == len(h)
        err = C.c_uint32(0xFFFFFFFF)
        st = self.eng.lib.shd_window_update_bandwidth(self.eng.ctx, len(h), N.ptr(h), N.ptr(down), N.ptr(up),
                                                      int(at_time), C.byref(err))
        if st != N.SHD_OK:
            e = N.ShdError(st, "shd_window_update_bandwidth")
            e.host = None if err.value == 0xFFFFFFFF else err.value
            raise e

    def records_host(self, o: Opened) -> Records:
        """``records`` in one engine call (``shd_window_records_host``): every array copied
        asynchronously, one wait.  ``o`` must be the last open."""
        r = o.records
        off = np.zeros(self.n_hosts + 1, np.uint32)
        pkt, time, kind = np.zeros(r.n_out, np.uint32), np.zeros(r.n_out, np.uint64), np.zeros(r.n_out, np.uint8)
        n = C.c_uint64(0)
        N.check(self.eng.lib.shd_window_records_host(self.eng.ctx, N.ptr(off), N.ptr(pkt), N.ptr(time), N.ptr(kind),
                                                     r.n_out, C.byref(n)), "shd_window_records_host")
        assert n.value == r.n_out, "not the last open"
        return Records(off, pkt, time, kind, r.n_stored, r.next_task_time)

    def closed_host(self, c: Closed) -> ClosedHost:
        """``closed`` in one engine call (``shd_window_sent_host``).  ``c`` must be the last close."""
        sp, ss = np.zeros(c.n_batch, np.uint32), np.zeros(c.n_batch, np.uint8)
        lo = np.zeros(self.n_hosts + 1, np.uint32)
        lp, lt = np.zeros(c.n_local, np.uint32), np.zeros(c.n_local, np.uint64)
        nb, nl = C.c_uint64(0), C.c_uint64(0)
        N.check(self.eng.lib.shd_window_sent_host(self.eng.ctx, N.ptr(sp), N.ptr(ss), c.n_batch, N.ptr(lo), N.ptr(lp),
                                                  N.ptr(lt), c.n_local, C.byref(nb), C.byref(nl)),
                "shd_window_sent_host")
        assert (nb.value, nl.value) == (c.n_batch, c.n_local), "not the last close"
        return ClosedHost(sp, ss, lo, lp, lt)

    def _copy(self, pairs):
        for dst, src in pairs:
            if dst.nbytes:
                N.check(self.eng.lib.shd_copy_to_host(self.eng.ctx, N.ptr(dst), C.c_void_p(src), dst.nbytes),
                        "shd_copy_to_host")

    def records(self, o: Opened) -> Records:
        """Host copies of an open's inbound records."""
        r = o.records
        off = np.zeros(self.n_hosts + 1, np.uint32)
        pkt, time, kind = np.zeros(r.n_out, np.uint32), np.zeros(r.n_out, np.uint64), np.zeros(r.n_out, np.uint8)
        self._copy(((off, r.off), (pkt, r.pkt), (time, r.time), (kind, r.kind)))
        return Records(off, pkt, time, kind, r.n_stored, r.next_task_time)

    def closed(self, c: Closed) -> ClosedHost:
        """Host copies of a close's sent ids, statuses and local deliveries."""
        sp, ss = np.zeros(c.n_batch, np.uint32), np.zeros(c.n_batch, np.uint8)
        lo = np.zeros(self.n_hosts + 1, np.uint32)
        lp, lt = np.zeros(c.n_local, np.uint32), np.zeros(c.n_local, np.uint64)
        self._copy(((sp, c.sent_pkt), (ss, c.sent_status), (lo, c.loc_off), (lp, c.loc_pkt), (lt, c.loc_time)))
        return ClosedHost(sp, ss, lo, lp, lt)
