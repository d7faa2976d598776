"""Host-side mirror of the packet ledger (``shd_ledger_*``): each relay batch's (total size,
packet id) per packet, kept on the MI355X engine from the round that sent the batch until its last
event has popped from the destination event queues.

A popped event carries only its tag, ``(batch number << 32) | index in that batch``;
``shd_inbound_advance`` wants the packet's total size and the caller's packet id.
``PacketLedger(engine, max_live_batches)``; ``record(batch, d_size, d_pkt, n_packets, n_live)``
keeps a batch's two device arrays (``record_sharded`` under a communicator of several ranks: each
sent packet's entry goes to the rank that owns its destination); ``gather_device(d_tag, n)`` turns a window's popped tags into
the two device arrays the inbound stage takes (``gather`` is the host-array form, for tests);
``stats()``.  No CPU fallback: without the native library or a gfx950 GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N

NONE = 2**64 - 1
REFUSED = 2**32 - 1   # both outputs of an event the gather refused


@dataclass
class LedgerStats:
    live_batches: int
    live_events: int
    entries_held: int      # the sum of n_packets from the oldest batch held to the newest
    oldest_batch: int | None


def _as_p(a):
    return a if a is None or isinstance(a, (int, C.c_void_p)) else N.ptr(a)


class PacketLedger:
    def __init__(self, engine, max_live_batches: int = 0):
        self.eng = engine
        N.check(engine.lib.shd_ledger_setup(engine.ctx, int(max_live_batches)), "shd_ledger_setup")

    def next_batch(self) -> int:
        """The number the event queues give the next non-NULL batch (``shd_equeue_next_batch``)."""
        b = C.c_uint64(0)
        N.check(self.eng.lib.shd_equeue_next_batch(self.eng.ctx, C.byref(b)), "shd_equeue_next_batch")
        return b.value

    def record(self, batch: int, d_size, d_pkt, n_packets: int, n_live: int) -> None:
        """Device pointers (ints, ctypes pointers or torch tensors)."""
        N.check(self.eng.lib.shd_ledger_record(self.eng.ctx, int(batch), _as_p(d_size), _as_p(d_pkt), int(n_packets),
                                               int(n_live)), "shd_ledger_record")

    def record_sharded(self, batch: int, d_size, d_pkt, d_dst_host, d_status, n_packets: int, relay_out,
                       local: int = N.SHD_OK) -> None:
        """``shd_ledger_record_sharded``, a collective: every rank of the engine's communicator
        calls it after a committed sharded round.  This rank's batch entries with their
        destinations and statuses (device pointers) and its ``shd_relay_round_sharded`` output
        (``_native.RelayOut``): its ``ev_pkt`` is rewritten on the device to the index in the batch
        recorded here under ``batch`` (this rank's own ``next_batch()``).  ``local``: a failure of
        the caller's own to carry into the call; every rank then raises with that status."""
        N.check(self.eng.lib.shd_ledger_record_sharded(
            self.eng.ctx, int(batch), _as_p(d_size), _as_p(d_pkt), _as_p(d_dst_host), _as_p(d_status),
            int(n_packets), C.byref(relay_out), int(local)), "shd_ledger_record_sharded")

    def gather_device(self, d_tag, n: int):
        """-> (d_size, d_pkt): engine-owned device pointers, valid until the next gather."""
        ds, dp = C.c_void_p(), C.c_void_p()
        N.check(self.eng.lib.shd_ledger_gather(self.eng.ctx, _as_p(d_tag), int(n), C.byref(ds), C.byref(dp)),
                "shd_ledger_gather")
        return ds.value, dp.value

    def gather(self, tag, check: bool = True):
        """Host tags -> host (size, pkt) copies.  ``check=False`` returns ``(status, size, pkt)``
        instead of raising, the arrays as the refused call left them."""
        import torch
        tag = np.ascontiguousarray(tag, np.uint64)
        n = len(tag)
        d_tag = torch.from_numpy(tag.view(np.int64)).cuda() if n else None
        torch.cuda.synchronize()
        ds, dp = C.c_void_p(), C.c_void_p()
        st = self.eng.lib.shd_ledger_gather(self.eng.ctx, _as_p(d_tag), n, C.byref(ds), C.byref(dp))
        if check:
            N.check(st, "shd_ledger_gather")
        size, pkt = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        for dst, src in ((size, ds), (pkt, dp)):
            if dst.nbytes:
                N.check(self.eng.lib.shd_copy_to_host(self.eng.ctx, N.ptr(dst), src, dst.nbytes), "shd_copy_to_host")
        return (size, pkt) if check else (st, size, pkt)

    def stats(self) -> LedgerStats:
        a, b, c, d = (C.c_uint64(0) for _ in range(4))
        N.check(self.eng.lib.shd_ledger_stats(self.eng.ctx, C.byref(a), C.byref(b), C.byref(c), C.byref(d)),
                "shd_ledger_stats")
        return LedgerStats(a.value, b.value, c.value, None if d.value == NONE else d.value)
