"""Host-side mirror of the outbound stage (``shd_outbound_*``): per source host the network
interface's queue under either queuing discipline (``interface_qdisc``: FIFO or round-robin), the
outbound relay's token bucket and the relay's state, kept on the MI355X engine.

Restates the outbound relay ``relay_inet_out`` (``src/main/host/host.rs:285-288``, ``:871-880``)
for every host at once: the interface's FIFO queuing discipline picks the packet of the lowest
priority (``network_interface.c:276-316``), ``Relay::forward_until_blocked``
(``relay/mod.rs:200-272``) takes tokens from the ``bw_up`` bucket, and a packet that conforms enters
``Worker::send_packet`` at the task's time (``router/mod.rs:49-55``).  With
``qdisc="round-robin"`` the interface keeps the rrQueue instead (``network_interface.c:235-273``,
``:366-392``): the sockets that have packets queued take turns, one packet each, and the per-offer
key is the offering socket's canonical handle (``sock=`` where FIFO takes ``prio=``).
``qdisc="fifo-sockets"`` and ``"round-robin-sockets"`` are the two disciplines over sockets with
both buffers of ``socket.c:432-437``: a packet of priority 0 (every TCP control packet) goes to its
socket's control list, which is pulled first, and under ``"fifo-sockets"`` the sockets stand in the
reference's array heap (``priority_queue.c``).  An offer then has both columns, ``prio=`` and
``sock=``, and priorities need not be unique.

``OutboundStage(engine, capacity, refill_increment, refill_interval, last_refill, first_host=0,
qdisc="fifo", max_sockets=64)`` -- bucket parameters per host, all three 0 for a host without a bucket; host ``h``'s global id is
``first_host + h`` -- or ``OutboundStage.from_bandwidth(engine, bytes_per_second, start)``.
``advance(off, time, prio, size, payload, dst, pkt, window_end=...)`` consumes one window's offers
grouped by host (host arrays; ``advance_device`` takes them as they lie on the GPU) and returns the
packets sent, as the batch a relay round takes, and the local deliveries.  ``OfferStages`` holds
the same offers as the worker threads stage them -- per thread the runs ``(host, count)`` and 8-
or 10-word records -- and ``group_stages`` (``shd_offers_group``) groups them by host on the
device into the arrays ``advance_device`` takes.  No CPU fallback: without
the native library or a gfx950 GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .tbucket import SIM_START, bandwidth_rows, create_token_bucket, update_buckets

IDLE = 2**64 - 1
NO_PKT = 2**32 - 1
QDISC = {"fifo": N.QDISC_FIFO, "round-robin": N.QDISC_ROUND_ROBIN, "fifo-sockets": N.QDISC_FIFO_SOCKETS,
         "round-robin-sockets": N.QDISC_ROUND_ROBIN_SOCKETS}
SOCKET_QDISCS = ("fifo-sockets", "round-robin-sockets")   # an offer is (priority, socket): two columns


@dataclass
class DeviceBatch:
    """What ``shd_outbound_advance`` returns: engine-owned device arrays (valid until the next
    advance) and the call's totals.  ``batch`` goes to ``shd_relay_round_device`` as it stands;
    ``src_off`` ... ``payload`` are its pointers, for ``Relay.round_device``."""
    batch: N.Batch
    sent_pkt: int          # device pointers
    loc_off: int
    loc_pkt: int
    loc_time: int
    n_sent: int
    n_local: int
    n_stored: int          # packets still queued or cached
    next_task_time: int    # earliest outstanding forward task, IDLE when none


@dataclass
class Sent:
    src_off: np.ndarray    # u32 [n_hosts + 1]: host h sent packets [src_off[h], src_off[h+1])
    send_time: np.ndarray  # u64
    dst_host: np.ndarray   # u32
    payload: np.ndarray    # u32
    sent_pkt: np.ndarray   # u32: the packet id of each batch entry
    loc_off: np.ndarray    # u32 [n_hosts + 1]: host h's local deliveries
    loc_pkt: np.ndarray    # u32
    loc_time: np.ndarray   # u64
    n_stored: int
    next_task_time: int

    def sent_for(self, h: int):
        a, b = int(self.src_off[h]), int(self.src_off[h + 1])
        return list(zip(self.sent_pkt[a:b].tolist(), self.send_time[a:b].tolist(), self.dst_host[a:b].tolist(),
                        self.payload[a:b].tolist()))

    def local_for(self, h: int):
        a, b = int(self.loc_off[h]), int(self.loc_off[h + 1])
        return list(zip(self.loc_pkt[a:b].tolist(), self.loc_time[a:b].tolist()))


OFFER_WORDS, OFFER_WORDS_SOCK = 8, 10   # u32 words per staged offer (csrc/offer_stage.h)


def group_offers(run_host, run_count, offers, words: int, time_base: int, n_hosts: int, first_host: int = 0):
    """The numpy statement of ``shd_offers_group``: per-thread stages (lists of ``run_host``,
    ``run_count`` and ``[n, words]`` u32 record arrays) -> ``(off, time, prio, sock, size, payload,
    dst, pkt)`` grouped by host in host order, each host's offers in the order its run holds them
    (``sock`` is None at width 8).  Raises ValueError where the engine refuses."""
    if words not in (OFFER_WORDS, OFFER_WORDS_SOCK):
        raise ValueError("offer_words")
    host = np.concatenate([np.asarray(h, np.uint32) for h in run_host] + [np.zeros(0, np.uint32)]).astype(np.int64)
    count = np.concatenate([np.asarray(c, np.uint32) for c in run_count] + [np.zeros(0, np.uint32)]).astype(np.int64)
    for c, o in zip(run_count, offers):
        if int(np.asarray(c, np.int64).sum()) != len(np.asarray(o).reshape(-1, words)):
            raise ValueError("a stage's run counts do not add up to its offers")
    rec = np.concatenate([np.asarray(o, np.uint32).reshape(-1, words) for o in offers] +
                         [np.zeros((0, words), np.uint32)])
    local = host - first_host
    if ((local < 0) | (local >= n_hosts)).any():
        raise ValueError("a run of a host outside the stage")
    if len(np.unique(local)) != len(local):
        raise ValueError("a host with two runs")
    owner = np.repeat(local, count)                   # each record's host, in stage order
    order = np.argsort(owner, kind="stable")          # the group-by: stable, so a run keeps its order
    rec = rec[order]
    off = np.zeros(n_hosts + 1, np.uint32)
    off[1:] = np.cumsum(np.bincount(owner, minlength=n_hosts))
    u64 = lambda lo: rec[:, lo].astype(np.uint64) | (rec[:, lo + 1].astype(np.uint64) << np.uint64(32))  # noqa: E731
    return (off, np.uint64(time_base) + rec[:, 0].astype(np.uint64), u64(6), u64(8) if words == OFFER_WORDS_SOCK else None,
            rec[:, 2].copy(), rec[:, 3].copy(), rec[:, 1].copy(), rec[:, 4].copy())


class OfferStages:
    """One window's offers as the worker threads stage them for ``shd_offers_group`` /
    ``shd_window_close_staged``: per thread the runs ``(host, count)`` and the ``words``-word
    records, run after run.  ``from_grouped`` deals the hosts of grouped offers to threads, as a
    thread-per-core scheduler does; ``pinned`` moves every array into ``shd_host_alloc`` memory, where
    the engine reads it in place."""

    def __init__(self, run_host, run_count, offers, words: int):
        self.words = int(words)
        self.run_host = [np.ascontiguousarray(h, np.uint32) for h in run_host]
        self.run_count = [np.ascontiguousarray(c, np.uint32) for c in run_count]
        self.offers = [np.ascontiguousarray(o, np.uint32).reshape(-1, self.words) for o in offers]
        self.lib, self.allocs = None, []
        self._point([(h.ctypes.data, c.ctypes.data, o.ctypes.data)
                     for h, c, o in zip(self.run_host, self.run_count, self.offers)])

    def _point(self, ptrs):
        n = len(self.run_host)
        self.n_stages = n
        self.n_offers = sum(len(o) for o in self.offers)
        self.stage_runs = (C.c_uint32 * max(n, 1))(*[len(h) for h in self.run_host])
        self.stage_offers = (C.c_uint64 * max(n, 1))(*[len(o) for o in self.offers])
        self.p_host, self.p_count, self.p_offers = ((C.c_void_p * max(n, 1))(*[p[i] for p in ptrs]) for i in range(3))

    @classmethod
    def from_grouped(cls, off, time, prio, size, payload, dst, pkt, *, time_base: int, n_threads: int,
                     first_host: int = 0, sock=None, words: int | None = None, seed: int = 7, idle=(),
                     keep_empty: float = 0.5):
        """Offers grouped by host (``OutboundStage.advance``'s arrays) -> stages.  Every host goes
        to one of the ``n_threads`` threads not listed in ``idle`` and each thread runs its hosts
        in a shuffled order; a host without offers keeps a run of count 0 with probability
        ``keep_empty``.  ``words``: 10 when ``sock`` is given, else 8."""
        words = words or (OFFER_WORDS_SOCK if sock is not None else OFFER_WORDS)
        rng = np.random.default_rng(seed)
        off = np.asarray(off, np.int64)
        H, n = len(off) - 1, int(off[-1])
        rec = np.zeros((n, words), np.uint32)
        t = np.asarray(time, np.uint64) - np.uint64(time_base)
        assert n == 0 or int(t.max()) < 2**32, "time_off is 32 bits"
        lo32, hi32 = (lambda a: (np.asarray(a, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32),
                      lambda a: (np.asarray(a, np.uint64) >> np.uint64(32)).astype(np.uint32))
        rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4] = t.astype(np.uint32), dst, size, payload, pkt
        rec[:, 6], rec[:, 7] = lo32(prio), hi32(prio)
        if words == OFFER_WORDS_SOCK and sock is not None:
            rec[:, 8], rec[:, 9] = lo32(sock), hi32(sock)
        busy = np.array([k for k in range(n_threads) if k not in set(idle)], np.int64)
        cnt = np.diff(off)
        thread = busy[rng.integers(0, len(busy), H)] if H else np.zeros(0, np.int64)
        staged = (cnt > 0) | (rng.random(H) < keep_empty)
        run_host, run_count, offers = [], [], []
        for k in range(n_threads):
            hs = np.flatnonzero((thread == k) & staged)
            rng.shuffle(hs)
            c = cnt[hs]
            idx = np.repeat(off[hs] - (np.cumsum(c) - c), c) + np.arange(int(c.sum()))
            run_host.append((hs + first_host).astype(np.uint32))
            run_count.append(c.astype(np.uint32))
            offers.append(rec[idx])
        return cls(run_host, run_count, offers, words)

    def grouped(self, time_base: int, n_hosts: int, first_host: int = 0):
        """``group_offers`` of these stages."""
        return group_offers(self.run_host, self.run_count, self.offers, self.words, time_base, n_hosts, first_host)

    def pinned(self, lib, which=None) -> "OfferStages":
        """A copy whose arrays lie in ``shd_host_alloc`` memory (``which``: only the stages it
        lists; the others stay pageable); ``free`` returns the memory."""
        p = OfferStages(self.run_host, self.run_count, self.offers, self.words)
        p.lib = lib
        ptrs = []
        for k, arrs in enumerate(zip(p.run_host, p.run_count, p.offers)):
            row = []
            for a in arrs:
                if which is not None and k not in which:
                    row.append(a.ctypes.data)
                    continue
                ptr = lib.shd_host_alloc(max(a.nbytes, 1))
                if not ptr:
                    p.free()
                    raise MemoryError("shd_host_alloc")
                p.allocs.append(ptr)
                C.memmove(ptr, a.ctypes.data, a.nbytes)
                row.append(ptr)
            ptrs.append(tuple(row))
        p._point(ptrs)
        return p

    def free(self):
        for ptr in self.allocs:
            self.lib.shd_host_free(ptr)
        self.allocs = []

    def args(self):
        """The stage arguments of ``shd_offers_group`` / ``shd_window_close_staged``."""
        return (self.n_stages, self.stage_runs, self.p_host, self.p_count, self.stage_offers, self.p_offers, self.words)


@dataclass
class GroupedOffers:
    """``shd_offers_group``'s outputs: engine-owned device pointers (valid until the next group),
    in the order ``OutboundStage.advance_device`` takes them (``d_sock`` by keyword)."""
    d_off: int
    d_time: int
    d_prio: int
    d_size: int
    d_payload: int
    d_dst: int
    d_pkt: int
    n_offers: int
    d_sock: int | None


def group_stages(engine, stages: OfferStages, time_base: int) -> GroupedOffers:
    """``shd_offers_group`` on the engine's outbound stage (``OutboundStage.group_stages``)."""
    o = [C.c_void_p() for _ in range(8)]
    n = C.c_uint64(0)
    N.check(engine.lib.shd_offers_group(engine.ctx, *stages.args(), int(time_base), *map(C.byref, o), C.byref(n)),
            "shd_offers_group")
    d_off, d_time, d_prio, d_sock, d_size, d_pay, d_dst, d_pkt = (x.value for x in o)
    return GroupedOffers(d_off, d_time, d_prio, d_size, d_pay, d_dst, d_pkt, n.value, d_sock)


class OutboundStage:
    def __init__(self, engine, capacity, refill_increment, refill_interval, last_refill=SIM_START,
                 first_host: int = 0, ring_capacity: int = 4096, qdisc: str = "fifo", max_sockets: int = 64):
        """``ring_capacity``: the packets a host may have queued; ``max_sockets`` (every discipline
        but ``"fifo"``): the sockets it may have in its rrQueue or heap at once."""
        if qdisc not in QDISC:
            raise ValueError(f"qdisc must be one of {sorted(QDISC)}, not {qdisc!r}")
        self.eng = engine
        self.qdisc = qdisc
        cap = np.ascontiguousarray(capacity, np.uint64)
        self.n_hosts = len(cap)
        self.first_host = int(first_host)
        inc = np.ascontiguousarray(np.broadcast_to(np.asarray(refill_increment, np.uint64), cap.shape))
        itv = np.ascontiguousarray(np.broadcast_to(np.asarray(refill_interval, np.uint64), cap.shape))
        last = np.ascontiguousarray(np.broadcast_to(np.asarray(last_refill, np.uint64), cap.shape))
        self.max_sockets = int(max_sockets)
        N.check(engine.lib.shd_outbound_setup_qdisc(engine.ctx, self.n_hosts, self.first_host, int(ring_capacity),
                                                    QDISC[qdisc], self.max_sockets, N.ptr(cap), N.ptr(inc),
                                                    N.ptr(itv), N.ptr(last)), "shd_outbound_setup_qdisc")

    @classmethod
    def from_bandwidth(cls, engine, bytes_per_second, start: int = SIM_START, first_host: int = 0,
                       ring_capacity: int = 4096, qdisc: str = "fifo", max_sockets: int = 64):
        """One ``create_token_bucket`` (relay/mod.rs:291-302) of ``bw_up / 8`` bytes per second per
        host, last refilled at ``start``; an entry of ``None`` (or a negative one) is a host without
        a bucket."""
        rows = [(0, 0, 0) if b is None or int(b) < 0 else create_token_bucket(int(b)) for b in bytes_per_second]
        cap, inc, itv = (np.array([r[i] for r in rows], np.uint64) for i in range(3))
        return cls(engine, cap, inc, itv, start, first_host, ring_capacity, qdisc, max_sockets)

    def advance_device(self, d_off, d_time, d_prio, d_size, d_payload, d_dst, d_pkt, n_offers: int,
                       window_end: int, bootstrap_end: int = 0, d_sock=None) -> DeviceBatch:
        """Device pointers (ints, ctypes pointers or torch tensors; all None for no offers).
        ``d_prio`` is the discipline's 64-bit key per offer: the packet priority under FIFO, the
        socket's canonical handle under round-robin.  The two socket disciplines take the packet
        priority (0: control) in ``d_prio`` and the socket's canonical handle in ``d_sock``; the
        other two ignore ``d_sock``."""
        as_p = lambda a: a if a is None or isinstance(a, (int, C.c_void_p)) else N.ptr(a)  # noqa: E731
        b = N.Batch()
        sp, lo, lp, lt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n_local, n_stored, nxt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        N.check(self.eng.lib.shd_outbound_advance_sockets(
            self.eng.ctx, as_p(d_off), as_p(d_time), as_p(d_prio), as_p(d_sock), as_p(d_size), as_p(d_payload),
            as_p(d_dst), as_p(d_pkt), int(n_offers), int(window_end), int(bootstrap_end), C.byref(b), C.byref(sp),
            C.byref(lo), C.byref(lp), C.byref(lt), C.byref(n_local), C.byref(n_stored), C.byref(nxt)),
            "shd_outbound_advance")
        return DeviceBatch(b, sp.value, lo.value, lp.value, lt.value, b.n_packets, n_local.value, n_stored.value,
                           nxt.value)

    def group_stages(self, stages: OfferStages, time_base: int) -> GroupedOffers:
        """``shd_offers_group``: the threads' staged offers grouped by host on the device, into
        the arrays ``advance_device`` takes: ``g = stage.group_stages(st, base)``, then
        ``stage.advance_device(g.d_off, g.d_time, g.d_prio, g.d_size, g.d_payload, g.d_dst, g.d_pkt,
        g.n_offers, window_end, d_sock=g.d_sock)``."""
        return group_stages(self.eng, stages, time_base)

    def grouped_host(self, g: GroupedOffers):
        """Host copies of a group's arrays: ``(off, time, prio, sock, size, payload, dst, pkt)``,
        ``sock`` None at width 8."""
        n = g.n_offers
        out = [np.zeros(self.n_hosts + 1, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64),
               np.zeros(n, np.uint64) if g.d_sock else None] + [np.zeros(n, np.uint32) for _ in range(4)]
        for dst, src in zip(out, (g.d_off, g.d_time, g.d_prio, g.d_sock, g.d_size, g.d_payload, g.d_dst, g.d_pkt)):
            if dst is not None and dst.nbytes:
                N.check(self.eng.lib.shd_copy_to_host(self.eng.ctx, N.ptr(dst), C.c_void_p(src), dst.nbytes),
                        "shd_copy_to_host")
        return tuple(out)

    def advance(self, off=None, time=None, prio=None, size=None, payload=None, dst=None, pkt=None, *,
                window_end: int, bootstrap_end: int = 0, sock=None) -> Sent:
        """Host arrays of one window's offers grouped by host (or none) -> host copies.  ``sock``
        (the offering sockets' canonical handles) is the round-robin spelling of ``prio``: the
        same column; giving both is an error.  Under the two socket disciplines ``prio`` and
        ``sock`` are two columns and both are given."""
        d_sock = None
        if self.qdisc in SOCKET_QDISCS:
            if off is not None and (prio is None or sock is None):
                raise ValueError(f"qdisc {self.qdisc!r} takes both prio and sock")
        elif sock is not None:
            if prio is not None:
                raise ValueError("prio and sock name the same column: give one")
            prio = sock
        keep = [None] * 7
        n = 0
        if off is not None:
            import torch
            n = len(time)
            dev = lambda a, np_dt, dt: torch.from_numpy(np.ascontiguousarray(a, np_dt).view(dt)).cuda()  # noqa: E731
            keep = [dev(off, np.uint32, np.int32), dev(time, np.uint64, np.int64), dev(prio, np.uint64, np.int64)] + \
                   [dev(a, np.uint32, np.int32) for a in (size, payload, dst, pkt)]
            assert len(keep[0]) == self.n_hosts + 1 and all(len(k) == n for k in keep[1:])
            if self.qdisc in SOCKET_QDISCS:
                d_sock = dev(sock, np.uint64, np.int64)
                assert len(d_sock) == n
            torch.cuda.synchronize()
        out = self.advance_device(*keep, n, window_end, bootstrap_end, d_sock)
        del keep, d_sock
        return self.sent(out)

    def sent(self, out: DeviceBatch) -> Sent:
        """Host copies of an advance's batch and local deliveries."""
        ns, nl = out.n_sent, out.n_local
        src_off, loc_off = np.zeros(self.n_hosts + 1, np.uint32), np.zeros(self.n_hosts + 1, np.uint32)
        t, d, p, sp = np.zeros(ns, np.uint64), np.zeros(ns, np.uint32), np.zeros(ns, np.uint32), np.zeros(ns, np.uint32)
        lp, lt = np.zeros(nl, np.uint32), np.zeros(nl, np.uint64)
        b = out.batch
        for dst, src in ((src_off, b.src_off), (t, b.send_time), (d, b.dst_host), (p, b.payload), (sp, out.sent_pkt),
                         (loc_off, out.loc_off), (lp, out.loc_pkt), (lt, out.loc_time)):
            if dst.nbytes:
                N.check(self.eng.lib.shd_copy_to_host(self.eng.ctx, N.ptr(dst), C.c_void_p(src), dst.nbytes),
                        "shd_copy_to_host")
        return Sent(src_off, t, d, p, sp, loc_off, lp, lt, out.n_stored, out.next_task_time)

    def update_buckets(self, hosts, capacity, refill_increment, refill_interval, at_time: int):
        """``shd_outbound_update_buckets``: the named hosts' ``bw_up`` buckets re-rated at
        ``at_time`` (>= the last ``window_end``; all three parameters 0: no bucket).  ``hosts`` are
        the stage's own indices (global id ``first_host + h``).  Queues, sockets, the cached packet
        and the outstanding task stay as they are.  A refusal (ShdError, ``.host`` the lowest
        failing host) changes nothing."""
        update_buckets(self.eng, "shd_outbound_update_buckets", hosts, capacity, refill_increment, refill_interval,
                       at_time)

    def update_bandwidth(self, hosts, bytes_per_second, at_time: int):
        """``update_buckets`` with ``create_token_bucket`` per entry, as ``from_bandwidth`` (None:
        no bucket)."""
        self.update_buckets(hosts, *bandwidth_rows(bytes_per_second), at_time)

    def sockets(self, host: int) -> list:
        """One host's queued sockets: ``[(handle, queued packets), ...]`` -- in rrQueue order under
        the round-robin disciplines, the heap array in index order under ``"fifo-sockets"``.  Not
        under ``"fifo"``."""
        hd, cn = np.zeros(self.max_sockets, np.uint64), np.zeros(self.max_sockets, np.uint32)
        n = C.c_uint32(0)
        N.check(self.eng.lib.shd_outbound_get_sockets(self.eng.ctx, int(host), N.ptr(hd), N.ptr(cn), len(hd),
                                                      C.byref(n)), "shd_outbound_get_sockets")
        return list(zip(hd[:n.value].tolist(), cn[:n.value].tolist()))

    def state(self, host: int) -> dict:
        """One host: ``task_time`` (None: Idle), ``cached`` ((pkt, size) or None), ``queue_len``,
        ``head_pkt`` (the packet the next pop takes, None: empty) and the bucket as
        ``TokenBuckets.state`` (None: no bucket)."""
        task, has, cp, cs = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        ql, hp, b = C.c_uint32(0), C.c_uint32(0), N.TbState()
        N.check(self.eng.lib.shd_outbound_get_state(self.eng.ctx, int(host), C.byref(task), C.byref(has),
                                                    C.byref(cp), C.byref(cs), C.byref(ql), C.byref(hp), C.byref(b)),
                "shd_outbound_get_state")
        bucket = {k: int(getattr(b, k)) for k, _ in N.TbState._fields_} if b.capacity else None
        return {"task_time": None if task.value == IDLE else task.value,
                "cached": (cp.value, cs.value) if has.value else None, "queue_len": ql.value,
                "head_pkt": None if hp.value == NO_PKT else hp.value, "bucket": bucket}
