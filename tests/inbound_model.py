"""CPU model of the inbound stage (test infrastructure): per host the reference's chain from
``Host::execute``'s packet branch (``src/main/host/host.rs:742-746``) through
``Router::route_incoming_packet`` and ``Relay::notify`` (``relay/mod.rs:110-135``) to the forward
task (``Relay::forward_until_blocked``, ``relay/mod.rs:200-272``), composed from the oracle's
``CoDelQueue`` and ``TokenBucket`` as they are.

A host consumes its packet events in order, merged with its own forward task; at equal time a
packet event runs before the task (``core/work/event.rs:102-110``).  A task at or after the
window's end stays outstanding for the next call.  Records are (kind, pkt, time) with kind
FORWARDED = 1 or DROPPED = 2, in the order they happened."""
from __future__ import annotations

import numpy as np

from oracle.codel import CoDelQueue
from oracle.token_bucket import TokenBucket, emutime_sat_add

FORWARDED, DROPPED = 1, 2
IDLE = 2**64 - 1


class InboundHost:
    def __init__(self, bucket):
        """bucket: (capacity, refill_increment, refill_interval, last_refill) or None (unlimited)."""
        self.q = CoDelQueue()
        self.tb = TokenBucket(*bucket) if bucket is not None else None
        self.task = None          # time of the outstanding forward task (RelayState::Pending)
        self.cached = None        # RelayInternal::next_packet
        self.size = {}            # pkt -> total size, for the packets held here
        self.max_depth = 0

    def stored(self) -> int:
        return len(self.q) + (self.cached is not None)

    def _forward(self, now, bootstrap_end, out, ctr):
        """forward_until_blocked at ``now``; returns the blocking duration or None."""
        boot = now < bootstrap_end                       # Worker::is_bootstrapping, once per task
        while True:
            pkt, self.cached = self.cached, None
            if pkt is None:
                before = len(self.q.dropped)
                pkt = self.q.pop(now)
                for d in self.q.dropped[before:]:        # the drops of a pop come before its packet
                    out.append((DROPPED, d, now))
                    del self.size[d]
                    ctr["drops"] += 1
                if pkt is None:
                    return None                          # ran out of packets: Idle
            if not boot and self.tb is not None:
                ok, v = self.tb.conforming_remove(self.size[pkt], now)
                if not ok:
                    self.cached = pkt
                    ctr["blocks"] += 1
                    return v
            out.append((FORWARDED, pkt, now))
            del self.size[pkt]
            ctr["boot_forwards"] += boot

    def advance(self, events, window_end, bootstrap_end, ctr):
        """events: [(time, size, pkt)] in order -> this window's records."""
        out = []
        ctr["carried"] += self.task is not None
        i = 0
        while True:
            t_ev = events[i][0] if i < len(events) else None
            if t_ev is not None and (self.task is None or t_ev <= self.task):
                _, size, pkt = events[i]
                i += 1
                ctr["ties"] += self.task == t_ev
                self.size[pkt] = size
                self.q.push(pkt, size, t_ev)             # Router::route_incoming_packet
                self.max_depth = max(self.max_depth, len(self.q))
                if self.task is None:                    # Relay::notify: forward_later(ZERO)
                    self.task = t_ev
            elif self.task is not None and self.task < window_end:
                now, self.task = self.task, None         # run_forward_task: Idle again
                d = self._forward(now, bootstrap_end, out, ctr)
                if d is not None:
                    self.task = emutime_sat_add(now, d)  # forward_later(blocking_dur)
            else:
                return out


class InboundModel:
    def __init__(self, buckets):
        self.hosts = [InboundHost(b) for b in buckets]
        self.counters = {"blocks": 0, "carried": 0, "ties": 0, "boot_forwards": 0, "drops": 0}

    def advance(self, off, time, size, pkt, window_end, bootstrap_end=0):
        """One window for every host -> (out_off, pkt, time, kind, n_stored, next_task_time)."""
        o_off, o_pkt, o_time, o_kind = [0], [], [], []
        for h, host in enumerate(self.hosts):
            a, b = (int(off[h]), int(off[h + 1])) if off is not None else (0, 0)
            ev = [(int(time[k]), int(size[k]), int(pkt[k])) for k in range(a, b)]
            for kind, p, t in host.advance(ev, window_end, bootstrap_end, self.counters):
                o_kind.append(kind); o_pkt.append(p); o_time.append(t)
            o_off.append(len(o_pkt))
        tasks = [x.task for x in self.hosts if x.task is not None]
        return (np.array(o_off, np.uint32), np.array(o_pkt, np.uint32), np.array(o_time, np.uint64),
                np.array(o_kind, np.uint8), sum(x.stored() for x in self.hosts), min(tasks) if tasks else IDLE)

    @property
    def max_depth(self):
        return max((x.max_depth for x in self.hosts), default=0)
