"""CPU model of the outbound stage (test infrastructure): per host the reference's outbound relay
``relay_inet_out`` (``src/main/host/host.rs:285-288``, ``:871-880``) -- the interface's FIFO
queuing discipline (``network_interface.c:276-316``: the lowest packet priority goes first; one
``heapq`` by priority per host, since every socket offers its packets in increasing priority),
``Relay::notify`` (``relay/mod.rs:110-135``) and the forward task
(``Relay::forward_until_blocked``, ``relay/mod.rs:200-272``) over the oracle's ``TokenBucket`` as it
is.

A host consumes its offers in order, merged with its own forward task; an offer at the task's own
time is inserted before the task runs (the sends of one event accumulate, ``relay/mod.rs:124-126``).
A task at or after the window's end stays outstanding for the next call.  Records are
(kind, pkt, time, dst, payload) with kind SENT = 1 (the packet enters ``Worker::send_packet``,
``router/mod.rs:49-55``) or LOCAL = 2 (``dst`` is the host itself: forwarded without the bucket,
back to the interface), in the order they happened."""
from __future__ import annotations

import heapq

import numpy as np

from oracle.token_bucket import TokenBucket, emutime_sat_add

SENT, LOCAL = 1, 2
IDLE = 2**64 - 1


class OutboundHost:
    def __init__(self, bucket, host_id):
        """bucket: (capacity, refill_increment, refill_interval, last_refill) or None (unlimited)."""
        self.q = []               # heap of (prio, pkt, size, payload, dst)
        self.tb = TokenBucket(*bucket) if bucket is not None else None
        self.id = host_id         # the global id a packet's dst is compared with
        self.task = None          # time of the outstanding forward task (RelayState::Pending)
        self.cached = None        # RelayInternal::next_packet: (prio, pkt, size, payload, dst)
        self.max_depth = 0

    def stored(self) -> int:
        return len(self.q) + (self.cached is not None)

    def _forward(self, now, bootstrap_end, out, ctr):
        """forward_until_blocked at ``now``; returns the blocking duration or None."""
        boot = now < bootstrap_end                       # Worker::is_bootstrapping, once per task
        while True:
            p, self.cached = self.cached, None
            if p is None:
                if not self.q:
                    return None                          # ran out of packets: Idle
                p = heapq.heappop(self.q)                # the FIFO discipline: lowest priority
            _, pkt, size, payload, dst = p
            local = dst == self.id                       # relay/mod.rs:222-230
            if not boot and not local and self.tb is not None:
                ok, v = self.tb.conforming_remove(size, now)
                if not ok:
                    self.cached = p
                    ctr["blocks"] += 1
                    return v
            out.append((LOCAL if local else SENT, pkt, now, dst, payload))
            ctr["local_forwards"] += local
            ctr["boot_forwards"] += boot and not local

    def advance(self, offers, window_end, bootstrap_end, ctr):
        """offers: [(time, prio, size, payload, dst, pkt)] in order -> this window's records."""
        out = []
        ctr["carried"] += self.task is not None
        i = 0
        while True:
            t_of = offers[i][0] if i < len(offers) else None
            if t_of is not None and (self.task is None or t_of <= self.task):
                _, prio, size, payload, dst, pkt = offers[i]
                i += 1
                ctr["ties"] += self.task == t_of
                ctr["out_of_order"] += bool(self.q) and prio < max(e[0] for e in self.q)
                heapq.heappush(self.q, (prio, pkt, size, payload, dst))
                self.max_depth = max(self.max_depth, len(self.q))
                if self.task is None:                    # Relay::notify: forward_later(ZERO)
                    self.task = t_of
            elif self.task is not None and self.task < window_end:
                now, self.task = self.task, None         # run_forward_task: Idle again
                d = self._forward(now, bootstrap_end, out, ctr)
                if d is not None:
                    self.task = emutime_sat_add(now, d)  # forward_later(blocking_dur)
            else:
                return out


class OutboundModel:
    def __init__(self, buckets, first_host=0):
        self.hosts = [OutboundHost(b, first_host + h) for h, b in enumerate(buckets)]
        self.counters = {"blocks": 0, "carried": 0, "ties": 0, "local_forwards": 0, "boot_forwards": 0,
                         "out_of_order": 0}

    def advance(self, off, time, prio, size, payload, dst, pkt, window_end, bootstrap_end=0):
        """One window for every host -> a dict: the batch (src_off, send_time, dst_host, payload,
        sent_pkt), the local CSR (loc_off, loc_pkt, loc_time), n_stored, next_task_time."""
        src_off, s_time, s_dst, s_pay, s_pkt = [0], [], [], [], []
        loc_off, l_pkt, l_time = [0], [], []
        for h, host in enumerate(self.hosts):
            a, b = (int(off[h]), int(off[h + 1])) if off is not None else (0, 0)
            of = [(int(time[k]), int(prio[k]), int(size[k]), int(payload[k]), int(dst[k]), int(pkt[k]))
                  for k in range(a, b)]
            for kind, p, t, d, pl in host.advance(of, window_end, bootstrap_end, self.counters):
                if kind == SENT:
                    s_pkt.append(p); s_time.append(t); s_dst.append(d); s_pay.append(pl)
                else:
                    l_pkt.append(p); l_time.append(t)
            src_off.append(len(s_pkt))
            loc_off.append(len(l_pkt))
        tasks = [x.task for x in self.hosts if x.task is not None]
        return dict(src_off=np.array(src_off, np.uint32), send_time=np.array(s_time, np.uint64),
                    dst_host=np.array(s_dst, np.uint32), payload=np.array(s_pay, np.uint32),
                    sent_pkt=np.array(s_pkt, np.uint32), loc_off=np.array(loc_off, np.uint32),
                    loc_pkt=np.array(l_pkt, np.uint32), loc_time=np.array(l_time, np.uint64),
                    n_stored=sum(x.stored() for x in self.hosts), next_task_time=min(tasks) if tasks else IDLE)

    @property
    def max_depth(self):
        return max((x.max_depth for x in self.hosts), default=0)
