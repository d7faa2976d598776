"""CPU model of the outbound stage under ``interface_qdisc: round-robin`` (test infrastructure):
the interface's rrQueue restated literally --

* ``RrSocketQueue`` (``network_queuing_disciplines.c:29-88``): a plain queue of sockets, ``find`` a
  linear search by canonical handle;
* a socket's own output buffer (``socket.c:434-467``): a FIFO of the packets it was offered;
* ``networkinterface_wantsSend`` (``network_interface.c:366-392``): find, else push at the tail;
* ``_networkinterface_selectRoundRobin`` (``network_interface.c:235-273``): pop the head socket,
  pull its first packet, push the socket back if it still has data, before the relay knows what
  becomes of the packet --

under the relay loop of ``tests/outbound_model.py``, which is reused as it is: ``OutboundHost``'s
``advance`` and ``_forward`` reach the discipline through the module name ``heapq`` alone
(``heappush(self.q, packet)`` at an offer, ``heappop(self.q)`` at a pop), so the two functions are
bound here a second time with that one name meaning the round-robin discipline.  The per-offer key
(``prio`` in the FIFO model) is the socket's canonical handle.

Counters beside the FIFO model's (``ties``, ``carried``, ``blocks``, ...):

* ``not_in_offer_order``  pops whose packet was not the oldest queued on the host: what a FIFO
                          discipline over ascending priorities would have taken instead;
* ``joins``               sockets pushed behind a non-empty rrQueue;
* ``reentries``           sockets pushed that had drained and left the rrQueue before;
* ``blocked_rotated``     blocks whose cached packet's socket is in the rrQueue (it has rotated).
"""
from __future__ import annotations

import types
from collections import deque

from tests import outbound_model as FM
from tests.outbound_model import IDLE, LOCAL, SENT, OutboundHost, OutboundModel  # noqa: F401 -- re-exported

RR_COUNTERS = ("not_in_offer_order", "joins", "reentries", "blocked_rotated")


class Socket:
    """What the interface sees of a socket: its canonical handle and its output buffer."""

    def __init__(self, handle):
        self.handle = handle
        self.out = deque()

    def has_data_to_send(self):
        return bool(self.out)

    def pull_out_packet(self):
        return self.out.popleft() if self.out else None


class RrInterface:
    """One host's sockets and its rrQueue."""

    def __init__(self, ctr):
        self.rr = deque()          # RrSocketQueue: the GQueue of sockets
        self.sockets = {}          # canonical handle -> Socket (every socket the host ever used)
        self.ctr = ctr
        self.seq = 0               # offers so far: the order a FIFO discipline would serve
        self.left = set()          # handles that have been in the rrQueue and left it
        self.max_sockets = 0
        self.passed = 0

    # rrsocketqueue_find: a linear search by canonical handle
    def find(self, sock):
        for s in self.rr:
            if s.handle == sock.handle:
                return True
        return False

    def wants_send(self, sock):
        """networkinterface_wantsSend, Q_DISC_MODE_ROUND_ROBIN."""
        if not sock.has_data_to_send():
            return
        if not self.find(sock):
            self.ctr["joins"] += bool(self.rr)
            self.ctr["reentries"] += sock.handle in self.left
            self.rr.append(sock)
            self.max_sockets = max(self.max_sockets, len(self.rr))

    def offer(self, packet):
        """The socket takes the packet into its buffer and tells the interface."""
        sock = self.sockets.setdefault(packet[0], Socket(packet[0]))
        sock.out.append(packet + (self.seq,))
        self.seq += 1
        self.passed += 1
        self.wants_send(sock)

    def select_round_robin(self):
        """_networkinterface_selectRoundRobin."""
        packet = None
        while packet is None and self.rr:
            sock = self.rr.popleft()
            oldest = min(s.out[0][-1] for s in [sock, *self.rr] if s.out)
            packet = sock.pull_out_packet()
            if packet is None:
                continue
            self.ctr["not_in_offer_order"] += packet[-1] != oldest
            if sock.has_data_to_send():
                self.rr.append(sock)
            else:
                self.left.add(sock.handle)
            return packet[:-1]
        return None

    # what the relay loop asks of its queue
    def __len__(self):
        return sum(len(s.out) for s in self.rr)

    def __iter__(self):
        return (p for s in self.rr for p in s.out)

    def head_pkt(self):
        return self.rr[0].out[0][1] if self.rr else None

    def listing(self):
        """[(handle, queued packets)] in rrQueue order: what shd_outbound_get_sockets returns."""
        return [(s.handle, len(s.out)) for s in self.rr]


class _RoundRobin:
    """The discipline under the two names the relay loop calls."""

    @staticmethod
    def heappush(q, packet):
        q.offer(packet)

    @staticmethod
    def heappop(q):
        return q.select_round_robin()


def _rebound(f):
    g = dict(f.__globals__)
    g["heapq"] = _RoundRobin
    return types.FunctionType(f.__code__, g, f.__name__, f.__defaults__, f.__closure__)


class RrOutboundHost(OutboundHost):
    def __init__(self, bucket, host_id, ctr):
        super().__init__(bucket, host_id)
        self.q = RrInterface(ctr)

    advance = _rebound(OutboundHost.advance)
    _forward_loop = _rebound(OutboundHost._forward)

    def _forward(self, now, bootstrap_end, out, ctr):
        d = self._forward_loop(now, bootstrap_end, out, ctr)
        if d is not None:   # blocked: the packet is cached, its socket went round at the pop
            ctr["blocked_rotated"] += any(s.handle == self.cached[0] for s in self.q.rr)
        return d


class RrOutboundModel(OutboundModel):
    """``OutboundModel`` with round-robin hosts: ``advance`` takes the handles where it takes the
    priorities.  (``out_of_order``, which the relay loop still counts, compares handles and means
    nothing here.)"""

    def __init__(self, buckets, first_host=0):
        super().__init__([], first_host)
        self.counters.update({k: 0 for k in RR_COUNTERS})
        self.hosts = [RrOutboundHost(b, first_host + h, self.counters) for h, b in enumerate(buckets)]

    @property
    def max_sockets(self):
        return max((x.q.max_sockets for x in self.hosts), default=0)

    @property
    def max_passed(self):
        return max((x.q.passed for x in self.hosts), default=0)


# the loop's two doors to its queue are where this module expects them
assert "heappush" in FM.OutboundHost.advance.__code__.co_names
assert "heappop" in FM.OutboundHost._forward.__code__.co_names
