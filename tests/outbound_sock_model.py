"""CPU model of the outbound stage's two socket disciplines (test infrastructure): the interface
with both output buffers of a socket, restated literally --

* ``Socket`` (``socket.c:432-437``, ``:182-189``, ``:466-467``): a packet of priority 0 goes to the
  control buffer, every other one to the data buffer; peek and pull take the control buffer first;
* ``PriorityQueue`` (``priority_queue.c:87-140``, ``:189-208``): the array heap, line for line, under
  ``_compareSocket`` (``network_queuing_disciplines.c:90-102``): the sockets' head priorities as
  they are *now*, a tie "smaller" both ways;
* ``FifoSockInterface``: ``networkinterface_wantsSend`` (``network_interface.c:366-392``: find, else
  push) and ``_networkinterface_selectFirstInFirstOut`` (``:276-316``: pop the root socket, pull its
  head packet, push the socket again if it still has data);
* ``RrSockInterface``: the same over the rrQueue (``:235-273``), a plain queue of sockets --

under the relay loop of ``tests/outbound_model.py``, bound the way ``tests/outbound_rr_model.py``
binds it: ``heappush`` and ``heappop`` mean the discipline.  The per-offer key is the pair
``(priority, socket handle)``.

Counters beside the FIFO model's:

* ``stale_key``        control offered to a socket that stands below the heap's root with an empty
                       control buffer: its key changes where it stands;
* ``control_heads3``   offers after which three or more queued sockets have a control head;
* ``not_lowest``       pops whose packet's priority is above the lowest head priority queued;
* ``blocked_rotated``  blocks whose cached packet's socket is queued again;
* ``slots_reused``     offers that would take a pool slot freed by a pop (the pool of
                       ``sock_queue.h``: an empty queue starts it over, one packet takes no slot).
"""
from __future__ import annotations

import types
from collections import deque

import numpy as np

from tests.outbound_model import IDLE, LOCAL, SENT, OutboundHost, OutboundModel  # noqa: F401 -- re-exported

SOCK_COUNTERS = ("stale_key", "control_heads3", "not_lowest", "blocked_rotated", "slots_reused")


class Socket:
    """What the interface sees of a socket: its canonical handle and its two output buffers."""

    def __init__(self, handle):
        self.handle = handle
        self.control = deque()     # outputControlBuffer
        self.out = deque()         # outputBuffer

    def add(self, packet):
        """socket.c:432-437; a packet is ((priority, handle), pkt, size, payload, dst)."""
        (self.control if packet[0][0] == 0 else self.out).append(packet)

    def has_data_to_send(self):
        return bool(self.control) or bool(self.out)

    def peek_next_packet_priority(self):
        """socket.c:182-189: the control buffer first; None: no packet."""
        if self.control:
            return self.control[0][0][0]
        return self.out[0][0][0] if self.out else None

    def pull_out_packet(self):
        """socket.c:466-467."""
        if self.control:
            return self.control.popleft()
        return self.out.popleft() if self.out else None

    def __len__(self):
        return len(self.control) + len(self.out)


def compare_socket(sa, sb):
    """network_queuing_disciplines.c:90-102."""
    pa = sa.peek_next_packet_priority()
    if pa is None:
        return -1
    pb = sb.peek_next_packet_priority()
    if pb is None:
        return +1
    return +1 if pa > pb else -1


class PriorityQueue:
    """priority_queue.c: the heap array; entries are compared when they move, never otherwise."""

    def __init__(self, compare):
        self.heap = []
        self.compare = compare

    def _swap_entries(self, i, j):
        self.heap[i], self.heap[j] = self.heap[j], self.heap[i]

    def _entry_smaller(self, i, j):
        return self.compare(self.heap[i], self.heap[j]) < 0

    def _heapify_up(self, index):
        while index > 0 and self._entry_smaller(index, (index - 1) // 2):
            self._swap_entries(index, (index - 1) // 2)
            index = (index - 1) // 2
        return index

    def _heapify_down(self, index, size):
        while True:
            child = 2 * index + 1
            if child >= size:
                break
            if child + 1 < size and self._entry_smaller(child + 1, child):
                child = child + 1
            if self._entry_smaller(child, index):
                self._swap_entries(index, child)
                index = child
            else:
                break
        return index

    def push(self, data):
        for i, e in enumerate(self.heap):
            if e is data:   # (the map's lookup; the interface never pushes a queued socket)
                self._heapify_up(self._heapify_down(i, len(self.heap)))
                return False
        self.heap.append(data)
        self._heapify_up(len(self.heap) - 1)
        return True

    def pop(self):
        if not self.heap:
            return None
        data = self.heap[0]
        self._swap_entries(0, len(self.heap) - 1)
        self.heap.pop()
        self._heapify_down(0, len(self.heap))
        return data

    def __len__(self):
        return len(self.heap)

    def __iter__(self):
        return iter(self.heap)


class _Fifo:
    """fifosocketqueue_*: the heap of sockets."""

    def __init__(self):
        self.pq = PriorityQueue(compare_socket)

    def push(self, sock):
        self.pq.push(sock)

    def pop(self):
        return self.pq.pop()

    def order(self):
        return list(self.pq.heap)     # the heap array in index order


class _Rr:
    """rrsocketqueue_*: a plain queue."""

    def __init__(self):
        self.dq = deque()

    def push(self, sock):
        self.dq.append(sock)

    def pop(self):
        return self.dq.popleft() if self.dq else None

    def order(self):
        return list(self.dq)


class SockInterface:
    """One host's sockets and the queue of those that have data."""
    queue_type = None

    def __init__(self, ctr):
        self.queue = self.queue_type()
        self.sockets = {}          # canonical handle -> Socket (every socket the host ever used)
        self.ctr = ctr
        self.max_sockets = 0
        self.passed = 0
        self.not_lowest = False    # a pop of this host took a packet above the lowest head priority
        self.free_slots = 0        # sock_queue.h's pool: slots on the free list
        self.lone = False          # the queue's one packet lies outside the pool

    def find(self, sock):
        return any(s.handle == sock.handle for s in self.queue.order())

    def wants_send(self, sock):
        """networkinterface_wantsSend."""
        if not sock.has_data_to_send():
            return
        if not self.find(sock):
            self.queue.push(sock)
            self.max_sockets = max(self.max_sockets, len(self.queue.order()))

    def offer(self, packet):
        """The socket takes the packet into the buffer its priority names, then tells the interface."""
        handle = packet[0][1]
        sock = self.sockets.setdefault(handle, Socket(handle))
        order = self.queue.order()
        if packet[0][0] == 0 and not sock.control and sock in order[1:]:
            self.ctr["stale_key"] += 1
        if len(self) == 0:         # the pool: a queue's one packet takes no slot ...
            self.lone = True
        elif self.lone:            # ... until a second one comes: both take fresh ones
            self.lone = False
        elif self.free_slots:
            self.free_slots -= 1
            self.ctr["slots_reused"] += 1
        sock.add(packet)
        self.passed += 1
        self.wants_send(sock)
        self.ctr["control_heads3"] += sum(bool(s.control) for s in self.queue.order()) >= 3

    def select(self):
        """_networkinterface_selectFirstInFirstOut / _networkinterface_selectRoundRobin."""
        packet = None
        while packet is None and self.queue.order():
            lowest = min(s.peek_next_packet_priority() for s in self.queue.order())
            sock = self.queue.pop()
            packet = sock.pull_out_packet()
            if packet is None:
                continue
            if packet[0][0] > lowest:
                self.ctr["not_lowest"] += 1
                self.not_lowest = True
            if sock.has_data_to_send():
                self.queue.push(sock)
            self.free_slots = 0 if len(self) == 0 else self.free_slots + 1   # (an empty queue starts the pool over)
            self.lone = False
            return packet
        return None

    # what the relay loop asks of its queue
    def __len__(self):
        return sum(len(s) for s in self.queue.order())

    def __iter__(self):
        return (p for s in self.queue.order() for p in (*s.control, *s.out))

    def head_pkt(self):
        """The packet the next pop takes."""
        order = self.queue.order()
        if not order:
            return None
        s = order[0]
        return (s.control[0] if s.control else s.out[0])[1]

    def listing(self):
        """[(handle, queued packets)] -- FIFO: the heap array in index order; round-robin: rrQueue
        order: what shd_outbound_get_sockets returns."""
        return [(s.handle, len(s)) for s in self.queue.order()]


class FifoSockInterface(SockInterface):
    queue_type = _Fifo


class RrSockInterface(SockInterface):
    queue_type = _Rr


class _Discipline:
    """The discipline under the two names the relay loop calls."""

    @staticmethod
    def heappush(q, packet):
        q.offer(packet)

    @staticmethod
    def heappop(q):
        return q.select()


def _rebound(f):
    g = dict(f.__globals__)
    g["heapq"] = _Discipline
    return types.FunctionType(f.__code__, g, f.__name__, f.__defaults__, f.__closure__)


class SockOutboundHost(OutboundHost):
    def __init__(self, bucket, host_id, ctr, interface):
        super().__init__(bucket, host_id)
        self.q = interface(ctr)

    advance = _rebound(OutboundHost.advance)
    _forward_loop = _rebound(OutboundHost._forward)

    def _forward(self, now, bootstrap_end, out, ctr):
        d = self._forward_loop(now, bootstrap_end, out, ctr)
        if d is not None:   # blocked: the packet is cached, its socket was pushed again at the pop
            ctr["blocked_rotated"] += any(s.handle == self.cached[0][1] for s in self.q.queue.order())
        return d


class SockOutboundModel(OutboundModel):
    """``OutboundModel`` over socket hosts; ``advance`` takes the priority column and the socket
    column.  ``qdisc``: "fifo-sockets", "round-robin-sockets" or a ``SockInterface`` class.  (``out_of_order``, which the relay
    loop still counts, compares the key pairs and means nothing here.)"""

    def __init__(self, buckets, first_host=0, qdisc="fifo-sockets"):
        super().__init__([], first_host)
        self.counters.update({k: 0 for k in SOCK_COUNTERS})
        itf = qdisc if isinstance(qdisc, type) else \
            {"fifo-sockets": FifoSockInterface, "round-robin-sockets": RrSockInterface}[qdisc]
        self.hosts = [SockOutboundHost(b, first_host + h, self.counters, itf) for h, b in enumerate(buckets)]

    def advance(self, off, time, prio, sock, size, payload, dst, pkt, window_end, bootstrap_end=0):
        """One window for every host -> the dict of ``OutboundModel.advance``."""
        src_off, s_time, s_dst, s_pay, s_pkt = [0], [], [], [], []
        loc_off, l_pkt, l_time = [0], [], []
        for h, host in enumerate(self.hosts):
            a, b = (int(off[h]), int(off[h + 1])) if off is not None else (0, 0)
            of = [(int(time[k]), (int(prio[k]), int(sock[k])), int(size[k]), int(payload[k]), int(dst[k]), int(pkt[k]))
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
    def max_sockets(self):
        return max((x.q.max_sockets for x in self.hosts), default=0)

    @property
    def max_passed(self):
        return max((x.q.passed for x in self.hosts), default=0)
