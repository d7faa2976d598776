"""CPU model of the packet ledger (shadow_amd/csrc/ledger.hip, ledger_book.h): a dict of batches
with the engine's refusals and its ``entries_held`` rule -- space comes back in batch order, so a
batch that drains before an older one stays held until the older one is gone."""
import numpy as np

NONE = None
REFUSED = 2**32 - 1


class LedgerRefused(Exception):
    """A refusal before anything runs: the ledger stays as it was."""


class LedgerDead(Exception):
    """SHD_ERR_STATE: a gather refused an event; only a setup brings the ledger back."""


class LedgerModel:
    def __init__(self, max_live_batches=0):
        if max_live_batches > 4096:
            raise LedgerRefused("max_live_batches")
        self.max_live = max_live_batches or 1024
        self.held = {}       # batch -> [size array, pkt array, live]   (held: oldest .. newest)
        self.last = None
        self.dead = False

    def _alive(self):
        if self.dead:
            raise LedgerDead()

    def record(self, batch, size, pkt, n_live):
        self._alive()
        n = len(size)
        if batch >= 2**32 - 1 or (self.last is not None and batch <= self.last) or n_live > n:
            raise LedgerRefused("batch number / n_live")
        if n_live and self.held and batch - min(self.held) >= self.max_live:
            raise LedgerRefused("table full")
        self.last = batch
        if n_live:
            self.held[batch] = [np.array(size, np.uint32), np.array(pkt, np.uint32), int(n_live)]

    def gather(self, tag):
        """-> (ok, size, pkt).  Not ok: the ledger is dead; a refused event has REFUSED in both
        outputs.  Of an overdrawn batch the model refuses every event of the call (the engine
        refuses at least the surplus: compare those events with ``overdrawn``)."""
        self._alive()
        tag = np.asarray(tag, np.uint64)
        size = np.full(len(tag), REFUSED, np.uint32)
        pkt = np.full(len(tag), REFUSED, np.uint32)
        pops = {}
        for k, t in enumerate(tag.tolist()):
            b, i = t >> 32, t & 0xFFFFFFFF
            e = self.held.get(b)
            if e is None or e[2] == 0 or i >= len(e[0]):
                continue
            pops.setdefault(b, []).append(k)
            size[k], pkt[k] = e[0][i], e[1][i]
        self.overdrawn = {b: ks for b, ks in pops.items() if len(ks) > self.held[b][2]}
        for ks in self.overdrawn.values():
            size[ks] = REFUSED
            pkt[ks] = REFUSED
        if (size == REFUSED).any() or self.overdrawn:
            self.dead = True
            return False, size, pkt
        for b, ks in pops.items():
            self.held[b][2] -= len(ks)
        while self.held and self.held[min(self.held)][2] == 0:
            del self.held[min(self.held)]
        return True, size, pkt

    def stats(self):
        """(live_batches, live_events, entries_held, oldest_batch)"""
        self._alive()
        live = [e[2] for e in self.held.values()]
        return (sum(1 for x in live if x), sum(live), sum(len(e[0]) for e in self.held.values()),
                min(self.held) if self.held else NONE)
