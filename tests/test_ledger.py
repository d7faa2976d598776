"""CPU tier of the packet ledger: the dict model's hand vectors (tests/ledger_model.py), and the
engine's host bookkeeping (shadow_amd/csrc/ledger_book.h) compiled into a program of its own
(tests/ledger_book_main.cpp) with the address and undefined-behaviour sanitizers and run against
the model on a scripted sequence: out-of-order drain, wrap, growth while batches are live, a full
table.  The program stands alone: nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from tests.ledger_model import REFUSED, LedgerDead, LedgerModel, LedgerRefused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tags(*pairs):
    return np.array([(b << 32) | i for b, i in pairs], np.uint64)


def test_model_gather_and_entries_held():
    m = LedgerModel()
    m.record(0, [100, 101, 102, 103, 104], [10, 11, 12, 13, 14], 3)
    m.record(1, [200], [20], 1)
    assert m.stats() == (2, 4, 6, 0)
    ok, size, pkt = m.gather(tags((1, 0), (0, 4)))
    assert ok and size.tolist() == [200, 104] and pkt.tolist() == [20, 14]
    # batch 1 has drained before batch 0: it stays held
    assert m.stats() == (1, 2, 6, 0)
    ok, size, pkt = m.gather(tags((0, 0), (0, 0)))   # the same packet twice is two pops
    assert ok and size.tolist() == [100, 100]
    assert m.stats() == (0, 0, 0, None)
    ok, _, _ = m.gather(tags())
    assert ok


def test_model_record_refusals_change_nothing():
    m = LedgerModel(2)
    m.record(3, [1, 2], [7, 8], 2)
    for bad in ((3, [1], [1], 1), (2, [1], [1], 1), (4, [1], [1], 2), (5, [1], [1], 1)):   # 5 - 3 >= 2: full
        with pytest.raises(LedgerRefused):
            m.record(*bad)
    assert m.stats() == (1, 2, 2, 3)
    m.record(4, [5], [9], 0)        # no live event: nothing stored, the number is used up
    assert m.stats() == (1, 2, 2, 3)
    with pytest.raises(LedgerRefused):
        m.record(4, [5], [9], 1)
    with pytest.raises(LedgerRefused):
        LedgerModel(4097)


@pytest.mark.parametrize("bad, n_refused", [((9, 0), 1), ((0, 2), 1), ((1, 0), 1)])
def test_model_gather_refusals(bad, n_refused):
    """A batch never recorded, an index past the batch, a batch already drained (held behind
    batch 0): REFUSED for that event, the good one right, then dead."""
    m = LedgerModel()
    m.record(0, [100, 101], [10, 11], 2)
    m.record(1, [200], [20], 1)
    assert m.gather(tags((1, 0)))[0]
    ok, size, pkt = m.gather(tags((0, 1), bad))
    assert not ok and size.tolist() == [101, REFUSED] and pkt.tolist() == [11, REFUSED]
    with pytest.raises(LedgerDead):
        m.stats()
    with pytest.raises(LedgerDead):
        m.record(2, [1], [1], 1)


def test_model_overdrawn():
    m = LedgerModel()
    m.record(0, [100, 101, 102], [10, 11, 12], 2)
    m.record(1, [200], [20], 1)
    ok, size, _ = m.gather(tags((0, 0), (1, 0), (0, 1), (0, 2)))
    assert not ok and size.tolist() == [REFUSED, 200, REFUSED, REFUSED] and m.overdrawn == {0: [0, 2, 3]}


@pytest.fixture(scope="module")
def book(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ledger_book") / "ledger_book")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "shadow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ledger_book_main.cpp"), "-o", exe])
    return exe


class Script:
    """The same steps into the model and into the program's script; the answers are compared after
    the one run."""

    def __init__(self, max_live, cap):
        self.m = LedgerModel(max_live)
        self.lines = [f"setup {max_live} {cap}"]
        self.want = []   # per line after the setup: a predicate over the answer's words

    def _stats(self):
        lb, le, eh, old = self.m.stats()
        self.lines.append("stats")
        self.want.append(lambda w, x=(lb, le, eh, -1 if old is None else old): tuple(map(int, w[:4])) == x)
        self.lines.append("verify")
        self.want.append(lambda w, n=len(self.m.held): w == ["ok", str(n)])

    def record(self, b, n, live, grew=None, base=None):
        try:
            self.m.record(b, np.arange(n), np.arange(n), live)
            first = "stored" if live else "nothing"
        except LedgerRefused:
            first = "refused"
        self.lines.append(f"record {b} {n} {live}")

        def ok(w):
            return w[0] == first and (grew is None or int(w[2]) == grew) and (base is None or int(w[1]) == base)
        self.want.append(ok)
        self._stats()

    def pop(self, b, k):
        i = np.arange(k) % len(self.m.held[b][0])
        assert self.m.gather((np.uint64(b) << np.uint64(32)) | i.astype(np.uint64))[0]
        self.lines.append(f"pop {b} {k}")
        self.want.append(lambda w: w == ["ok"])
        self._stats()

    def run(self, exe):
        out = subprocess.run([exe], input="\n".join(self.lines) + "\n", text=True, capture_output=True)
        assert out.returncode == 0, out.stderr[-2000:]
        answers = out.stdout.splitlines()
        assert len(answers) == len(self.want)
        for line, ans, ok in zip(self.lines[1:], answers, self.want):
            assert ok(ans.split()), (line, ans)
        return answers


def test_book_against_the_model_under_sanitizers(book):
    s = Script(8, 100)
    s.record(0, 40, 3, grew=0, base=0)
    s.record(1, 30, 2, base=40)
    s.record(2, 20, 1, base=70)
    s.pop(1, 2)                          # batch 1 drains before batch 0: held, 90 entries, oldest 0
    assert s.m.stats() == (2, 4, 90, 0)
    s.pop(0, 3)                          # now both go: the ring's used part is batch 2 at 70
    assert s.m.stats() == (1, 1, 20, 2)
    s.record(3, 50, 5, grew=0, base=0)   # 90 + 50 > 100: the slice starts again at 0 (wrap)
    s.record(4, 15, 15, grew=0, base=50)
    s.record(5, 30, 1, grew=1, base=85)  # 65 + 30 > 70: growth while wrapped; 2, 3, 4 move to 0, 20, 70
    s.pop(2, 1)
    s.record(6, 10, 0)                   # nothing stored, the number is used up
    s.record(6, 10, 1)                   # refused: not above the last one
    s.record(5, 10, 1)                   # refused
    s.record(7, 3, 4)                    # refused: more live than packets
    for b in (7, 8, 9, 10):
        s.record(b, 5, 2, grew=0)
    s.record(11, 5, 1)                   # refused: 11 - 3 = 8 numbers above the oldest held (3)
    s.pop(4, 15)
    s.pop(3, 5)                          # 3 and 4 go, the oldest is 5
    s.record(11, 5, 1, grew=0)           # ... and now there is a row for it
    for b in (5, 7, 8, 9, 10, 11):
        s.pop(b, s.m.held[b][2])
    assert s.m.stats() == (0, 0, 0, None)
    s.record(12, 1000, 7, grew=1, base=0)   # growth with nothing held
    s.record(13, 3000, 1, grew=1, base=1000)   # growth, not wrapped, a batch live
    s.pop(12, 7)
    s.record(14, 800, 1, grew=0, base=4000)
    s.record(15, 900, 900, grew=0, base=0)     # 4800 + 900 > 5000: the ring wraps again in the grown arena
    s.pop(14, 1)                               # drains behind 13: held
    s.pop(13, 1)
    s.pop(15, 900)
    answers = s.run(book)
    assert any(a.split()[-1] == "1" for a in answers if len(a.split()) == 6), "no step saw the ring wrapped"
