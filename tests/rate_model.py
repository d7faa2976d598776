"""The bucket re-rate as a CPU model (test infrastructure), built only from the oracle's
``TokenBucket`` and its ``lazy_refill``: what ``shd_tb_update`` / ``shd_*_update_buckets`` do to one
host's bucket.  The GPU tests apply it to ``model.hosts[h].tb``.

The reference builds a relay's bucket once and has no counterpart; the definition is put together
from ``token_bucket.rs:37-60`` (``new_inner``) and ``:127-157`` (``lazy_refill``):

* bucket -> bucket: ``lazy_refill(at)`` under the old parameters, then ``new_inner(C, I, N, at)``
  whose balance is ``min(refilled balance, C)`` instead of ``C``;
* none -> bucket: ``new_inner(C, I, N, at)``, full;
* bucket -> none (all three 0): the host is unlimited; none -> none: nothing.
"""
from __future__ import annotations

from oracle.token_bucket import ReferencePanic, TokenBucket  # noqa: F401  (ReferencePanic: what rerate raises)


def rerate(tb, at: int, capacity: int, increment: int, interval: int):
    """The bucket (or None) that replaces ``tb`` (a TokenBucket or None) after a re-rate at ``at``.
    Raises ReferencePanic where the old bucket's refill to ``at`` panics in the reference
    (``at`` before its ``last_refill`` among them) and ValueError for some-but-not-all-zero."""
    if not (capacity or increment or interval):
        if tb is not None:
            tb.lazy_refill(at)     # the old rate holds up to `at`: its panics are the call's
        return None
    new = TokenBucket(capacity, increment, interval, at)   # ValueError: partial zeros
    if tb is not None:
        tb.lazy_refill(at)
        new.balance = min(tb.balance, capacity)
    return new
