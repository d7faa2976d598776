"""The sharded scheduling window over the caller's host transport (shd_comm_init_host): two
PROCESSES on cuda:0 over gloo on 127.0.0.1, each with its own engine context, run the chain's
three windows -- open, then the collective close (the precondition agreement, the sharded round,
the sharded ledger record) -- and each holds its rank's outputs against the composed oracle, which
every process runs for itself.  The code paths are the RCCL runs' (RCCL refuses two ranks on one
GPU); only the transport differs."""
import pytest
import torch.distributed as dist

from tests.test_hostcomm import _init, _spawn

pytestmark = pytest.mark.gpu


def _window_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        from oracle.token_bucket import SIM_START as S
        from shadow_amd import dist as D
        from shadow_amd.routing import Engine
        from tests.test_outbound_gpu import ChainOracle, chain_case, chain_offers
        from tests.test_window_sharded_gpu import RankParts, run_windows
        eng = Engine(0)
        hc = D.HostComm(eng)
        o = ChainOracle(S + 10**12)
        _, _, _, _, rng0, out_b, in_b = chain_case()
        part = RankParts(eng, o, rng0, out_b, in_b)
        prio = [0] * o.H
        first = (S + 10**9, S + 10**9 + o.ra.get())
        run_windows([part], o, lambda k, ws, we: chain_offers(k, ws, we, o.H, prio), 3, first, all_ranks=False)
        st = part.ledger.stats()
        q.put((rank, dict(lo=part.lo, hi=part.hi, batches=len(o.batches), live=st.live_events)))
        del hc
        eng.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(not (dist.is_available() and dist.is_gloo_available()),
                    reason="torch.distributed was built without gloo: no host transport to run over")
@pytest.mark.timeout(300)
def test_host_comm_two_processes_three_windows():
    res = _spawn(_window_worker, 2, timeout=280)
    assert [(res[r]["lo"], res[r]["hi"]) for r in (0, 1)] == [(0, 32), (32, 64)]
    assert res[0]["batches"] == res[1]["batches"] >= 2
