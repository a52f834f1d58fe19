"""GPU: calls of different kinds on one chain ensemble back to back.  Every call uploads its per-chain table into the
handle's one device buffer through the handle's pinned staging; what keeps a call's table from the next call's is the
stream's order and the staging's events alone.  So the same sequence is run twice -- as written, with no host wait between
the calls but hp_slice's own, and on a fresh ensemble with a synchronise after every call -- and everything the two
return and leave behind must be equal bit for bit."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import smc_helpers as H

pytestmark = pytest.mark.gpu

SPECS = [(orc.BB, 0), (orc.GP, 0), (orc.NICH, 0)]      # three features: the marginal block's tail is more than one entry
N, K, NCHAINS, ROUNDS = 96, 8, 3, 3


def _coords(ens):
    from common_amd import hypers, models
    from common_amd.scalar_functions import log_exponential
    return hypers.EnsembleHpSlice(ens, [models.bb, models.gp, models.nich],
                                  cparam={"alpha": (log_exponential(1.0), 1.0)}).coords


def _run(gpu_ctx, wait):
    """the sequence on a fresh ensemble -> (every tensor and array the calls returned, in order; what is left behind)"""
    feats, _, view = H.data(gpu_ctx, SPECS, N, K, seed=5)
    ens = H.ensemble(gpu_ctx, feats, K, NCHAINS)
    ens.seat(view, seed=100)
    coords = _coords(ens)
    got = []            # (device tensors stay alive until the end: nothing is read back between the calls)

    def done(*tensors):
        got.extend(tensors)
        if wait:
            gpu_ctx.synchronize()

    for r in range(ROUNDS):
        s = 10 * r
        ens.sweep(view, 1, 200 + s, sweep=1 + s)
        done()
        done(ens.score_joint())
        sm = ens.split_merge(view, 300 + s, sweep=2 * s, nproposals=2, want_log=True)
        done(sm.counters, sm.log)
        done(*ens.predictive_logp(view, per_chain=True))
        vals, chains, groups = ens.sample_predictive(view, seed=400 + s, sweep=r)
        done(chains, groups, *[vals[f] for f in sorted(vals)])
        ens.clone([0, 0, 2])
        done()
        done(ens.visit(view, 0, N // 2, 500 + s, sweep=2 + s, want_logp=True))
        done(ens.visit(view, N // 2, N - N // 2, 500 + s, sweep=2 + s, want_logp=True))
        done(*ens.hp_slice(coords, 600 + s, sweep=r))
    gpu_ctx.synchronize()
    bits = [np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t).tobytes() for t in got]
    left = [H.ensemble_bits(ens)] + [[st.get_hp(f).tobytes() for f in range(len(SPECS))] +
                                      [np.float32(st.get_alpha()).tobytes()] for st in ens.states]
    ens.close()
    return bits, left


def test_back_to_back_calls_equal_synchronised_calls(gpu_ctx):
    bits, left = _run(gpu_ctx, wait=False)
    bits_w, left_w = _run(gpu_ctx, wait=True)
    assert len(bits) == len(bits_w) == ROUNDS * (1 + 2 + 2 + 2 + len(SPECS) + 2 + 2)
    for i, (a, b) in enumerate(zip(bits, bits_w)):
        assert a == b, "returned tensor %d differs" % i
    assert left == left_w
