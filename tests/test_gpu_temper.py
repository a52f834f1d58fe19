"""GPU: the tempered ensemble's steps between sweeps (msc_chains_exchange, msc_chains_anneal_weights;
ChainEnsemble.exchange / anneal_weights) -- the exchange rule and the annealing weights against their numpy restatements
(tests/temper_helpers.py) exactly, on joint rows written by hand and on rows msc_chains_score_joint wrote; a broken
ladder through the device error word; the arguments."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import smc_helpers as H
from tests import temper_helpers as TH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R", [4, 5])
def test_the_exchange_rule(gpu_ctx, R):
    """hand-written joint rows, no sweep: 3 ladders, both parities, one NaN and one -inf likelihood, a padded row stride.
    beta, rung and the counters equal the restatement exactly after every call; rung stays a permutation per ladder and
    beta[c] == betas[rung[c]].  A broken permutation leaves that ladder as it was and surfaces at the next call."""
    import common_amd
    from common_amd import tempering
    dev, nl, F = gpu_ctx.torch_device, 3, 2
    ens = common_amd.ChainEnsemble(gpu_ctx, [(orc.BB, 0), (orc.NICH, 0)], 8, nl * R)
    rng = np.random.default_rng(40 + R)
    betas = tempering.ladder(R, "linear")
    joint = rng.normal(-20.0, 4.0, (nl * R, F + 4))                  # (a padded row: ld_joint = F + 4)
    joint[1, 2] = np.nan
    joint[R + 2, 3] = -np.inf
    rung = np.concatenate([rng.permutation(R) for _ in range(nl)]).astype(np.int32)
    beta = betas[rung]
    prop = acc = np.zeros((nl, R - 1), dtype=np.int32)
    jt = torch.from_numpy(joint).to(dev)
    bt, rt = torch.from_numpy(beta).to(dev), torch.from_numpy(rung).to(dev)
    pt, at = (torch.zeros((nl, R - 1), dtype=torch.int32, device=dev) for _ in range(2))
    for step, parity in enumerate((0, 1, 2, 3, 1, 0)):
        ens.exchange(jt, bt, rt, R, parity, 77, 10 + step, (pt, at))
        beta, rung, prop, acc, bad = TH.exchange_np(joint, F, R, beta, rung, parity, 77, 10 + step, prop, acc)
        assert not bad
        assert bt.cpu().numpy().tobytes() == beta.tobytes(), step
        assert np.array_equal(rt.cpu().numpy(), rung), step
        assert np.array_equal(pt.cpu().numpy(), prop) and np.array_equal(at.cpu().numpy(), acc), step
        for l in range(nl):
            assert sorted(rung[l * R:(l + 1) * R].tolist()) == list(range(R))
        assert np.array_equal(beta, betas[rung])
    print("exchange R=%d: proposed %s accepted %s" % (R, prop.sum(0), acc.sum(0)))
    assert 0 < acc.sum() < prop.sum()
    # a ladder whose rungs are no permutation is left as it was; the others go on; the next call reports it
    broken = rung.copy()
    broken[R] = broken[R + 1]
    rt.copy_(torch.from_numpy(broken))
    ens.exchange(jt, bt, rt, R, 0, 77, 99, (pt, at))
    beta2, rung2, prop2, acc2, bad = TH.exchange_np(joint, F, R, beta, broken, 0, 77, 99, prop, acc)
    assert bad == [1]
    assert bt.cpu().numpy().tobytes() == beta2.tobytes() and np.array_equal(rt.cpu().numpy(), rung2)
    assert np.array_equal(rung2[R:2 * R], broken[R:2 * R]) and np.array_equal(beta2[R:2 * R], beta[R:2 * R])
    assert np.array_equal(pt.cpu().numpy(), prop2) and np.array_equal(prop2[1], prop[1])
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        ens.exchange(jt, bt, rt, R, 1, 77, 100, (pt, at))
    assert e.value.code == -6 and "msc_chains_exchange" in str(e.value)
    assert np.array_equal(rt.cpu().numpy(), rung2)                  # (the refused call launched nothing)
    rt.copy_(torch.from_numpy(rung))
    ens.exchange(jt, bt, rt, R, 1, 77, 100, (pt, at))               # (reported once)
    ens.close()


def test_exchange_and_weights_on_the_joint_of_an_ensemble(gpu_ctx):
    """the rows msc_chains_score_joint wrote for 12 chains of the small mix: two ladders of six rungs exchange as the
    restatement does on the downloaded rows, and the weights of a step are (beta_to - beta_from) L to the bit"""
    from common_amd import tempering
    N, K, nchains, R = 200, 12, 12, 6
    feats, masks, view = H.data(gpu_ctx, H.C3_SMALL, N, K, seed=91, mask_col=2)
    F, dev = len(feats), gpu_ctx.torch_device
    ens = H.ensemble(gpu_ctx, feats, K, nchains)
    ens.seat(view, seed=17)
    ens.sweep(view, 2, 17, sweep=1)
    joint = ens.score_joint()
    rows = joint.cpu().numpy()
    assert np.isfinite(rows).all() and len({TH.chain_loglik(r, F) for r in rows}) > 1
    beta = np.tile(tempering.ladder(R, "linear"), nchains // R)             # chain l R + j starts on rung j
    rung = np.tile(np.arange(R, dtype=np.int32), nchains // R)
    bt, rt = torch.from_numpy(beta).to(dev), torch.from_numpy(rung).to(dev)
    pt, at = (torch.zeros((nchains // R, R - 1), dtype=torch.int32, device=dev) for _ in range(2))
    prop = acc = np.zeros((nchains // R, R - 1), dtype=np.int32)
    for i in range(8):
        ens.exchange(joint, bt, rt, R, i, 5, i, (pt, at))
        beta, rung, prop, acc, bad = TH.exchange_np(rows, F, R, beta, rung, i, 5, i, prop, acc)
        assert not bad and bt.cpu().numpy().tobytes() == beta.tobytes() and np.array_equal(rt.cpu().numpy(), rung), i
    assert np.array_equal(pt.cpu().numpy(), prop) and np.array_equal(at.cpu().numpy(), acc) and acc.sum() > 0
    # the weights of a step towards the rung above; the chains on rung 0 stay where they are and weigh nothing
    to = torch.from_numpy(tempering.ladder(R, "linear")[np.maximum(rung - 1, 0)]).to(dev)
    ens.logw.fill_(0.25)
    ens.anneal_weights(joint, bt, to)
    want = TH.anneal_np(rows, F, beta, to.cpu().numpy(), np.full(nchains, 0.25))
    assert ens.logw.cpu().numpy().tobytes() == want.tobytes()
    assert np.all(want[rung == 0] == 0.25) and np.all(want[rung != 0] != 0.25)
    # the sweep that follows is the one that would have followed without them: no state was touched
    twin = H.ensemble(gpu_ctx, feats, K, nchains)
    twin.seat(view, seed=17)
    twin.sweep(view, 2, 17, sweep=1)
    ens.sweep(view, 1, 17, sweep=3)
    twin.sweep(view, 1, 17, sweep=3)
    assert ens.z.cpu().numpy().tobytes() == twin.z.cpu().numpy().tobytes()
    twin.close()
    ens.close()


def test_arguments(gpu_ctx):
    import common_amd
    lib, dev = gpu_ctx.lib, gpu_ctx.torch_device
    for name in ("msc_chains_exchange", "msc_chains_anneal_weights"):
        assert hasattr(lib, name) and name in common_amd.EXPORTS
    nchains, F = 6, 2
    ens = common_amd.ChainEnsemble(gpu_ctx, [(orc.NICH, 0), (orc.BB, 0)], 8, nchains)
    rows = np.random.default_rng(5).normal(-9.0, 2.0, (nchains, F + 3))
    joint = torch.from_numpy(rows).to(dev)
    beta = torch.ones(nchains, dtype=torch.float32, device=dev)
    rung = torch.arange(3, dtype=torch.int32).repeat(2).to(dev)
    prop, acc = (torch.zeros((2, 2), dtype=torch.int32, device=dev) for _ in range(2))
    logw = torch.zeros(nchains, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    ex = lib.msc_chains_exchange
    # msc_chains_exchange: MSC_EINVAL launches nothing, so nothing changes
    assert ex(ens._h, p(joint), F + 3, 3, p(beta), p(rung), 0, 1, 0, p(prop), p(acc)) == 0
    for bad in ((None, p(joint), F + 3, 3, p(beta), p(rung), 0, 1, 0, p(prop), p(acc)),
                (ens._h, None, F + 3, 3, p(beta), p(rung), 0, 1, 0, p(prop), p(acc)),
                (ens._h, p(joint), F + 3, 3, None, p(rung), 0, 1, 0, p(prop), p(acc)),
                (ens._h, p(joint), F + 3, 3, p(beta), None, 0, 1, 0, p(prop), p(acc)),
                (ens._h, p(joint), F + 3, 3, p(beta), p(rung), 0, 1, 0, None, p(acc)),
                (ens._h, p(joint), F + 3, 3, p(beta), p(rung), 0, 1, 0, p(prop), None),
                (ens._h, p(joint), F + 3, 0, p(beta), p(rung), 0, 1, 0, p(prop), p(acc)),
                (ens._h, p(joint), F + 3, 4, p(beta), p(rung), 0, 1, 0, p(prop), p(acc)),
                (ens._h, p(joint), F + 2, 3, p(beta), p(rung), 0, 1, 0, p(prop), p(acc))):
        assert ex(*bad) == -1, bad
    assert int(prop.sum().item()) == 2                              # the one good call's pairs, and no other
    aw = lib.msc_chains_anneal_weights
    half = torch.full((nchains,), 0.5, dtype=torch.float32, device=dev)
    for bad in ((None, p(joint), F + 3, p(half), p(beta), p(logw)), (ens._h, None, F + 3, p(half), p(beta), p(logw)),
                (ens._h, p(joint), F + 3, None, p(beta), p(logw)), (ens._h, p(joint), F + 3, p(half), None, p(logw)),
                (ens._h, p(joint), F + 3, p(half), p(beta), None), (ens._h, p(joint), F + 2, p(half), p(beta), p(logw))):
        assert aw(*bad) == -1, bad
    assert not logw.any().item()
    # equal temperatures leave an entry alone, an infinite likelihood included; an infinite one otherwise is -inf
    rows[2, 2] = rows[4, 3] = -np.inf
    frm, to = half.clone(), beta.clone()
    to[2] = 0.5
    ens.anneal_weights(torch.from_numpy(rows).to(dev), frm, to, logw)
    want = TH.anneal_np(rows, F, frm.cpu().numpy(), to.cpu().numpy(), np.zeros(nchains))
    assert logw.cpu().numpy().tobytes() == want.tobytes() and want[2] == 0.0 and want[4] == -np.inf and want[0] != 0.0
    # the binding's own checks
    with pytest.raises(ValueError):
        ens.exchange(joint, beta, rung, 4, 0, 1, 0, (prop, acc))
    with pytest.raises(ValueError):
        ens.exchange(joint, beta.double(), rung, 3, 0, 1, 0, (prop, acc))
    with pytest.raises(ValueError):
        ens.exchange(joint, beta, rung.cpu(), 3, 0, 1, 0, (prop, acc))
    with pytest.raises(ValueError):
        ens.exchange(joint[:, :F + 2], beta, rung, 3, 0, 1, 0, (prop, acc))
    with pytest.raises(ValueError):
        ens.exchange(joint, beta, rung, 3, 0, 1, 0, (prop[:1], acc))
    with pytest.raises(ValueError):
        ens.anneal_weights(joint, half, beta[:3], logw)
    ens.close()
