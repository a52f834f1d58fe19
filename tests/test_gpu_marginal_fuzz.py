"""Row predictive log-density, fuzzed (the style of test_gpu_fuzz.py: a few cases on every run): random scalar feature
lists, 38-384 groups, 33 k-70 k rows, a sample of rows against the oracle's double twin under the gates of
test_gpu_marginal.py."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.gpu_helpers import random_hp
from tests.test_gpu_marginal import Case, check_case

pytestmark = pytest.mark.gpu
POOL = [(orc.BB, 0), (orc.BBNC, 0), (orc.GP, 0), (orc.BNB, 0), (orc.DD, 3), (orc.DD, 17), (orc.NICH, 0)]


@pytest.mark.parametrize("seed", [101, 202, 303, 404])
def test_random_scalar_feature_lists(gpu_ctx, seed):
    rng = np.random.default_rng(seed)
    specs = [POOL[i] for i in rng.integers(0, len(POOL), int(rng.integers(1, 9)))]
    K = int(rng.integers(38, 385))
    N = int(rng.integers(33000, 70001))
    hrng = np.random.default_rng((7919, seed))       # the hyperparameters' own stream: the seed's shapes and data stay
    c = Case(gpu_ctx, specs, N, K, seed=seed, alpha=float(rng.choice([0.5, 1.5, 4.0])), used=K - int(rng.integers(1, 6)),
             hp_of=lambda j, family, dim: random_hp(family, dim, hrng))
    name = "fuzz_%d" % seed
    check_case(c, name, nsample=1024)
    check_case(c, name, z=c.loo_z(seed), nsample=1024)
