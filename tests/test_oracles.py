"""CPU self-tests of tests/oracles.py: the visible mean is tree_truth on K = 0 data, the tolerance behaves at binade edges and near 0,
the power check sees one key where it claims to, and the poison helper never touches a live slot."""
import pytest
import torch

import oracles
from deft_amd.memory_pool import TokenToKVPool
from truth import tree_truth


def _paths(seed, pool_size=3000, nq=7):
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(pool_size, generator=g).tolist()
    prefix, rest = perm[:900], perm[900:]
    return [prefix + rest[i * 40 : i * 40 + 10 + 5 * i] for i in range(nq)]


def test_visible_mean_is_tree_truth_on_zero_keys():
    g = torch.Generator().manual_seed(1)
    Hkv, G, D = 3, 2, 16
    paths = _paths(1)
    v = oracles.dyadic_(torch.empty((3000, Hkv, D), dtype=torch.float16), g)
    k = torch.zeros_like(v)
    q = torch.randn((len(paths), Hkv * G, D)).half()
    truth = tree_truth(q, k, v, paths, Hkv * G, Hkv, D ** -0.5)  # [nq, Hq, D]
    mean = oracles.visible_mean(v, paths, chunk=512).reshape(len(paths), Hkv, D)
    want = truth.reshape(len(paths), Hkv, G, D)
    for gg in range(G):
        assert float((mean - want[:, :, gg]).abs().max()) < 1e-12
    # exact dyadic values: |v| <= 3, multiples of 2^-9
    assert float(v.abs().max()) <= 3 and bool(((v.double() * 512).frac() == 0).all())


def test_visible_mean_refuses_a_path_that_holds_a_slot_twice():
    with pytest.raises(AssertionError):
        oracles.visible_mean(torch.zeros((8, 4)), [[1, 2, 1]])


def test_fp16_ulp_and_tolerance_at_binade_edges_and_near_zero():
    x = torch.tensor([1.0, 1.0 - 2.0 ** -12, 2.0, 2.0 - 2.0 ** -11, 0.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, -3.0, 65504.0],
                     dtype=torch.float64)
    want = torch.tensor([2.0 ** -10, 2.0 ** -11, 2.0 ** -9, 2.0 ** -10, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9, 32.0],
                        dtype=torch.float64)
    assert torch.equal(oracles.fp16_ulp(x), want)
    # the ulp is the distance to the next fp16 above the value, for every binade
    for e in range(-14, 15):
        for a in (torch.tensor([2.0 ** e], dtype=torch.float16), torch.tensor([-1.75 * 2.0 ** e], dtype=torch.float16)):
            up = (a.view(torch.int16) + 1).view(torch.float16)  # (the next fp16 away from 0)
            assert float((up.double() - a.double()).abs()) == float(oracles.fp16_ulp(a.double()))
    assert float(oracles.tolerance(torch.zeros(1))) == 2.0 ** -24 + oracles.FLOOR
    assert oracles.FLOOR < 1e-6


def test_power_check_sees_one_key_and_says_when_it_cannot():
    g = torch.Generator().manual_seed(3)
    v = oracles.dyadic_(torch.empty((70000, 2, 64), dtype=torch.float16), g)
    f = oracles.power_check(v, [list(range(66000))])
    assert f >= 4
    # 450k keys of random rows: one key is below 4 tolerances; the antithetic rows bring the mean to 0, where it is not
    big = oracles.dyadic_(torch.empty((450000, 1, 64), dtype=torch.float16), g)
    path = [list(range(450000))]
    with pytest.raises(AssertionError, match="cannot see one key"):
        oracles.power_check(big, path)
    oracles.antithetic_(big, path)
    assert oracles.power_check(big, path) >= 4


def test_poison_never_touches_a_live_slot():
    pool = TokenToKVPool(500, torch.float16, 2, 16, 3, device="cpu")
    g = torch.Generator().manual_seed(4)
    oracles.dyadic_(pool._storage, g)
    before = pool._storage.clone()
    paths = [[3, 4, 5, 100], [3, 4, 7]]
    live = oracles.live_slots(paths, extra=[499])
    for kind in ("nan", "inf"):
        pool._storage.copy_(before)
        n = oracles.poison_pool(pool, live, kind)
        assert n == 500 - 6
        st = pool._storage
        assert torch.equal(st[:, live], before[:, live])
        dead = torch.ones(500, dtype=torch.bool)
        dead[live] = False
        if kind == "nan":
            assert bool(st[:, dead].isnan().all())
        else:
            assert bool((st[:, dead, 0] == float("inf")).all()) and bool((st[:, dead, 1] == float("-inf")).all())


def test_running_max_rises_in():
    s = torch.tensor([0.0, 0, 5, 0, 0, 10, 0], dtype=torch.float64)
    assert oracles.running_max_rises_in(s, 5, 7) and oracles.running_max_rises_in(s, 2, 3)
    assert not oracles.running_max_rises_in(s, 3, 5)
