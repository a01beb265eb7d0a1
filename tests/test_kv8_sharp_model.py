"""No GPU: the inputs of tests/test_kv8_sharp.py -- the same tensors, built by tests/kv8_shapes.py at the same shapes -- (i) drive the
data-dependent branches where each pattern says (the branch-taken conditions, from the dequantised inputs alone) and (ii) separate a
right softmax from two wrong ones at the GPU test's tolerance: an fp64 model that does not rescale the running O by alpha where the max
rises, and one that sums a tile's four wave-private (l, O) without the exp(m_w - M) factors, each miss the tolerance by at least 4x in some
element.  So the GPU test has the power to fail.

One (model, pattern) pair cannot fail by construction, and is asserted to be exactly that: `no_alpha` under `sink`.  The sink is the
path's FIRST key: the max never rises after tile 0, every later alpha is exp(0) = 1, and skipping a multiplication by 1 changes nothing
(the model's output equals the right one's to rounding).  Every other pair must fail."""
import pytest
import torch

import kv8_model
import kv8_shapes as ks
from tools.error_bound import bound_bf16, dense_attention

F16, BF16 = torch.float16, torch.bfloat16
GEOMS = [(4, 4), (8, 2), (3, 3)]
K_SCALES = [0.73, 1.9, 1.21, 0.57]  # tests/test_kv8_gpu.py
V_SCALES = [0.61, 0.7, 0.37, 0.53]
PREFIX, WIDTH, BRANCH = 1000, 8, 150
_TREES = {}


def _paths(Hkv):
    if Hkv not in _TREES:
        _, paths, size = ks.cpu_few_shot_tree(PREFIX, WIDTH, BRANCH, Hkv)
        _TREES[Hkv] = (paths, size)
    return _TREES[Hkv]


def test_the_grid_helpers():
    vals = set(kv8_model.code_values()[:127].tolist())
    assert ks.grid_at_least(74.4) == 80.0 and ks.grid_at_least(80.0) == 80.0 and ks.grid_at_least(2.0 ** -9) == 2.0 ** -9
    assert all(ks.BOTTOM + ks.STEP * i in vals or -(ks.BOTTOM + ks.STEP * i) in vals for i in range(10))
    assert all(abs(v) in vals for v in ks.V_VALUES)
    assert [r // 32 for r in ks.RISE_AT] == [0, 1, 2, 3]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_branches_are_taken_and_wrong_models_fail(geom, dtype):
    Hq, Hkv = geom
    paths, size = _paths(Hkv)
    scales = K_SCALES[:Hkv]
    k_sc = torch.tensor(scales, dtype=torch.float32)[:, None]
    v_sc = torch.tensor(V_SCALES[:Hkv], dtype=torch.float32)[:, None]
    tile = ks.SPIKE_TILE[geom]
    for pattern in ks.PATTERNS:
        codes, q, heads = ks.shaped_case(pattern, paths, size, PREFIX, Hq, Hkv, scales, tile, dtype)
        k64 = kv8_model.dequantize(codes[:, 0], k_sc)
        v64 = kv8_model.dequantize(codes[:, 1], v_sc)
        s = ks.path_scores(q, k64, paths, Hq, Hkv)
        diff = ks.assert_branch_taken(pattern, heads, s, PREFIX, Hq, Hkv, tile)
        truth, A = dense_attention(q, k64, v64, paths, Hq, Hkv, ks.D ** -0.5, with_abs=True)
        tol = 5e-4 + 2.0 ** -11 * truth.abs() if dtype == F16 else bound_bf16(truth, A)
        outs = ks.model_outputs(s, v64, paths, Hq, Hkv)
        assert float((outs["right"] - truth).abs().max()) < 1e-9  # (the model is right but for the omission)
        miss = {name: float(((outs[name] - truth).abs() / tol).max()) for name in ("no_alpha", "no_wave_factors")}
        print(f"[kv8] power {pattern} {Hq}x{Hkv} {'fp16' if dtype == F16 else 'bf16'}: no-alpha misses by {miss['no_alpha']:.3g} x tol, "
              f"no-wave-factors by {miss['no_wave_factors']:.3g} x tol; smallest cross-wave gap {diff:.1f} nats", flush=True)
        assert miss["no_wave_factors"] >= 4.0, (pattern, miss)
        if pattern == "sink":
            assert miss["no_alpha"] < 1e-3, (pattern, miss)  # cannot expose it: every alpha after the first key is 1 (module docstring)
        else:
            assert miss["no_alpha"] >= 4.0, (pattern, miss)
