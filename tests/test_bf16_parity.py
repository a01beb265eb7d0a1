"""bfloat16 end to end against dense fp64 truth: Flatten, Node and the sequential comparator at every kernel family and at the shapes
where the plan's launch rules fire, with the a-priori bound of tests/bf16_util.py on EVERY element (every query row, head and
dim) and the RMS tripwire against the reference's arithmetic on the randn cases.  The truth reads the same bf16 tensors."""
import pytest
import torch

import deft_amd
import oracles
from bf16_util import BF16, check_against_truth, few_shot_tree
from deft_amd.utils.workloads import GEOMETRY, WORKLOADS, Workload, build_forest, build_tree
from truth import product_leaf_paths

pytestmark = pytest.mark.gpu


def _randn_step(tree, pool, Hq, Hkv, D, nq, seed, q_scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    pool._storage.normal_(generator=g)
    q = (torch.randn((nq, Hq * D), dtype=torch.float32, device="cuda", generator=g) * q_scale).to(BF16)
    k_new = torch.randn((nq, Hkv * D), dtype=BF16, device="cuda", generator=g)
    v_new = torch.randn((nq, Hkv * D), dtype=BF16, device="cuda", generator=g)
    return q, k_new, v_new


def _check_modes(tree, pool, Hq, Hkv, D, modes, tag, seed=0, q_scale=1.0):
    nq = len(tree.leaves)
    q, k_new, v_new = _randn_step(tree, pool, Hq, Hkv, D, nq, seed, q_scale)
    paths = product_leaf_paths(tree)
    for mode in modes:
        out = oracles.eager_step(tree, pool, mode, Hq, Hkv, D, q, k_new, v_new)
        assert out.dtype == BF16
        # (the step's rows are in the pool now: the truth reads them there)
        check_against_truth(out, q, pool.get_key_buffer(0), pool.get_value_buffer(0), paths, Hq, Hkv, D ** -0.5, f"{tag} {mode}")


@pytest.mark.parametrize("branch_len", [1, 50, 200, 230])
def test_north_star_tree_at_the_plan_rules_branch_lengths(branch_len):
    """32 / 32 / 128, 4096-token prefix x 32 branches at 1, 50, 200 and 230 tokens per branch: the 7-, 6- and 4-chunk prefix rules, leaf
    groups of three and of four (tests/test_plan_rules.py pins the shapes)."""
    w = Workload(**{**WORKLOADS["northstar_4kx32"].__dict__, "branch_len": branch_len})
    tree, pool = build_tree(w, 1, "cuda", dtype=BF16)
    _check_modes(tree, pool, 32, 32, 128, ("flatten", "node", "seq"), f"northstar 4096x32x{branch_len}", seed=branch_len)


def test_seven_query_heads_per_kv_head():
    """Qwen2-7B's 28 / 4 / 128 on the north-star shape: G = 7, 224 virtual rows per tile."""
    tree, pool, _ = few_shot_tree(4096, 32, 200, 4, 128)
    _check_modes(tree, pool, 28, 4, 128, ("flatten", "node", "seq"), "28/4/128 4096x32x200", seed=7)


@pytest.mark.parametrize("name", ["medusa64_node", "medusa64_tree_flatten", "tot50_4k", "gqa_4kx32", "northstar_4kx32_d64"])
def test_workloads_built_in_bf16(name):
    w = WORKLOADS[name]
    Hq, Hkv, D, _ = GEOMETRY[w.model]
    tree, pool = build_tree(w, 1, "cuda", dtype=BF16)
    assert pool._storage.dtype == BF16
    _check_modes(tree, pool, Hq, Hkv, D, (w.mode, "seq"), name, seed=len(name))


@pytest.mark.parametrize("geom", [(4, 4, 64), (3, 3, 64), (4, 2, 32), (4, 4, 16)], ids=lambda g: "x".join(map(str, g)))
def test_small_head_dim_families(geom):
    """head_dim 64 as head pairs and as an odd pool (the tile-per-workgroup kernel), 32 and 16."""
    Hq, Hkv, D = geom
    tree, pool, _ = few_shot_tree(300, 5, 140, Hkv, D)
    _check_modes(tree, pool, Hq, Hkv, D, ("flatten", "node", "node_chunk", "seq"), "x".join(map(str, geom)), seed=D + Hq)


def test_scores_spread_eight_times():
    """q scaled 8x: scores of standard deviation 8 (|score| stays below ~40), a sharp softmax -- the bound's fp32 term at work."""
    tree, pool, _ = few_shot_tree(2000, 8, 150, 8, 128)
    _check_modes(tree, pool, 32, 8, 128, ("flatten", "node"), "32/8/128 2000x8x150 q x8", seed=3, q_scale=8.0)


def test_strided_q_rows():
    """q and the output as views of a wider buffer (token stride > Hq * D, as a fused qkv projection leaves them)."""
    Hq, Hkv, D = 32, 8, 128
    tree, pool, _ = few_shot_tree(1500, 16, 100, Hkv, D)
    nq = len(tree.leaves)
    g = torch.Generator(device="cuda").manual_seed(11)
    pool._storage.normal_(generator=g)
    wide = torch.randn((nq, Hq + 2 * Hkv, D), dtype=BF16, device="cuda", generator=g)
    q = wide[:, :Hq]
    assert q.stride(0) == (Hq + 2 * Hkv) * D
    outs, _ = oracles.operators(tree, pool, q)
    paths = product_leaf_paths(tree)
    for mode, out in outs.items():
        check_against_truth(out.contiguous(), q.contiguous(), pool.get_key_buffer(0), pool.get_value_buffer(0), paths, Hq, Hkv,
                            D ** -0.5, f"strided q {mode}")


def test_forest_of_eight_trees():
    """Eight independent trees in one pool, one operator call over all of them (Llama-3-8B heads; 2k-token prefixes keep it quick)."""
    w = Workload("forest", "llama3-8b", "flatten", "few_shot", 2048, 8, 64, 8)
    Hq, Hkv, D, _ = GEOMETRY[w.model]
    forest, pool = build_forest(w, 8, 1, "cuda", dtype=BF16)
    assert isinstance(forest, deft_amd.Forest) and pool._storage.dtype == BF16
    nq = sum(len(t.leaves) for t in forest.trees)
    q, k_new, v_new = _randn_step(forest, pool, Hq, Hkv, D, nq, 5)
    paths = [p for t in forest.trees for p in product_leaf_paths(t)]
    for mode in ("flatten", "node"):
        out = oracles.eager_step(forest, pool, mode, Hq, Hkv, D, q, k_new, v_new)
        check_against_truth(out, q, pool.get_key_buffer(0), pool.get_value_buffer(0), paths, Hq, Hkv, D ** -0.5, f"forest 8 x 2048x8x64 {mode}")
