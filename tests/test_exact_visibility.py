"""Exact visibility at full size (tests/oracles.py): K = 0 everywhere, dyadic V, so every visible key has probability 1 exactly and
each query's output is the fp64 MEAN of V over the exact multiset of keys on its path -- held per query, head and dim to one fp16 ulp
plus 2^-20.  At these sizes one dropped, doubled or foreign key moves some output by >= 4 x that (each test runs the power check on its
own data first); with N(0,1) logits and 5e-4 it moves it by far less than the tolerance.

Covered: every workload bench.py times, through bench.Bench itself -- the frozen, fused-append, graph-captured step that is timed --
plus the north-star tree at the branch lengths where the plan rules switch, the small head dims, prefill, and window-plan sessions
through replans, speculative resets and a straddling GQA group.  These inputs are for correctness only: no timing is taken from them."""
import os
import sys

import numpy as np
import pytest
import torch

import deft_amd
import oracles
from deft_amd.utils.workloads import GEOMETRY, WORKLOADS, Workload, build_tree
from truth import product_leaf_paths

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

# the headline, its two branch-length variants and every `other_workloads` entry of bench.py, and the two long prefixes
BENCH_WORKLOADS = ["northstar_4kx32", "northstar_4kx32@1", "northstar_4kx32@400", "fewshot_1kx32", "medusa64_node",
                   "medusa64_tree_node", "medusa64_tree_flatten", "tot50_4k", "gqa_4kx32", "forest_8kx8_single",
                   "northstar_4kx32_node", "northstar_4kx32_node_chunk", "northstar_4kx32_seq", "fewshot_1kx32_seq",
                   "northstar_4kx32_d64", "fewshot_16kx32", "fewshot_64kx8_gqa", "forest_8kx8"]
WORST = {}  # test id -> residual of the run (printed with -s; the largest against the tolerance is what the floor must cover)


def _note(tag, res):
    WORST[tag] = res
    print(f"[visibility] {tag}: max_err {res['max_err']:.3e}  err/tol {res['ratio']:.3f}  beyond one ulp {res['over_ulp']:.3e}")


def _workload(name):
    if "@" in name:
        base, bl = name.split("@")
        return Workload(**{**WORKLOADS[base].__dict__, "branch_len": int(bl)})
    return WORKLOADS[name]


@pytest.mark.parametrize("name", BENCH_WORKLOADS)
def test_bench_workload_sees_exactly_its_keys(name):
    w = _workload(name)
    saved = dict(deft_amd.BLOCK_CONFIG)
    try:
        b = bench.Bench(w, 2, torch.device("cuda"), seed=1)
        g = torch.Generator(device="cuda").manual_seed(len(name))
        oracles.visibility_pool(b.pool, g)
        b.k_new.zero_()
        oracles.dyadic_(b.v_new, g)
        b.prepare(use_graph=True)
        assert b.graph is not None, "the step was not captured"
        b.step()  # one more replay of the captured step
        torch.cuda.synchronize()
        paths = [p for t in b.forest.trees for p in product_leaf_paths(t)]
        assert len(paths) == b.nq
        loc = b.loc.long()
        for l in range(b.layers):
            vb = b.pool.get_value_buffer(l)
            assert torch.equal(vb[loc].reshape(b.nq, -1), b.v_new[l])  # (the fused append wrote the step's rows)
            if l == 0:
                oracles.power_check(vb, paths, (0, b.nq - 1))
            expected = oracles.per_query_head(oracles.visible_mean(vb, paths), b.Hq, b.Hkv)
            _note(f"{name} layer {l}", oracles.assert_visible_mean(b.outs[l], expected, (name, l)))
    finally:
        deft_amd.BLOCK_CONFIG.clear()
        deft_amd.BLOCK_CONFIG.update(saved)
        b = None
        torch.cuda.empty_cache()


def _check_operators(tree, pool, Hq, Hkv, D, tag, seed, antithetic=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    oracles.visibility_pool(pool, g)
    paths = product_leaf_paths(tree)
    nq = len(paths)
    vb = pool.get_value_buffer(0)
    if antithetic:
        oracles.antithetic_(vb, paths)
    factor = oracles.power_check(vb, paths, (0, nq - 1))
    q = oracles.dyadic_(torch.empty((nq, Hq, D), dtype=torch.float16, device="cuda"), g)
    expected = oracles.per_query_head(oracles.visible_mean(vb, paths), Hq, Hkv)
    outs, md = oracles.operators(tree, pool, q)
    for mode, out in outs.items():
        _note(f"{tag} {mode} (one key = {factor:.1f} x tolerance)", oracles.assert_visible_mean(out, expected, (tag, mode)))
    return md


@pytest.mark.parametrize("branch_len", [1, 3, 50, 200, 230, 254, 278])
def test_north_star_operators_at_the_plan_rule_edges(branch_len):
    """Prefix chunk counts (7 / 6 / 4), leaf groups of three and four, both edges of the fours band: Flatten and Node."""
    w = Workload(**{**WORKLOADS["northstar_4kx32"].__dict__, "branch_len": branch_len})
    tree, pool = build_tree(w, 1, "cuda")
    _check_operators(tree, pool, 32, 32, 128, f"north-star @{branch_len}", branch_len)


@pytest.mark.parametrize("geom", [(32, 32, 64), (6, 3, 64), (8, 2, 32), (4, 4, 16), (28, 4, 128)], ids=lambda g: "x".join(map(str, g)))
def test_head_dims_and_groups_see_exactly_their_keys(geom):
    """D = 64 head pairs and odd Hkv, D = 32, D = 16, and a group of seven query heads, on a 2k-prefix tree of 16 two-tile branches."""
    Hq, Hkv, D = geom
    tree, pool, _ = oracles.few_shot_tree(2048, 16, 200, Hkv, D)
    _check_operators(tree, pool, Hq, Hkv, D, f"heads {geom}", Hq * D)


@pytest.mark.parametrize("shape", [(4, 2, 100_000, 48), (2, 1, 450_000, 3)], ids=["100kx48", "450kx3"])
def test_merge_pass_shapes_see_exactly_their_keys(shape):
    """test_gpu_parity's merge-pass shapes: a 100k-token prefix under 48 branches (~37k Flatten partial rows: several passes of the
    merge's LDS row list, and more than the per-query row lists hold, so the merge scans) and a 450k-token prefix under 3 (3516 Flatten
    blocks, past the unit kernel's LDS tables).  At 450k keys one key moves a mean of size ~1/sqrt(N) by less than 4 of its fp16 ulps:
    the V rows pair up as +x / -x along the path, so the means sit near 0 where the grid is fine."""
    Hq, Hkv, prefix, width = shape
    tree, pool, _ = oracles.few_shot_tree(prefix, width, 3, Hkv, 128)
    md = _check_operators(tree, pool, Hq, Hkv, 128, f"merge passes {shape}", prefix, antithetic=prefix > 250_000)
    if width == 48:
        assert md.block_q.shape[0] > 15 * 1024  # (Flatten partial rows beyond QROWS_MAX: the merge scans row_q)
    else:
        assert md.block_q_cnts.shape[0] > 3500


@pytest.mark.parametrize("shape", [(8, 4, 1500, 40, 130), (4, 4, 700, 70, 20)], ids=["40q", "70q"])
def test_nodes_of_more_than_32_queries_see_exactly_their_keys(shape):
    """A prefix node shared by 40 / 70 leaves: Node cuts it into entries of at most 32 queries, Flatten into alternating blocks."""
    Hq, Hkv, prefix, width, bl = shape
    tree, pool, _ = oracles.few_shot_tree(prefix, width, bl, Hkv, 128)
    _check_operators(tree, pool, Hq, Hkv, 128, f"{width} queries", width)


@pytest.mark.parametrize("lens", [[255, 256, 257], [1, 2, 130, 700], [4096]], ids=["edges", "ragged", "4096"])
def test_prefill_rows_are_running_means(lens):
    """K = 0: prefill row i of a sequence is the mean of V[0 .. i]."""
    Hq, Hkv, D = 32, 8, 128
    T = sum(lens)
    g = torch.Generator(device="cuda").manual_seed(T)
    q = oracles.dyadic_(torch.empty((T, Hq, D), dtype=torch.float16, device="cuda"), g)
    k = torch.zeros((T, Hkv, D), dtype=torch.float16, device="cuda")
    v = oracles.dyadic_(torch.empty((T, Hkv, D), dtype=torch.float16, device="cuda"), g)
    start = np.cumsum([0] + lens[:-1])
    i = int(np.argmax(lens))  # (the longest sequence's last row: its path is the whole sequence)
    oracles.power_check(v, [list(range(int(start[i]), int(start[i]) + lens[i]))])
    o = torch.full((T, Hq, D), float("nan"), dtype=torch.float16, device="cuda")
    deft_amd.context_attention_fwd(q, k, v, o, torch.tensor(start, dtype=torch.int32, device="cuda"),
                                   torch.tensor(lens, dtype=torch.int32, device="cuda"), max(lens))
    torch.cuda.synchronize()
    exp = []
    for s0, n in zip(start, lens):
        c = v[s0 : s0 + n].to(torch.float64).reshape(n, -1).cumsum(0)
        exp.append(c / torch.arange(1, n + 1, dtype=torch.float64, device="cuda")[:, None])
    expected = oracles.per_query_head(torch.cat(exp), Hq, Hkv)
    _note(f"prefill {lens}", oracles.assert_visible_mean(o.reshape(T, -1), expected, lens))


def _session(tree, pool, Hq, Hkv, D, mode, steps, seed, speculative=False):
    """DecodeSession(incremental=True) on visibility inputs; every step against the visible mean over the pool after the step."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    oracles.visibility_pool(pool, g)
    nq = len(tree.leaves)
    q = oracles.dyadic_(torch.empty((1, nq, Hq * D), dtype=torch.float16, device="cuda"), g)
    k = torch.zeros((1, nq, Hkv * D), dtype=torch.float16, device="cuda")
    v = oracles.dyadic_(torch.empty((1, nq, Hkv * D), dtype=torch.float16, device="cuda"), g)
    sess = deft_amd.DecodeSession(tree, Hq, Hkv, D, 1, lambda l: (q[l], k[l], v[l]), mode=mode, incremental=True)
    rng = np.random.default_rng(seed)
    worst = None
    for s in range(steps):
        for leaf in tree.leaves.values():
            leaf.append_token(7)
        oracles.dyadic_(q, g)  # (fresh rows every step: a patch that points at another token of the same leaf changes the mean)
        oracles.dyadic_(v, g)
        out = sess.step()[0]
        torch.cuda.synchronize()
        paths = product_leaf_paths(tree)
        vb = pool.get_value_buffer(0)
        if s == 0:
            oracles.power_check(vb, paths, (0, nq - 1))
        res = oracles.assert_visible_mean(out, oracles.per_query_head(oracles.visible_mean(vb, paths), Hq, Hkv), (mode, s))
        worst = res if worst is None or res["ratio"] > worst["ratio"] else worst
        if speculative:
            accept = int(rng.integers(1, 5))
            lv = sorted(tree.leaves.values(), key=lambda n: n.id)
            before = len(tree.root.kv_indices)
            for lf in lv[:accept]:
                tree.merge_nodes(tree.root, lf, pruneB_flag=False)
            tree.reset_nodes_KV(lv, len(tree.root.kv_indices) - before)
    assert sess.device_errors() == 0 and sess.step_kinds["legacy"] == 0, sess.step_kinds
    return sess.step_kinds, worst


@pytest.mark.parametrize("mode", ["flatten", "node"])
def test_north_star_window_session_from_195_tokens(mode):
    """The north-star tree from 195 tokens per branch, 45 window steps (leaf groups of three, then four; replans on the way)."""
    w = Workload(**{**WORKLOADS["northstar_4kx32"].__dict__, "branch_len": 195})
    tree, pool = build_tree(w, 1, "cuda", extra_slots=32 * 45 + 256)
    kinds, worst = _session(tree, pool, 32, 32, 128, mode, 45, 195)
    assert kinds["replan"] >= 2 and kinds["patch"] >= 20, kinds
    _note(f"north-star session {mode}", worst)


def test_speculative_window_session():
    tree, pool, _ = oracles.few_shot_tree(1000, 24, 0, 8, 128, extra=24 * 40 + 512)
    kinds, worst = _session(tree, pool, 32, 8, 128, "flatten", 40, 24, speculative=True)
    assert kinds["patch"] >= 25, kinds
    _note("speculative session", worst)


def test_straddling_group_of_seven_window_session():
    tree, pool, _ = oracles.few_shot_tree(700, 12, 0, 4, 128, extra=12 * 60 + 512)
    kinds, worst = _session(tree, pool, 28, 4, 128, "node", 60, 7)
    assert kinds["replan"] >= 2 and kinds["patch"] >= 40, kinds
    _note("G=7 session", worst)
