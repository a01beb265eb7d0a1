"""Unused pool slots may hold NaN or Inf (csrc/deft_kernels.hip: the pool is torch.empty, as the reference's memory_pool.py makes it;
a runner may reserve slots).  Here the first slots of the pool are RESERVED before the tree is grown -- on no path, slot 0 among them --
and every row that is not on a live path is poisoned, K and V, every layer: with NaN, and with K = +Inf / V = -Inf.  A kernel that
reads a dead row -- even one whose probability is 0, since 0 x NaN = NaN in the P.V product and in the merge -- gives NaN.  What
must hold: outputs finite and BIT-IDENTICAL to the same run with those rows finite.

The window plans of DecodeSession(incremental=True) used to point every overflow position without a key at slot 0 (csrc/window.h);
these are the tests that saw it.  Poisoning is data only: no index of any table changes."""
import numpy as np
import pytest
import torch

import deft_amd
import oracles
from truth import product_leaf_paths

pytestmark = pytest.mark.gpu

RESERVE = 3
FAMILIES = [(4, 4, 128), (8, 2, 128), (4, 4, 64), (3, 3, 64), (4, 2, 32), (4, 4, 16)]  # MHA, GQA, D=64 pairs, odd Hkv, 32, 16


def _live(tree):
    return oracles.live_slots(product_leaf_paths(tree))


@pytest.mark.parametrize("geom", FAMILIES, ids=lambda g: "x".join(map(str, g)))
def test_eager_step_never_reads_a_dead_row(geom):
    """Flatten, Node, node_chunk and the sequential comparator (its page-table rows are zero beyond each leaf's length: slot 0,
    reserved and poisoned) at every kernel family; K = 0 and dyadic V, so the finite run is also held against the visible mean."""
    Hq, Hkv, D = geom
    tree, pool, reserved = oracles.few_shot_tree(300, 5, 140, Hkv, D, reserve=RESERVE)
    assert int(reserved[0]) == 0 and 0 not in set(_live(tree).tolist())
    g = torch.Generator(device="cuda").manual_seed(D + Hq)
    oracles.visibility_pool(pool, g)
    nq = len(tree.leaves)
    q = oracles.dyadic_(torch.empty((nq, Hq * D), dtype=torch.float16, device="cuda"), g)
    k_new = torch.zeros((nq, Hkv * D), dtype=torch.float16, device="cuda")
    v_new = oracles.dyadic_(torch.empty((nq, Hkv * D), dtype=torch.float16, device="cuda"), g)
    clean = pool._storage.clone()
    paths = product_leaf_paths(tree)
    live = oracles.live_slots(paths)
    oracles.power_check(pool.get_value_buffer(0), paths, (0, nq - 1))
    for mode in ("flatten", "node", "node_chunk", "seq"):
        pool._storage.copy_(clean)
        ref = oracles.eager_step(tree, pool, mode, Hq, Hkv, D, q, k_new, v_new).clone()
        expected = oracles.per_query_head(oracles.visible_mean(pool.get_value_buffer(0), paths), Hq, Hkv)
        oracles.assert_visible_mean(ref, expected, (geom, mode))
        for kind in ("nan", "inf"):
            pool._storage.copy_(clean)
            oracles.poison_pool(pool, live, kind)
            out = oracles.eager_step(tree, pool, mode, Hq, Hkv, D, q, k_new, v_new)
            assert bool(torch.isfinite(out).all()) and torch.equal(out, ref), (geom, mode, kind)


def test_prefill_never_reads_rows_beyond_the_batch():
    """context_attention_fwd over a ragged batch of T tokens whose q / k / v buffers hold more rows than T: the rows beyond are
    poisoned."""
    Hq, Hkv, D = 8, 2, 128
    lens = [255, 1, 257, 300]
    T, extra = sum(lens), 300
    g = torch.Generator(device="cuda").manual_seed(9)
    q, k, v = (oracles.dyadic_(torch.empty((T + extra, h, D), dtype=torch.float16, device="cuda"), g) for h in (Hq, Hkv, Hkv))
    start = torch.tensor(np.cumsum([0] + lens[:-1]), dtype=torch.int32, device="cuda")
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")

    def run():
        o = torch.full((T + extra, Hq, D), float("nan"), dtype=torch.float16, device="cuda")
        deft_amd.context_attention_fwd(q, k, v, o, start, ln, max(lens))
        torch.cuda.synchronize()
        return o[:T].clone()

    ref = run()
    for t in (q, k, v):
        t[T:] = float("nan")
    out = run()
    assert bool(torch.isfinite(out).all()) and torch.equal(out, ref)


def test_forest_step_never_reads_a_dead_row():
    """Three trees in one pool behind the reserved slots, decoded as ONE batch (deft_amd.Forest, as bench.py runs forest_8kx8),
    Flatten and Node: the dead rows -- reserved slots and the pool's tail -- poisoned."""
    from deft_amd.memory_pool import ReqToTokenPool, TokenToKVPool
    from deft_amd.utils.workloads import GEOMETRY, Workload, build_tree

    w = Workload("forest_poison", "llama3-8b", "flatten", "few_shot", 700, 5, 140)
    Hq, Hkv, D, _ = GEOMETRY[w.model]
    n_trees = 3
    req = ReqToTokenPool(n_trees * 72, 700 + 140 + 16, device="cuda")
    pool = TokenToKVPool(RESERVE + n_trees * (700 + 5 * 140) + 256, torch.float16, Hkv, D, 1, device="cuda")
    pool.alloc(RESERVE)
    forest = deft_amd.Forest([build_tree(w, 1, "cuda", pools=(req, pool))[0] for _ in range(n_trees)])
    paths = [p for t in forest.trees for p in product_leaf_paths(t)]
    live = oracles.live_slots(paths)
    assert 0 not in set(live.tolist())
    g = torch.Generator(device="cuda").manual_seed(3)
    oracles.visibility_pool(pool, g)
    nq = len(paths)
    q = oracles.dyadic_(torch.empty((nq, Hq * D), dtype=torch.float16, device="cuda"), g)
    k_new = torch.zeros((nq, Hkv * D), dtype=torch.float16, device="cuda")
    v_new = oracles.dyadic_(torch.empty((nq, Hkv * D), dtype=torch.float16, device="cuda"), g)
    clean = pool._storage.clone()
    for mode in ("flatten", "node"):
        pool._storage.copy_(clean)
        ref = oracles.eager_step(forest, pool, mode, Hq, Hkv, D, q, k_new, v_new).clone()
        expected = oracles.per_query_head(oracles.visible_mean(pool.get_value_buffer(0), paths), Hq, Hkv)
        oracles.assert_visible_mean(ref, expected, ("forest", mode))
        pool._storage.copy_(clean)
        oracles.poison_pool(pool, live)
        out = oracles.eager_step(forest, pool, mode, Hq, Hkv, D, q, k_new, v_new)
        assert bool(torch.isfinite(out).all()) and torch.equal(out, ref), mode


def _session_run(mode, Hq, Hkv, poison, speculative, steps, seed):
    """A window-plan session over a tree grown behind RESERVE reserved slots; `poison`: before every step every row off the live
    paths -- the reserved slots, the pool's unused tail, the slots the last step's resets freed -- is NaN.  Returns the outputs of
    every step and the step kinds."""
    D, layers, prefix, width = 128, 2, 300, (12 if speculative else 6)
    tree, pool, reserved = oracles.few_shot_tree(prefix, width, 0, Hkv, D, layers=layers, reserve=RESERVE, extra=steps * width + 512)
    g = torch.Generator(device="cuda").manual_seed(seed)
    oracles.dyadic_(pool._storage, g)
    q = oracles.dyadic_(torch.empty((layers, width, Hq * D), dtype=torch.float16, device="cuda"), g)
    k = oracles.dyadic_(torch.empty((layers, width, Hkv * D), dtype=torch.float16, device="cuda"), g)
    v = oracles.dyadic_(torch.empty((layers, width, Hkv * D), dtype=torch.float16, device="cuda"), g)
    sess = deft_amd.DecodeSession(tree, Hq, Hkv, D, layers, lambda l: (q[l], k[l], v[l]), mode=mode, incremental=True)
    rng = np.random.default_rng(seed)
    outs = []
    for s in range(steps):
        for leaf in tree.leaves.values():
            leaf.append_token(7)
        for t in (q, k, v):  # (fresh rows every step, the same in both runs)
            oracles.dyadic_(t, g)
        if poison:
            oracles.poison_pool(pool, _live(tree))
        out = sess.step()
        torch.cuda.synchronize()
        outs.append([o.clone() for o in out])
        if speculative:  # accept 1-4 leaves' tokens into the root, reset every leaf (test_session's speculative loop)
            accept = int(rng.integers(1, 5))
            lv = sorted(tree.leaves.values(), key=lambda n: n.id)
            before = len(tree.root.kv_indices)
            for lf in lv[:accept]:
                tree.merge_nodes(tree.root, lf, pruneB_flag=False)
            tree.reset_nodes_KV(lv, len(tree.root.kv_indices) - before)
    assert sess.device_errors() == 0
    return outs, dict(sess.step_kinds)


@pytest.mark.parametrize("speculative", [False, True], ids=["replans", "speculative"])
@pytest.mark.parametrize("heads", [(8, 2), (28, 4)], ids=["gqa", "g7"])
@pytest.mark.parametrize("mode", ["flatten", "node"])
def test_window_session_never_reads_a_dead_row(mode, heads, speculative):
    """Window steps through replans (6 leaves: a 128-slot overflow tile lasts ~21 steps) and through speculative-decoding resets (the
    cleared positions of a reset leaf), G = 4 and the straddling G = 7: against the same run over a finite pool, bit for bit."""
    Hq, Hkv = heads
    steps = 40 if speculative else 60
    ref, kinds = _session_run(mode, Hq, Hkv, False, speculative, steps, 5)
    out, kinds_p = _session_run(mode, Hq, Hkv, True, speculative, steps, 5)
    assert kinds == kinds_p and kinds["legacy"] == 0 and kinds["patch"] >= steps // 2, kinds
    if not speculative:
        assert kinds["replan"] >= 2, kinds
    for s, (a, b) in enumerate(zip(ref, out)):
        for l, (x, y) in enumerate(zip(a, b)):
            assert bool(torch.isfinite(y).all()), (s, l, kinds, "non-finite output of a poisoned run")
            assert torch.equal(x, y), (s, l)
