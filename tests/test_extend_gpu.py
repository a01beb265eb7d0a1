"""Extend steps on the GPU: the block arrays `TreeMetadata.for_extend` builds against the numpy model (tests/extend_model.py) with
no attention involved, then `DeFTAttention.forward(ForwardMode.EXTEND)` on exact-visibility inputs, random data against fp64 truth,
the fused append on a poisoned pool, and one extend call against the decode steps it replaces.

The tree of the array / visibility cases: a 200-token root (two blocks, the second partial), leaves with 5 / 130 / 0 / 3 private
tokens, the last one left out of every step."""
import numpy as np
import pytest
import torch

import bf16_util
import deft_amd
import extend_model as em
import oracles
from truth import max_err, tree_truth

pytestmark = pytest.mark.gpu

PRIVATE = (5, 130, 0, 3)
DRAFT = em.draft_tree_parents([1, 2, 4])


def _mk(Hkv, D, width, private, dtype=torch.float16, prefix=200, extra=1100):
    size = prefix + sum(private) + extra
    req = deft_amd.ReqToTokenPool(max(width, 8) + 8, prefix + max(private, default=0) + 1100, device="cuda")
    pool = deft_amd.TokenToKVPool(size, dtype, Hkv, D, 1, device="cuda")
    tree = deft_amd.TreeCache(dtype, Hkv, D, 1, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, prefix + 1, dtype=torch.int32))
    kids = tree.branch(tree.root, width)
    for kid, n in zip(kids, private):
        if n:
            tree.extend_leaf(kid, torch.arange(n, dtype=torch.int32))
    return tree, kids, pool


# name -> (leaves of the 4-leaf tree, tokens per leaf, local parents per leaf or None = chain)
STEPS = {
    "chain_1_7_33": ((0, 1, 2), (1, 7, 33), None),   # 41 rows: the root's blocks in two chunks; 33 crosses a 32-row piece
    "chain_33_1_7": ((0, 1, 2), (33, 1, 7), None),
    "chain_7_33_1": ((0, 1, 2), (7, 33, 1), None),
    "chain_1": ((1,), (1,), None),
    "draft_1_2_4": ((0, 2), (7, 7), DRAFT),
}


def _step(tree, kids, name):
    leaves, counts, local = STEPS[name]
    toks = {kids[i]: list(range(n)) for i, n in zip(leaves, counts)}
    parents = None if local is None else {kids[i]: local for i in leaves}
    return tree.alloc_extend(toks, parents)


def _built(md):
    """The arrays on the host; the device's own error flags and counts agree with what the host sized."""
    arr = em.md_arrays(md)
    dims = md._ext_dims.cpu().tolist()
    assert dims[4] == 0, f"device error flags {dims[4]}"
    assert dims[0] == len(arr["block_q_cnts"]) and dims[1] == len(arr["block_q"]), (dims[:4], md._ext_sizes)
    return arr


@pytest.mark.parametrize("name", list(STEPS))
def test_arrays_are_what_the_semantics_say(name):
    tree, kids, pool = _mk(2, 64, 4, PRIVATE)
    step = _step(tree, kids, name)
    md = deft_amd.TreeMetadata.for_extend(tree, step)
    assert md.query_num == step.num_rows and md.node_q.numel() == 0 and md.node_kv.numel() == 0
    arr = _built(md)
    em.check_invariants(arr, step.num_rows)
    em.check_against_model(arr, em.key_sets(tree, step))
    # the tree itself is untouched, and an ordinary decode step still builds on the same device copy
    assert [len(k.kv_indices) for k in kids] == list(PRIVATE)
    if name == "chain_1_7_33":
        assert len(arr["block_q_cnts"]) == 8 and len(arr["block_q"]) == 130  # (tests/test_extend_host.py derives these)
        assert em.new_key_blocks(arr, step.slots) == 3


@pytest.mark.parametrize("width,per_leaf,blocks", [(32, 1, 1), (24, 4, 3), (40, 1, 2)])
def test_small_pieces_pack_into_few_new_key_blocks(width, per_leaf, blocks):
    """32 leaves x 1 token: ONE new-key block, not 32 tiles; 24 leaves x 4 chain tokens: three.  40 leaves: the tree's own blocks
    already come in two chunks of leaves."""
    tree, kids, pool = _mk(2, 64, width, ())
    step = tree.alloc_extend({k: list(range(per_leaf)) for k in kids})
    md = deft_amd.TreeMetadata.for_extend(tree, step)
    arr = _built(md)
    em.check_invariants(arr, step.num_rows)
    em.check_against_model(arr, em.key_sets(tree, step))
    assert em.new_key_blocks(arr, step.slots) == blocks


def test_long_chain_and_deep_draft_tree():
    """One leaf, 300 chain tokens (pieces whose keys take up to three blocks), next to a leaf with a 2-ary draft tree of 63 tokens
    whose second piece sees keys of the first."""
    tree, kids, pool = _mk(2, 64, 3, (5, 130, 0))
    step = tree.alloc_extend({kids[0]: range(300), kids[2]: range(63)},
                             parents={kids[2]: em.draft_tree_parents([1, 2, 4, 8, 16, 32])})
    md = deft_amd.TreeMetadata.for_extend(tree, step)
    arr = _built(md)
    em.check_invariants(arr, step.num_rows)
    em.check_against_model(arr, em.key_sets(tree, step))


def test_decode_builds_on_the_device_copy_an_extend_step_uploaded():
    """An extend step that opens an epoch uploads the tree WITHOUT the decode output buffers (it takes trees a decode step
    refuses).  Whoever syncs next and wants them -- `from_tree_cache`, a DecodeSession's `dt.sync()` -- finds them sized, on the
    same upload; `_upload` / `apply_journal` keep taking no argument (tests count uploads by wrapping them)."""
    from deft_amd import tree_cache as tcm

    tree, kids, pool = _mk(2, 64, 3, (5, 130, 2))
    uploads, orig = 0, tcm._DeviceTree._upload

    def counting(self):
        nonlocal uploads
        uploads += 1
        return orig(self)

    tcm._DeviceTree._upload = counting
    try:
        step = tree.alloc_extend({kids[0]: [1, 2, 3]})
        _built(deft_amd.TreeMetadata.for_extend(tree, step))
        dt = tree._device_tree
        assert uploads == 1 and dt.out is None
        assert dt.sync() is False and dt.out is not None and set(dt.cap_lens) >= {"block_q", "block_kv"}  # (what a session reads)
        tree.commit_extend(step)  # journalled: the copy stays inside its epoch
        dev = deft_amd.TreeMetadata.from_tree_cache(tree, device_build=True, copy=True)
        host = deft_amd.TreeMetadata.from_tree_cache(tree, device_build=False)
        torch.cuda.synchronize()
        for f in ("node_q", "node_kv", "node_q_len", "node_kv_len", "block_q", "block_q_cnts", "block_q_offset", "block_bitmasks",
                  "block_kv", "block_lens"):
            assert torch.equal(getattr(dev, f).cpu(), getattr(host, f).cpu()), f
        assert uploads == 1 and dt.dims()[9] == 0
    finally:
        tcm._DeviceTree._upload = orig


def test_node_operator_refuses_extend_metadata():
    tree, kids, pool = _mk(2, 64, 4, PRIVATE)
    step = _step(tree, kids, "chain_1")
    deft_amd.register_tree_metadata(deft_amd.TreeMetadata.for_extend(tree, step))
    try:
        attn = deft_amd.DeFTAttention(4, 64, 64 ** -0.5, 2, 0)
        meta = deft_amd.InputMetadata(deft_amd.ForwardMode.TREE_DECODE_NODE, step.updater(pool), pool)
        x = torch.zeros((1, 4 * 64), dtype=torch.float16, device="cuda")
        with pytest.raises(deft_amd.DeftLibraryError, match="extend step"):
            attn(x, x[:, :128], x[:, :128], meta)
    finally:
        deft_amd.unregister_tree_metadata()


WIDE = {"pack_24x4": (24, 4), "pack_32x1": (32, 1), "rows_33x5": (33, 5)}  # name -> (leaves, chain tokens per leaf)


def _forward(tree, pool, step, q, k_new, v_new, Hq, Hkv, D, **kw):
    md = deft_amd.TreeMetadata.for_extend(tree, step)
    deft_amd.register_tree_metadata(md)
    try:
        meta = deft_amd.InputMetadata(deft_amd.ForwardMode.EXTEND, step.updater(pool), pool)
        out = deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, 0)(q, k_new, v_new, meta, **kw)
        torch.cuda.synchronize()
        assert md._ext_dims.cpu().tolist()[4] == 0
        return out
    finally:
        deft_amd.unregister_tree_metadata()


@pytest.mark.parametrize("geom", [(4, 4, 128), (8, 2, 128), (4, 2, 64)], ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("name", ["chain_1_7_33", "chain_7_33_1", "draft_1_2_4", "pack_24x4", "pack_32x1", "rows_33x5"])
def test_every_row_sees_exactly_its_keys(name, geom):
    """K = 0 everywhere (pool and k_new), dyadic V: row t's output is the fp64 mean of V over its key set, to one fp16 ulp + 2^-20
    (oracles.tolerance).  An off-by-one in causality or a doubled key moves it by >= 4 x that (the power check).
    pack_32x1: 32 leaves x 1 token, all new keys in ONE block; rows_33x5: 165 rows on 33 leaves -- more leaves than a query list
    holds, more rows than one 128-row pass of the plan."""
    Hq, Hkv, D = geom
    if name in WIDE:
        width, per_leaf = WIDE[name]
        tree, kids, pool = _mk(Hkv, D, width, ())
        step = tree.alloc_extend({k: list(range(per_leaf)) for k in kids})
    else:
        tree, kids, pool = _mk(Hkv, D, 4, PRIVATE)
        step = _step(tree, kids, name)
    R = step.num_rows
    g = torch.Generator(device="cuda").manual_seed(Hq * D + R)
    oracles.visibility_pool(pool, g)
    q = oracles.dyadic_(torch.empty((R, Hq * D), dtype=torch.float16, device="cuda"), g)
    k_new = torch.zeros((R, Hkv * D), dtype=torch.float16, device="cuda")
    v_new = oracles.dyadic_(torch.empty((R, Hkv * D), dtype=torch.float16, device="cuda"), g)
    out = _forward(tree, pool, step, q, k_new, v_new, Hq, Hkv, D)
    vb = pool.get_value_buffer(0)
    assert torch.equal(vb[step.cache_loc.long()].reshape(R, -1), v_new)
    keys = em.key_sets(tree, step)
    oracles.power_check(vb, keys, (0, R - 1))
    expected = oracles.per_query_head(oracles.visible_mean(vb, keys), Hq, Hkv)
    res = oracles.assert_visible_mean(out, expected, (name, geom))
    print(f"[extend visibility] {name} {geom}: {res}")


def test_random_data_against_fp64_truth():
    """N(0,1) q / K / V, fp16, against tests/truth.py at the tolerance the fp16 truth tests use (5e-4: fp64 truth, fp32 folds, fp16
    output)."""
    Hq, Hkv, D = 8, 2, 128
    tree, kids, pool = _mk(Hkv, D, 4, PRIVATE)
    step = _step(tree, kids, "chain_1_7_33")
    R = step.num_rows
    g = torch.Generator(device="cuda").manual_seed(11)
    pool._storage.copy_(torch.randn(pool._storage.shape, dtype=torch.float32, device="cuda", generator=g))
    q, k_new, v_new = (torch.randn((R, h * D), dtype=torch.float32, device="cuda", generator=g).half() for h in (Hq, Hkv, Hkv))
    out = _forward(tree, pool, step, q, k_new, v_new, Hq, Hkv, D)
    truth = tree_truth(q, pool.get_key_buffer(0), pool.get_value_buffer(0), em.key_sets(tree, step), Hq, Hkv, D ** -0.5)
    err = max_err(out, truth)
    print(f"[extend truth fp16] max err {err:.3e}")
    assert err < 5e-4


def test_random_data_bf16_within_the_per_element_bound():
    Hq, Hkv, D = 8, 2, 128
    tree, kids, pool = _mk(Hkv, D, 4, PRIVATE, dtype=torch.bfloat16)
    step = _step(tree, kids, "draft_1_2_4")
    R = step.num_rows
    g = torch.Generator(device="cuda").manual_seed(12)
    pool._storage.copy_(torch.randn(pool._storage.shape, dtype=torch.float32, device="cuda", generator=g))
    q, k_new, v_new = (torch.randn((R, h * D), dtype=torch.float32, device="cuda", generator=g).bfloat16() for h in (Hq, Hkv, Hkv))
    out = _forward(tree, pool, step, q, k_new, v_new, Hq, Hkv, D)
    bf16_util.check_against_truth(out, q, pool.get_key_buffer(0), pool.get_value_buffer(0), em.key_sets(tree, step), Hq, Hkv,
                                  D ** -0.5, "extend draft tree")


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_fused_append_writes_the_step_rows_and_nothing_else(kind):
    """Every pool row that is on no row's cached path -- the step's own slots among them, which the fused append must fill before
    anybody reads them -- is poisoned.  Afterwards: the rows at cache_loc are bit for bit what kv_append writes, no other byte of
    the pool moved, and the outputs are finite and equal to the run on a clean pool."""
    Hq, Hkv, D = 8, 2, 128
    tree, kids, pool = _mk(Hkv, D, 4, PRIVATE)
    step = _step(tree, kids, "chain_7_33_1")
    R = step.num_rows
    g = torch.Generator(device="cuda").manual_seed(5)
    pool._storage.copy_(torch.randn(pool._storage.shape, dtype=torch.float32, device="cuda", generator=g))
    q, k_new, v_new = (torch.randn((R, h * D), dtype=torch.float32, device="cuda", generator=g).half() for h in (Hq, Hkv, Hkv))
    clean = pool._storage.clone()
    ref = _forward(tree, pool, step, q, k_new, v_new, Hq, Hkv, D).clone()
    pool._storage.copy_(clean)
    cached = oracles.live_slots([tree.leaf_path_slots(tree.leaves[l]) for l in step.leaf_rows])
    assert not set(cached.tolist()) & set(step.slots.tolist())
    oracles.poison_pool(pool, cached, kind)
    before = pool._storage.clone()
    out = _forward(tree, pool, step, q, k_new, v_new, Hq, Hkv, D)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, ref)
    want = before.clone()
    deft_amd.kv_append(want[0], step.cache_loc, k_new, v_new)
    torch.cuda.synchronize()
    assert torch.equal(pool._storage.view(torch.int16), want.view(torch.int16))  # (bit patterns: NaN == NaN)
    loc = step.cache_loc.long()
    assert torch.equal(pool._storage[0, loc, 0].reshape(R, -1), k_new) and torch.equal(pool._storage[0, loc, 1].reshape(R, -1), v_new)


def test_rotary_embedding_runs_in_front_with_the_step_positions():
    """`forward(..., rotary_emb, positions)` in EXTEND mode = the rotation's own launch, then the extend call on rotated q / k."""
    Hq, Hkv, D = 4, 4, 128
    tree, kids, pool = _mk(Hkv, D, 4, PRIVATE)
    step = _step(tree, kids, "draft_1_2_4")
    R = step.num_rows
    g = torch.Generator(device="cuda").manual_seed(6)
    pool._storage.copy_(torch.randn(pool._storage.shape, dtype=torch.float32, device="cuda", generator=g))
    q, k_new, v_new = (torch.randn((R, h * D), dtype=torch.float32, device="cuda", generator=g).half() for h in (Hq, Hkv, Hkv))
    clean = pool._storage.clone()
    rope = deft_amd.get_rope(D, D, 4096, 10000.0)
    pos = torch.from_numpy(step.positions).cuda()
    q1, k1 = q.clone(), k_new.clone()
    out = _forward(tree, pool, step, q1, k1, v_new, Hq, Hkv, D, rotary_emb=rope, positions=pos).clone()
    pool_rot = pool._storage.clone()
    pool._storage.copy_(clean)
    q2, k2 = q.clone(), k_new.clone()
    rot = rope(pos, q2, k2)
    q2, k2 = rot if rot is not None else (q2, k2)
    ref = _forward(tree, pool, step, q2, k2, v_new, Hq, Hkv, D)
    assert not torch.equal(k2, k_new) and torch.equal(out, ref) and torch.equal(pool._storage, pool_rot)


def test_one_extend_equals_the_decode_steps_it_replaces():
    """A 5-token chain on three leaves: one extend call against five ordinary decode steps fed the same per-token q / k / v.  The
    decode tree's allocator is steered (free slots masked while it allocates) to the slot numbering the extend step got, so the
    two pools can be compared bit for bit.  Outputs: the same keys folded in another partition -- tests/test_session.py's bound
    between two partitions, 1e-3 + one fp16 step of the value."""
    Hq, Hkv, D, n = 8, 2, 128, 5
    g = torch.Generator(device="cuda").manual_seed(21)
    trees = [_mk(Hkv, D, 3, (5, 130, 0), extra=64) for _ in range(3)]
    init = torch.randn(trees[0][2]._storage.shape, dtype=torch.float32, device="cuda", generator=g).half()
    for _, _, pool in trees:
        pool._storage.copy_(init)
    (ta, ka, pa), (tb, kb, pb), (tc, kc, pc) = trees
    R = 3 * n
    q, k_new, v_new = (torch.randn((R, h * D), dtype=torch.float32, device="cuda", generator=g).half() for h in (Hq, Hkv, Hkv))
    # ---- one extend call
    step = ta.alloc_extend({k: list(range(50, 50 + n)) for k in ka})
    out_ext = _forward(ta, pa, step, q, k_new, v_new, Hq, Hkv, D).clone()
    ta.commit_extend(step)
    # ---- five decode steps
    s0 = int(step.slots[0])
    assert step.slots.tolist() == list(range(s0, s0 + R)) and pb.used_size() == s0
    attn = deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, 0)
    outs = []
    for i in range(n):
        rows = [l * n + i for l in range(3)]  # token i of every leaf
        hold = np.setdiff1d(np.arange(s0, s0 + R), [s0 + r for r in rows])
        hold = hold[pb.mem_state[hold] == 0]
        pb.mem_state[hold] = 1  # (only this step's three slots are free below s0 + R)
        for leaf, r in zip(kb, rows):
            leaf.append_token(50 + i)
        upd = tb.alloc()
        pb.mem_state[hold] = 0
        pb._lo = min(pb._lo, s0)
        assert upd.cache_loc.tolist() == [s0 + r for r in rows]
        deft_amd.register_tree_metadata(deft_amd.TreeMetadata.from_tree_cache(tb))
        meta = deft_amd.InputMetadata(deft_amd.ForwardMode.TREE_DECODE_FLATTEN, upd, pb)
        outs.append(attn(q[rows], k_new[rows], v_new[rows], meta).clone())
        deft_amd.unregister_tree_metadata()
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        ref = o.float()
        got = out_ext[[l * n + i for l in range(3)]].float()
        err = (got - ref).abs()
        assert bool((err <= 1e-3 + ref.abs() * 2.0 ** -10).all()), (i, float(err.max()))
    assert torch.equal(pa._storage, pb._storage)
    # ---- the committed tree is the tree extend_leaf builds
    for leaf in kc:
        tc.extend_leaf(leaf, list(range(50, 50 + n)))
    ma, mc = deft_amd.TreeMetadata.from_tree_cache(ta, copy=True), deft_amd.TreeMetadata.from_tree_cache(tc, copy=True)
    assert (ma.query_num, ma.node_num, ma.total_kv_len, ma.leaf_to_q) == (mc.query_num, mc.node_num, mc.total_kv_len, mc.leaf_to_q)
    for f in ("node_q", "node_kv", "node_q_len", "node_kv_len", "node_q_offset", "node_kv_offset", "block_q", "block_q_cnts",
              "block_q_offset", "block_bitmasks", "block_kv", "block_lens"):
        assert torch.equal(getattr(ma, f), getattr(mc, f)), f
    for a, c in zip(ka, kc):
        assert a.kv_indices.tolist() == c.kv_indices.tolist() and a.token_ids == c.token_ids and list(a.positions) == list(c.positions)
