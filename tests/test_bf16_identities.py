"""What holds bit for bit in fp16 holds bit for bit in bfloat16: the fused append, the fused rotary embedding, the module forward, a
legacy DecodeSession.  Then the exact cases on the bf16 grid (exact visibility, poisoned pools), a window-plan session, the rotary
embedding and the prefill against fp64.  Bounds and oracles: tests/bf16_util.py."""
import numpy as np
import pytest
import torch

import deft_amd
import oracles
from bf16_util import (BF16, assert_visible_mean_bf16, bf16_ulp, bound, check_against_truth, dyadic_bf16_, few_shot_tree, power_check_bf16,
                       report, visibility_pool_bf16)
from deft_amd.tree_attention import flatten_append_attention, node_append_attention
from truth import product_leaf_paths

pytestmark = pytest.mark.gpu


def _step_inputs(tree, pool, Hq, Hkv, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    pool._storage.normal_(generator=g)
    nq = len(tree.leaves)
    q = torch.randn((nq, Hq * D), dtype=BF16, device="cuda", generator=g)
    k_new = torch.randn((nq, Hkv * D), dtype=BF16, device="cuda", generator=g)
    v_new = torch.randn((nq, Hkv * D), dtype=BF16, device="cuda", generator=g)
    leaves = sorted(tree.leaves.values(), key=lambda n: n.id)
    loc = torch.tensor([lf.kv_indices[-1] for lf in leaves], dtype=torch.int32, device="cuda")
    return q, k_new, v_new, loc


# ---- bit-exact identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(32, 8, 128), (4, 4, 128), (4, 4, 64), (3, 3, 64), (4, 2, 32)], ids=lambda g: "x".join(map(str, g)))
def test_fused_append_equals_kv_append_then_attention_and_the_module_forward(geom):
    """deft_*_decode_append_bf16 == deft_kv_append_bf16 followed by deft_*_decode_bf16 -- outputs and pool bytes -- and
    DeFTAttention.forward gives what the operator call gives."""
    Hq, Hkv, D = geom
    tree, pool, _ = few_shot_tree(700, 6, 150, Hkv, D)
    q, k_new, v_new, loc = _step_inputs(tree, pool, Hq, Hkv, D, 17)
    start = pool._storage.clone()
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    q3 = q.view(-1, Hq, D)
    flat = (md.block_len, md.block_q, md.block_q_cnts, md.block_q_offset, md.block_bitmasks, md.block_kv, md.block_lens)
    node = (md.node_kv, md.node_kv_offset, md.node_kv_len, md.node_q, md.node_q_offset, md.node_q_len)
    for mode, two_calls, fused in (("flatten", deft_amd.tree_attention_subtree_fwd, flatten_append_attention),
                                   ("node", deft_amd.tree_attention_fwd, node_append_attention)):
        args = flat if mode == "flatten" else node
        pool._storage.copy_(start)
        deft_amd.kv_append(pool.kv_data[0], loc, k_new, v_new)
        o_two = torch.full_like(q3, float("nan"))
        two_calls(q3, pool.get_key_buffer(0), pool.get_value_buffer(0), o_two, *args)
        torch.cuda.synchronize()
        pool_two = pool._storage.clone()
        assert not torch.equal(pool_two, start)
        pool._storage.copy_(start)
        o_fused = torch.full_like(q3, float("nan"))
        fused(q3, pool.kv_data[0], o_fused, loc, k_new, v_new, *args)
        torch.cuda.synchronize()
        assert torch.equal(pool._storage, pool_two), (geom, mode)
        assert bool(torch.isfinite(o_fused).all()) and torch.equal(o_fused, o_two), (geom, mode)
        pool._storage.copy_(start)
        o_module = oracles.eager_step(tree, pool, mode, Hq, Hkv, D, q, k_new, v_new)
        assert o_module.dtype == BF16 and torch.equal(o_module.view(-1, Hq, D), o_fused), (geom, mode)
        assert torch.equal(pool._storage, pool_two), (geom, mode)


@pytest.mark.parametrize("mode", ["flatten", "node"])
@pytest.mark.parametrize("geom", [(8, 2, 128), (32, 32, 128)], ids=lambda g: "x".join(map(str, g)))
def test_fused_rope_equals_rope_then_fused_append(geom, mode):
    """deft_*_decode_rope_append_bf16 == deft_rope_qk_bf16 followed by deft_*_decode_append_bf16: outputs and pool bytes, q / k rows
    of a fused qkv projection; the fused form leaves them unrotated."""
    Hq, Hkv, D = geom
    outs, pools = [], []
    rope = deft_amd.get_rope(D, D, 4096, 10000.0, True)
    for fused in (False, True):
        tree, pool, _ = few_shot_tree(600, 7, 139, Hkv, D)
        for leaf in list(tree.leaves.values()):
            leaf.append_token(9)
        updater = tree.alloc()
        md = deft_amd.TreeMetadata.from_tree_cache(tree)
        nq = md.query_num
        g = torch.Generator(device="cuda").manual_seed(5)
        pool.kv_data[0].normal_(generator=g)
        qkv = torch.randn((nq, (Hq + 2 * Hkv) * D), dtype=BF16, device="cuda", generator=g)
        q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        positions = torch.tensor([len(tree.leaf_path_slots(lf)) - 1 + 37 * i for i, lf in
                                  enumerate(sorted(tree.leaves.values(), key=lambda n: n.id))], dtype=torch.int64, device="cuda")
        before = qkv.clone()
        attn = deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, layer_id=0)
        meta = deft_amd.InputMetadata(deft_amd.forward_mode_from_cli(mode), updater, pool)
        deft_amd.register_tree_metadata(md)
        try:
            if fused:
                o = attn(q, k, v, meta, rotary_emb=rope, positions=positions, fuse_rope=True)
                torch.cuda.synchronize()
                assert torch.equal(qkv, before)
            else:
                rope(positions, q, k)
                o = attn(q, k, v, meta)
                torch.cuda.synchronize()
                assert not torch.equal(qkv, before)
        finally:
            deft_amd.unregister_tree_metadata()
        assert o.dtype == BF16
        outs.append(o.clone())
        pools.append(pool.kv_data[0].clone())
    assert torch.equal(pools[0], pools[1])
    assert torch.equal(outs[0], outs[1])
    assert bool(torch.isfinite(outs[1]).all()) and float(outs[1].float().abs().max()) > 0


def _two_trees(Hkv, D, layers, prefix, width, size, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    kv_init = torch.randn((layers, size, 2, Hkv, D), dtype=BF16, device="cuda", generator=g)
    trees = []
    for _ in range(2):
        req = deft_amd.ReqToTokenPool(64, size, device="cuda")
        pool = deft_amd.TokenToKVPool(size, BF16, Hkv, D, layers, device="cuda")
        tree = deft_amd.TreeCache(BF16, Hkv, D, layers, req, pool, None, True, False)
        tree.init_prompt(torch.arange(1, prefix + 1, dtype=torch.int32))
        tree.branch(tree.root, width)
        pool._storage.copy_(kv_init)
        trees.append((tree, pool))
    return trees, g


def _session_run(mode, incremental, phases, Hq=8, Hkv=2, D=128, layers=2, prefix=700, width=6, size=4096, check=None):
    """Decode through `phases` = [steps, structural change or None, steps, ...] eagerly and through a DecodeSession; `check(s, l, out,
    ref, q_l, te, pe)` sees every step and layer."""
    (te, pe), (ts, ps) = _two_trees(Hkv, D, layers, prefix, width, size, 3)[0]
    g = torch.Generator(device="cuda").manual_seed(4)
    cap = 16
    q = torch.randn((layers, cap, Hq * D), dtype=BF16, device="cuda", generator=g)
    k = torch.randn((layers, cap, Hkv * D), dtype=BF16, device="cuda", generator=g)
    v = torch.randn((layers, cap, Hkv * D), dtype=BF16, device="cuda", generator=g)
    nq_now = [width]
    sess = deft_amd.DecodeSession(ts, Hq, Hkv, D, layers, lambda l: (q[l, : nq_now[0]], k[l, : nq_now[0]], v[l, : nq_now[0]]),
                                  mode=mode, incremental=incremental)
    assert sess.dtype == BF16 and all(o.dtype == BF16 for o in sess.out)
    attn = [deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, l) for l in range(layers)]
    fmode = deft_amd.forward_mode_from_cli(mode)
    s = 0
    for phase in phases:
        if callable(phase):
            for tree in (te, ts):
                phase(tree)
            continue
        for _ in range(phase):
            for tree in (te, ts):
                for leaf in tree.leaves.values():
                    leaf.append_token(7)
            upd = te.alloc()
            md = deft_amd.TreeMetadata.from_tree_cache(te)
            deft_amd.register_tree_metadata(md)
            n = md.query_num
            nq_now[0] = n
            ref = [attn[l](q[l, :n], k[l, :n], v[l, :n], deft_amd.InputMetadata(fmode, upd, pe)) for l in range(layers)]
            out = sess.step()
            torch.cuda.synchronize()
            for l in range(layers):
                check(s, l, out[l][:n], ref[l], q[l, :n], te, pe)
            assert torch.equal(pe._storage, ps._storage)
            assert torch.equal(te.req_to_token_pool.req_to_token, ts.req_to_token_pool.req_to_token)
            s += 1
    deft_amd.unregister_tree_metadata()
    assert sess.device_errors() == 0
    return sess


@pytest.mark.parametrize("mode", ["flatten", "node"])
def test_legacy_session_equals_the_eager_path_bit_for_bit(mode):
    """30 steps of a captured legacy session (incremental=False) through one cut and one branch."""
    def cut(tree):
        tree.cut(sorted(tree.leaves.values(), key=lambda n: n.id)[1])

    def branch(tree):
        tree.branch(sorted(tree.leaves.values(), key=lambda n: n.id)[0], 3)

    def check(s, l, out, ref, q_l, te, pe):
        assert out.dtype == BF16 and torch.equal(out, ref), (s, l)

    sess = _session_run(mode, False, [10, cut, 10, branch, 10], check=check)
    kinds = sess.step_kinds  # (an epoch's first step uploads the tree; three epochs, their graphs replayed)
    assert kinds["legacy"] + kinds["upload"] == 30 and kinds["patch"] == kinds["replan"] == 0 and sess.captures >= 2, (kinds, sess.captures)


@pytest.mark.parametrize("mode", ["flatten", "node"])
def test_window_plan_session_against_truth_through_replans(mode):
    """incremental=True: most steps patch the plan; the session and the eager path are each held to the bound against fp64 truth."""
    Hq, Hkv, D = 8, 2, 128

    def check(s, l, out, ref, q_l, te, pe):
        paths = product_leaf_paths(te)
        for side, t in (("session", out), ("eager", ref)):
            check_against_truth(t, q_l, pe.get_key_buffer(l), pe.get_value_buffer(l), paths, Hq, Hkv, D ** -0.5,
                                f"window {mode} step {s} layer {l} {side}")

    sess = _session_run(mode, True, [48], check=check)
    kinds = sess.step_kinds
    assert kinds["replan"] >= 2 and kinds["patch"] >= 30 and kinds["legacy"] == 0, kinds


def test_session_and_module_refuse_a_q_that_is_not_of_the_pool_s_type():
    """A bf16 pool under fp16 q / k / v (and the other way round): TypeError from DecodeSession and from DeFTAttention, nothing runs."""
    Hq, Hkv, D = 8, 2, 128
    for pool_dtype, other in ((BF16, torch.float16), (torch.float16, BF16)):
        tree, pool, _ = few_shot_tree(300, 4, 10, Hkv, D, dtype=pool_dtype)
        g = torch.Generator(device="cuda").manual_seed(1)
        pool._storage.normal_(generator=g)
        before = pool._storage.clone()
        q, k, v = (torch.randn((4, h * D), dtype=other, device="cuda", generator=g) for h in (Hq, Hkv, Hkv))
        with pytest.raises(TypeError):
            oracles.eager_step(tree, pool, "flatten", Hq, Hkv, D, q, k, v)
        with pytest.raises(TypeError):  # q of the pool's type, new rows not
            oracles.eager_step(tree, pool, "node", Hq, Hkv, D, q.to(pool_dtype), k, v)
        sess = deft_amd.DecodeSession(tree, Hq, Hkv, D, 1, lambda l: (q, k, v), mode="flatten", incremental=False)
        assert sess.dtype == pool_dtype
        for leaf in tree.leaves.values():
            leaf.append_token(7)
        with pytest.raises(TypeError):
            sess.step()
        torch.cuda.synchronize()
        assert torch.equal(pool._storage, before)


# ---- exact cases on the bf16 grid -------------------------------------------------------------------------------------------------
FAMILIES = [(4, 4, 128), (8, 2, 128), (4, 4, 64)]  # one MHA, one GQA, one head_dim-64 geometry


def _visibility_step(Hq, Hkv, D, reserve=0, prefix=300, width=5, branch_len=140):
    tree, pool, reserved = few_shot_tree(prefix, width, branch_len, Hkv, D, reserve=reserve)
    g = torch.Generator(device="cuda").manual_seed(D + Hq)
    visibility_pool_bf16(pool, g)
    nq = len(tree.leaves)
    q = dyadic_bf16_(torch.empty((nq, Hq * D), dtype=BF16, device="cuda"), g)
    k_new = torch.zeros((nq, Hkv * D), dtype=BF16, device="cuda")
    v_new = dyadic_bf16_(torch.empty((nq, Hkv * D), dtype=BF16, device="cuda"), g)
    return tree, pool, reserved, q, k_new, v_new


SMALL, FULL = (300, 5, 140), (4096, 32, 200)


@pytest.mark.parametrize("geom,shape", [(g, SMALL) for g in FAMILIES + [(3, 3, 64), (4, 2, 32), (4, 4, 16)]] + [(g, FULL) for g in FAMILIES],
                         ids=lambda x: "x".join(map(str, x)))
def test_exact_visibility(geom, shape):
    """K = 0 and dyadic V: every visible key has P = 1 exactly, the output is the fp64 mean of V over the path to within one bf16 ulp.
    The power check runs first, on the CPU side of the data, before anything is launched: one dropped or doubled key moves some
    element by at least four times that tolerance at these path lengths."""
    Hq, Hkv, D = geom
    tree, pool, _, q, k_new, v_new = _visibility_step(Hq, Hkv, D, prefix=shape[0], width=shape[1], branch_len=shape[2])
    paths = product_leaf_paths(tree)
    nq = len(paths)
    start = pool._storage.clone()
    # the step's own rows are on the paths: place them before the power check looks at the data, then restore the pool
    leaves = sorted(tree.leaves.values(), key=lambda n: n.id)
    loc = torch.tensor([lf.kv_indices[-1] for lf in leaves], dtype=torch.int64, device="cuda")
    pool.get_value_buffer(0)[loc] = v_new.view(nq, Hkv, D)
    factor = power_check_bf16(pool.get_value_buffer(0), paths, (0, nq - 1))
    report(f"bf16 power check {geom} {shape}: one key moves the mean by {factor:.1f} x the tolerance")
    expected = oracles.per_query_head(oracles.visible_mean(pool.get_value_buffer(0), paths), Hq, Hkv)
    for mode in ("flatten", "node", "seq"):
        pool._storage.copy_(start)
        out = oracles.eager_step(tree, pool, mode, Hq, Hkv, D, q, k_new, v_new)
        assert_visible_mean_bf16(out, expected, (geom, shape, mode))


@pytest.mark.parametrize("geom", FAMILIES, ids=lambda g: "x".join(map(str, g)))
def test_poisoned_pool_eager(geom):
    """Dead rows NaN / +-Inf: outputs finite and bit-identical to the clean run (a kernel that reads a dead row gives NaN)."""
    Hq, Hkv, D = geom
    tree, pool, reserved, q, k_new, v_new = _visibility_step(Hq, Hkv, D, reserve=3)
    assert int(reserved[0]) == 0
    clean = pool._storage.clone()
    paths = product_leaf_paths(tree)
    live = oracles.live_slots(paths)
    assert 0 not in set(live.tolist())
    for mode in ("flatten", "node", "seq"):
        pool._storage.copy_(clean)
        ref = oracles.eager_step(tree, pool, mode, Hq, Hkv, D, q, k_new, v_new).clone()
        for kind in ("nan", "inf"):
            pool._storage.copy_(clean)
            assert oracles.poison_pool(pool, live, kind) > 0
            out = oracles.eager_step(tree, pool, mode, Hq, Hkv, D, q, k_new, v_new)
            assert bool(torch.isfinite(out).all()) and torch.equal(out, ref), (geom, mode, kind)


@pytest.mark.parametrize("geom", FAMILIES, ids=lambda g: "x".join(map(str, g)))
def test_poisoned_pool_window_plan_session(geom):
    """The same through a window-plan DecodeSession: 40 steps, clean and poisoned, bit-identical step for step."""
    Hq, Hkv, D = geom
    layers, steps = 1, 40

    def run(kind):
        tree, pool, reserved = few_shot_tree(300, 5, 20, Hkv, D, layers=layers, reserve=3, extra=5 * steps + 256)
        g = torch.Generator(device="cuda").manual_seed(D)
        pool._storage.normal_(generator=g)
        q = torch.randn((layers, 5, Hq * D), dtype=BF16, device="cuda", generator=g)
        k = torch.randn((layers, 5, Hkv * D), dtype=BF16, device="cuda", generator=g)
        v = torch.randn((layers, 5, Hkv * D), dtype=BF16, device="cuda", generator=g)
        if kind:
            oracles.poison_pool(pool, oracles.live_slots(product_leaf_paths(tree)), kind)
        sess = deft_amd.DecodeSession(tree, Hq, Hkv, D, layers, lambda l: (q[l], k[l], v[l]), mode="flatten", incremental=True)
        outs = []
        for _ in range(steps):
            for leaf in tree.leaves.values():
                leaf.append_token(7)
            out = sess.step()
            torch.cuda.synchronize()
            outs.append(out[0].clone())
        assert sess.device_errors() == 0 and sess.step_kinds["patch"] > 0
        return outs

    ref = run(None)
    for kind in ("nan", "inf"):
        got = run(kind)
        for s, (a, b) in enumerate(zip(got, ref)):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (geom, kind, s)


# ---- rotary embedding and prefill ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,D,rot,neox", [(8, 2, 128, 128, True), (4, 4, 64, 64, True), (4, 2, 128, 64, False), (4, 4, 32, 32, False)])
def test_rope_within_one_ulp_of_fp64(Hq, Hkv, D, rot, neox):
    n = 37
    g = torch.Generator(device="cuda").manual_seed(rot + D)
    qkv = torch.randn((n, (Hq + 2 * Hkv) * D), dtype=BF16, device="cuda", generator=g)
    q, k, _ = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    positions = torch.randint(0, 2048, (n,), dtype=torch.int64, device="cuda", generator=g)
    mod = deft_amd.get_rope(D, rot, 2048, 10000.0, neox).cuda()
    cache = mod.cos_sin_cache[positions].to(torch.float64)  # [n, rot]: cos | sin
    cos, sin = cache[:, None, : rot // 2], cache[:, None, rot // 2:]
    want = []
    for x, H in ((q, Hq), (k, Hkv)):
        x = x.reshape(n, H, D).to(torch.float64)
        x1, x2 = (x[..., : rot // 2], x[..., rot // 2: rot]) if neox else (x[..., 0:rot:2], x[..., 1:rot:2])
        o1, o2 = x1 * cos - x2 * sin, x2 * cos + x1 * sin
        y = x.clone()
        if neox:
            y[..., : rot // 2], y[..., rot // 2: rot] = o1, o2
        else:
            y[..., 0:rot:2], y[..., 1:rot:2] = o1, o2
        want.append(y)
    mod(positions, q, k)
    torch.cuda.synchronize()
    for name, got, ref, H in (("q", q, want[0], Hq), ("k", k, want[1], Hkv)):
        err = (got.reshape(n, H, D).to(torch.float64) - ref).abs()
        worst = float((err / (bf16_ulp(ref) + 2.0 ** -30)).max())
        report(f"bf16 rope {name} D={D} rot={rot} neox={neox}: max err / ulp {worst:.3f}")
        assert worst <= 1.0
        assert torch.equal(got.reshape(n, H, D)[..., rot:].to(torch.float64), ref[..., rot:])  # beyond rotary_dim: untouched


@pytest.mark.parametrize("Hq,Hkv,D", [(8, 2, 128), (4, 4, 64), (32, 32, 128)])
def test_prefill_against_causal_truth(Hq, Hkv, D):
    """context_attention_fwd over a ragged batch: every element within the bound of fp64 causal attention, A over the causal prefix."""
    lens = [255, 1, 257, 300, 128]
    T = sum(lens)
    g = torch.Generator(device="cuda").manual_seed(D + Hq)
    q = torch.randn((T, Hq, D), dtype=BF16, device="cuda", generator=g)
    k = torch.randn((T, Hkv, D), dtype=BF16, device="cuda", generator=g)
    v = torch.randn((T, Hkv, D), dtype=BF16, device="cuda", generator=g)
    start = torch.tensor(np.cumsum([0] + lens[:-1]), dtype=torch.int32, device="cuda")
    o = torch.full((T, Hq, D), float("nan"), dtype=BF16, device="cuda")
    deft_amd.context_attention_fwd(q, k, v, o, start, torch.tensor(lens, dtype=torch.int32, device="cuda"), max(lens))
    torch.cuda.synchronize()
    assert o.dtype == BF16 and bool(torch.isfinite(o).all())
    G = Hq // Hkv
    worst, sq, sq_ref, count = 0.0, 0.0, 0.0, 0
    for b, ln in enumerate(lens):
        s0 = int(start[b])
        causal = torch.tril(torch.ones((ln, ln), dtype=torch.bool, device="cuda"))
        res = {}
        for dt in (torch.float64, torch.float32):
            qq = q[s0: s0 + ln].to(dt).view(ln, Hkv, G, D)
            kk, vv = k[s0: s0 + ln].to(dt), v[s0: s0 + ln].to(dt)
            s = torch.einsum("nhgd,shd->nhgs", qq, kk) * D ** -0.5
            s.masked_fill_(~causal[:, None, None, :], float("-inf"))
            p = torch.softmax(s, dim=-1)
            res[dt] = (torch.einsum("nhgs,shd->nhgd", p, vv).reshape(ln, Hq, D), torch.einsum("nhgs,shd->nhgd", p, vv.abs()).reshape(ln, Hq, D))
        truth, A = res[torch.float64]
        err = (o[s0: s0 + ln].to(torch.float64) - truth).abs()
        worst = max(worst, float((err / bound(truth, A)).max()))
        sq += float(err.pow(2).sum())
        sq_ref += float((res[torch.float32][0].to(BF16).to(torch.float64) - truth).pow(2).sum())
        count += err.numel()
    ratio = (sq / sq_ref) ** 0.5
    report(f"bf16 prefill {Hq}/{Hkv}/{D} lens {lens}: max err/tol {worst:.3f}  rms / reference arithmetic {ratio:.3f}  ({count} elements)")
    assert worst <= 1.0
    assert ratio <= 2.0
