"""fp8 KV pools on the GPU: the quantising append bit for bit against tests/kv8_model.py, and the kv8 operators
against fp64 truth over the DEQUANTISED tensors at exactly the tolerance the 16-bit operators are held to on the same tensors (fp16 5e-4,
bf16 the a-priori bound of tests/bf16_util.py) -- the conversion e4m3 -> T is exact and the scales stay fp32, so there is no new error
term.  Shapes are the smallest at which the kernel can go wrong: a prefix of three tiles under leaves of two (a), chunks with follower
tiles (b), more than 32 queries (c), one token (d); MHA, GQA and an odd head count; both element types; Flatten and Node.  Beyond random
data: more than 1024 MHA queries (the only launches of stage1_kv8_kernel<T, false>), every finite e4m3 code through the decode kernel's
conversion, a negative and a zero softmax scale, a head stride other than D, and the append followed by the decode replayed from one
captured graph (the scales are read on the device).  Shaped scores are tests/test_kv8_sharp.py's.

Every figure is printed before it is asserted (`pytest -s`; profiles/kv8_error.txt is made of those lines)."""
import ctypes

import pytest
import torch

import bf16_util
import deft_amd
import kv8_model
import oracles
from deft_amd import _lib
from states_model import path_lse
from tools.error_bound import bound_bf16, dense_attention
from truth import product_leaf_paths, tree_truth

pytestmark = pytest.mark.gpu
FP8, F16, BF16, F32 = torch.float8_e4m3fn, torch.float16, torch.bfloat16, torch.float32
NAME = {F16: "fp16", BF16: "bf16"}
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
D = 128
GEOMS = [(4, 4), (8, 2), (3, 3)]
SHAPES = {"a-300x5x140": (300, 5, 140), "b-1100x3x5": (1100, 3, 5), "c-200x40x3": (200, 40, 3), "d-chain1": (1, 0, 0)}
WIDE = {"e-130x1030x2": (130, 1030, 2)}  # more than 1024 queries: test_more_than_1024_mha_queries alone
# per-head scales, none a power of two.  The head with the sharp softmax (k_scale 1.9) has outputs that reach 1 (the largest |output| is
# printed); not beyond: fp16's 5e-4 is a tolerance for outputs up to 1 (half an fp16 ulp alone is 4.9e-4 from 1.0 on)
K_SCALES = [0.73, 1.9, 1.21, 0.57]
V_SCALES = [0.61, 0.7, 0.37, 0.53]
_TREES = {}


def report(line):
    print("[kv8] " + line, flush=True)


def _tree(shape, Hkv, reserve=0):
    """(tree, paths, metadata, pool size) of a few-shot tree (a chain when width = 0), built once per (shape, heads)."""
    key = (shape, Hkv, reserve)
    if key not in _TREES:
        prefix, width, branch_len = {**SHAPES, **WIDE}[shape]
        if width:
            tree, pool, _ = oracles.few_shot_tree(prefix, width, branch_len, Hkv, D, reserve=reserve)
        else:
            req = deft_amd.ReqToTokenPool(8, prefix + 64, device="cuda")
            pool = deft_amd.TokenToKVPool(prefix + 64, F16, Hkv, D, 1, device="cuda")
            tree = deft_amd.TreeCache(F16, Hkv, D, 1, req, pool, None, True, False)
            tree.init_prompt(torch.arange(1, prefix + 1, dtype=torch.int32))
        _TREES[key] = (tree, product_leaf_paths(tree), deft_amd.TreeMetadata.from_tree_cache(tree), pool.size)
    return _TREES[key]


def _codes(size, Hkv, seed, amp=1.0):
    """One layer of an fp8 pool, [size, 2, Hkv, D]: fp16 N(0, amp) storage quantised with unit scales (tests/kv8_model.py)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    st = (torch.randn((size, 2, Hkv, D), device="cuda", generator=g) * amp).to(F16)
    return kv8_model.quantize(st, 1.0), g


def _flat(md):
    return (md.block_len, md.block_q, md.block_q_cnts, md.block_q_offset, md.block_bitmasks, md.block_kv, md.block_lens)


def _nodes(md):
    return (md.node_kv, md.node_kv_offset, md.node_kv_len, md.node_q, md.node_q_offset, md.node_q_len)


def _run8(mode, q, codes, md, ks=None, vs=None, with_lse=False, scale=None):
    kb, vb = codes[:, 0], codes[:, 1]
    out = torch.full_like(q, float("nan"))
    lse = torch.full(q.shape[:2], 777.0, dtype=F32, device="cuda") if with_lse else None
    kw = dict(k_scale=ks, v_scale=vs, scale=scale)
    if mode == "flatten":
        if with_lse:
            deft_amd.tree_attention_subtree_fwd_kv8_lse(q, kb, vb, out, lse, *_flat(md), **kw)
        else:
            deft_amd.tree_attention_subtree_fwd_kv8(q, kb, vb, out, *_flat(md), **kw)
    else:
        if with_lse:
            deft_amd.tree_attention_fwd_kv8_lse(q, kb, vb, out, lse, *_nodes(md), **kw)
        else:
            deft_amd.tree_attention_fwd_kv8(q, kb, vb, out, *_nodes(md), **kw)
    torch.cuda.synchronize()
    return (out, lse) if with_lse else out


def _run16(mode, q, kv16, md):
    out = torch.full_like(q, float("nan"))
    if mode == "flatten":
        deft_amd.tree_attention_subtree_fwd(q, kv16[:, 0], kv16[:, 1], out, *_flat(md))
    else:
        deft_amd.tree_attention_fwd(q, kv16[:, 0], kv16[:, 1], out, *_nodes(md))
    torch.cuda.synchronize()
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _check(out, q, k64, v64, paths, Hq, Hkv, tag):
    """The 16-bit operators' own tolerance against fp64 truth over the tensors k64 / v64 (fp64 [size, Hkv, D]): fp16 5e-4 per element, bf16
    the a-priori bound u A + 2 u |o| + 2e-5.  Returns the worst error / tolerance."""
    truth, A = dense_attention(q, k64, v64, paths, Hq, Hkv, D ** -0.5, with_abs=True)
    assert float((truth - tree_truth(q, k64, v64, paths, Hq, Hkv, D ** -0.5)).abs().max()) < 1e-12
    got = out.reshape(truth.shape).to(torch.float64)
    assert bool(torch.isfinite(got).all()), (tag, "non-finite output")
    err = (got - truth).abs()
    tol = torch.full_like(truth, 5e-4) if out.dtype == F16 else bound_bf16(truth, A)
    worst = float((err / tol).max())
    report(f"{tag}: worst err {float(err.max()):.3e}  err/tol {worst:.3f}  largest |output| {float(truth.abs().max()):.2f}  ({truth.numel()} elements)")
    assert worst <= 1.0, (tag, worst)
    return worst


# ---- 1. the append, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_append_quantises_bit_for_bit(dtype):
    Hkv, slots = 3, 64
    loc = torch.tensor([0, 63, 7, 8, 31], dtype=torch.int32, device="cuda")
    n = loc.shape[0]
    ks = torch.tensor([1.0, 0.5, 0.0371], dtype=F32, device="cuda")
    vs = torch.tensor([0.0371, 1.0, 0.5], dtype=F32, device="cuda")
    edge = kv8_model.edge_inputs().to("cuda")
    assert edge.numel() <= n * D
    g = torch.Generator(device="cuda").manual_seed(8)
    # every head's [n, D] rows hold all the edge inputs (a head with scale s sees them divided by s), then N(0, 100) -- beyond +-448 too
    x = torch.randn((2, n, Hkv, D), device="cuda", generator=g) * 100.0
    for t in range(2):
        for h in range(Hkv):
            flat = x[t, :, h].reshape(-1).clone()
            flat[: edge.numel()] = edge
            x[t, :, h] = flat.reshape(n, D)
    k_new, v_new = x[0].to(dtype).reshape(n, Hkv * D), x[1].to(dtype).reshape(n, Hkv * D)
    assert bool(torch.isnan(k_new).any()) and bool((k_new.float().abs() > 448).any())
    kv = torch.full((slots, 2, Hkv, D), 0x55, dtype=torch.uint8, device="cuda").view(FP8)
    deft_amd.kv_append_kv8(kv, loc, k_new, v_new, ks, vs)
    torch.cuda.synchronize()
    want_k = kv8_model.quantize(k_new.reshape(n, Hkv, D).cpu(), ks.cpu()[:, None])
    want_v = kv8_model.quantize(v_new.reshape(n, Hkv, D).cpu(), vs.cpu()[:, None])
    got = kv.view(torch.uint8).cpu()  # (indexed as bytes)
    li = loc.cpu().long()
    for name, g8, w8 in (("K", got[li, 0].view(FP8), want_k), ("V", got[li, 1].view(FP8), want_v)):
        diff = int(((g8.view(torch.uint8) != w8.view(torch.uint8)) & ~(kv8_model.is_nan_code(g8) & kv8_model.is_nan_code(w8))).sum())
        report(f"append {NAME[dtype]} {name}: {diff} of {w8.numel()} codes differ from the model")
        assert kv8_model.same_codes(g8, w8), (name, diff)
    assert bool(kv8_model.is_nan_code(got[li, 0].view(FP8)).any())  # NaN in -> a NaN code out
    untouched = torch.ones(slots, dtype=torch.bool)
    untouched[li] = False
    assert bool((got[untouched] == 0x55).all())
    # null scales = ones
    kv2 = torch.full((slots, 2, Hkv, D), 0x55, dtype=torch.uint8, device="cuda").view(FP8)
    deft_amd.kv_append_kv8(kv2, loc, k_new, v_new)
    kv3 = torch.full((slots, 2, Hkv, D), 0x55, dtype=torch.uint8, device="cuda").view(FP8)
    deft_amd.kv_append_kv8(kv3, loc, k_new, v_new, torch.ones_like(ks), torch.ones_like(vs))
    torch.cuda.synchronize()
    assert torch.equal(kv2.view(torch.uint8), kv3.view(torch.uint8))
    assert kv8_model.same_codes(kv2.view(torch.uint8).cpu()[li, 0].view(FP8), kv8_model.quantize(k_new.reshape(n, Hkv, D).cpu(), 1.0))


# ---- 2. decode against fp64 truth over the dequantised tensors ----------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_decode_against_truth_of_the_dequantised_pool(shape, geom):
    Hq, Hkv = geom
    tree, paths, md, size = _tree(shape, Hkv)
    codes, g = _codes(size, Hkv, seed=len(shape) + Hq)
    deq = kv8_model.dequantize(codes)  # fp64 [size, 2, Hkv, D]
    for dtype in (F16, BF16):
        kv16 = codes.to(dtype)  # exact
        assert torch.equal(kv16.to(torch.float64), deq)
        q = torch.randn((len(paths), Hq, D), device="cuda", generator=g).to(dtype)
        for mode in ("flatten", "node"):
            tag = f"{shape} {Hq}x{Hkv} {mode} {NAME[dtype]}"
            o16 = _run16(mode, q, kv16, md)
            _check(o16, q, deq[:, 0], deq[:, 1], paths, Hq, Hkv, tag + " 16-bit operator on the dequantised pool")
            o8 = _run8(mode, q, codes, md)
            _check(o8, q, deq[:, 0], deq[:, 1], paths, Hq, Hkv, tag + " kv8")
            report(f"{tag}: largest |kv8 - 16-bit| {float((o8.float() - o16.float()).abs().max()):.3e}")


# ---- 3. scales -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_scales(geom, dtype):
    Hq, Hkv = geom
    G = Hq // Hkv
    tree, paths, md, size = _tree("a-300x5x140", Hkv)
    codes, g = _codes(size, Hkv, seed=31 + Hq)
    q = torch.randn((len(paths), Hq, D), device="cuda", generator=g).to(dtype)
    ks = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
    vs = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
    k64 = kv8_model.dequantize(codes[:, 0], ks[:, None])
    v64 = kv8_model.dequantize(codes[:, 1], vs[:, None])
    for mode in ("flatten", "node"):
        tag = f"scales {Hq}x{Hkv} {mode} {NAME[dtype]}"
        base = _run8(mode, q, codes, md, ks, vs)
        _check(base, q, k64, v64, paths, Hq, Hkv, tag + " (i) per-head scales")  # (i)
        # (ii) doubling every v_scale doubles every output exactly (elements that are normal numbers of T in both runs)
        dbl = _run8(mode, q, codes, md, ks, 2 * vs)
        tiny = torch.finfo(dtype).tiny
        normal = (base.float().abs() >= tiny) & (dbl.float().abs() >= tiny)
        assert int(normal.sum()) > 0.99 * base.numel()
        assert torch.equal(dbl.float()[normal], 2 * base.float()[normal]), tag
        # (iii) doubling every k_scale while halving the softmax scale: bit-identical
        assert _same_bits(_run8(mode, q, codes, md, 2 * ks, vs, scale=0.5 * D ** -0.5), base), tag
        # (iv) null scales = all ones, bit for bit
        ones = torch.ones(Hkv, dtype=F32, device="cuda")
        plain = _run8(mode, q, codes, md)
        assert _same_bits(plain, _run8(mode, q, codes, md, ones, ones)) and _same_bits(plain, _run8(mode, q, codes, md, None, ones)), tag
        # (v) swapping two heads' scales changes exactly those heads' outputs
        if Hkv >= 2:
            perm = list(range(Hkv))
            perm[0], perm[1] = 1, 0
            sw = _run8(mode, q, codes, md, ks[perm], vs[perm])
            changed = (sw != base).reshape(len(paths), Hkv, G, D).any(dim=-1)  # [nq, Hkv, G]
            assert bool(changed[:, :2].all()) and not bool(changed[:, 2:].any()), tag


# ---- 4. poisoned pool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_a_dead_slot_may_hold_any_byte(geom):
    Hq, Hkv = geom
    tree, paths, md, size = _tree("a-300x5x140", Hkv, reserve=3)
    live = oracles.live_slots(paths)
    assert 0 not in set(live.tolist())  # slot 0 is reserved: on no path
    codes, g = _codes(size, Hkv, seed=77 + Hq)
    dead = torch.ones(size, dtype=torch.bool)
    dead[live] = False
    dead = dead.to("cuda")
    assert int(dead.sum()) > 100
    zeroed, poisoned = codes.clone(), codes.clone()
    zeroed.view(torch.uint8)[dead] = 0
    poisoned.view(torch.uint8)[dead] = 0x7F
    for dtype in (F16, BF16):
        q = torch.randn((len(paths), Hq, D), device="cuda", generator=g).to(dtype)
        for mode in ("flatten", "node"):
            ref = _run8(mode, q, zeroed, md)
            out = _run8(mode, q, poisoned, md)
            assert bool(torch.isfinite(out).all()) and _same_bits(out, ref), (geom, mode, dtype)


# ---- 5. exact visibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("shape", ["a-300x5x140", "c-200x40x3"])
def test_exact_visibility(shape, geom):
    """K codes all zero: every score is 0, every visible key weighs 1 exactly, the output is the mean of the visible V rows."""
    Hq, Hkv = geom
    tree, paths, md, size = _tree(shape, Hkv)
    g = torch.Generator(device="cuda").manual_seed(5 + Hq)
    values = torch.tensor([0, 0.25, -0.25, 0.5, -0.5, 1, -1, 1.5, -1.5, 2, -2, 3, -3], dtype=F32, device="cuda")  # exact in e4m3
    v = values[torch.randint(0, values.numel(), (size, Hkv, D), device="cuda", generator=g)]
    codes = torch.zeros((size, 2, Hkv, D), dtype=torch.uint8, device="cuda").view(FP8)
    codes[:, 1] = v.to(FP8)
    assert torch.equal(codes[:, 1].to(F32), v)
    expected = oracles.per_query_head(oracles.visible_mean(codes[:, 1].to(F16), paths), Hq, Hkv)
    oracles.power_check(codes[:, 1].to(F16), paths, (0, len(paths) - 1))
    for dtype in (F16, BF16):
        q = torch.randn((len(paths), Hq, D), device="cuda", generator=g).to(dtype)
        for mode in ("flatten", "node"):
            out = _run8(mode, q, codes, md).reshape(len(paths), Hq * D)
            if dtype == F16:
                res = oracles.assert_visible_mean(out, expected, (shape, geom, mode))
                report(f"visibility {shape} {Hq}x{Hkv} {mode} fp16: err/tol {res['ratio']:.3f}")
            else:
                bf16_util.assert_visible_mean_bf16(out, expected, (shape, geom, mode))


# ---- 6. log-sum-exp ----------------------------------------------------------------------------------------------------------------------
def _composed_tol(o, A, dtype):  # tests/test_states_gpu.py: the single call's tolerance, one more rounding of each part and of the result
    if dtype == F16:
        return 5e-4 + 2.0 ** -11 * (A + o.abs())
    return bound_bf16(o, A) + U[BF16] * (A + o.abs())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_lse_forms_and_a_split_merged(geom, dtype):
    Hq, Hkv = geom
    tree, paths, md, size = _tree("a-300x5x140", Hkv)
    nq = len(paths)
    codes, g = _codes(size, Hkv, seed=61 + Hq)
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(dtype)
    ks = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
    vs = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
    k64 = kv8_model.dequantize(codes[:, 0], ks[:, None])
    v64 = kv8_model.dequantize(codes[:, 1], vs[:, None])
    want = path_lse(q, k64, paths, Hq, Hkv, D ** -0.5)
    tol = U[dtype] + 2e-5
    for mode in ("flatten", "node"):
        plain = _run8(mode, q, codes, md, ks, vs)
        out, lse = _run8(mode, q, codes, md, ks, vs, with_lse=True)
        assert _same_bits(out, plain), (mode, "out differs from the plain kv8 call's")
        err = float((lse.to(torch.float64) - want).abs().max())
        report(f"lse {Hq}x{Hkv} {mode} {NAME[dtype]}: worst |lse - fp64| {err:.3e}  err/tol {err / tol:.3f}")
        assert err <= tol, (mode, err)
    # the Flatten blocks in two kv8 calls (cut inside the shared prefix), the two states merged
    truth, A = dense_attention(q, k64, v64, paths, Hq, Hkv, D ** -0.5, with_abs=True)
    _, block_q, cnts, off, masks, kv, lens = _flat(md)
    NB = cnts.shape[0]
    prefix = set(int(s) for s in tree.root.kv_indices)
    first = kv[::128].tolist()
    k = 1
    assert 0 < k < NB and int(first[k - 1]) in prefix and int(first[k]) in prefix
    ok = int(off[k])
    halves = [(block_q[:ok], cnts[:k], off[:k], masks[: 128 * k], kv[: 128 * k], lens[:k]),
              (block_q[ok:], cnts[k:], off[k:] - ok, masks[128 * k :], kv[128 * k :], lens[k:])]
    states = []
    for arrays in halves:
        o = torch.full_like(q, float("nan"))
        l = torch.full((nq, Hq), 777.0, dtype=F32, device="cuda")
        deft_amd.tree_attention_subtree_fwd_kv8_lse(q, codes[:, 0], codes[:, 1], o, l, 128, *[a.contiguous() for a in arrays], k_scale=ks,
                                                    v_scale=vs)
        states.append((o, l))
    out, lse = deft_amd.merge_attention_states(states[0][0], states[0][1], states[1][0], states[1][1])
    torch.cuda.synchronize()
    err = (out.to(torch.float64) - truth).abs()
    ctol = _composed_tol(truth, A, dtype)
    el = float((lse.to(torch.float64) - want).abs().max())
    report(f"split {Hq}x{Hkv} {NAME[dtype]} at block {k} of {NB}: worst err {float(err.max()):.3e}  err/tol {float((err / ctol).max()):.3f}  "
           f"merged lse err {el:.3e}")
    assert bool((err <= ctol).all()), float((err / ctol).max())
    assert el <= tol + 4e-6, el


# ---- 7. the module: DeFTAttention.forward on an fp8 pool -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_module_decode_steps_on_an_fp8_pool(geom, dtype):
    Hq, Hkv = geom
    prefix, width, branch_len = 300, 5, 3
    size = prefix + width * (branch_len + 8) + 64
    req = deft_amd.ReqToTokenPool(72, size + 8, device="cuda")
    pool = deft_amd.TokenToKVPool(size, FP8, Hkv, D, 1, device="cuda")
    assert pool.is_fp8 and pool.kv_data[0].dtype == FP8
    tree = deft_amd.TreeCache(dtype, Hkv, D, 1, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, prefix + 1, dtype=torch.int32))
    tree.branch(tree.root, width)
    codes, g = _codes(size, Hkv, seed=91 + Hq)
    pool._storage[0].copy_(codes)
    ks = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
    vs = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
    pool.set_kv_scales(0, ks, vs)

    def grow(n):
        for _ in range(n):
            for leaf in list(tree.leaves.values()):
                leaf.append_token(7)
            tree.alloc()

    grow(branch_len)
    for step, mode in enumerate(("flatten", "node", "node_chunk", "flatten")):  # (four steps: the tree grows between them)
        paths = product_leaf_paths(tree)
        nq = len(paths)
        q = torch.randn((nq, Hq * D), device="cuda", generator=g).to(dtype)
        k_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
        v_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
        out = oracles.eager_step(tree, pool, mode, Hq, Hkv, D, q, k_new, v_new)
        loc = torch.tensor([p[-1] for p in paths], dtype=torch.int64)
        want_k = kv8_model.quantize(k_new.reshape(nq, Hkv, D).cpu(), ks.cpu()[:, None])  # (the CPU model, as in the append test)
        want_v = kv8_model.quantize(v_new.reshape(nq, Hkv, D).cpu(), vs.cpu()[:, None])
        kv = pool.kv_data[0]
        rows = kv.view(torch.uint8).cpu()[loc]
        assert kv8_model.same_codes(rows[:, 0].view(FP8), want_k) and kv8_model.same_codes(rows[:, 1].view(FP8), want_v), (step, mode)
        k64 = kv8_model.dequantize(kv[:, 0], ks[:, None])
        v64 = kv8_model.dequantize(kv[:, 1], vs[:, None])
        _check(out, q, k64, v64, paths, Hq, Hkv, f"module step {step} {mode} {Hq}x{Hkv} {NAME[dtype]}")
        grow(1)


def test_module_prefill_quantises_the_prompt_then_decodes():
    """ForwardMode.PREFILL on an fp8 pool: causal attention over the prompt's own 16-bit rows -- the output of the same call on a 16-bit
    pool, bit for bit -- and store_kv_cache quantises the rows into the pool; a Flatten decode step over that pool then meets the decode
    tolerance against the dequantised prompt."""
    Hq, Hkv, n = 8, 2, 200
    g = torch.Generator(device="cuda").manual_seed(17)
    q, k, v = (torch.randn((n, h * D), device="cuda", generator=g).to(F16) for h in (Hq, Hkv, Hkv))
    ks = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
    vs = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
    outs, trees = {}, {}
    for pool_dtype in (F16, FP8):
        req = deft_amd.ReqToTokenPool(8, 512, device="cuda")
        pool = deft_amd.TokenToKVPool(512, pool_dtype, Hkv, D, 1, device="cuda")
        if pool_dtype == FP8:
            pool._storage.view(torch.uint8).fill_(0x7F)  # (nothing but the appended rows may be read later)
            pool.set_kv_scales(0, ks, vs)
        tree = deft_amd.TreeCache(F16, Hkv, D, 1, req, pool, None, True, False)
        updater = tree.init_prompt(torch.arange(1, n + 1, dtype=torch.int32))
        meta = deft_amd.InputMetadata(deft_amd.ForwardMode.PREFILL, updater, pool, req, start_loc=torch.zeros(1, dtype=torch.int32, device="cuda"),
                                      seq_lens=torch.tensor([n], dtype=torch.int64, device="cuda"), max_seq_len=n)
        outs[pool_dtype] = deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, 0)(q, k, v, meta)
        trees[pool_dtype] = (tree, pool)
    torch.cuda.synchronize()
    assert _same_bits(outs[FP8], outs[F16])
    tree, pool = trees[FP8]
    slots = torch.tensor([int(s) for s in tree.root.kv_indices], dtype=torch.int64)
    rows = pool.kv_data[0].view(torch.uint8).cpu()[slots]
    assert kv8_model.same_codes(rows[:, 0].view(FP8), kv8_model.quantize(k.reshape(n, Hkv, D).cpu(), ks.cpu()[:, None]))
    assert kv8_model.same_codes(rows[:, 1].view(FP8), kv8_model.quantize(v.reshape(n, Hkv, D).cpu(), vs.cpu()[:, None]))
    tree.branch(tree.root, 2)
    for leaf in list(tree.leaves.values()):
        leaf.append_token(7)
    tree.alloc()
    paths = product_leaf_paths(tree)
    q1, k1, v1 = (torch.randn((2, h * D), device="cuda", generator=g).to(F16) for h in (Hq, Hkv, Hkv))
    out = oracles.eager_step(tree, pool, "flatten", Hq, Hkv, D, q1, k1, v1)
    kv = pool.kv_data[0]
    _check(out, q1, kv8_model.dequantize(kv[:, 0], ks[:, None]), kv8_model.dequantize(kv[:, 1], vs[:, None]), paths, Hq, Hkv,
           "module prefill then a flatten step 8x2 fp16")


# ---- the item loop of a capped grid ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 2, 1500, 70, 3), (4, 4, 300, 5, 40), (3, 3, 300, 5, 40)], ids=lambda s: "x".join(map(str, s)))
def test_item_loop_of_a_capped_grid(shape):
    """No shape of this file comes near the grid cap (2 or 6 workgroups per CU), so a workgroup never takes a second work item above.  The
    knob that forces a tiny grid exists in the EXPERIMENTS build only: the check runs in a child process bound to it
    (tests/exp_kv8_items.py), as tests/test_gpu_parity.py does for the 16-bit kernel."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exp = os.path.join(root, "deft_amd", "lib", "libdeft_amd_exp.so")
    assert os.path.exists(exp), "build the experiments library: make -C deft_amd/csrc exp (__graft_entry__.build() does)"
    env = dict(os.environ, DEFT_AMD_LIB=exp, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "exp_kv8_items.py"), *[str(x) for x in shape]], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout, flush=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "items identical" in r.stdout


# ---- 8. ABI errors through real tensors ------------------------------------------------------------------------------------------------
def test_abi_errors_on_real_tensors():
    Hq, Hkv = 4, 2
    tree, paths, md, size = _tree("d-chain1", Hkv)
    codes, g = _codes(size, Hkv, seed=3)
    q = torch.randn((1, Hq, D), device="cuda", generator=g).to(F16)
    out = torch.empty_like(q)
    mdl = [t.data_ptr() for t in _flat(md)[1:]]
    NB, P = md.block_q_cnts.shape[0], md.block_q.shape[0]
    ws_bytes = _lib.lib.deft_flatten_workspace_bytes(NB, P, 1, Hq, Hkv, D)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    kb, vb = codes[:, 0], codes[:, 1]

    def call(k_ptr=None, ss=None, d=D, wsb=ws_bytes):
        return _lib.lib.deft_flatten_decode_f16_kv8(q.data_ptr(), q.stride(0), q.stride(1), kb.data_ptr() if k_ptr is None else k_ptr, vb.data_ptr(),
                                                    kb.stride(0) if ss is None else ss, kb.stride(1), None, None, out.data_ptr(), out.stride(0),
                                                    out.stride(1), *mdl, NB, P, 1, Hq, Hkv, d, D ** -0.5, None, ws.data_ptr(), wsb, None)

    err = lambda: _lib.lib.deft_last_error().decode()  # noqa: E731
    assert call(d=64) == -2 and err() == "fp8 KV pool: head_dim 64 is not supported (head_dim must be 128; 64, 32 and 16 are not built for fp8 pools)"
    assert call(ss=kb.stride(0) + 1) == -1 and err() == f"fp8 KV pool: odd slot stride {kb.stride(0) + 1} (the plan addresses rows in 2-byte units)"
    assert call(k_ptr=kb.data_ptr() + 8) == -1 and err() == ("fp8 KV pool: base pointers and the slot stride must be 16-byte aligned, the head "
                                                             "stride a multiple of 16")
    assert call(wsb=ws_bytes - 1) == -4 and err() == f"workspace too small: {ws_bytes - 1} < {ws_bytes}"
    assert call() == 0
    torch.cuda.synchronize()
    deq = kv8_model.dequantize(codes)
    _check(out, q, deq[:, 0], deq[:, 1], paths, Hq, Hkv, "raw ABI call, plan built per call")
    assert ctypes.CDLL(_lib.LIB_PATH).deft_abi_version() == 2


# ---- 9. more than 1024 MHA queries: stage1_kv8_kernel<T, false> ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_more_than_1024_mha_queries(dtype):
    """launch_stage1_kv8 takes K / V rows by non-temporal DMA (`nt`) when `G > 1 || nq <= 1024`: an MHA launch (Hq == Hkv) of more than
    1024 queries is the only one that picks stage1_kv8_kernel<T, false> -- ordinary cache policy, a kernel compiled and register-allocated
    on its own -- and no other shape of this file (nor of tests/exp_kv8_items.py) has more than 70 queries.  A 130-token prefix under 1030
    two-token leaves, geometry 2x2: against fp64 truth of the dequantised pool with per-head scales, and with exact visibility.  The
    block count is printed: leaders x Hkv against the MHA grid cap (6 workgroups per CU) says whether a workgroup took a second item."""
    Hq, Hkv = 2, 2
    shape = "e-130x1030x2"
    tree, paths, md, size = _tree(shape, Hkv)
    nq = len(paths)
    assert nq > 1024 and Hq == Hkv, (nq, Hq, Hkv)
    report(f"{shape} {Hq}x{Hkv}: {nq} queries, {md.block_q_cnts.shape[0]} Flatten blocks, {md.block_q.shape[0]} (query, block) pairs, pool of {size} slots")
    codes, g = _codes(size, Hkv, seed=1030, amp=0.5)  # (paths of 132 keys: at unit amplitude the softmax is sharp enough for outputs near 2, and 5e-4 is a tolerance for outputs up to 1)
    ks = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
    vs = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
    k64 = kv8_model.dequantize(codes[:, 0], ks[:, None])
    v64 = kv8_model.dequantize(codes[:, 1], vs[:, None])
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(dtype)
    for mode in ("flatten", "node"):
        _check(_run8(mode, q, codes, md, ks, vs), q, k64, v64, paths, Hq, Hkv, f"{shape} {Hq}x{Hkv} {mode} {NAME[dtype]} kv8")
    # exact visibility: K codes zero, every visible key weighs 1
    values = torch.tensor([0, 0.25, -0.25, 0.5, -0.5, 1, -1, 1.5, -1.5, 2, -2, 3, -3], dtype=F32, device="cuda")
    v = values[torch.randint(0, values.numel(), (size, Hkv, D), device="cuda", generator=g)]
    vis = torch.zeros((size, 2, Hkv, D), dtype=torch.uint8, device="cuda").view(FP8)
    vis[:, 1] = v.to(FP8)
    expected = oracles.per_query_head(oracles.visible_mean(vis[:, 1].to(F16), paths), Hq, Hkv)
    oracles.power_check(vis[:, 1].to(F16), paths, (0, nq - 1))
    for mode in ("flatten", "node"):
        out = _run8(mode, q, vis, md).reshape(nq, Hq * D)
        if dtype == F16:
            res = oracles.assert_visible_mean(out, expected, (shape, mode))
            report(f"visibility {shape} {Hq}x{Hkv} {mode} fp16: err/tol {res['ratio']:.3f}")
        else:
            bf16_util.assert_visible_mean_bf16(out, expected, (shape, mode))


# ---- 10. every finite code through the decode kernel's conversion -----------------------------------------------------------------------
_FINITE = [c for c in range(256) if (c & 0x7F) != 0x7F]  # 254 byte codes
_SUBNORMAL = [c for c in range(256) if (c & 0x78) == 0]  # 16: +-0 and +-m 2^-9, m = 1..7
ALL_CODE_V_SCALES = [1.22, 1.4, 0.97, 1.06]  # (none a power of two; >= 0.97 so that one subnormal step, 2^-9, stays 4x above the tolerance)


def _code_pool(paths, size, Hkv, kind):
    """uint8 [size, Hkv, D]: a fixed permutation of the code list per (position on the path, head, dim) -- 37 and 91 are coprime to 254
    and to 16, so a column walks through every code along a path and a key row through every code across its 128 columns; every column
    and every one of the 32 key rows of a wave slice meets subnormal, small and large codes (asserted by the caller).  Dead slots: 0x7F.
      plain       all 254 finite codes
      antithetic  all 254, the key at depth 2i + 1 holding MINUS the key at depth 2i (the sign bit flipped): every path sums to exactly 0
      subnormal   the 16 codes of exponent 0"""
    dep = torch.full((size,), -1, dtype=torch.int64)
    for p in paths:
        dep[torch.as_tensor(p)] = torch.arange(len(p))
    table = torch.tensor(_SUBNORMAL if kind == "subnormal" else _FINITE, dtype=torch.int64)
    pos = dep.clamp_min(0) // 2 if kind == "antithetic" else dep.clamp_min(0)
    idx = (37 * pos[:, None, None] + 17 * torch.arange(Hkv)[None, :, None] + 91 * torch.arange(D)[None, None, :]) % table.numel()
    code = table[idx]
    if kind == "antithetic":
        code = code ^ (0x80 * (dep.clamp_min(0) & 1))[:, None, None]
    code[dep < 0] = 0x7F
    return code.to(torch.uint8), dep


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_every_finite_code_through_the_decode_kernel(geom):
    """K codes all zero (every visible key weighs 1 exactly), the V of a-300x5x140 holds all 254 finite codes -- subnormals and +-448
    included, NaN codes in dead slots only -- through ds_read_b64_tr_b8, the byte-to-element map and v_cvt_scalef32_pk_*_fp8.  Expected:
    the fp64 visible mean of kv8_model.code_values() (the format's definition, not torch's cast) times v_scale.

    A plain mean of values up to 448 has no one-ulp power (the mean is ~6, its fp16 ulp 2^-8; the fp32 sums round).  Three passes instead:

      antithetic  keys 2i and 2i + 1 of every path hold +x and -x, per (head, dim).  Every value is a multiple of 2^-9; any partial sum the
                  kernel can form (any 16 keys of an MFMA step in any order, on top of complete pairs, which cancel) stays below 2^13,
                  so it needs at most 22 bits: every fp32 sum is EXACT, l = n exactly, and the output is exactly 0.  Tolerance: the
                  visibility tolerance at 0 (one ulp + 2^-20 = 1.0e-6).  Converting ONE code of ONE key one step wrong moves an element by
                  at least 2^-9 v_scale / n = 4.3e-6 (n = 440, v_scale >= 0.97): 4x the tolerance (asserted).  Blind to a conversion that is
                  wrong by the same amount for +x and -x: the next two passes.
      subnormal   only the 16 codes of exponent 0 (|x| <= 7 2^-9), unpaired: sums exact again (below 2^12 units of 2^-9), held to the
                  visibility tolerance (one ulp of the expectation + 2^-20).  A kernel that flushed subnormal codes would return 0.
      plain       all 254 codes unpaired: the fp32 sums round, so this is held to the _check tolerance scaled by the largest |output|
                  (fp16 5e-4 max|o|, which also covers half an fp16 ulp, <= 2^-11 |o|; bf16 its a-priori bound, relative already).  Catches a
                  wrong exponent or mantissa map of the normal codes, symmetric ones included.

    And one pass with K holding all the codes (|k| up to 448 times k_scale) under a Q small enough that no score passes 20 nats."""
    Hq, Hkv = geom
    tree, paths, md, size = _tree("a-300x5x140", Hkv)
    nq, n = len(paths), len(paths[0])
    assert all(len(p) == n for p in paths) and n % 2 == 0
    vs = torch.tensor(ALL_CODE_V_SCALES[:Hkv], dtype=F32, device="cuda")
    values = kv8_model.code_values()
    sub = set(_SUBNORMAL) - {0x00, 0x80}
    g = torch.Generator(device="cuda").manual_seed(254 + Hq)
    for kind in ("antithetic", "subnormal", "plain"):
        code, dep = _code_pool(paths, size, Hkv, kind)
        live = code[dep >= 0]
        assert not bool(((live & 0x7F) == 0x7F).any())  # no NaN code in a live slot
        if kind != "subnormal":
            assert set(live.unique().tolist()) == set(_FINITE)
            # every column, and every key row (mod 32) of the prefix, meets subnormal, small and large codes
            pre = code[torch.as_tensor(paths[0][:288])].reshape(9, 32, Hkv, D).long()
            mag = values[pre].abs()
            is_sub = torch.isin(pre, torch.tensor(sorted(sub)))
            for cls in (is_sub, (mag > 0) & (mag < 1), mag >= 64):
                assert bool(cls.any(dim=0).any(dim=-1).all()) and bool(cls.any(dim=0).any(dim=0).all()), kind  # rows; columns
        else:
            assert set(live.unique().tolist()) == set(_SUBNORMAL)
        v64 = values[code.long()].to("cuda") * vs.to(torch.float64)[None, :, None]  # [size, Hkv, D], NaN in dead slots
        expected = oracles.per_query_head(oracles.visible_mean(v64, paths), Hq, Hkv)  # fp64 [nq, Hq * D]
        codes = torch.zeros((size, 2, Hkv, D), dtype=torch.uint8, device="cuda")
        codes[:, 1] = code.to("cuda")
        codes = codes.view(FP8)
        if kind == "antithetic":
            assert float(expected.abs().max()) == 0.0
            power = 2.0 ** -9 * float(vs.min()) / n / float(oracles.tolerance(torch.zeros(1, dtype=torch.float64)))
            report(f"all codes {Hq}x{Hkv} antithetic: one code step of one key moves an element by {power:.2f} x the tolerance")
            assert power >= 4.0
        for dtype in (F16, BF16):
            q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(dtype)
            for mode in ("flatten", "node"):
                out = _run8(mode, q, codes, md, None, vs).reshape(nq, Hq * D).to(torch.float64)
                assert bool(torch.isfinite(out).all()), (kind, mode, dtype)
                err = (out - expected).abs()
                if kind == "plain":
                    big = float(expected.abs().max())
                    if dtype == F16:
                        tol = torch.full_like(expected, 5e-4 * max(1.0, big))
                    else:
                        A = oracles.per_query_head(oracles.visible_mean(v64.abs(), paths), Hq, Hkv)
                        tol = bound_bf16(expected, A)
                else:
                    tol = oracles.tolerance(expected) if dtype == F16 else bf16_util.tolerance_bf16(expected)
                worst = float((err / tol).max())
                report(f"all codes {Hq}x{Hkv} {kind} {mode} {NAME[dtype]}: worst err {float(err.max()):.3e}  err/tol {worst:.3f}  largest |expected| "
                       f"{float(expected.abs().max()):.3e}")
                assert worst <= 1.0, (kind, mode, dtype, worst)
    # K holds every code; Q ~ N(0, sigma^2) with sigma chosen for a score deviation of 3.5 nats on the head with the largest k_scale
    kcode, dep = _code_pool(paths, size, Hkv, "plain")
    codes = torch.zeros((size, 2, Hkv, D), dtype=torch.uint8, device="cuda")
    codes[:, 0] = kcode.to("cuda")
    small = torch.tensor([0, 0.25, -0.25, 0.5, -0.5, 1, -1], dtype=F32, device="cuda")  # |v| v_scale <= 0.7: the 5e-4 tolerance is for outputs up to 1
    codes[:, 1] = small[torch.randint(0, small.numel(), (size, Hkv, D), device="cuda", generator=g)].to(FP8).view(torch.uint8)
    dead = (dep < 0).to("cuda")
    codes[dead] = 0x7F
    codes = codes.view(FP8)
    ks = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
    vs = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
    live = (~dead).nonzero().squeeze(1)
    k64 = torch.zeros((size, Hkv, D), dtype=torch.float64, device="cuda")
    v64 = torch.zeros_like(k64)
    as_bytes = codes.view(torch.uint8)  # (indexed as bytes)
    k64[live] = kv8_model.dequantize(as_bytes[live, 0].view(FP8), ks[:, None])
    v64[live] = kv8_model.dequantize(as_bytes[live, 1].view(FP8), vs[:, None])
    rms = float(values[_FINITE].pow(2).mean().sqrt())
    sigma = 3.5 / (rms * max(K_SCALES[:Hkv]))
    for dtype in (F16, BF16):
        q = (torch.randn((nq, Hq, D), device="cuda", generator=g) * sigma).to(dtype)
        idx = torch.as_tensor(paths, dtype=torch.int64, device="cuda")
        s = torch.einsum("rhgd,rnhd->rhgn", q.to(torch.float64).reshape(nq, Hkv, Hq // Hkv, D), k64[idx]) * D ** -0.5
        report(f"all codes in K {Hq}x{Hkv} {NAME[dtype]}: |k| up to {float(k64.abs().max()):.0f}, q sigma {sigma:.4f}, scores {float(s.min()):.1f} .. "
               f"{float(s.max()):.1f} nats")
        assert 8.0 < float(s.abs().max()) < 20.0
        for mode in ("flatten", "node"):
            _check(_run8(mode, q, codes, md, ks, vs), q, k64, v64, paths, Hq, Hkv, f"all codes in K {Hq}x{Hkv} {mode} {NAME[dtype]}")


# ---- 11. the softmax scale's edges through the Python operators ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_negative_and_zero_scale(geom, dtype):
    """tests/test_gpu_parity.py test_any_scale_through_the_c_abi for the kv8 kernel, through `scale=` of the Python operators and with
    per-head scales: the kernel applies |scale| k_scale inside the exp2 argument and negates the Q fragments for a negative scale, so
    attention(q, scale = -s) equals attention(-q, scale = +s) bit for bit (negating a 16-bit float is exact); scale = 0 gives every
    visible key weight 1: the mean of the visible V rows times v_scale, finite, within the visibility tolerance."""
    Hq, Hkv = geom
    tree, paths, md, size = _tree("a-300x5x140", Hkv)
    nq = len(paths)
    codes, g = _codes(size, Hkv, seed=43 + Hq)
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(dtype)
    ks = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
    vs = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
    values = torch.tensor([0, 0.25, -0.25, 0.5, -0.5, 1, -1, 1.5, -1.5, 2, -2, 3, -3], dtype=F32, device="cuda")
    v = values[torch.randint(0, values.numel(), (size, Hkv, D), device="cuda", generator=g)]
    uniform = codes.clone()
    uniform[:, 1] = v.to(FP8)  # (K stays random: a zero scale must silence it)
    v64 = v.to(torch.float64) * vs.to(torch.float64)[None, :, None]
    expected = oracles.per_query_head(oracles.visible_mean(v64, paths), Hq, Hkv)
    s = D ** -0.5
    for mode in ("flatten", "node"):
        neg = _run8(mode, q, codes, md, ks, vs, scale=-s)
        assert bool(torch.isfinite(neg).all()) and _same_bits(neg, _run8(mode, -q, codes, md, ks, vs, scale=s)), (mode, "scale = -s")
        assert not _same_bits(neg, _run8(mode, q, codes, md, ks, vs, scale=s))  # (the sign did something)
        out = _run8(mode, q, uniform, md, ks, vs, scale=0.0).reshape(nq, Hq * D)
        assert bool(torch.isfinite(out).all()), (mode, "scale = 0")
        err = (out.to(torch.float64) - expected).abs()
        tol = oracles.tolerance(expected) if dtype == F16 else bf16_util.tolerance_bf16(expected)
        worst = float((err / tol).max())
        report(f"scale 0 {Hq}x{Hkv} {mode} {NAME[dtype]}: worst |out - visible mean x v_scale| {float(err.max()):.3e}  err/tol {worst:.3f}")
        assert worst <= 1.0, (mode, worst)


# ---- 12. a head stride other than D ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_padded_head_stride(dtype):
    """The pool as a [size, 2, Hkv, D] view of a [size, 2, Hkv, D + 16] byte buffer (head stride 144: `a multiple of 16`, which the host
    accepts), every pad byte 0x7F -- a NaN code, should anything read it.  The kernel steps heads by kvh * kv_sh bytes, the append by
    hd * kv_sh: the append writes the codes a dense pool gets and no pad byte, the decode's output is the dense pool's bit for bit."""
    Hq, Hkv = 8, 2
    tree, paths, md, size = _tree("a-300x5x140", Hkv)
    nq = len(paths)
    g = torch.Generator(device="cuda").manual_seed(144)
    ks = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
    vs = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
    buf = torch.full((size, 2, Hkv, D + 16), 0x7F, dtype=torch.uint8, device="cuda")
    padded = buf[..., :D].view(FP8)
    assert padded.shape == (size, 2, Hkv, D) and padded.stride() == (2 * Hkv * (D + 16), Hkv * (D + 16), D + 16, 1)
    dense = torch.full((size, 2, Hkv, D), 0x7F, dtype=torch.uint8, device="cuda").view(FP8)
    loc = torch.randperm(size, device="cuda", generator=g).to(torch.int32)  # every slot, in a scrambled order
    k_new = torch.randn((size, Hkv * D), device="cuda", generator=g).to(dtype)
    v_new = torch.randn((size, Hkv * D), device="cuda", generator=g).to(dtype)
    deft_amd.kv_append_kv8(padded, loc, k_new, v_new, ks, vs)
    deft_amd.kv_append_kv8(dense, loc, k_new, v_new, ks, vs)
    torch.cuda.synchronize()
    assert bool((buf[..., D:] == 0x7F).all()), "the append wrote a pad byte"
    assert torch.equal(buf[..., :D], dense.view(torch.uint8))
    li = loc.long().cpu()
    want_k = kv8_model.quantize(k_new.reshape(size, Hkv, D).cpu(), ks.cpu()[:, None])
    assert kv8_model.same_codes(buf[..., :D].cpu()[li, 0].view(FP8), want_k)
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(dtype)
    for mode in ("flatten", "node"):
        ref = _run8(mode, q, dense, md, ks, vs)
        out = _run8(mode, q, padded, md, ks, vs)
        assert bool(torch.isfinite(out).all()) and _same_bits(out, ref), (mode, "padded head stride")
    _check(out, q, kv8_model.dequantize(dense[:, 0], ks[:, None]), kv8_model.dequantize(dense[:, 1], vs[:, None]), paths, Hq, Hkv,
           f"padded head stride 8x2 node {NAME[dtype]}")


# ---- 13. the append and the decode captured in one graph ----------------------------------------------------------------------------------
def test_append_and_decode_captured_in_one_graph():
    """The scales are device pointers (no host read, no sync), which is what makes kv_append_kv8 followed by the kv8 decode capturable: a
    linear chain of launches on a side stream under torch.cuda.graph.  Replayed twice with new contents in q / k_new / v_new, each replay
    equals the eager pair bit for bit; with the CONTENTS of v_scale overwritten between replays the output follows them."""
    Hq, Hkv = 8, 2
    tree, paths, md, size = _tree("a-300x5x140", Hkv)
    nq = len(paths)
    base, g = _codes(size, Hkv, seed=97)
    loc = torch.tensor([p[-1] for p in paths], dtype=torch.int32, device="cuda")
    ks = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
    vs = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
    kv = base.clone()
    q = torch.zeros((nq, Hq, D), dtype=F16, device="cuda")
    k_new = torch.zeros((nq, Hkv * D), dtype=F16, device="cuda")
    v_new = torch.zeros((nq, Hkv * D), dtype=F16, device="cuda")
    out = torch.zeros_like(q)

    def pair(kv_, q_, k_, v_, out_, vs_):
        deft_amd.kv_append_kv8(kv_, loc, k_, v_, ks, vs_)
        deft_amd.tree_attention_subtree_fwd_kv8(q_, kv_[:, 0], kv_[:, 1], out_, *_flat(md), k_scale=ks, v_scale=vs_)

    def fill():
        return (torch.randn((nq, Hq, D), device="cuda", generator=g).to(F16), torch.randn((nq, Hkv * D), device="cuda", generator=g).to(F16),
                torch.randn((nq, Hkv * D), device="cuda", generator=g).to(F16))

    def eager(qq, kk, vv, vs_):
        kv_e, out_e = base.clone(), torch.full_like(q, float("nan"))
        pair(kv_e, qq, kk, vv, out_e, vs_)
        torch.cuda.synchronize()
        return kv_e, out_e

    eager(*fill(), vs)  # (the plan of this metadata is built and cached before the capture)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            pair(kv, q, k_new, v_new, out, vs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    vs_values = vs.clone()
    for replay in range(3):
        qq, kk, vv = fill()
        q.copy_(qq)
        k_new.copy_(kk)
        v_new.copy_(vv)
        if replay == 2:  # new CONTENTS in the same scale tensor: the third replay must follow them
            vs.copy_(vs_values * torch.tensor([1.7, 0.6], dtype=F32, device="cuda"))
        kv.copy_(base)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        kv_e, out_e = eager(qq, kk, vv, vs.clone())
        assert torch.equal(kv.view(torch.uint8), kv_e.view(torch.uint8)), (replay, "the appended rows")
        assert bool(torch.isfinite(out).all()) and _same_bits(out, out_e), (replay, "the decode's output")
        if replay == 2:
            stale = eager(qq, kk, vv, vs_values)[1]
            assert not _same_bits(out, stale), "the replay used the scales it was captured with"
    report(f"graph: append + flatten decode 8x2 fp16 captured once, 3 replays equal the eager pair bit for bit (one after v_scale's contents changed)")
