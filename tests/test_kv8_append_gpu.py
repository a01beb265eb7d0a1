"""The fused quantising append over fp8 KV pools on the GPU: deft_*_decode_append_*_kv8 against deft_kv_append_*_kv8
followed by deft_*_decode_*_kv8, BIT FOR BIT -- outputs, lse and every byte of the pool -- which is the contract: the codes that reach
the MFMA are the codes the pool receives.  A step is made as tests/test_bf16_identities.py makes it (the last slot of every leaf is this
step's new row) and the pool is restored between the two arms.  Shapes put the new row into each of the four waves' 32-key ranges, at the
first and the last position of a tile and into a tile that holds nothing else; many new rows into one tile; more new rows than
workgroups; a padded head stride; one layer in a captured graph; the module.  One case per element type stands against fp64 truth over
the dequantised pool at the 16-bit tolerance, so the file does not rest on the two-launch path alone.

Every figure is printed before it is asserted (`pytest -s`)."""
import pytest
import torch

import deft_amd
import kv8_model
import oracles
from tools.error_bound import bound_bf16, dense_attention
from truth import product_leaf_paths, tree_truth

pytestmark = pytest.mark.gpu
FP8, F16, BF16, F32 = torch.float8_e4m3fn, torch.float16, torch.bfloat16, torch.float32
NAME = {F16: "fp16", BF16: "bf16"}
D = 128
GEOMS = [(4, 4), (8, 2), (3, 3)]
# per-head scales, none a power of two (tests/test_kv8_gpu.py)
K_SCALES = [0.73, 1.9, 1.21, 0.57]
V_SCALES = [0.61, 0.7, 0.37, 0.53]
_TREES = {}


def report(line):
    print("[kv8-append] " + line, flush=True)


def _tree(prefix, width, branch_len, Hkv):
    """(tree, paths, metadata, pool size, cache_loc) of a few-shot tree, built once per shape and head count; cache_loc = the last slot of
    every leaf, in the order of the query rows."""
    key = (prefix, width, branch_len, Hkv)
    if key not in _TREES:
        tree, pool, _ = oracles.few_shot_tree(prefix, width, branch_len, Hkv, D)
        paths = product_leaf_paths(tree)
        loc = torch.tensor([p[-1] for p in paths], dtype=torch.int32, device="cuda")
        assert len(set(loc.tolist())) == len(paths)
        _TREES[key] = (tree, paths, deft_amd.TreeMetadata.from_tree_cache(tree), pool.size, loc)
    return _TREES[key]


def _codes(size, Hkv, g):
    """One layer of an fp8 pool, [size, 2, Hkv, D]: N(0, 1) quantised with unit scales (tests/kv8_model.py)."""
    return kv8_model.quantize(torch.randn((size, 2, Hkv, D), device="cuda", generator=g).to(F16), 1.0)


def _flat(md):
    return (md.block_len, md.block_q, md.block_q_cnts, md.block_q_offset, md.block_bitmasks, md.block_kv, md.block_lens)


def _nodes(md):
    return (md.node_kv, md.node_kv_offset, md.node_kv_len, md.node_q, md.node_q_offset, md.node_q_len)


def _two_launches(mode, q, kv, md, loc, k_new, v_new, ks=None, vs=None, with_lse=False):
    """deft_kv_append_*_kv8, then the kv8 operator: the parent's path.  Returns (out, lse or None)."""
    deft_amd.kv_append_kv8(kv, loc, k_new, v_new, ks, vs)
    kb, vb = kv[:, 0], kv[:, 1]
    out = torch.full_like(q, float("nan"))
    lse = torch.full(q.shape[:2], 777.0, dtype=F32, device="cuda") if with_lse else None
    kw = dict(k_scale=ks, v_scale=vs)
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
    return out, lse


def _fused(mode, q, kv, md, loc, k_new, v_new, ks=None, vs=None, with_lse=False, sync=True, out=None):
    out = torch.full_like(q, float("nan")) if out is None else out
    lse = torch.full(q.shape[:2], 777.0, dtype=F32, device="cuda") if with_lse else None
    kw = dict(k_scale=ks, v_scale=vs)
    if mode == "flatten":
        if with_lse:
            deft_amd.flatten_append_attention_kv8_lse(q, kv, out, lse, loc, k_new, v_new, *_flat(md), **kw)
        else:
            deft_amd.flatten_append_attention_kv8(q, kv, out, loc, k_new, v_new, *_flat(md), **kw)
    else:
        if with_lse:
            deft_amd.node_append_attention_kv8_lse(q, kv, out, lse, loc, k_new, v_new, *_nodes(md), **kw)
        else:
            deft_amd.node_append_attention_kv8(q, kv, out, loc, k_new, v_new, *_nodes(md), **kw)
    if sync:
        torch.cuda.synchronize()
    return out, lse


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _assert_identical(tag, base, mode, q, md, loc, k_new, v_new, ks, vs, with_lse):
    """Both arms from the same pool bytes; outputs, lse and all pool bytes compared as bits."""
    kv_two, kv_fused = base.clone(), base.clone()
    o_two, l_two = _two_launches(mode, q, kv_two, md, loc, k_new, v_new, ks, vs, with_lse)
    o_fused, l_fused = _fused(mode, q, kv_fused, md, loc, k_new, v_new, ks, vs, with_lse)
    assert not torch.equal(kv_two.view(torch.uint8), base.view(torch.uint8)), (tag, "the append changed nothing")
    assert torch.equal(kv_fused.view(torch.uint8), kv_two.view(torch.uint8)), (tag, "pool bytes")
    assert bool(torch.isfinite(o_two).all()), (tag, "two-launch output")
    assert _same_bits(o_fused, o_two), (tag, "output", float((o_fused.float() - o_two.float()).abs().max()))
    if with_lse:
        assert bool(torch.isfinite(l_two).all()) and _same_bits(l_fused, l_two), (tag, "lse")
    return o_fused


def _scales(Hkv, which):
    if which == "null":
        return None, None
    return torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda"), torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")


# ---- 1. fused against append-then-decode, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("branch_len", [1, 33, 70, 128, 129])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_fused_equals_append_then_decode(dtype, geom, branch_len):
    """few_shot_tree(300, 5, L): in Node mode a leaf's entry holds its L tokens from position 0, so the new row is key L - 1 of the
    entry -- wave 0 alone in its tile (L = 1), wave 1 (33), wave 2 (70), the last key of a full tile (128, wave 3) and the first key of a
    tile that holds nothing else (129); in Flatten mode the leaves' tokens follow the prefix's remainder inside the blocks, which moves the
    row to other positions again."""
    Hq, Hkv = geom
    tree, paths, md, size, loc = _tree(300, 5, branch_len, Hkv)
    nq = len(paths)
    g = torch.Generator(device="cuda").manual_seed(1000 * branch_len + 10 * Hq + (dtype == BF16))
    base = _codes(size, Hkv, g)
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(dtype)
    k_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
    v_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
    for mode in ("flatten", "node"):
        for which in ("per-head", "null"):
            ks, vs = _scales(Hkv, which)
            for with_lse in (False, True):
                tag = f"L={branch_len} {Hq}x{Hkv} {NAME[dtype]} {mode} {which} scales lse={with_lse}"
                _assert_identical(tag, base, mode, q, md, loc, k_new, v_new, ks, vs, with_lse)


# ---- 2. many new rows in one tile ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("geom", [(8, 2), (3, 3)], ids=lambda g: "x".join(map(str, g)))
def test_many_new_rows_in_one_tile(geom, dtype):
    """40 leaves of one token under a 200-token prefix: the Flatten split packs the leaves' tokens into one block -- several flagged rows
    per DMA instruction, more than 32 queries (two passes over the tile)."""
    Hq, Hkv = geom
    tree, paths, md, size, loc = _tree(200, 40, 1, Hkv)
    nq = len(paths)
    assert nq == 40
    kv_of_block = md.block_kv.reshape(-1, 128)
    new = set(loc.tolist())
    most = max(sum(int(s) in new for s in row.tolist()) for row in kv_of_block)
    report(f"200x40x1 {Hq}x{Hkv}: {kv_of_block.shape[0]} Flatten blocks, the fullest holds {most} of this step's rows")
    assert most >= 9, most  # (a DMA instruction moves eight rows: at least one carries two flagged ones)
    g = torch.Generator(device="cuda").manual_seed(40 + Hq + (dtype == BF16))
    base = _codes(size, Hkv, g)
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(dtype)
    k_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
    v_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
    ks, vs = _scales(Hkv, "per-head")
    for mode in ("flatten", "node"):
        _assert_identical(f"200x40x1 {Hq}x{Hkv} {NAME[dtype]} {mode}", base, mode, q, md, loc, k_new, v_new, ks, vs, True)


# ---- 3. more new rows than workgroups -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_more_new_rows_than_workgroups(dtype):
    """A one-token chain (nq = 1), Hkv = 3: a grid of a few workgroups.  200 new rows, of which the chain's own is one; the others go to
    free slots and carry kv8_model.edge_inputs() (beyond +-448, subnormals, NaN, +-0).  Workgroup W - 1 - b copies rows W - 1 - b, + W, ...:
    with 200 rows every workgroup walks the + W stride many times.  cache_loc / n_new never depended on nq."""
    Hq, Hkv, n_new, own = 3, 3, 200, 137
    req = deft_amd.ReqToTokenPool(8, 72, device="cuda")
    pool = deft_amd.TokenToKVPool(256, F16, Hkv, D, 1, device="cuda")
    tree = deft_amd.TreeCache(F16, Hkv, D, 1, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, 2, dtype=torch.int32))
    paths = product_leaf_paths(tree)
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    assert len(paths) == 1 and len(paths[0]) == 1
    slot = int(paths[0][0])
    free = [s for s in range(pool.size) if s != slot]
    g = torch.Generator(device="cuda").manual_seed(200 + (dtype == BF16))
    order = torch.randperm(len(free), generator=torch.Generator().manual_seed(3))[: n_new - 1].tolist()
    slots = [free[i] for i in order]
    slots.insert(own, slot)
    loc = torch.tensor(slots, dtype=torch.int32, device="cuda")
    assert loc.shape[0] == n_new and len(set(slots)) == n_new
    edge = kv8_model.edge_inputs().to("cuda")
    x = torch.randn((2, n_new, Hkv, D), device="cuda", generator=g) * 100.0
    for t in range(2):
        for h in range(Hkv):
            flat = x[t, :, h].reshape(-1).clone()
            at = (own + 1) * D  # (behind the chain's own row)
            flat[at : at + edge.numel()] = edge
            x[t, :, h] = flat.reshape(n_new, D)
    x[:, own] = torch.randn((2, Hkv, D), device="cuda", generator=g)  # the row the attention reads: ordinary values
    k_new, v_new = x[0].to(dtype).reshape(n_new, Hkv * D), x[1].to(dtype).reshape(n_new, Hkv * D)
    assert bool(torch.isnan(k_new).any()) and bool((k_new.float().abs() > 448).any()) and not bool(torch.isnan(k_new[own]).any())
    base = _codes(pool.size, Hkv, g)
    q = torch.randn((1, Hq, D), device="cuda", generator=g).to(dtype)
    ks = torch.tensor([1.0, 0.5, 0.0371], dtype=F32, device="cuda")
    vs = torch.tensor([0.0371, 1.0, 0.5], dtype=F32, device="cuda")
    for mode in ("flatten", "node"):
        _assert_identical(f"chain1 200 new rows {NAME[dtype]} {mode}", base, mode, q, md, loc, k_new, v_new, ks, vs, True)
    # ... and the bytes both arms agree on are the model's (tests/kv8_model.py), NaN codes, clamped and subnormal ones included
    kv = base.clone()
    _fused("flatten", q, kv, md, loc, k_new, v_new, ks, vs)
    rows = kv.view(torch.uint8).cpu()[torch.tensor(slots)]
    assert kv8_model.same_codes(rows[:, 0].view(FP8), kv8_model.quantize(k_new.reshape(n_new, Hkv, D).cpu(), ks.cpu()[:, None]))
    assert kv8_model.same_codes(rows[:, 1].view(FP8), kv8_model.quantize(v_new.reshape(n_new, Hkv, D).cpu(), vs.cpu()[:, None]))
    assert bool(kv8_model.is_nan_code(rows[:, 0].view(FP8)).any())
    untouched = torch.ones(pool.size, dtype=torch.bool)
    untouched[torch.tensor(slots)] = False
    assert torch.equal(kv.view(torch.uint8).cpu()[untouched], base.view(torch.uint8).cpu()[untouched])


# ---- 4. a head stride other than D ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_padded_head_stride(dtype):
    """The pool as a [size, 2, Hkv, D] view of a [size, 2, Hkv, D + 16] byte buffer (head stride 144), every pad byte 0x7F: the fused call
    gives the dense pool's results bit for bit and writes no pad byte."""
    Hq, Hkv = 8, 2
    tree, paths, md, size, loc = _tree(300, 5, 70, Hkv)
    nq = len(paths)
    g = torch.Generator(device="cuda").manual_seed(144 + (dtype == BF16))
    dense = _codes(size, Hkv, g)
    buf = torch.full((size, 2, Hkv, D + 16), 0x7F, dtype=torch.uint8, device="cuda")
    buf[..., :D] = dense.view(torch.uint8)
    padded = buf[..., :D].view(FP8)
    assert padded.stride() == (2 * Hkv * (D + 16), Hkv * (D + 16), D + 16, 1)
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(dtype)
    k_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
    v_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
    ks, vs = _scales(Hkv, "per-head")
    for mode in ("flatten", "node"):
        kv_d = dense.clone()
        o_d, l_d = _fused(mode, q, kv_d, md, loc, k_new, v_new, ks, vs, True)
        b2 = buf.clone()
        kv_p = b2[..., :D].view(FP8)
        o_p, l_p = _fused(mode, q, kv_p, md, loc, k_new, v_new, ks, vs, True)
        assert bool(torch.isfinite(o_p).all()) and _same_bits(o_p, o_d) and _same_bits(l_p, l_d), mode
        assert bool((b2[..., D:] == 0x7F).all()), "the fused append wrote a pad byte"
        assert torch.equal(b2[..., :D], kv_d.view(torch.uint8)), mode
        o_two, _ = _two_launches(mode, q, dense.clone(), md, loc, k_new, v_new, ks, vs)
        assert _same_bits(o_p, o_two), mode


# ---- 5. one fused layer in a captured graph ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flatten", "node"])
def test_one_fused_layer_in_a_captured_graph(mode):
    """One fused call captured under torch.cuda.graph; replayed twice with new contents in q / k_new / v_new / v_scale, each replay equals
    the eager two-launch pair bit for bit (the scales and the new rows are read on the device)."""
    Hq, Hkv = 8, 2
    tree, paths, md, size, loc = _tree(300, 5, 70, Hkv)
    nq = len(paths)
    g = torch.Generator(device="cuda").manual_seed(97)
    base = _codes(size, Hkv, g)
    ks, vs = _scales(Hkv, "per-head")
    vs_values = vs.clone()
    kv = base.clone()
    q = torch.zeros((nq, Hq, D), dtype=F16, device="cuda")
    k_new = torch.zeros((nq, Hkv * D), dtype=F16, device="cuda")
    v_new = torch.zeros((nq, Hkv * D), dtype=F16, device="cuda")
    out = torch.zeros_like(q)

    def fill():
        return (torch.randn((nq, Hq, D), device="cuda", generator=g).to(F16), torch.randn((nq, Hkv * D), device="cuda", generator=g).to(F16),
                torch.randn((nq, Hkv * D), device="cuda", generator=g).to(F16))

    _fused(mode, q, base.clone(), md, loc, k_new, v_new, ks, vs)  # (the plan of this metadata and cache_loc is built and cached before the capture)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _fused(mode, q, kv, md, loc, k_new, v_new, ks, vs, sync=False, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for replay in range(2):
        qq, kk, vv = fill()
        q.copy_(qq)
        k_new.copy_(kk)
        v_new.copy_(vv)
        vs.copy_(vs_values * torch.tensor([1.7, 0.6] if replay else [0.9, 1.3], dtype=F32, device="cuda"))
        kv.copy_(base)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        kv_e = base.clone()
        out_e, _ = _two_launches(mode, qq, kv_e, md, loc, kk, vv, ks, vs.clone())
        assert torch.equal(kv.view(torch.uint8), kv_e.view(torch.uint8)), (replay, "the appended rows")
        assert bool(torch.isfinite(out).all()) and _same_bits(out, out_e), (replay, "the output")
        stale, _ = _two_launches(mode, qq, base.clone(), md, loc, kk, vv, ks, vs_values)
        assert not _same_bits(out, stale), "the replay used the scales it was captured with"


# ---- 6. the module -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_module_forward_equals_the_operator_call(dtype):
    """DeFTAttention.forward over an fp8 pool (TREE_DECODE_FLATTEN, TREE_DECODE_NODE) against the fused operator call on the same step:
    output and pool bytes, bit for bit."""
    Hq, Hkv = 8, 2
    prefix, width, branch_len = 300, 5, 33
    size = prefix + width * (branch_len + 2) + 64
    req = deft_amd.ReqToTokenPool(72, size + 8, device="cuda")
    pool = deft_amd.TokenToKVPool(size, FP8, Hkv, D, 1, device="cuda")
    tree = deft_amd.TreeCache(dtype, Hkv, D, 1, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, prefix + 1, dtype=torch.int32))
    tree.branch(tree.root, width)
    for _ in range(branch_len):
        for leaf in list(tree.leaves.values()):
            leaf.append_token(7)
        tree.alloc()
    g = torch.Generator(device="cuda").manual_seed(33 + (dtype == BF16))
    base = _codes(size, Hkv, g)
    ks, vs = _scales(Hkv, "per-head")
    pool.set_kv_scales(0, ks, vs)
    paths = product_leaf_paths(tree)
    nq = len(paths)
    loc = torch.tensor([p[-1] for p in paths], dtype=torch.int32, device="cuda")
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    q = torch.randn((nq, Hq * D), device="cuda", generator=g).to(dtype)
    k_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
    v_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
    for mode in ("flatten", "node"):
        pool._storage[0].copy_(base)
        o_module = oracles.eager_step(tree, pool, mode, Hq, Hkv, D, q, k_new, v_new)
        pool_module = pool._storage[0].clone()
        kv = base.clone()
        o_op, _ = _fused(mode, q.view(nq, Hq, D), kv, md, loc, k_new, v_new, ks, vs)
        assert o_module.dtype == dtype and bool(torch.isfinite(o_op).all())
        assert _same_bits(o_module.view(nq, Hq, D), o_op), mode
        assert torch.equal(pool_module.view(torch.uint8), kv.view(torch.uint8)), mode
        assert not torch.equal(kv.view(torch.uint8), base.view(torch.uint8))


# ---- 7. against fp64 truth over the dequantised pool -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_fused_call_against_truth_of_the_dequantised_pool(dtype):
    """The fused call alone: its output against fp64 attention over the pool it leaves behind, dequantised with the scales -- the new rows
    are in it, as the model's codes (kv8_model.quantize) -- at the tolerance of the 16-bit operators: fp16 5e-4 per element, bf16
    tools.error_bound.bound_bf16.  The shape, scales and tolerance of tests/test_kv8_gpu.py test_scales."""
    Hq, Hkv = 8, 2
    tree, paths, md, size, loc = _tree(300, 5, 140, Hkv)
    nq = len(paths)
    g = torch.Generator(device="cuda").manual_seed(31 + Hq)
    base = _codes(size, Hkv, g)
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(dtype)
    k_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
    v_new = torch.randn((nq, Hkv * D), device="cuda", generator=g).to(dtype)
    ks, vs = _scales(Hkv, "per-head")
    want_k = kv8_model.quantize(k_new.reshape(nq, Hkv, D).cpu(), ks.cpu()[:, None])
    want_v = kv8_model.quantize(v_new.reshape(nq, Hkv, D).cpu(), vs.cpu()[:, None])
    for mode in ("flatten", "node"):
        kv = base.clone()
        out, _ = _fused(mode, q, kv, md, loc, k_new, v_new, ks, vs)
        rows = kv.view(torch.uint8).cpu()[loc.cpu().long()]
        assert kv8_model.same_codes(rows[:, 0].view(FP8), want_k) and kv8_model.same_codes(rows[:, 1].view(FP8), want_v), mode
        k64 = kv8_model.dequantize(kv[:, 0], ks[:, None])
        v64 = kv8_model.dequantize(kv[:, 1], vs[:, None])
        truth, A = dense_attention(q, k64, v64, paths, Hq, Hkv, D ** -0.5, with_abs=True)
        assert float((truth - tree_truth(q, k64, v64, paths, Hq, Hkv, D ** -0.5)).abs().max()) < 1e-12
        got = out.reshape(truth.shape).to(torch.float64)
        assert bool(torch.isfinite(got).all()), mode
        err = (got - truth).abs()
        tol = torch.full_like(truth, 5e-4) if dtype == F16 else bound_bf16(truth, A)
        worst = float((err / tol).max())
        report(f"fused {Hq}x{Hkv} {mode} {NAME[dtype]} against fp64 truth: worst err {float(err.max()):.3e}  err/tol {worst:.3f}  largest |output| "
               f"{float(truth.abs().max()):.2f}  ({truth.numel()} elements)")
        assert worst <= 1.0, (mode, worst)
