"""Attention states on the GPU (deft_amd/states.py): the log-sum-exp the *_lse operators return, the merge of two states, and the two
compositions the feature is for -- a tree split over two calls, and a prefill onto a cached prefix.

  * exact form: K = 0 on every slot, so every score is 0 and row r's lse is ln(len(path_r)); n and L are exact integers in fp32 and only
    the hardware log's error remains: 4e-6 max(1, ln n).  One case per site that finishes a row.  Outputs bit-identical to the plain
    entry point's (same kernels, one more store).
  * random form: |lse - fp64| <= u + 2e-5 (stage 1 sums the probabilities AFTER rounding them to the element type, DESIGN section 5: L is
    off by at most a relative u, log(1 + u) <= u; 2e-5 is the fp32 slack of tests/bf16_util.py).
  * prefill: 2e-5 + 4e-6 |lse| (the prefill kernel sums unrounded exponentials: no u term).
  * merge: one rounding of an fp32 convex combination, u |o| + 1e-6; the identities bit for bit.
  * compositions, per element, A_e = sum_i p_i |v_ie|: fp16 5e-4 + 2^-11 (A_e + |o_e|); bf16 bound_bf16(o, A) + 2^-8 (A_e + |o_e|) -- the
    single call's tolerance, one more rounding of each part (<= u A_e), one of the result (u |o_e|).  The single full call is held to
    its own tolerance on the same inputs first, so that a failure of the composed form is the new code's.

Every figure is printed before it is asserted (`pytest -s`; profiles/states_error.txt is made of those lines)."""
import math

import numpy as np
import pytest
import torch

import bf16_util
import deft_amd
import oracles
from deft_amd.tree_attention import flatten_append_attention, node_append_attention
from scenarios import SCENARIOS
from states_model import causal_lse, merge_model, path_lse
from tools.error_bound import bound_bf16, dense_attention
from truth import product_leaf_paths, tree_truth

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
NAME = {F16: "fp16", BF16: "bf16"}
NINF = float("-inf")


def report(line):
    print("[states] " + line, flush=True)


def _scenario_tree(name, Hkv, D, dtype=F16):
    sc = SCENARIOS[name]
    req = deft_amd.ReqToTokenPool(128, sc.pool_size + 8, device="cuda")
    pool = deft_amd.TokenToKVPool(sc.pool_size, dtype, Hkv, D, 1, device="cuda")
    tree = deft_amd.TreeCache(dtype, Hkv, D, 1, req, pool, None, True, False)
    sc.script(tree, lambda n: torch.arange(1, n + 1, dtype=torch.int32))
    return tree, pool


def _flat(md):
    return (md.block_len, md.block_q, md.block_q_cnts, md.block_q_offset, md.block_bitmasks, md.block_kv, md.block_lens)


def _nodes(md):
    return (md.node_kv, md.node_kv_offset, md.node_kv_len, md.node_q, md.node_q_offset, md.node_q_len)


def _run(mode, q, pool, md, with_lse):
    """One operator call on layer 0: (out, lse or None); out NaN-filled and lse filled with 777 beforehand (every row must be written)."""
    kb, vb = pool.get_key_buffer(0), pool.get_value_buffer(0)
    out = torch.full_like(q, float("nan"))
    lse = torch.full(q.shape[:2], 777.0, dtype=F32, device="cuda") if with_lse else None
    if mode == "flatten":
        if with_lse:
            deft_amd.tree_attention_subtree_fwd_lse(q, kb, vb, out, lse, *_flat(md))
        else:
            deft_amd.tree_attention_subtree_fwd(q, kb, vb, out, *_flat(md))
    else:
        if with_lse:
            deft_amd.tree_attention_fwd_lse(q, kb, vb, out, lse, *_nodes(md))
        else:
            deft_amd.tree_attention_fwd(q, kb, vb, out, *_nodes(md))
    torch.cuda.synchronize()
    return out, lse


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _visibility(pool, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dtype == F16:
        oracles.visibility_pool(pool, g)
    else:
        bf16_util.visibility_pool_bf16(pool, g)
    return g


def _check_log_len(lse, paths, tag):
    want = torch.tensor([math.log(len(p)) for p in paths], dtype=torch.float64, device="cuda")[:, None]
    tol = 4e-6 * want.clamp_min(1.0)
    err = (lse.to(torch.float64) - want).abs()
    report(f"exact {tag}: worst |lse - ln n| {float(err.max()):.3e}  err/tol {float((err / tol).max()):.3f}  (n up to {max(len(p) for p in paths)})")
    assert bool(torch.isfinite(lse).all()) and bool((err <= tol).all()), (tag, float(err.max()))


# ---- LSE of the decode operators, exact form: one case per store site --------------------------------------------------------------
EXACT = [
    # id, tree, (Hq, Hkv, D), modes, dtypes
    ("cfgA-coop-small", "cfgA_256x2", (8, 2, 128), ("flatten", "node"), (F16, BF16)),   # merge_coop_kernel, n <= 8: wave 0 alone
    ("wide40-inline", "wide40", (8, 2, 128), ("flatten", "node"), (F16, BF16)),          # merge_kernel, inline lists (more than 16 queries)
    ("cfgA-d64-pairs", "cfgA_256x2", (4, 4, 64), ("flatten", "node"), (F16,)),            # head_dim 64, two KV heads per pool row
    ("multilevel-d32-scan", "multilevel", (4, 4, 32), ("flatten",), (F16,)),              # stage1_kernel, merge without a plan: the scan
]


@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_lse_is_the_log_of_the_path_length(case):
    tag, name, (Hq, Hkv, D), modes, dtypes = case
    for dtype in dtypes:
        tree, pool = _scenario_tree(name, Hkv, D, dtype)
        g = _visibility(pool, dtype, Hq * D)
        paths = product_leaf_paths(tree)
        md = deft_amd.TreeMetadata.from_tree_cache(tree)
        q = torch.randn((len(paths), Hq, D), device="cuda", generator=g).to(dtype)
        for mode in modes:
            plain, _ = _run(mode, q, pool, md, False)
            out, lse = _run(mode, q, pool, md, True)
            assert _same_bits(out, plain), (tag, mode, "out differs from the plain entry point's")
            _check_log_len(lse, paths, f"{tag} {mode} {NAME[dtype]}")


def test_lse_through_the_four_wave_combine():
    """test_sharp_softmax's 32kx8-coop shape: every query's row list is longer than 8, so merge_coop_kernel's four waves each fold a
    quarter and wave 0 combines -- and stores the lse there."""
    Hq, Hkv, D = 8, 2, 128
    tree, pool, _ = oracles.few_shot_tree(32768, 8, 3, Hkv, D)
    g = _visibility(pool, F16, 32768)
    paths = product_leaf_paths(tree)
    nq = len(paths)
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    lead = oracles.flatten_leaders(md, pool, Hq, Hkv, D)
    rows_per_query = sum(1 for rows, _ in lead if rows == min(32, nq * (Hq // Hkv)))  # (chunks whose rows hold every query)
    assert nq <= 16 and rows_per_query > 8, (nq, rows_per_query)
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(F16)
    plain, _ = _run("flatten", q, pool, md, False)
    out, lse = _run("flatten", q, pool, md, True)
    assert _same_bits(out, plain)
    _check_log_len(lse, paths, f"32kx8 four-wave combine flatten fp16 ({rows_per_query}+ rows per query)")


@pytest.mark.parametrize("mode", ["flatten", "node"])
def test_lse_of_the_fused_append_twins(mode):
    """A step's new rows on s_cfgA: every leaf's last slot takes k_new (= 0) / v_new through the fused append; out equals the plain
    fused-append call's bit for bit, the pool holds the rows, and lse = ln(len(path)) with the new row counted."""
    Hq, Hkv, D = 8, 2, 128
    tree, pool = _scenario_tree("cfgA_256x2", Hkv, D)
    g = _visibility(pool, F16, 5)
    paths = product_leaf_paths(tree)
    nq = len(paths)
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(F16)
    loc = torch.tensor([p[-1] for p in paths], dtype=torch.int32, device="cuda")
    k_new = torch.zeros((nq, Hkv * D), dtype=F16, device="cuda")
    v_new = oracles.dyadic_(torch.empty((nq, Hkv * D), dtype=F16, device="cuda"), g)
    kv = pool.kv_data[0]
    kv[loc.long(), 0] = 1.0  # (stale rows the append must overwrite: left in place they would change every lse)
    args = _flat(md) if mode == "flatten" else _nodes(md)
    plain_fn, lse_fn = ((flatten_append_attention, deft_amd.flatten_append_attention_lse) if mode == "flatten" else
                        (node_append_attention, deft_amd.node_append_attention_lse))
    plain = torch.full_like(q, float("nan"))
    plain_fn(q, kv, plain, loc, k_new, v_new, *args)
    kv[loc.long(), 0] = 1.0
    out = torch.full_like(q, float("nan"))
    lse = torch.full((nq, Hq), 777.0, dtype=F32, device="cuda")
    lse_fn(q, kv, out, lse, loc, k_new, v_new, *args)
    torch.cuda.synchronize()
    assert _same_bits(out, plain)
    assert torch.equal(kv[loc.long(), 0].reshape(nq, -1), k_new) and torch.equal(kv[loc.long(), 1].reshape(nq, -1), v_new)
    _check_log_len(lse, paths, f"cfgA fused append {mode} fp16")


# ---- LSE of the decode operators, random form --------------------------------------------------------------------------------------
def _randn_pool(pool, g):
    st = pool._storage
    st.copy_(torch.randn(st.shape, device="cuda", generator=g).to(st.dtype))


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", ["multilevel", "cfgA_256x2"])
def test_lse_of_random_inputs(name, dtype):
    Hq, Hkv, D = 8, 2, 128
    tree, pool = _scenario_tree(name, Hkv, D, dtype)
    g = torch.Generator(device="cuda").manual_seed(len(name))
    _randn_pool(pool, g)
    paths = product_leaf_paths(tree)
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    q = torch.randn((len(paths), Hq, D), device="cuda", generator=g).to(dtype)
    want = path_lse(q, pool.get_key_buffer(0), paths, Hq, Hkv, D ** -0.5)
    tol = U[dtype] + 2e-5
    for mode in ("flatten", "node"):
        plain, _ = _run(mode, q, pool, md, False)
        out, lse = _run(mode, q, pool, md, True)
        assert _same_bits(out, plain)
        err = float((lse.to(torch.float64) - want).abs().max())
        report(f"random {name} {mode} {NAME[dtype]}: worst |lse - fp64| {err:.3e}  err/tol {err / tol:.3f}")
        assert err <= tol, (name, mode, err)


# ---- prefill LSE ---------------------------------------------------------------------------------------------------------------------
PREFILL = [([1], (4, 4, 128), False), ([255, 256, 257], (8, 2, 128), False), ([255, 256, 257], (8, 2, 64), False),
           ([257, 1, 64], (4, 2, 32), False), ([300], (2, 1, 16), False), ([255, 256, 257], (8, 2, 128), True)]


@pytest.mark.parametrize("lens, geom, strided", PREFILL, ids=[f"{l}-{'x'.join(map(str, g))}{'-views' if s else ''}" for l, g, s in PREFILL])
def test_prefill_lse(lens, geom, strided):
    """Against fp64 causal attention; `strided`: q / k / v as views of the fused qkv (as in test_gpu_prefill_edges_and_strided_views) and
    lse as a column-strided view of a wider buffer."""
    Hq, Hkv, D = geom
    T = sum(lens)
    g = torch.Generator(device="cuda").manual_seed(T + D)
    qkv = torch.randn((T, (Hq + 2 * Hkv) * D), device="cuda", generator=g).to(F16)
    q, k, v = (t.view(T, -1, D) for t in qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1))
    if not strided:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    start = torch.tensor(np.concatenate([[0], np.cumsum(lens)[:-1]]), dtype=torch.int32, device="cuda")
    blen = torch.tensor(lens, dtype=torch.int32, device="cuda")
    plain = torch.full((T, Hq, D), float("nan"), dtype=F16, device="cuda")
    deft_amd.context_attention_fwd(q, k, v, plain, start, blen, max(lens))
    out = torch.full_like(plain, float("nan"))
    wide = torch.full((T, 2 * Hq + 1), 777.0, dtype=F32, device="cuda")
    lse = wide[:, 1::2] if strided else torch.full((T, Hq), 777.0, dtype=F32, device="cuda")
    assert lse.shape == (T, Hq)
    deft_amd.context_attention_fwd_lse(q, k, v, out, lse, start, blen, max(lens))
    torch.cuda.synchronize()
    assert _same_bits(out, plain)
    if strided:
        assert bool((wide[:, 0::2] == 777.0).all())  # (nothing beside the view was written)
    want = causal_lse(q, k, v, start.tolist(), lens, D ** -0.5)
    err = (lse.to(torch.float64) - want).abs()
    tol = 2e-5 + 4e-6 * want.abs()
    report(f"prefill {lens} {geom}{' views' if strided else ''}: worst |lse - fp64| {float(err.max()):.3e}  err/tol {float((err / tol).max()):.3f}")
    assert bool(torch.isfinite(lse).all()) and bool((err <= tol).all()), float(err.max())


# ---- merge_attention_states ----------------------------------------------------------------------------------------------------------
def _state_tensor(n, Hq, D, dtype, offset, fill=None, g=None):
    """[n, Hq, D] of `dtype`; `offset`: a view that starts 2 elements (4 bytes) into its buffer -- the 4-byte path."""
    base = torch.empty(n * Hq * D + 8, dtype=dtype, device="cuda")
    t = base[2 if offset else 0 :][: n * Hq * D].view(n, Hq, D)
    assert t.data_ptr() % 16 == (4 if offset else 0)
    if fill is None:
        t.copy_(torch.randn((n, Hq, D), device="cuda", generator=g).to(dtype))
    else:
        t.fill_(fill)
    return t


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset2"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
@pytest.mark.parametrize("n, Hq", [(1, 1), (5, 1), (64, 8)], ids=["1", "5", "64x8"])
def test_merge_attention_states(n, Hq, D, dtype, offset):
    g = torch.Generator(device="cuda").manual_seed(n * Hq + D)
    mk = lambda fill=None: _state_tensor(n, Hq, D, dtype, offset, fill, g)  # noqa: E731
    o_a, o_b = mk(), mk()
    lse_a = (torch.rand((n, Hq), device="cuda", generator=g) * 60 - 30).to(F32)
    lse_b = (torch.rand((n, Hq), device="cuda", generator=g) * 60 - 30).to(F32)
    if n * Hq > 4:  # some pairs a fraction of a nat apart (both weights matter), one far apart
        lse_b[::2] = lse_a[::2] + (torch.rand((n, Hq), device="cuda", generator=g)[::2] - 0.5)
    empty = torch.full((n, Hq), NINF, dtype=F32, device="cuda")
    nan_o = mk(float("nan"))

    # merge(a, empty) = a bit for bit, lse_a preserved -- with the empty side's o NaN-filled, on either side
    for args in ((o_a, lse_a, nan_o, empty), (nan_o, empty, o_a, lse_a)):
        out, lse = deft_amd.merge_attention_states(*args, out=mk(7.0))
        assert _same_bits(out, o_a) and torch.equal(lse, lse_a)
    # merge(empty, empty) = (0, -inf)
    out, lse = deft_amd.merge_attention_states(nan_o, empty, nan_o, empty, out=mk(7.0))
    assert bool((out == 0).all()) and torch.equal(lse, empty)
    # merge(a, a) = a bit for bit, lse = lse_a + ln 2
    out, lse = deft_amd.merge_attention_states(o_a, lse_a, o_a, lse_a)
    assert _same_bits(out, o_a)
    e2 = float((lse.to(torch.float64) - (lse_a.to(torch.float64) + math.log(2.0))).abs().max())
    assert e2 <= 2e-6, e2
    # random states against the fp64 model: one rounding of an fp32 convex combination
    out, lse = deft_amd.merge_attention_states(o_a, lse_a, o_b, lse_b, out=mk(7.0))
    want_o, want_lse = merge_model(o_a, lse_a, o_b, lse_b)
    err = (out.to(torch.float64) - want_o).abs()
    tol = U[dtype] * want_o.abs() + 1e-6
    el = float((lse.to(torch.float64) - want_lse).abs().max())
    report(f"merge n*Hq={n * Hq} D={D} {NAME[dtype]} {'4-byte' if offset else '16-byte'}: worst err {float(err.max()):.3e}  err/tol "
           f"{float((err / tol).max()):.3f}  lse err {el:.3e}  merge(a,a) lse err {e2:.3e}")
    assert bool((err <= tol).all()), float((err / tol).max())
    assert el <= 4e-6, el  # (fp32 lse of magnitude <= 31: an ulp is 1.9e-6)
    # in place (out = o_a, lse_out = lse_a) = out of place, bit for bit; o_b untouched
    o_b_before = o_b.clone()
    a2, la2 = mk(), lse_a.clone()
    a2.copy_(o_a)
    got_o, got_l = deft_amd.merge_attention_states(a2, la2, o_b, lse_b, out=a2, lse_out=la2)
    assert got_o is a2 and got_l is la2 and _same_bits(a2, out) and torch.equal(la2, lse) and _same_bits(o_b, o_b_before)
    b2, lb2 = mk(), lse_b.clone()
    b2.copy_(o_b)
    deft_amd.merge_attention_states(o_a, lse_a, b2, lb2, out=b2, lse_out=lb2)
    torch.cuda.synchronize()
    assert _same_bits(b2, out) and torch.equal(lb2, lse)


# ---- compositions --------------------------------------------------------------------------------------------------------------------
def _composed_tol(o, A, dtype):
    if dtype == F16:
        return 5e-4 + 2.0 ** -11 * (A + o.abs())
    return bound_bf16(o, A) + U[BF16] * (A + o.abs())


def _split_case(name):
    """One tree, split at every k of interest; returns how many (query, half) states came back empty."""
    Hq, Hkv, D = 8, 2, 128
    tree, pool = _scenario_tree(name, Hkv, D)
    g = torch.Generator(device="cuda").manual_seed(len(name) + 1)
    _randn_pool(pool, g)
    paths = product_leaf_paths(tree)
    nq = len(paths)
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    kb, vb = pool.get_key_buffer(0), pool.get_value_buffer(0)
    q = torch.randn((nq, Hq, D), device="cuda", generator=g).to(F16)
    truth, A = dense_attention(q, kb, vb, paths, Hq, Hkv, D ** -0.5, with_abs=True)
    assert float((truth - tree_truth(q, kb, vb, paths, Hq, Hkv, D ** -0.5)).abs().max()) < 1e-12
    want_lse = path_lse(q, kb, paths, Hq, Hkv, D ** -0.5)
    # the single full call first, at its own tolerance (5e-4 against fp64 on the fixed trees)
    full, full_lse = _run("flatten", q, pool, md, True)
    e_full = float((full.to(torch.float64) - truth).abs().max())
    report(f"split {name}: the single full call's worst err {e_full:.3e} (tolerance 5e-4)")
    assert e_full <= 5e-4

    _, block_q, cnts, off, masks, kv, lens = _flat(md)
    NB = cnts.shape[0]
    prefix = set(int(s) for s in tree.root.kv_indices)
    first = kv[::128].tolist()  # first slot of every block
    in_prefix = [b for b in range(NB) if int(first[b]) in prefix]
    assert len(in_prefix) >= 3
    # block boundaries inside the shared prefix: behind its first block, and in its middle
    empty_states = 0
    for k in sorted({1, in_prefix[len(in_prefix) // 2]}):
        assert 0 < k < NB and int(first[k - 1]) in prefix and int(first[k]) in prefix
        ok = int(off[k])
        halves = [(block_q[:ok], cnts[:k], off[:k], masks[: 128 * k], kv[: 128 * k], lens[:k]),
                  (block_q[ok:], cnts[k:], off[k:] - ok, masks[128 * k :], kv[128 * k :], lens[k:])]  # (block_q_offset re-based)
        states, empty_here = [], 0
        for h, arrays in enumerate(halves):
            o = torch.full_like(q, float("nan"))
            lse = torch.full((nq, Hq), 777.0, dtype=F32, device="cuda")
            deft_amd.tree_attention_subtree_fwd_lse(q, kb, vb, o, lse, 128, *[a.contiguous() for a in arrays])
            torch.cuda.synchronize()
            listed = set(int(r) for r in arrays[0].tolist())
            for r in range(nq):
                if r not in listed:  # no block in this half: the empty state
                    empty_here += 1
                    assert bool((o[r] == 0).all()) and bool((lse[r] == NINF).all()), (name, k, h, r)
                else:
                    assert bool(torch.isfinite(lse[r]).all()) and bool(torch.isfinite(o[r].float()).all()), (name, k, h, r)
            states.append((o, lse))
        empty_states += empty_here
        out, lse = deft_amd.merge_attention_states(states[0][0], states[0][1], states[1][0], states[1][1])
        torch.cuda.synchronize()
        err = (out.to(torch.float64) - truth).abs()
        tol = _composed_tol(truth, A, F16)
        el = float((lse.to(torch.float64) - want_lse).abs().max())
        report(f"split {name} at block {k} of {NB} ({empty_here} empty (query, half) states): worst err {float(err.max()):.3e}  err/tol "
               f"{float((err / tol).max()):.3f}  merged lse err {el:.3e}  vs the full call's lse {float((lse - full_lse).abs().max()):.3e}")
        assert bool((err <= tol).all()), (name, k, float((err / tol).max()))
        assert el <= U[F16] + 2e-5 + 4e-6, (name, k, el)  # (each half's lse at the random form's tolerance, one more fp32 rounding)
    return empty_states


def test_a_tree_split_over_two_calls():
    """Blocks [0, k) and [k, NB) of the Flatten metadata in two calls (k inside the shared prefix), the two states merged: the whole
    tree's attention.  A query with no block in a half comes back from that call as (0, -inf) -- which happens on wide40, whose first
    prefix block holds 32 of the 40 queries."""
    empty = {name: _split_case(name) for name in ("multilevel", "wide40")}
    assert empty["wide40"] > 0, empty


CACHED = [(1, 1, 128, F16), (127, 33, 128, F16), (128, 32, 128, F16), (300, 257, 128, F16), (127, 33, 64, F16), (128, 32, 128, BF16)]


@pytest.mark.parametrize("n0, n1, D, dtype", CACHED, ids=[f"{a}+{b}-d{d}-{NAME[t]}" for a, b, d, t in CACHED])
def test_prefill_onto_a_cached_prefix(n0, n1, D, dtype):
    """The prefix goes into the pool through ForwardMode.PREFILL; prefill_with_cached_prefix then attends the n1 new tokens over it and
    appends their rows.  Rows n0.. against tree_truth over the pool AFTER the call (leaf_paths[r] = prefix + new_slots[: r + 1]: this
    proves the append too), the merged lse against the fp64 LSE of the whole causal row."""
    Hq, Hkv = 4, 2
    N = n0 + n1
    g = torch.Generator(device="cuda").manual_seed(N + D)
    qkv = torch.randn((N, (Hq + 2 * Hkv) * D), device="cuda", generator=g).to(dtype)
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    req = deft_amd.ReqToTokenPool(8, 1024, device="cuda")
    pool = deft_amd.TokenToKVPool(1024, dtype, Hkv, D, 1, device="cuda")
    tree = deft_amd.TreeCache(dtype, Hkv, D, 1, req, pool, None, True, False)
    updater = tree.init_prompt(torch.arange(1, n0 + 1, dtype=torch.int32))
    meta = deft_amd.InputMetadata(deft_amd.ForwardMode.PREFILL, updater, pool, req, start_loc=torch.zeros(1, dtype=torch.int32, device="cuda"),
                                  seq_lens=torch.tensor([n0], dtype=torch.int64, device="cuda"), max_seq_len=n0)
    deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, 0)(q[:n0], k[:n0], v[:n0], meta)
    path_slots = [int(s) for s in tree.root.kv_indices]
    new_slots = [int(s) for s in pool.alloc(n1).tolist()]
    assert len(path_slots) == n0 and len(new_slots) == n1 and not set(path_slots) & set(new_slots)

    q3, k3, v3 = (t.view(N, -1, D) for t in (q, k, v))
    start, lens = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.tensor([N], dtype=torch.int32, device="cuda")
    whole = torch.full((N, Hq, D), float("nan"), dtype=dtype, device="cuda")
    deft_amd.context_attention_fwd(q3, k3, v3, whole, start, lens, N)

    out = torch.full((n1, Hq, D), float("nan"), dtype=dtype, device="cuda")
    lse = torch.full((n1, Hq), 777.0, dtype=F32, device="cuda")
    deft_amd.prefill_with_cached_prefix(q3[n0:], k3[n0:], v3[n0:], out, pool.kv_data[0], path_slots, new_slots, lse=lse)
    torch.cuda.synchronize()

    kb, vb = pool.get_key_buffer(0), pool.get_value_buffer(0)
    paths = [path_slots + new_slots[: r + 1] for r in range(n1)]
    truth, A = dense_attention(q3[n0:], kb, vb, paths, Hq, Hkv, D ** -0.5, with_abs=True)
    assert float((truth - tree_truth(q3[n0:], kb, vb, paths, Hq, Hkv, D ** -0.5)).abs().max()) < 1e-12
    # the whole-prompt prefill first, at its own tolerance on these inputs
    all_paths = [list(range(r + 1)) for r in range(N)]
    t_all, A_all = dense_attention(q3, k3, v3, all_paths, Hq, Hkv, D ** -0.5, with_abs=True)
    e_whole = (whole.to(torch.float64) - t_all).abs()
    tol_whole = 5e-4 + 2.0 ** -11 * t_all.abs() if dtype == F16 else bound_bf16(t_all, A_all)
    report(f"cached prefix {n0}+{n1} D={D} {NAME[dtype]}: whole-prompt prefill worst err {float(e_whole.max()):.3e}  err/tol "
           f"{float((e_whole / tol_whole).max()):.3f}")
    assert bool((e_whole <= tol_whole).all())
    assert float((truth - t_all[n0:]).abs().max()) < 1e-9  # (the pool holds exactly the prompt's rows: prefix and appended)

    err = (out.to(torch.float64) - truth).abs()
    tol = _composed_tol(truth, A, dtype)
    want_lse = causal_lse(q3, k3, v3, [0], [N], D ** -0.5)[n0:]
    el = (lse.to(torch.float64) - want_lse).abs()
    tol_l = U[dtype] + 2e-5 + 4e-6 * want_lse.abs().clamp_min(1.0)  # the cached part's random-form tolerance + the prefill part's
    report(f"cached prefix {n0}+{n1} D={D} {NAME[dtype]}: composed worst err {float(err.max()):.3e}  err/tol {float((err / tol).max()):.3f}  "
           f"lse err {float(el.max()):.3e}  err/tol {float((el / tol_l).max()):.3f}")
    assert bool(torch.isfinite(out.float()).all()) and bool((err <= tol).all()), float((err / tol).max())
    assert bool((el <= tol_l).all()), float(el.max())
