"""Shaped scores through the kv8 operators, and log-sum-exps built from partials tens of nats apart.

stage1_kv8_kernel has its own online softmax (each wave keeps a private (m, l, O) over its 32 keys of every tile), its own four-wave
epilogue (exp2(m_w - M), v_scale before the division) and feeds the merge.  With N(0,1) scores the running max settles in the first
tiles and all of that is all but dead: here the max moves where a test says (tests/kv8_shapes.py: inputs on the e4m3 grid -- sink,
staircase, spike, mixed), which tests/test_kv8_sharp_model.py shows, without a GPU and on these very tensors, to fail a softmax that
forgets alpha or the cross-wave factors by three orders of magnitude.

  * out: fp64 truth over the DEQUANTISED K and V with the per-head scales, as test_kv8_gpu._check does; fp16 at the sharp-softmax rule
    5e-4 + 2^-11 |truth| (a sink makes outputs as large as one V row), bf16 at bound_bf16(truth, A).
  * lse: |lse - fp64| <= u + 2e-5 + 4e-6 |lse| -- the random form's two terms (L sums probabilities rounded to T, so it is
    off by a relative u; 2e-5 of fp32 slack) plus the prefill rule's relative term, because M + log L is an fp32 number of magnitude
    up to ~100 here.  out of an *_lse call is bit-identical to the plain call's.
  * the 16-bit *_lse operators under test_sharp_softmax's own patterns on the same tree, and one 32k x 8 case (merge_coop_kernel's four
    waves each fold a quarter of a list whose partial lses are tens of nats apart, then store the lse) for the 16-bit and the kv8 form.

Every figure is printed before it is asserted (`pytest -s`): `[kv8]` lines go to profiles/kv8_error.txt, `[states]` lines to
profiles/states_error.txt."""
import math

import pytest
import torch

import bf16_util
import deft_amd
import kv8_model
import kv8_shapes as ks
import oracles
import test_sharp_softmax as sharp
from states_model import path_lse
from test_kv8_gpu import K_SCALES, V_SCALES, _flat, _nodes, _run8, _same_bits, report
from tools.error_bound import bound_bf16, dense_attention
from truth import product_leaf_paths, tree_truth

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NAME = {F16: "fp16", BF16: "bf16"}
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
D = 128
GEOMS = [(4, 4), (8, 2), (3, 3)]
PREFIX, WIDTH, BRANCH = 1000, 8, 150
_TREES, _CASES = {}, {}


def report_states(line):
    print("[states] " + line, flush=True)


def _tree(geom):
    """The tree of test_shaped_scores_through_flatten_and_node, once per geometry: (paths, metadata, pool size, spike tile)."""
    if geom not in _TREES:
        Hq, Hkv = geom
        tree, pool, _ = oracles.few_shot_tree(PREFIX, WIDTH, BRANCH, Hkv, D)
        paths = product_leaf_paths(tree)
        md = deft_amd.TreeMetadata.from_tree_cache(tree)
        ends = sharp._prefix_chunk_ends(md, pool, Hq, Hkv, D, len(paths))
        report(f"sharp {Hq}x{Hkv}: last tiles of the prefix's chunks {ends}")
        assert ends[0] == ks.SPIKE_TILE[geom], (geom, ends)  # (the CPU power check put its spike in the same tile)
        assert [list(map(int, p)) for p in paths] == [list(map(int, p)) for p in ks.cpu_few_shot_tree(PREFIX, WIDTH, BRANCH, Hkv)[1]]
        _TREES[geom] = (paths, md, pool.size, ends[0])
    return _TREES[geom]


def _case(geom, dtype, pattern):
    """One pattern's inputs on the GPU with their fp64 reading, built once: codes, q, k64, v64, scales, fp64 scores."""
    key = (geom, dtype, pattern)
    if key not in _CASES:
        Hq, Hkv = geom
        paths, md, size, tile = _tree(geom)
        codes, q, heads = ks.shaped_case(pattern, paths, size, PREFIX, Hq, Hkv, K_SCALES[:Hkv], tile, dtype)
        codes, q = codes.to("cuda"), q.to("cuda")
        k_sc = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
        v_sc = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
        k64 = kv8_model.dequantize(codes[:, 0], k_sc[:, None])
        v64 = kv8_model.dequantize(codes[:, 1], v_sc[:, None])
        s = ks.path_scores(q, k64, paths, Hq, Hkv).cpu()
        gap = ks.assert_branch_taken(pattern, heads, s, PREFIX, Hq, Hkv, tile)
        if math.isfinite(gap):
            report(f"sharp {pattern} {Hq}x{Hkv} {NAME[dtype]}: smallest gap between a tile's four 32-key wave maxima {gap:.1f} nats; scores span "
                   f"{float(s.min()):.0f} .. {float(s.max()):.0f} nats")
        _CASES[key] = (codes, q, k64, v64, k_sc, v_sc)
    return _CASES[key]


def _lse_tol(want, dtype):
    return U[dtype] + 2e-5 + 4e-6 * want.abs()


# ---- out under shaped scores -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_shaped_scores_through_the_kv8_operators(geom, dtype):
    Hq, Hkv = geom
    paths, md, size, tile = _tree(geom)
    for pattern in ks.PATTERNS:
        codes, q, k64, v64, k_sc, v_sc = _case(geom, dtype, pattern)
        truth, A = dense_attention(q, k64, v64, paths, Hq, Hkv, D ** -0.5, with_abs=True)
        assert float((truth - tree_truth(q, k64, v64, paths, Hq, Hkv, D ** -0.5)).abs().max()) < 1e-12
        tol = 5e-4 + 2.0 ** -11 * truth.abs() if dtype == F16 else bound_bf16(truth, A)
        for mode in ("flatten", "node"):
            out = _run8(mode, q, codes, md, k_sc, v_sc)
            got = out.reshape(truth.shape).to(torch.float64)
            err = (got - truth).abs()
            worst = float((err / tol).max())
            report(f"sharp {pattern} {Hq}x{Hkv} {mode} {NAME[dtype]}: worst err {float(err.max()):.3e}  err/tol {worst:.3f}  largest |output| "
                   f"{float(truth.abs().max()):.2f}")
            assert bool(torch.isfinite(got).all()) and worst <= 1.0, (pattern, mode, worst)


# ---- lse under shaped scores: the kv8 forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_kv8_lse_under_shaped_scores(geom, dtype):
    Hq, Hkv = geom
    paths, md, size, tile = _tree(geom)
    for pattern in ("sink", "staircase", "spike"):
        codes, q, k64, v64, k_sc, v_sc = _case(geom, dtype, pattern)
        want = path_lse(q, k64, paths, Hq, Hkv, D ** -0.5)
        tol = _lse_tol(want, dtype)
        for mode in ("flatten", "node"):
            plain = _run8(mode, q, codes, md, k_sc, v_sc)
            out, lse = _run8(mode, q, codes, md, k_sc, v_sc, with_lse=True)
            err = (lse.to(torch.float64) - want).abs()
            report(f"sharp lse {pattern} {Hq}x{Hkv} {mode} {NAME[dtype]}: worst |lse - fp64| {float(err.max()):.3e}  err/tol "
                   f"{float((err / tol).max()):.3f}  (lse {float(want.min()):.1f} .. {float(want.max()):.1f})")
            assert _same_bits(out, plain), (pattern, mode, "out differs from the plain kv8 call's")
            assert bool(torch.isfinite(lse).all()) and bool((err <= tol).all()), (pattern, mode, float((err / tol).max()))


# ---- lse under shaped scores: the 16-bit operators, test_sharp_softmax's own patterns -----------------------------------------------------
def _run16_lse(mode, q, pool, md):
    kb, vb = pool.get_key_buffer(0), pool.get_value_buffer(0)
    outs = []
    for with_lse in (False, True):
        out = torch.full_like(q, float("nan"))
        lse = torch.full(q.shape[:2], 777.0, dtype=F32, device="cuda")
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
        outs.append((out, lse))
    return outs[0][0], outs[1][0], outs[1][1]


def _check16_lse(tag, q, pool, md, paths, Hq, Hkv, Dh, dtype, modes=("flatten", "node")):
    want = path_lse(q, pool.get_key_buffer(0), paths, Hq, Hkv, Dh ** -0.5)
    tol = _lse_tol(want, dtype)
    for mode in modes:
        plain, out, lse = _run16_lse(mode, q, pool, md)
        err = (lse.to(torch.float64) - want).abs()
        report_states(f"sharp lse {tag} {mode} {NAME[dtype]}: worst |lse - fp64| {float(err.max()):.3e}  err/tol {float((err / tol).max()):.3f}  "
                      f"(lse {float(want.min()):.1f} .. {float(want.max()):.1f})")
        assert _same_bits(out, plain), (tag, mode, "out differs from the plain entry point's")
        assert bool(torch.isfinite(lse).all()) and bool((err <= tol).all()), (tag, mode, float((err / tol).max()))


def _assert_rises_bf16(pattern, k_buf, q, paths, Dh, Hq, Hkv, tile):
    """bf16 keeps 8 bits of the ramp's a: it has plateaus of a few keys, so `the last key is the max` cannot be asked; the max still
    rises in every 128-key tile of every path.  Sink and spike as the fp16 form asks."""
    G = Hq // Hkv
    for h in range(Hkv):
        for r, p in enumerate(paths):
            s, n = sharp._scores(k_buf, q, p, r, h, h * G, Dh), len(p)
            if pattern == "ramp":
                assert all(oracles.running_max_rises_in(s, lo, min(lo + 128, n)) for lo in range(0, n, 128)), (h, r)
            elif pattern == "sink":
                assert float(s[0]) > float(s[1:].max()) + 20, (h, r)
            else:
                assert oracles.running_max_rises_in(s, tile * 128, (tile + 1) * 128), (h, r)


@pytest.mark.parametrize("geom", sharp.GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_16bit_lse_under_shaped_scores(geom):
    """The *_lse operators of a 16-bit pool on the inputs of test_shaped_scores_through_flatten_and_node (fp16: its four patterns, its own
    branch-taken assertion), and at head_dim 128 on a bf16 pool (sink, ramp, spike)."""
    Hq, Hkv, Dh = geom
    for dtype in ((F16, BF16) if Dh == 128 else (F16,)):
        make = oracles.few_shot_tree if dtype == F16 else bf16_util.few_shot_tree
        tree, pool, _ = make(PREFIX, WIDTH, BRANCH, Hkv, Dh)
        paths = product_leaf_paths(tree)
        nq = len(paths)
        kb = pool.get_key_buffer(0)
        md = deft_amd.TreeMetadata.from_tree_cache(tree)
        tile = sharp._prefix_chunk_ends(md, pool, Hq, Hkv, Dh, nq)[0]
        for pattern in (sharp.PATTERNS if dtype == F16 else ["sink", "ramp", "spike"]):
            g = torch.Generator(device="cuda").manual_seed(Dh + Hq)
            q = torch.empty((nq, Hq, Dh), dtype=dtype, device="cuda")
            a, b = sharp._shape(pattern, paths, kb.shape[0], Hkv, Hq, Dh, tile)
            oracles.shaped_inputs(kb, q, a, b, g)
            if dtype == F16:
                sharp._assert_branch_taken(pattern, kb, q, paths, Dh, Hq, Hkv, tile)
            else:
                _assert_rises_bf16(pattern, kb, q, paths, Dh, Hq, Hkv, tile)
            _check16_lse(f"{pattern} {Hq}x{Hkv} D={Dh}", q, pool, md, paths, Hq, Hkv, Dh, dtype)


# ---- the four-wave merge storing an lse built from partials tens of nats apart -------------------------------------------------------------
def test_lse_through_the_four_wave_combine_under_shaped_scores():
    """The shape of test_lse_through_the_four_wave_combine (32k x 8, D = 128, Flatten) with a sink in the first tile of one prefix chunk
    and a spike in the last tile of another, as test_shaped_scores_through_long_merge_lists places them -- for the 16-bit *_lse form and
    for the kv8 *_lse form (codes on the grid, per-head scales, both element types; its out against fp64 truth as well)."""
    Hq, Hkv, prefix, width = 8, 2, 32768, 8
    tree, pool, _ = oracles.few_shot_tree(prefix, width, 3, Hkv, D)
    paths = product_leaf_paths(tree)
    nq = len(paths)
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    ends = sharp._prefix_chunk_ends(md, pool, Hq, Hkv, D, nq)
    assert nq <= 16 and len(ends) > 8, ends  # (every query has more than 8 partial rows: the four-wave path)
    sink_tile, spike_tile = ends[len(ends) // 3 - 1] + 1, ends[(2 * len(ends)) // 3]
    assert 0 < sink_tile < spike_tile < prefix // 128
    sink_slot, spike_slot, last_slot = paths[0][sink_tile * 128 + 7], paths[0][spike_tile * 128 + 100], paths[1][-1]
    # two smaller rises in the two tiles before the spike's, inside waves 1 and 2 -- the same chunk: wave-private maxima that rise in a
    # LATER tile of a chunk (the alpha rescale of a non-empty O), the 12-nat one 6 nats under the spike: e^-6 of a V row, 5x the tolerance
    assert ends[(2 * len(ends)) // 3 - 1] < spike_tile - 2, ends
    step_slots = [(paths[0][(spike_tile - 2) * 128 + 37], 6.0), (paths[0][(spike_tile - 1) * 128 + 69], 12.0)]
    size = pool.size

    def far_apart(s0):
        assert oracles.running_max_rises_in(s0, sink_tile * 128, (sink_tile + 1) * 128)
        assert float(s0.max()) - float(s0[: sink_tile * 128].max()) > 20  # (partial LSEs tens of nats apart)

    # 16-bit
    kb, vb = pool.get_key_buffer(0), pool.get_value_buffer(0)
    g = torch.Generator(device="cuda").manual_seed(prefix)
    oracles.dyadic_(vb, g)
    q = torch.empty((nq, Hq, D), dtype=F16, device="cuda")
    kk = math.sqrt(D) / sharp.B
    a = torch.zeros((kb.shape[0], Hkv), dtype=torch.float64)
    a[sink_slot, 0] = 25.0 * kk
    a[spike_slot, :] = 18.0 * kk
    for slot, nats in step_slots:
        a[slot, :] = nats * kk
    a[last_slot, -1] = 30.0 * kk
    oracles.shaped_inputs(kb, q, a, torch.full((Hq,), sharp.B, dtype=torch.float64), g)
    far_apart(sharp._scores(kb, q, paths[0], 0, 0, 0, D))
    _check16_lse("32kx8 four-wave combine", q, pool, md, paths, Hq, Hkv, D, F16, modes=("flatten",))

    # kv8
    npc = ks.nats_per_code(K_SCALES[:Hkv])
    a8 = torch.zeros((size, Hkv), dtype=torch.float64)
    a8[sink_slot, 0] = ks.grid_at_least(25.0 / npc[0])
    for h in range(Hkv):
        a8[spike_slot, h] = ks.grid_at_least(18.0 / npc[h])
        for slot, nats in step_slots:
            a8[slot, h] = ks.grid_at_least(nats / npc[h])
    a8[last_slot, -1] = ks.grid_at_least(30.0 / npc[-1])
    k_sc = torch.tensor(K_SCALES[:Hkv], dtype=F32, device="cuda")
    v_sc = torch.tensor(V_SCALES[:Hkv], dtype=F32, device="cuda")
    for dtype in (F16, BF16):  # (GQA of 8 queries: the DYN instantiation of either element type, its alpha rescale included)
        codes, q8 = ks.codes_and_q(a8, nq, Hq, torch.full((Hq,), ks.B, dtype=torch.float64), dtype, prefix)
        codes, q8 = codes.to("cuda"), q8.to("cuda")
        k64 = kv8_model.dequantize(codes[:, 0], k_sc[:, None])
        v64 = kv8_model.dequantize(codes[:, 1], v_sc[:, None])
        far_apart(ks.path_scores(q8[:1], k64, paths[:1], Hq, Hkv)[0, 0].cpu())
        want = path_lse(q8, k64, paths, Hq, Hkv, D ** -0.5)
        tol = _lse_tol(want, dtype)
        plain = _run8("flatten", q8, codes, md, k_sc, v_sc)
        out, lse = _run8("flatten", q8, codes, md, k_sc, v_sc, with_lse=True)
        err = (lse.to(torch.float64) - want).abs()
        report(f"sharp lse 32kx8 four-wave combine flatten {NAME[dtype]}: worst |lse - fp64| {float(err.max()):.3e}  err/tol "
               f"{float((err / tol).max()):.3f}  (lse {float(want.min()):.1f} .. {float(want.max()):.1f})")
        truth, A = dense_attention(q8, k64, v64, paths, Hq, Hkv, D ** -0.5, with_abs=True)
        assert float((truth - tree_truth(q8, k64, v64, paths, Hq, Hkv, D ** -0.5)).abs().max()) < 1e-12
        eo = (out.to(torch.float64) - truth).abs()
        worst = float((eo / (5e-4 + 2.0 ** -11 * truth.abs() if dtype == F16 else bound_bf16(truth, A))).max())
        report(f"sharp 32kx8 four-wave combine flatten {NAME[dtype]}: worst err {float(eo.max()):.3e}  err/tol {worst:.3f}")
        assert _same_bits(out, plain)
        assert bool(torch.isfinite(lse).all()) and bool((err <= tol).all()), float((err / tol).max())
        assert worst <= 1.0, worst
