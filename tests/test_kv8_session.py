"""deft_amd.DecodeSession over fp8 KV pools ("In the captured session"): twin trees over twin fp8 pools, one decoded
eagerly (tree.alloc + TreeMetadata.from_tree_cache + DeFTAttention.forward), one through the session, compared at EVERY step:

  * pool bytes (as uint8) and page tables bit for bit, always;
  * steps that rebuild the plan (an epoch's upload step, legacy steps): outputs bit for bit, both forms of a layer -- the fused quantising
    append and the append as a launch of its own;
  * window steps: the 16-bit session's rules -- fp16 |out - eager| <= 1e-3 + 2^-10 |eager| (tests/test_session.py::_agree), bf16 both
    sides within the a-priori bound of fp64 truth (tools/error_bound.py);
  * both sides against fp64 truth over the DEQUANTISED pool (kv8_model.dequantize with the layer's scales) at the 16-bit operators'
    tolerance (tests/test_kv8_gpu.py::_check: fp16 5e-4, bf16 u A + 2 u |o| + 2e-5), outputs finite.

Both pools are filled with the byte 0x7f -- a NaN code -- before anything else; only the prompt's slots then get seeded finite codes, so a
read of a dead or never-written slot poisons an output.  Per-head scales are test_kv8_gpu's (none a power of two), per layer in another
order.  Values (V codes and new v rows) at a quarter: every leaf appends the same row at every step, and 5e-4 against truth is a
tolerance for fp16 outputs below ~0.5 (tests/test_session.py, above STRADDLING)."""
import numpy as np
import pytest
import torch

import deft_amd
import kv8_model
from test_kv8_gpu import K_SCALES, V_SCALES
from tools.error_bound import bound_bf16, dense_attention
from truth import product_leaf_paths

pytestmark = pytest.mark.gpu
FP8, F16, BF16, F32 = torch.float8_e4m3fn, torch.float16, torch.bfloat16, torch.float32
NAME = {F16: "fp16", BF16: "bf16"}
D = 128
FORMS = {"two-launch": False, "fused": True}


def _scales(l, Hkv, shift=0):
    """Layer l's per-head scales: test_kv8_gpu's, rotated by the layer (and by `shift`: a second set for the replay test)."""
    r = (l + shift) % 4
    return (K_SCALES[r:] + K_SCALES[:r])[:Hkv], (V_SCALES[r:] + V_SCALES[:r])[:Hkv]


class Twins:
    """An eager tree and a session tree over twin fp8 pools, and one decode step of both with every check of the module docstring."""

    def __init__(self, Hq, Hkv, layers, prefix, width, size, elem, mode, incremental, fused, seed, use_graph=True, cap=16, eager=True, **kw):
        self.Hq, self.Hkv, self.layers, self.elem, self.mode, self.incremental = Hq, Hkv, layers, elem, mode, incremental
        g = torch.Generator(device="cuda").manual_seed(seed)
        x = torch.randn((layers, prefix, 2, Hkv, D), device="cuda", generator=g)
        x[:, :, 1] *= 0.25
        codes = kv8_model.quantize(x.to(F16), 1.0)
        assert not bool(kv8_model.is_nan_code(codes).any())
        self.trees = []
        for _ in range(2 if eager else 1):
            req = deft_amd.ReqToTokenPool(64, size, device="cuda")
            pool = deft_amd.TokenToKVPool(size, FP8, Hkv, D, layers, device="cuda")
            pool._storage.view(torch.uint8).fill_(0x7F)  # every slot a NaN code ...
            tree = deft_amd.TreeCache(elem, Hkv, D, layers, req, pool, None, True, False)
            tree.init_prompt(torch.arange(1, prefix + 1, dtype=torch.int32))
            slots = torch.as_tensor(np.asarray(tree.root.kv_indices), dtype=torch.int64, device="cuda")
            pool._storage.view(torch.uint8)[:, slots] = codes.view(torch.uint8)  # ... but the prompt's
            tree.branch(tree.root, width)
            for l in range(layers):
                pool.set_kv_scales(l, *_scales(l, Hkv))
            self.trees.append((tree, pool))
        (self.te, self.pe), (self.ts, self.ps) = self.trees[0], self.trees[-1]
        self.q = torch.randn((layers, cap, Hq * D), device="cuda", generator=g).to(elem)
        self.k = torch.randn((layers, cap, Hkv * D), device="cuda", generator=g).to(elem)
        self.v = (torch.randn((layers, cap, Hkv * D), device="cuda", generator=g) * 0.25).to(elem)
        self.n = [width]
        self.sess = deft_amd.DecodeSession(self.ts, Hq, Hkv, D, layers, self.qkv, mode=mode, incremental=incremental, use_graph=use_graph,
                                           elem_dtype=elem, kv8_fused_append=fused, **kw)
        assert self.sess.dtype == elem and self.sess.kv8
        self.attn = [deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, l) for l in range(layers)]
        self.fmode = deft_amd.forward_mode_from_cli(mode)
        self.steps = 0

    def qkv(self, l):
        n = self.n[0]
        return self.q[l, :n], self.k[l, :n], self.v[l, :n]

    def grow(self):
        for tree, _ in self.trees:
            for leaf in tree.leaves.values():
                leaf.append_token(7)

    def eager_step(self):
        upd = self.te.alloc()
        md = deft_amd.TreeMetadata.from_tree_cache(self.te)
        deft_amd.register_tree_metadata(md)
        n = self.n[0] = md.query_num
        meta = deft_amd.InputMetadata(self.fmode, upd, self.pe)
        return [self.attn[l](self.q[l, :n], self.k[l, :n], self.v[l, :n], meta) for l in range(self.layers)], upd.cache_loc

    def session_step(self):
        """One step of the session; returns (outputs, did the step run on a window plan)."""
        before = dict(self.sess.step_kinds)
        out = self.sess.step()
        kind = [k for k, c in self.sess.step_kinds.items() if c != before[k]]
        assert len(kind) == 1, (before, self.sess.step_kinds)
        torch.cuda.synchronize()
        assert all(o.dtype == self.elem for o in out)
        return out, kind[0] in ("replan", "patch")

    def truth(self, pool, tree, l):
        n = self.n[0]
        ks, vs = pool.k_scale[l], pool.v_scale[l]
        kv = pool.kv_data[l]
        k64 = kv8_model.dequantize(kv[:, 0], ks[:, None])
        v64 = kv8_model.dequantize(kv[:, 1], vs[:, None])
        o, A = dense_attention(self.q[l, :n], k64, v64, product_leaf_paths(tree), self.Hq, self.Hkv, D ** -0.5, with_abs=True)
        assert bool(torch.isfinite(o).all()), "the truth itself read a NaN code: a live slot was never written"
        return o, (torch.full_like(o, 5e-4) if self.elem == F16 else bound_bf16(o, A))

    def against_truth(self, t, o, tol, tag):
        got = t.reshape(o.shape).to(torch.float64)
        assert bool(torch.isfinite(got).all()), (tag, "non-finite output")
        worst = float(((got - o).abs() / tol).max())
        assert worst <= 1.0, (tag, "err / tol against fp64 truth of the dequantised pool", worst, float(o.abs().max()))

    def agree(self, out, ref, window, tag):
        """Session against eager: bit for bit unless the step ran on a window plan; then fp16 by tests/test_session.py::_agree's rule
        (bf16: both sides are held to the a-priori bound of truth in `step`, as tools/fuzz_session.py --bf16 does)."""
        if not window:
            assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), (tag, float((out.float() - ref.float()).abs().max()))
        elif self.elem == F16:
            err = (out.float() - ref.float()).abs()
            assert bool((err <= 1e-3 + ref.float().abs() * 2.0 ** -10).all()), (tag, float(err.max()))

    def same_pools(self, tag):
        assert torch.equal(self.pe._storage.view(torch.uint8), self.ps._storage.view(torch.uint8)), (tag, "pool bytes")
        assert torch.equal(self.te.req_to_token_pool.req_to_token, self.ts.req_to_token_pool.req_to_token), (tag, "page tables")

    def step(self):
        self.grow()
        ref, loc = self.eager_step()
        out, window = self.session_step()
        n, tag = self.n[0], (self.steps, "window" if window else "rebuilt")
        self.same_pools(tag)
        for l in range(self.layers):
            self.agree(out[l][:n], ref[l], window, tag + (l,))
            o, tol = self.truth(self.pe, self.te, l)
            self.against_truth(out[l][:n], o, tol, tag + (l, "session"))
            self.against_truth(ref[l], o, tol, tag + (l, "eager"))
        self.steps += 1
        return loc, window

    def restructure(self):
        for tree, _ in self.trees:  # cut two leaves, branch one
            lv = sorted(tree.leaves.values(), key=lambda x: x.id)
            tree.cut(lv[1])
            tree.cut(lv[4])
            tree.branch(lv[0], 3)

    def speculative_update(self, accept):
        for tree, _ in self.trees:  # the accepted leaves' tokens go to the root, every leaf is reset (tests/test_session.py)
            lv = sorted(tree.leaves.values(), key=lambda x: x.id)
            before = len(tree.root.kv_indices)
            for lf in lv[:accept]:
                tree.merge_nodes(tree.root, lf, pruneB_flag=False)
            tree.reset_nodes_KV(lv, len(tree.root.kv_indices) - before)


# ---- 1. step for step ----------------------------------------------------------------------------------------------------------------
def _step_for_step(mode, incremental, form, elem, use_graph):
    t = Twins(8, 2, 2, 250, 6, 1024, elem, mode, incremental, FORMS[form], seed=3, use_graph=use_graph, win_tiles=1)
    for _ in range(50):  # 6 tokens a step into one 128-slot overflow tile: a window lasts 21 steps
        t.step()
    sess = t.sess
    per_epoch = 2 if incremental else 1  # (window plans: a replan graph and a patch graph)
    assert sess.captures == (per_epoch if use_graph else 0)
    if incremental:
        assert sess.step_kinds["patch"] >= 40 and sess.step_kinds["replan"] >= 2 and sess.step_kinds["legacy"] == 0, sess.step_kinds
    else:
        assert sess.step_kinds["patch"] == 0 and sess.step_kinds["replan"] == 0 and sess.step_kinds["legacy"] == 49, sess.step_kinds
    t.restructure()
    for _ in range(12):
        t.step()
    assert sess.captures == (2 * per_epoch if use_graph else 0)
    assert sess.step_kinds["upload"] == 2 and (not incremental or sess.step_kinds["legacy"] == 0), sess.step_kinds
    assert sess.device_errors() == 0


@pytest.mark.parametrize("elem", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("incremental", [False, True], ids=["legacy", "window"])
@pytest.mark.parametrize("mode", ["flatten", "node"])
def test_session_equals_eager_step_for_step(mode, incremental, form, elem):
    _step_for_step(mode, incremental, form, elem, True)


@pytest.mark.parametrize("mode, incremental, form, elem", [("flatten", False, "two-launch", F16), ("node", True, "fused", BF16),
                                                           ("flatten", True, "two-launch", F16)],
                         ids=["legacy", "window-fused", "window-two-launch"])
def test_session_without_graphs(mode, incremental, form, elem):
    _step_for_step(mode, incremental, form, elem, False)


# ---- 2. geometries: MHA and an odd KV-head count --------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("heads", [(4, 4), (3, 3)], ids=["4x4", "3x3"])
def test_mha_and_odd_head_counts_on_window_plans(heads, form):
    t = Twins(heads[0], heads[1], 2, 200, 5, 1024, F16, "flatten", True, FORMS[form], seed=heads[0] * 7, win_tiles=1)
    for _ in range(20):
        t.step()
    kinds = t.sess.step_kinds
    assert kinds["patch"] >= 17 and kinds["legacy"] == 0 and t.sess.device_errors() == 0, kinds


# ---- 3. a GQA group that straddles two 32-row passes (Qwen2-7B's 28 / 4) ---------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("mode", ["flatten", "node"])
def test_straddling_gqa_group(mode, form):
    Hq, Hkv, width = 28, 4, 12
    t = Twins(Hq, Hkv, 1, 200, width, 1024, F16, mode, True, FORMS[form], seed=59, win_tiles=1)
    for _ in range(20):
        t.step()
    kinds = t.sess.step_kinds
    if deft_amd.lib.deft_window_supported(width, 32, Hq, Hkv):
        assert kinds["patch"] >= 15 and kinds["legacy"] == 0, kinds
    else:  # (every step then rebuilt its plan: `step` held each one to the eager path bit for bit)
        assert kinds["legacy"] == 19 and kinds["patch"] == 0 and kinds["replan"] == 0, kinds
    assert t.sess.device_errors() == 0


# ---- 4. speculative-decoding steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("incremental", [False, True], ids=["legacy", "window"])
def test_speculative_decoding_steps_replay_one_capture_set(incremental, form):
    t = Twins(8, 2, 2, 250, 12, 2048, F16, "flatten", incremental, FORMS[form], seed=17)
    rng = np.random.default_rng(3)
    for step in range(30):
        t.step()
        t.speculative_update(int(rng.integers(1, 5)))
    # epochs: the first step; the first merge into a root without room.  Everything after replays the second epoch's graph(s) -- one
    # capture set for the loop, not one per step: the journal of merges and resets rides in the step's upload
    assert t.sess.captures <= (3 if incremental else 2), t.sess.captures
    if incremental:  # a leaf is reset and refilled every step: its overflow position is reused, the window lasts
        assert t.sess.step_kinds["patch"] >= 20 and t.sess.step_kinds["legacy"] == 0, t.sess.step_kinds
    assert t.sess.device_errors() == 0


# ---- 5. the scales are device pointers, read at replay --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("incremental", [False, True], ids=["legacy", "window"])
def test_scales_are_read_at_replay(incremental, form):
    Hq, Hkv, layers = 8, 2, 2
    t = Twins(Hq, Hkv, layers, 250, 6, 1024, F16, "flatten", incremental, FORMS[form], seed=29, win_tiles=1)
    for _ in range(10):
        t.step()
    captures = t.sess.captures
    assert captures == (2 if incremental else 1)
    for _, pool in t.trees:
        for l in range(layers):
            pool.set_kv_scales(l, *_scales(l, Hkv, shift=2))  # (the stored codes keep their bytes and mean other numbers now: on both sides)
    for _ in range(6):
        loc, _ = t.step()
        n = t.n[0]
        li = loc.to(torch.int64).cpu()
        for l in range(layers):
            ks, vs = (torch.tensor(s, dtype=F32)[:, None] for s in _scales(l, Hkv, shift=2))
            rows = t.ps.kv_data[l].view(torch.uint8).cpu()[li]
            want_k = kv8_model.quantize(t.k[l, :n].reshape(n, Hkv, D).cpu(), ks)
            want_v = kv8_model.quantize(t.v[l, :n].reshape(n, Hkv, D).cpu(), vs)
            assert kv8_model.same_codes(rows[:, 0].view(FP8), want_k) and kv8_model.same_codes(rows[:, 1].view(FP8), want_v), l
            old_k = kv8_model.quantize(t.k[l, :n].reshape(n, Hkv, D).cpu(), torch.tensor(_scales(l, Hkv)[0], dtype=F32)[:, None])
            assert not kv8_model.same_codes(rows[:, 0].view(FP8), old_k)  # (the new scales really give other codes)
    assert t.sess.captures == captures and t.sess.device_errors() == 0


# ---- 6. the step's words fetched by the step's first kernel --------------------------------------------------------------------------
def test_staging_by_kernel():
    t = Twins(8, 2, 2, 250, 5, 1024, F16, "flatten", True, False, seed=5, win_tiles=1, staging="kernel")
    for _ in range(20):
        t.step()
    kinds = t.sess.step_kinds
    assert t.sess.staging == "kernel" and kinds["patch"] >= 17 and kinds["legacy"] == 0 and t.sess.device_errors() == 0, kinds


# ---- 7. the two forms agree -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("incremental", [False, True], ids=["legacy", "window"])
@pytest.mark.parametrize("mode", ["flatten", "node"])
def test_the_two_forms_agree(mode, incremental, elem):
    a, b = (Twins(8, 2, 2, 250, 6, 1024, elem, mode, incremental, fused, seed=41, win_tiles=1, eager=False) for fused in (False, True))
    assert a.sess.kv8_fused == {"legacy": False, "window": False} and b.sess.kv8_fused == {"legacy": True, "window": True}
    for step in range(30):
        outs = []
        for t in (a, b):
            t.grow()
            outs.append(t.session_step())
        (oa, wa), (ob, wb) = outs
        assert wa == wb, step
        assert torch.equal(a.ps._storage.view(torch.uint8), b.ps._storage.view(torch.uint8)), step
        assert torch.equal(a.ts.req_to_token_pool.req_to_token, b.ts.req_to_token_pool.req_to_token), step
        for l in range(2):
            assert bool(torch.isfinite(oa[l]).all()) and bool(torch.isfinite(ob[l]).all()), (step, l)
            if not wa:
                assert torch.equal(oa[l].view(torch.int16), ob[l].view(torch.int16)), (step, l)
            elif elem == F16:
                err = (oa[l].float() - ob[l].float()).abs()
                assert bool((err <= 1e-3 + ob[l].float().abs() * 2.0 ** -10).all()), (step, l, float(err.max()))
            else:  # bf16 window steps: each form within the a-priori bound of fp64 truth over its own (identical) pool
                o, tol = b.truth(b.ps, b.ts, l)
                a.against_truth(oa[l], o, tol, (step, l, "two-launch"))
                b.against_truth(ob[l], o, tol, (step, l, "fused"))
    assert a.sess.device_errors() == 0 and b.sess.device_errors() == 0
    if incremental:
        assert a.sess.step_kinds == b.sess.step_kinds and a.sess.step_kinds["patch"] >= 20, (a.sess.step_kinds, b.sess.step_kinds)
