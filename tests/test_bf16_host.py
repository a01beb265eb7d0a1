"""The bfloat16 surface that needs no GPU: every fp16 data entry point has a `_bf16` twin with the same parameter list, declared in the
header, exported by the library and bound in deft_amd._lib; null pointers come back as an error code with a message; the Python
operators take float16 or bfloat16 and refuse anything else, and refuse a call whose tensors do not share one element type."""
import ctypes
import os
import re

import pytest
import torch

import deft_amd
from deft_amd._lib import ELEM_ENTRY_POINTS, EXPORTED, LIB_PATH, entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _declarations():
    """{name: parameter list with comments removed and whitespace collapsed} of every function the header declares."""
    header = open(os.path.join(ROOT, "include", "deft_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(deft_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header)}


def test_every_f16_entry_point_has_a_bf16_twin_with_the_same_parameters():
    decl = _declarations()
    f16 = sorted(n for n in decl if n.endswith("_f16"))
    assert len(f16) == 12 and sorted(n[:-4] for n in f16) == sorted(ELEM_ENTRY_POINTS), f16
    so = ctypes.CDLL(LIB_PATH)
    for name in f16:
        twin = name[:-4] + "_bf16"
        assert twin in decl, f"{twin} is not declared"
        assert decl[twin] == decl[name], (name, decl[name], decl[twin])
        assert hasattr(so, twin) and twin in EXPORTED, twin
        assert getattr(deft_amd.lib, twin).argtypes == getattr(deft_amd.lib, name).argtypes
    assert sorted(n for n in decl if n.endswith("_bf16")) == [n[:-4] + "_bf16" for n in f16]
    assert so.deft_abi_version() == 2  # additive: the version stays


def test_entry_points_are_picked_by_dtype():
    for base in ELEM_ENTRY_POINTS:
        assert entry(base, F16)[1] == base + "_f16" and entry(base, BF16)[1] == base + "_bf16"
        with pytest.raises(TypeError):
            entry(base, F32)


def test_null_pointers_are_reported_not_thrown():
    lib = deft_amd.lib
    rc = lib.deft_flatten_decode_bf16(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 4, 4, 128, 0.1, 0, 0, 0, 0)
    assert rc == -1 and b"null" in lib.deft_last_error()
    rc = lib.deft_node_decode_bf16(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 128, 1, 4, 4, 128, 0.1, 0, 0, 0, 0)
    assert rc == -1 and b"null" in lib.deft_last_error()
    rc = lib.deft_seq_decode_bf16(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 128, 4, 4, 128, 0.1, 0, 0, 0)
    assert rc == -1 and lib.deft_last_error()
    rc = lib.deft_flatten_decode_append_bf16(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 4, 4, 128, 0.1, 0, 0, 0, 0, 1,
                                             0, 0, 0, 0)
    assert rc == -1 and b"fused append" in lib.deft_last_error()
    node_md = (0, 0, 0, 0, 0, 0, 1, 1, 128, 1, 4, 4, 128, 0.1)
    rc = lib.deft_node_decode_append_bf16(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, *node_md, 0, 0, 0, 0, 1, 0, 0, 0, 0)
    assert rc == -1 and b"fused append" in lib.deft_last_error()
    rc = lib.deft_seq_decode_append_bf16(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 128, 4, 4, 128, 0.1, 0, 0, 0, 0, 1, 0, 0, 0)
    assert rc == -1 and b"fused append" in lib.deft_last_error()
    rc = lib.deft_flatten_decode_rope_append_bf16(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 4, 4, 128, 0.1, 0, 0, 0, 0, 1,
                                                  0, 128, 1, 0, 0, 0, 0)
    assert rc == -1 and b"fused append" in lib.deft_last_error()
    rc = lib.deft_node_decode_rope_append_bf16(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, *node_md, 0, 0, 0, 0, 1, 0, 128, 1, 0, 0, 0, 0)
    assert rc == -1 and b"fused append" in lib.deft_last_error()
    assert lib.deft_kv_append_bf16(0, 0, 0, 0, 0, 0, 0, 0, 1, 4, 128, 0) == -1 and b"kv_append" in lib.deft_last_error()
    assert lib.deft_rope_qk_bf16(0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 128, 1, 128, 128, 1, 0) == -1 and b"rope" in lib.deft_last_error()
    assert lib.deft_prefill_bf16(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 4, 4, 4, 128, 0.1, 0) == -1
    assert b"prefill" in lib.deft_last_error()
    assert lib.deft_flatten_stage1_bf16(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 4, 4, 128, 0.1, 0, 0, 0, 0) == -1


def _flatten_call(q, k, v, o):
    i64 = torch.zeros(128, dtype=torch.int64)
    deft_amd.tree_attention_subtree_fwd(q, k, v, o, 128, i64[:1], i64[:1], i64[:1], i64, i64, i64[:1])


def _node_call(q, k, v, o):
    i64 = torch.zeros(128, dtype=torch.int64)
    deft_amd.tree_attention_fwd(q, k, v, o, i64, i64[:1], i64[:1], i64[:1], i64[:1], i64[:1])


@pytest.mark.parametrize("call", [_flatten_call, _node_call], ids=["flatten", "node"])
def test_tree_operators_refuse_mixed_dtypes_and_fp32(call):
    def t(dtype, n=1):
        return torch.zeros(n, 4, 128, dtype=dtype)

    for dq, dk, dv, do in ((BF16, F16, F16, BF16), (BF16, BF16, F16, BF16), (F16, BF16, BF16, F16), (BF16, BF16, BF16, F16),
                           (F32, F32, F32, F32), (F32, BF16, BF16, F32)):
        with pytest.raises(TypeError):
            call(t(dq), t(dk, 8), t(dv, 8), t(do))
    # one element type, CPU tensors: past the dtype checks, stopped by the device check (there is no CPU path)
    with pytest.raises(deft_amd.DeftLibraryError, match="no CPU path"):
        call(t(BF16), t(BF16, 8), t(BF16, 8), t(BF16))


def test_other_operators_refuse_mixed_dtypes_and_fp32():
    i32 = torch.zeros(1, dtype=torch.int32)
    four = torch.tensor([4], dtype=torch.int32)
    for dq, dk in ((BF16, F16), (F16, BF16), (F32, F32)):
        q, k = torch.zeros(4, 2, 128, dtype=dq), torch.zeros(4, 2, 128, dtype=dk)
        with pytest.raises(TypeError):
            deft_amd.context_attention_fwd(q, k, k, q.clone(), i32, four, 4)
        with pytest.raises(TypeError):
            deft_amd.get_rope(128, 128, 64, 10000.0)(torch.zeros(4, dtype=torch.int64), q.view(4, -1), k.view(4, -1))
        kv_layer = torch.zeros(8, 2, 2, 128, dtype=dq)
        with pytest.raises(TypeError):
            deft_amd.kv_append(kv_layer, torch.zeros(4, dtype=torch.int32), k.view(4, -1), k.view(4, -1))
    q = torch.zeros(4, 2, 128, dtype=BF16)
    with pytest.raises(TypeError):  # the output too
        deft_amd.context_attention_fwd(q, q, q, q.to(F16), i32, four, 4)
    with pytest.raises(deft_amd.DeftLibraryError, match="no CPU path"):
        deft_amd.context_attention_fwd(q, q, q, q.clone(), i32, four, 4)
    with pytest.raises(deft_amd.DeftLibraryError, match="no CPU path"):
        deft_amd.get_rope(128, 128, 64, 10000.0)(torch.zeros(4, dtype=torch.int64), q.view(4, -1), q.view(4, -1).clone())


def test_builders_take_a_dtype_keyword_with_the_old_default():
    import inspect

    from deft_amd.replay import TemplateReplay
    from deft_amd.utils import workloads

    for fn in (workloads.build_tree, workloads.build_forest, workloads.build_forest_tree, TemplateReplay.__init__):
        assert inspect.signature(fn).parameters["dtype"].default is torch.float16, fn


def test_dense_attention_is_tree_truth_and_counts_a_repeated_slot_twice():
    """tools/error_bound.py::dense_attention -- what the bf16 bound's A comes from, and the fuzzers' truth -- equals tests/truth.py::
    tree_truth on paths without a repeated slot; a slot that lies twice on a path (a speculative-decoding merge without its reset)
    counts twice, as attention over the path as a LIST does."""
    from tools.error_bound import bound_bf16, dense_attention
    from truth import tree_truth

    g = torch.Generator().manual_seed(0)
    Hq, Hkv, D = 8, 2, 16
    q = torch.randn((3, Hq * D), generator=g).to(BF16)
    k, v = (torch.randn((40, Hkv, D), generator=g).to(BF16) for _ in range(2))
    paths = [list(range(0, 20)), list(range(0, 12)) + [30, 31, 32], [5]]
    o, A = dense_attention(q, k, v, paths, Hq, Hkv, D ** -0.5, with_abs=True)
    assert float((o - tree_truth(q, k, v, paths, Hq, Hkv, D ** -0.5)).abs().max()) < 1e-13
    assert bool((A >= o.abs() - 1e-15).all()) and bool((bound_bf16(o, A) > 2e-5).all())
    dup = [paths[0] + [3, 3], paths[1] + [0], paths[2]]
    got = dense_attention(q, k, v, dup, Hq, Hkv, D ** -0.5)
    for r, p in enumerate(dup):  # attention over the list, slot by slot
        kk = k[p].double().repeat_interleave(Hq // Hkv, dim=1).transpose(0, 1)
        vv = v[p].double().repeat_interleave(Hq // Hkv, dim=1).transpose(0, 1)
        s = torch.einsum("hd,hsd->hs", q[r].view(Hq, D).double(), kk) * D ** -0.5
        assert float((got[r] - torch.einsum("hs,hsd->hd", torch.softmax(s, dim=-1), vv)).abs().max()) < 1e-13
    assert float((got[0] - o[0]).abs().max()) > 1e-4  # (and it does differ from the set)
