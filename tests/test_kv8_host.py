"""fp8 KV pools without a GPU: the ten *_kv8 symbols are declared, listed and exported with the stated parameter lists; a malformed call
gets its pinned code and deft_last_error text before the library touches HIP; the fp8 pool's shape, dtype and scales; every refusal of
an fp8 pool by the parts that do not read one; the model's self-checks (tests/kv8_model.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import deft_amd
import kv8_model
from deft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = deft_amd.lib
P = 0x1000  # a non-null, 16-byte aligned "pointer"
FP8, F16, BF16, F32 = torch.float8_e4m3fn, torch.float16, torch.bfloat16, torch.float32
NEW = ("deft_flatten_decode{}_kv8", "deft_flatten_decode{}_kv8_lse", "deft_node_decode{}_kv8", "deft_node_decode{}_kv8_lse",
       "deft_kv_append{}_kv8")


def test_model_self_checks():
    kv8_model.self_check()
    assert kv8_model.edge_inputs().numel() > 254 + 2 * 126


def test_ten_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "deft_amd.h")).read()
    declared = set(re.findall(r"\b(deft_[a-z0-9_]+)\s*\(", header))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert tuple(_lib.KV8_ENTRY_POINTS) == NEW
    names = [base.format(sfx) for base in NEW for sfx in ("_f16", "_bf16")]
    assert len(set(names)) == 10
    for base in NEW:
        for sfx, dtype in (("_f16", F16), ("_bf16", BF16)):
            name = base.format(sfx)
            assert name in declared and name in _lib.EXPORTED and name in defined, name
            assert _lib.entry(base, dtype)[1] == name
            assert not name.endswith("_f16") and not name.endswith("_bf16")  # (those names are the plain surface's: tests/test_bf16_host.py)
            assert name in integration, name
    assert declared == set(_lib.EXPORTED) == defined and len(_lib.EXPORTED) == len(set(_lib.EXPORTED))  # the three tables stay equal
    assert ctypes.CDLL(_lib.LIB_PATH).deft_abi_version() == 2  # additive: the version stays


def test_kv8_siblings_take_the_plain_parameter_list_plus_the_two_scales():
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "deft_amd.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(deft_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header)}
    scales = "const float* k_scale, const float* v_scale, "
    vp = ctypes.c_void_p
    for plain, at in (("deft_flatten_decode", 7), ("deft_node_decode", 7), ("deft_kv_append", 4)):
        for sfx in ("_f16", "_bf16"):
            want = decl[plain + sfx].replace("int64_t kv_stride_head, ", "int64_t kv_stride_head, " + scales)
            assert want != decl[plain + sfx] and decl[plain + sfx + "_kv8"] == want, plain + sfx
            plain_types = list(getattr(lib, plain + sfx).argtypes)
            kv8_types = plain_types[:at] + [vp, vp] + plain_types[at:]
            assert list(getattr(lib, plain + sfx + "_kv8").argtypes) == kv8_types
            if plain != "deft_kv_append":  # ... and the _kv8_lse form is the _lse sibling with the same two pointers
                want_lse = decl[plain + sfx + "_lse"].replace("int64_t kv_stride_head, ", "int64_t kv_stride_head, " + scales)
                assert decl[plain + sfx + "_kv8_lse"] == want_lse, plain + sfx
                assert list(getattr(lib, plain + sfx + "_kv8_lse").argtypes) == kv8_types[:12] + [vp, ctypes.c_int64, ctypes.c_int64] + kv8_types[12:]


# ---- malformed calls: code and text, before any HIP call ---------------------------------------------------------------------------
_QKV = dict(q=P, q_stride_tok=1024, q_stride_head=128, k_base=P, v_base=P, kv_stride_slot=512, kv_stride_head=128, k_scale=0, v_scale=0)
_OUT = dict(out=P, o_stride_tok=1024, o_stride_head=128)
_LSE = dict(lse=P, lse_stride_tok=8, lse_stride_head=1)
_BLOCKS = dict(block_q=P, block_q_cnts=P, block_q_offset=P, block_bitmasks=P, block_kv=P, block_lens=P)
_NODES = dict(node_kv=P, node_kv_offset=P, node_kv_len=P, node_q=P, node_q_offset=P, node_q_len=P)
_FDIMS = dict(NB=1, P=1, nq=1, Hq=8, Hkv=2, D=128, scale=0.088)
_NDIMS = dict(NE=1, P=1, total_kv=128, nq=1, Hq=8, Hkv=2, D=128, scale=0.088)
_SCRATCH = dict(plan=0, workspace=P, workspace_bytes=0, stream=0)
SPEC = {
    "deft_flatten_decode{}_kv8": {**_QKV, **_OUT, **_BLOCKS, **_FDIMS, **_SCRATCH},
    "deft_flatten_decode{}_kv8_lse": {**_QKV, **_OUT, **_LSE, **_BLOCKS, **_FDIMS, **_SCRATCH},
    "deft_node_decode{}_kv8": {**_QKV, **_OUT, **_NODES, **_NDIMS, **_SCRATCH},
    "deft_node_decode{}_kv8_lse": {**_QKV, **_OUT, **_LSE, **_NODES, **_NDIMS, **_SCRATCH},
    "deft_kv_append{}_kv8": dict(k_base=P, v_base=P, kv_stride_slot=512, kv_stride_head=128, k_scale=0, v_scale=0, cache_loc=P, k_new=P,
                                v_new=P, new_stride_tok=256, n=1, Hkv=2, D=128, stream=0),
}
_D = "fp8 KV pool: head_dim {} is not supported (head_dim must be 128; 64, 32 and 16 are not built for fp8 pools)"
_ODD = "fp8 KV pool: odd slot stride 511 (the plan addresses rows in 2-byte units)"
_ALIGN = "fp8 KV pool: base pointers and the slot stride must be 16-byte aligned, the head stride a multiple of 16"
_BADAPP = "kv_append (fp8 pool): new rows must be 16-byte aligned, pool rows 8-byte aligned"
DECODE = [n for n in NEW if "decode" in n]
ROWS = (
    # the workspace sizes are the 16-bit call's (tests/test_states_host.py pins the same figures): they do not depend on the pool's type
    [(n, dict(), -4, "workspace too small: 0 < " + ("20480" if "flatten" in n else "33280")) for n in DECODE]
    + [(n, dict(D=64, kv_stride_head=64), -2, _D.format(64)) for n in DECODE]
    + [(n, dict(D=32), -2, _D.format(32)) for n in DECODE]
    + [(n, dict(kv_stride_slot=511), -1, _ODD) for n in DECODE]
    + [(n, dict(k_base=P + 8), -1, _ALIGN) for n in DECODE]
    + [(n, dict(v_base=P + 1), -1, _ALIGN) for n in DECODE]
    + [(n, dict(kv_stride_slot=520), -1, _ALIGN) for n in DECODE]
    + [(n, dict(kv_stride_head=136), -1, _ALIGN) for n in DECODE]
    + [(n, dict(k_scale=P + 2), -1, "fp8 KV pool: k_scale / v_scale must be 4-byte aligned") for n in DECODE]
    + [(n, dict(q=0), -1, "null tensor pointer") for n in DECODE]
    + [(n, dict(workspace=0), -1, "null workspace") for n in DECODE]
    + [(n, dict(D=64, q=0), -2, _D.format(64)) for n in DECODE]  # (order: the pool's own checks come first)
    + [(n, dict(lse=0), -1, "null lse (the plain entry point returns no log-sum-exp)") for n in DECODE if n.endswith("_lse")]
    + [("deft_kv_append{}_kv8", dict(n=0), 0, None),
       ("deft_kv_append{}_kv8", dict(k_base=0), -1, "bad kv_append arguments (n=1 Hkv=2 D=128)"),
       ("deft_kv_append{}_kv8", dict(D=12), -1, "bad kv_append arguments (n=1 Hkv=2 D=12)"),
       ("deft_kv_append{}_kv8", dict(k_new=P + 8), -1, _BADAPP),
       ("deft_kv_append{}_kv8", dict(k_base=P + 4), -1, _BADAPP),
       ("deft_kv_append{}_kv8", dict(kv_stride_slot=508), -1, _BADAPP)]
)


def _cases():
    for name, overrides, code, msg in ROWS:
        for fn in (name.format("_f16"), name.format("_bf16")):
            ident = fn + "(" + ", ".join(f"{k}={v:#x}" if v >= P else f"{k}={v}" for k, v in overrides.items()) + ")"
            yield pytest.param(fn, name, overrides, code, msg, id=ident)


@pytest.mark.parametrize("fn, name, overrides, code, msg", _cases())
def test_malformed_calls_get_their_code_and_text(fn, name, overrides, code, msg):
    args = dict(SPEC[name])
    assert set(overrides) <= set(args), (fn, overrides)
    args.update(overrides)
    rc = getattr(lib, fn)(*args.values())
    assert rc == code, (fn, rc, lib.deft_last_error())
    if msg is not None:
        assert lib.deft_last_error().decode() == msg


# ---- the pool ------------------------------------------------------------------------------------------------------------------------
def test_fp8_pool_shape_dtype_and_scales():
    pool = deft_amd.TokenToKVPool(40, FP8, 3, 128, 2, device="cpu")
    assert pool.is_fp8 and pool._storage.shape == (2, 40, 2, 3, 128) and pool._storage.dtype == FP8
    assert pool._storage.element_size() == 1 and pool.kv_data[1].stride(0) == 2 * 3 * 128
    assert pool.get_key_buffer(1).shape == (40, 3, 128) and pool.get_value_buffer(0).dtype == FP8
    for s in (pool.k_scale, pool.v_scale):
        assert s.shape == (2, 3) and s.dtype == F32 and s.device == pool._storage.device and bool((s == 1).all())
    pool.set_kv_scales(1, [0.5, 1.0, 2.0], torch.tensor([3.0, 4.0, 5.0]))
    assert pool.k_scale[1].tolist() == [0.5, 1.0, 2.0] and pool.v_scale[1].tolist() == [3.0, 4.0, 5.0]
    assert bool((pool.k_scale[0] == 1).all()) and bool((pool.v_scale[0] == 1).all())
    with pytest.raises(ValueError, match="k_scale"):
        pool.set_kv_scales(0, [1.0, 2.0], [1.0, 1.0, 1.0])
    plain = deft_amd.TokenToKVPool(8, F16, 3, 128, 1, device="cpu")
    assert not plain.is_fp8 and plain.k_scale is None and plain.v_scale is None
    with pytest.raises(TypeError, match="float8_e4m3fn"):
        plain.set_kv_scales(0, [1.0] * 3, [1.0] * 3)


# ---- refusals, on CPU tensors ----------------------------------------------------------------------------------------------------------
def _cpu(Hq=4, Hkv=2, D=128, nq=3, slots=16, dtype=F16):
    q = torch.zeros((nq, Hq, D), dtype=dtype)
    kv = torch.zeros((slots, 2, Hkv, D), dtype=torch.uint8).view(FP8)
    return q, kv, torch.zeros_like(q)


_MD = [torch.zeros(1, dtype=torch.int64)] * 6


def test_generic_operators_refuse_an_fp8_pool_with_type_error():
    q, kv, o = _cpu()
    kb, vb = kv[:, 0], kv[:, 1]
    loc = torch.zeros(3, dtype=torch.int32)
    new = torch.zeros((3, 2 * 128), dtype=F16)
    lse = torch.zeros((3, 4), dtype=F32)
    with pytest.raises(TypeError, match="key_buffer"):
        deft_amd.tree_attention_subtree_fwd(q, kb, vb, o, 128, *_MD)
    with pytest.raises(TypeError, match="key_buffer"):
        deft_amd.tree_attention_fwd(q, kb, vb, o, *_MD)
    with pytest.raises(TypeError, match="key_buffer"):
        deft_amd.tree_attention_subtree_fwd_lse(q, kb, vb, o, lse, 128, *_MD)
    with pytest.raises(TypeError, match="key_buffer"):
        deft_amd.flatten_append_attention_lse(q, kv, o, lse, loc, new, new, 128, *_MD)
    with pytest.raises(TypeError, match="kv_layer"):
        deft_amd.kv_append(kv, loc, new, new)


def test_kv8_operators_name_the_wrong_argument():
    q, kv, o = _cpu()
    kb, vb = kv[:, 0], kv[:, 1]
    ones = torch.ones(2, dtype=F32)
    f16_pool = torch.zeros((16, 2, 128), dtype=F16)
    for fn, md in ((deft_amd.tree_attention_subtree_fwd_kv8, (128, *_MD)), (deft_amd.tree_attention_fwd_kv8, tuple(_MD))):
        with pytest.raises(TypeError, match="key_buffer"):
            fn(q, f16_pool, f16_pool, o, *md)
        with pytest.raises(TypeError, match="value_buffer"):
            fn(q, kb, f16_pool, o, *md)
        with pytest.raises(TypeError, match="output"):
            fn(q, kb, vb, o.to(BF16), *md)
        with pytest.raises(TypeError, match="query_states"):
            fn(q.to(F32), kb, vb, o, *md)
        with pytest.raises(TypeError, match="k_scale"):
            fn(q, kb, vb, o, *md, k_scale=ones.to(torch.float64))
        with pytest.raises(TypeError, match="v_scale"):
            fn(q, kb, vb, o, *md, v_scale=torch.ones(3, dtype=F32))
        with pytest.raises(TypeError, match="k_scale"):
            fn(q, kb, vb, o, *md, k_scale=[1.0, 1.0])
        with pytest.raises(deft_amd.DeftLibraryError, match="CUDA"):  # well-typed CPU tensors: no CPU path, like the 16-bit operators
            fn(q, kb, vb, o, *md, k_scale=ones, v_scale=ones)
    with pytest.raises(TypeError, match="lse"):
        deft_amd.tree_attention_subtree_fwd_kv8_lse(q, kb, vb, o, None, 128, *_MD)
    with pytest.raises(TypeError, match="lse"):
        deft_amd.tree_attention_fwd_kv8_lse(q, kb, vb, o, torch.zeros((3, 4), dtype=F16), *_MD)
    loc = torch.zeros(3, dtype=torch.int32)
    new = torch.zeros((3, 2 * 128), dtype=F16)
    with pytest.raises(TypeError, match="kv_layer"):
        deft_amd.kv_append_kv8(torch.zeros((16, 2, 2, 128), dtype=F16), loc, new, new)
    with pytest.raises(TypeError, match="cache_v"):
        deft_amd.kv_append_kv8(kv, loc, new, new.to(BF16))
    with pytest.raises(TypeError, match="cache_k"):
        deft_amd.kv_append_kv8(kv, loc, new.to(F32), new)
    with pytest.raises(TypeError, match="v_scale"):
        deft_amd.kv_append_kv8(kv, loc, new, new, ones, torch.ones(5, dtype=F32))
    with pytest.raises(deft_amd.DeftLibraryError, match="CUDA"):
        deft_amd.kv_append_kv8(kv, loc, new, new, ones, ones)


def _fp8_tree(Hkv=2, D=128):
    req = deft_amd.ReqToTokenPool(8, 64, device="cpu")
    pool = deft_amd.TokenToKVPool(64, FP8, Hkv, D, 1, device="cpu")
    tree = deft_amd.TreeCache(F16, Hkv, D, 1, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, 9, dtype=torch.int32))
    tree.branch(tree.root, 2)
    return tree, pool, req


def test_everything_else_refuses_an_fp8_pool_loudly():
    """NotImplementedError whose text names fp8: extend steps, the sequential comparator, the rope-fused path, prefill onto a cached
    prefix, DecodeSession, Forest -- on CPU tensors, before any library call."""
    tree, pool, req = _fp8_tree()
    Hq, Hkv, D = 4, 2, 128
    attn = deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, 0)
    q = torch.zeros((2, Hq * D), dtype=F16)
    k = torch.zeros((2, Hkv * D), dtype=F16)
    upd = deft_amd.KVCacheUpdater(True, pool, torch.zeros(2, dtype=torch.int32), None, False)
    for mode in (deft_amd.ForwardMode.EXTEND, deft_amd.ForwardMode.DECODE):
        with pytest.raises(NotImplementedError, match="fp8"):
            attn(q, k, k, deft_amd.InputMetadata(mode, upd, pool))
    with pytest.raises(NotImplementedError, match="fp8"):
        attn(q, k, k, deft_amd.InputMetadata(deft_amd.ForwardMode.TREE_DECODE_FLATTEN, upd, pool), rotary_emb=object(),
             positions=torch.zeros(2, dtype=torch.int64), fuse_rope=True)
    q3, kv, o = _cpu(Hq, Hkv, D, 2, 64)
    table = torch.zeros((8, 64), dtype=torch.int32)
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="fp8"):
        deft_amd.token_attention_fwd(q3, kv[:, 0], kv[:, 1], o, table, z, z, z, 8, 0, 16)
    with pytest.raises(NotImplementedError, match="fp8"):
        deft_amd.prefill_with_cached_prefix(q3, q3[:, :Hkv], q3[:, :Hkv], o, kv, [0, 1, 2], [3, 4])
    with pytest.raises(NotImplementedError, match="fp8"):
        deft_amd.DecodeSession(tree, Hq, Hkv, D, 1, lambda l: (q, k, k))
    with pytest.raises(NotImplementedError, match="fp8"):
        deft_amd.Forest([tree])
