"""The fused quantising append over fp8 KV pools without a GPU: the eight *_decode_append_*_kv8 symbols are declared, listed, exported and
named in INTEGRATION.md; their parameter lists are the 16-bit *_decode_append_* siblings' with the two scale pointers behind
kv_stride_head, in the header and in the ctypes argtypes; a malformed call gets its code and deft_last_error text before the library
touches HIP; the four Python operators name the wrong argument and have no CPU path; the five-name table of the unfused entry points is
what it was (tests/test_kv8_host.py pins it)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import deft_amd
from deft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = deft_amd.lib
P = 0x1000  # a non-null, 16-byte aligned "pointer"
FP8, F16, BF16, F32 = torch.float8_e4m3fn, torch.float16, torch.bfloat16, torch.float32
NEW = ("deft_flatten_decode_append{}_kv8", "deft_flatten_decode_append{}_kv8_lse", "deft_node_decode_append{}_kv8",
       "deft_node_decode_append{}_kv8_lse")
UNFUSED = ("deft_flatten_decode{}_kv8", "deft_flatten_decode{}_kv8_lse", "deft_node_decode{}_kv8", "deft_node_decode{}_kv8_lse",
           "deft_kv_append{}_kv8")


def test_eight_symbols_are_declared_listed_exported_and_documented():
    header = open(os.path.join(ROOT, "include", "deft_amd.h")).read()
    declared = set(re.findall(r"\b(deft_[a-z0-9_]+)\s*\(", header))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert tuple(_lib.KV8_APPEND_ENTRY_POINTS) == NEW
    assert tuple(_lib.KV8_ENTRY_POINTS) == UNFUSED  # unchanged: the new names live in a tuple of their own
    names = [base.format(sfx) for base in NEW for sfx in ("_f16", "_bf16")]
    assert len(set(names)) == 8
    for base in NEW:
        for sfx, dtype in (("_f16", F16), ("_bf16", BF16)):
            name = base.format(sfx)
            assert name in declared and name in _lib.EXPORTED and name in defined, name
            assert _lib.entry(base, dtype)[1] == name
            assert not name.endswith("_f16") and not name.endswith("_bf16")  # (those names are the plain surface's)
            assert name in integration, name
    assert declared == set(_lib.EXPORTED) == defined and len(_lib.EXPORTED) == len(set(_lib.EXPORTED))  # the three tables stay equal
    assert ctypes.CDLL(_lib.LIB_PATH).deft_abi_version() == 2  # additive: the version stays


def test_parameter_lists_are_the_16_bit_append_siblings_plus_the_two_scales():
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "deft_amd.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(deft_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header)}
    scales = "const float* k_scale, const float* v_scale, "
    vp = ctypes.c_void_p
    for plain in ("deft_flatten_decode_append", "deft_node_decode_append"):
        for sfx in ("_f16", "_bf16"):
            want = decl[plain + sfx].replace("int64_t kv_stride_head, ", "int64_t kv_stride_head, " + scales)
            assert want != decl[plain + sfx] and decl[plain + sfx + "_kv8"] == want, plain + sfx
            want_lse = decl[plain + sfx + "_lse"].replace("int64_t kv_stride_head, ", "int64_t kv_stride_head, " + scales)
            assert want_lse != decl[plain + sfx + "_lse"] and decl[plain + sfx + "_kv8_lse"] == want_lse, plain + sfx
            plain_types = list(getattr(lib, plain + sfx).argtypes)
            kv8_types = plain_types[:7] + [vp, vp] + plain_types[7:]
            assert list(getattr(lib, plain + sfx + "_kv8").argtypes) == kv8_types
            assert list(getattr(lib, plain + sfx + "_kv8_lse").argtypes) == kv8_types[:12] + [vp, ctypes.c_int64, ctypes.c_int64] + kv8_types[12:]
            assert getattr(lib, plain + sfx + "_kv8").restype == ctypes.c_int and getattr(lib, plain + sfx + "_kv8_lse").restype == ctypes.c_int


# ---- malformed calls: code and text, before any HIP call ---------------------------------------------------------------------------
_QKV = dict(q=P, q_stride_tok=1024, q_stride_head=128, k_base=P, v_base=P, kv_stride_slot=512, kv_stride_head=128, k_scale=0, v_scale=0)
_OUT = dict(out=P, o_stride_tok=1024, o_stride_head=128)
_LSE = dict(lse=P, lse_stride_tok=8, lse_stride_head=1)
_BLOCKS = dict(block_q=P, block_q_cnts=P, block_q_offset=P, block_bitmasks=P, block_kv=P, block_lens=P)
_NODES = dict(node_kv=P, node_kv_offset=P, node_kv_len=P, node_q=P, node_q_offset=P, node_q_len=P)
_FDIMS = dict(NB=1, P=1, nq=1, Hq=8, Hkv=2, D=128, scale=0.088)
_NDIMS = dict(NE=1, P=1, total_kv=128, nq=1, Hq=8, Hkv=2, D=128, scale=0.088)
_APPEND = dict(cache_loc=P, k_new=P, v_new=P, new_stride_tok=256, n_new=1)
_SCRATCH = dict(plan=0, workspace=P, workspace_bytes=0, stream=0)
SPEC = {
    "deft_flatten_decode_append{}_kv8": {**_QKV, **_OUT, **_BLOCKS, **_FDIMS, **_APPEND, **_SCRATCH},
    "deft_flatten_decode_append{}_kv8_lse": {**_QKV, **_OUT, **_LSE, **_BLOCKS, **_FDIMS, **_APPEND, **_SCRATCH},
    "deft_node_decode_append{}_kv8": {**_QKV, **_OUT, **_NODES, **_NDIMS, **_APPEND, **_SCRATCH},
    "deft_node_decode_append{}_kv8_lse": {**_QKV, **_OUT, **_LSE, **_NODES, **_NDIMS, **_APPEND, **_SCRATCH},
}
_D = "fp8 KV pool: head_dim {} is not supported (head_dim must be 128; 64, 32 and 16 are not built for fp8 pools)"
_ODD = "fp8 KV pool: odd slot stride 511 (the plan addresses rows in 2-byte units)"
_ALIGN = "fp8 KV pool: base pointers and the slot stride must be 16-byte aligned, the head stride a multiple of 16"
_SCALE = "fp8 KV pool: k_scale / v_scale must be 4-byte aligned"
_NEEDS = "fused append needs k_new, v_new and cache_loc"  # (make_append's refusal, the 16-bit append entry points' own)
ROWS = (
    # a well-formed call reaches the workspace check: the sizes are the 16-bit call's and the unfused kv8 call's (tests/test_kv8_host.py)
    [(n, dict(), -4, "workspace too small: 0 < " + ("20480" if "flatten" in n else "33280")) for n in NEW]
    + [(n, dict(D=64, kv_stride_head=64), -2, _D.format(64)) for n in NEW]
    + [(n, dict(D=32), -2, _D.format(32)) for n in NEW]
    + [(n, dict(kv_stride_slot=511), -1, _ODD) for n in NEW]
    + [(n, dict(kv_stride_slot=520), -1, _ALIGN) for n in NEW]
    + [(n, dict(k_base=P + 8), -1, _ALIGN) for n in NEW]
    + [(n, dict(kv_stride_head=136), -1, _ALIGN) for n in NEW]
    + [(n, dict(k_scale=P + 2), -1, _SCALE) for n in NEW]
    + [(n, dict(v_scale=P + 1), -1, _SCALE) for n in NEW]
    + [(n, dict(k_new=0), -1, _NEEDS) for n in NEW]
    + [(n, dict(v_new=0), -1, _NEEDS) for n in NEW]
    + [(n, dict(cache_loc=0), -1, _NEEDS) for n in NEW]
    + [(n, dict(cache_loc=0, n_new=0), -1, _NEEDS) for n in NEW]  # (all three are required whatever n_new says, as for the 16-bit calls)
    + [(n, dict(D=64, q=0), -2, _D.format(64)) for n in NEW]  # (order: the pool's own checks come before the tensors')
    + [(n, dict(q=0), -1, "null tensor pointer") for n in NEW]
    + [(n, dict(new_stride_tok=100), -1, "bad fused-append arguments (n_new=1 new_stride=100)") for n in NEW]
    + [(n, dict(k_new=P + 8), -1, "bad fused-append arguments (n_new=1 new_stride=256)") for n in NEW]
    + [(n, dict(workspace=0), -1, "null workspace") for n in NEW]
    + [(n, dict(lse=0), -1, "null lse (the plain entry point returns no log-sum-exp)") for n in NEW if n.endswith("_lse")]
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
    assert len(args) == len(getattr(lib, fn).argtypes), fn
    rc = getattr(lib, fn)(*args.values())
    assert rc == code, (fn, rc, lib.deft_last_error())
    assert lib.deft_last_error().decode() == msg


# ---- the Python operators, on CPU tensors --------------------------------------------------------------------------------------------
_MD = [torch.zeros(1, dtype=torch.int64)] * 6


def _operators():
    return ((deft_amd.flatten_append_attention_kv8, (128, *_MD), False), (deft_amd.node_append_attention_kv8, tuple(_MD), False),
            (deft_amd.flatten_append_attention_kv8_lse, (128, *_MD), True), (deft_amd.node_append_attention_kv8_lse, tuple(_MD), True))


def test_operators_are_exported_and_name_the_wrong_argument():
    from deft_amd import states

    Hq, Hkv, D, nq = 4, 2, 128, 3
    q = torch.zeros((nq, Hq, D), dtype=F16)
    o = torch.zeros_like(q)
    kv = torch.zeros((16, 2, Hkv, D), dtype=torch.uint8).view(FP8)
    loc = torch.zeros(nq, dtype=torch.int32)
    new = torch.zeros((nq, Hkv * D), dtype=F16)
    ones = torch.ones(Hkv, dtype=F32)
    for fn, md, with_lse in _operators():
        assert fn.__name__ in states.__all__ and getattr(states, fn.__name__) is fn
        lse = (torch.zeros((nq, Hq), dtype=F32),) if with_lse else ()

        def call(q_=q, kv_=kv, o_=o, k_=new, v_=new, lse_=lse, **kw):
            return fn(q_, kv_, o_, *lse_, loc, k_, v_, *md, **kw)

        with pytest.raises(TypeError, match="kv_layer"):
            call(kv_=torch.zeros((16, 2, Hkv, D), dtype=F16))
        with pytest.raises(TypeError, match="output"):
            call(o_=o.to(BF16))
        with pytest.raises(TypeError, match="query_states"):
            call(q_=q.to(F32))
        with pytest.raises(TypeError, match="cache_k"):
            call(k_=new.to(BF16))
        with pytest.raises(TypeError, match="cache_v"):
            call(v_=new.to(F32))
        with pytest.raises(TypeError, match="k_scale"):
            call(k_scale=ones.to(torch.float64))
        with pytest.raises(TypeError, match="v_scale"):
            call(v_scale=torch.ones(3, dtype=F32))
        with pytest.raises(TypeError, match="k_scale"):
            call(k_scale=[1.0, 1.0])
        if with_lse:
            with pytest.raises(TypeError, match="lse"):
                call(lse_=(None,))
            with pytest.raises(TypeError, match="lse"):
                call(lse_=(torch.zeros((nq, Hq), dtype=F16),))
        with pytest.raises(deft_amd.DeftLibraryError, match="CUDA"):  # well-typed CPU tensors: no CPU path
            call(k_scale=ones, v_scale=ones)
        with pytest.raises(deft_amd.DeftLibraryError, match="CUDA"):
            call()
