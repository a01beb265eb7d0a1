"""DecodeSession over an fp8 KV pool without a GPU: what the constructor accepts and refuses -- `elem_dtype` (the 16-bit type of q, the new
rows and the outputs, which an fp8 pool does not name), head_dim 128 only -- on CPU tensors, before the device assertion and before any
library call; and the C surface stays what it was (no new symbol: the two-launch form's window steps go through deft_window_patch with
a new-row stride of 0)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import deft_amd
from deft_amd import _lib
from test_kv8_host import _fp8_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8, F16, BF16, F32 = torch.float8_e4m3fn, torch.float16, torch.bfloat16, torch.float32
Hq, Hkv, D = 4, 2, 128


def _qkv(dtype=F16):
    q = torch.zeros((2, Hq * D), dtype=dtype)
    k = torch.zeros((2, Hkv * D), dtype=dtype)
    return lambda l: (q, k, k)


def _f16_tree(dtype=F16):
    req = deft_amd.ReqToTokenPool(8, 64, device="cpu")
    pool = deft_amd.TokenToKVPool(64, dtype, Hkv, D, 1, device="cpu")
    tree = deft_amd.TreeCache(dtype, Hkv, D, 1, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, 9, dtype=torch.int32))
    tree.branch(tree.root, 2)
    return tree


@pytest.mark.parametrize("cls", [deft_amd.DecodeSession, deft_amd.FlattenDecodeSession])
def test_fp8_pool_without_elem_dtype_is_still_refused_and_the_text_names_the_argument(cls):
    tree, _, _ = _fp8_tree()
    with pytest.raises(NotImplementedError, match="fp8") as e:
        cls(tree, Hq, Hkv, D, 1, _qkv())
    assert "elem_dtype" in str(e.value)


@pytest.mark.parametrize("cls", [deft_amd.DecodeSession, deft_amd.FlattenDecodeSession])
@pytest.mark.parametrize("bad", [F32, torch.float64, FP8, torch.int8])
def test_fp8_pool_takes_a_16_bit_elem_dtype_only(cls, bad):
    tree, _, _ = _fp8_tree()
    with pytest.raises(TypeError, match="elem_dtype"):
        cls(tree, Hq, Hkv, D, 1, _qkv(), elem_dtype=bad)


@pytest.mark.parametrize("elem", [F16, BF16])
def test_head_dim_64_over_an_fp8_pool_is_a_value_error_that_names_fp8(elem):
    tree, _, _ = _fp8_tree(Hkv=2, D=64)
    with pytest.raises(ValueError, match="fp8"):
        deft_amd.DecodeSession(tree, Hq, Hkv, 64, 1, _qkv(elem), elem_dtype=elem)
    with pytest.raises(ValueError, match="fp8"):  # (whichever form is asked for)
        deft_amd.DecodeSession(tree, Hq, Hkv, 64, 1, _qkv(elem), elem_dtype=elem, kv8_fused_append=True)


@pytest.mark.parametrize("pool_dtype, elem", [(F16, BF16), (BF16, F16), (F16, F32)])
def test_16_bit_pool_refuses_another_elem_dtype(pool_dtype, elem):
    tree = _f16_tree(pool_dtype)
    with pytest.raises(TypeError, match="elem_dtype"):
        deft_amd.DecodeSession(tree, Hq, Hkv, D, 1, _qkv(pool_dtype), elem_dtype=elem)


@pytest.mark.parametrize("kw", [dict(elem_dtype=F16), dict(elem_dtype=BF16, kv8_fused_append=True), dict(elem_dtype=F16, kv8_fused_append=False)])
def test_every_check_comes_before_the_device_assertion(kw):
    """A well-formed fp8 session over CPU tensors gets as far as the device assertion (there is no CPU path), and so does a 16-bit
    session that names its pool's own type -- `kv8_fused_append` is ignored there."""
    tree, _, _ = _fp8_tree()
    with pytest.raises(AssertionError):
        deft_amd.DecodeSession(tree, Hq, Hkv, D, 1, _qkv(kw["elem_dtype"]), **kw)
    with pytest.raises(AssertionError):
        deft_amd.DecodeSession(_f16_tree(), Hq, Hkv, D, 1, _qkv(), elem_dtype=F16, kv8_fused_append=True)


def test_class_defaults_are_booleans():
    assert isinstance(deft_amd.DecodeSession.kv8_fused_append, bool) and isinstance(deft_amd.DecodeSession.kv8_fused_append_window, bool)


def test_the_c_surface_is_unchanged():
    """Header, exports and binding stay equal, and no symbol was added for the session: the patch kernel's pool-offset form is chosen by
    deft_window_patch's existing new_stride_tok argument."""
    header = open(os.path.join(ROOT, "include", "deft_amd.h")).read()
    declared = set(re.findall(r"\b(deft_[a-z0-9_]+)\s*\(", header))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    exports = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "deft_amd", "csrc", "exports.map")).read(), flags=re.S)
    assert declared == set(_lib.EXPORTED) == defined
    assert re.findall(r"global:\s*([^;]+);", exports) == ["deft_*"] and all(n.startswith("deft_") for n in defined)
    assert ctypes.CDLL(_lib.LIB_PATH).deft_abi_version() == 2
    # deft_window_patch with a new-row stride of 0 is a call like any other: refused only for what it always refused
    P = 0x1000
    args = [0, 1, 1, P, P, P, P, P, P, P, P, 0, 0, 0, 0, P, P, P, 32, 1, 8, 2, 256, 0, P, 0, 0, 0, 0, 0, 0]
    assert deft_amd.lib.deft_window_patch(*args) == -1
    assert deft_amd.lib.deft_last_error().decode() == "deft_window_patch: bad arguments (nodes=0 nq=1 tiles=1)"
