"""Attention states without a GPU: the twelve new symbols are declared, listed and exported; a malformed call of each gets its pinned
code and deft_last_error text before the library touches HIP (in the manner of tests/test_abi_errors.py: the default arguments of an
entry point are a well-formed call whose scratch size is 0, a row overrides some of them); the Python operators refuse what they
must; cached_prefix_blocks against a direct enumeration."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import deft_amd
from deft_amd import _lib
from deft_amd.tree_attention import flatten_append_attention, node_append_attention  # noqa: F401  (the plain siblings exist)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = deft_amd.lib
P = 0x1000  # a non-null, 16-byte aligned "pointer"
# "{}" = _f16 / _bf16: the element type sits inside the name (deft_flatten_decode_f16_lse = the _lse form of deft_flatten_decode_f16)
NEW = ("deft_flatten_decode{}_lse", "deft_flatten_decode_append{}_lse", "deft_node_decode{}_lse", "deft_node_decode_append{}_lse",
       "deft_prefill{}_lse", "deft_merge{}_states")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def test_new_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "deft_amd.h")).read()
    declared = set(re.findall(r"\b(deft_[a-z0-9_]+)\s*\(", header))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert tuple(_lib.STATE_ENTRY_POINTS) == NEW
    for base in NEW:
        for sfx, dtype in (("_f16", F16), ("_bf16", BF16)):
            name = base.format(sfx)
            assert name in declared and name in _lib.EXPORTED and name in defined, name
            assert _lib.entry(base, dtype)[1] == name
            assert not name.endswith(sfx)  # (names ending in _f16 / _bf16 are the plain surface's: tests/test_bf16_host.py)
    assert declared == set(_lib.EXPORTED) == defined and len(_lib.EXPORTED) == len(set(_lib.EXPORTED))  # the three tables stay equal
    assert ctypes.CDLL(_lib.LIB_PATH).deft_abi_version() == 2  # additive: the version stays


def test_lse_siblings_take_the_plain_parameter_list_plus_lse_behind_out():
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "deft_amd.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(deft_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header)}
    lse = "float* lse, int64_t lse_stride_tok, int64_t lse_stride_head, "
    for plain in ("deft_flatten_decode", "deft_flatten_decode_append", "deft_node_decode", "deft_node_decode_append", "deft_prefill"):
        for sfx in ("_f16", "_bf16"):
            want = decl[plain + sfx].replace("int64_t o_stride_head, ", "int64_t o_stride_head, " + lse)
            assert want != decl[plain + sfx] and decl[plain + sfx + "_lse"] == want, plain + sfx
            plain_types = list(getattr(lib, plain + sfx).argtypes)
            at = 10 if plain != "deft_prefill" else 12
            assert list(getattr(lib, plain + sfx + "_lse").argtypes) == plain_types[:at] + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + plain_types[at:]


_QKV = dict(q=P, q_stride_tok=1024, q_stride_head=128, k_base=P, v_base=P, kv_stride_slot=256, kv_stride_head=128)
_OUT = dict(out=P, o_stride_tok=1024, o_stride_head=128)
_LSE = dict(lse=P, lse_stride_tok=8, lse_stride_head=1)
_BLOCKS = dict(block_q=P, block_q_cnts=P, block_q_offset=P, block_bitmasks=P, block_kv=P, block_lens=P)
_NODES = dict(node_kv=P, node_kv_offset=P, node_kv_len=P, node_q=P, node_q_offset=P, node_q_len=P)
_FDIMS = dict(NB=1, P=1, nq=1, Hq=8, Hkv=2, D=128, scale=0.088)
_NDIMS = dict(NE=1, P=1, total_kv=128, nq=1, Hq=8, Hkv=2, D=128, scale=0.088)
_APPEND = dict(cache_loc=P, k_new=P, v_new=P, new_stride_tok=256, n_new=1)
_SCRATCH = dict(plan=0, workspace=P, workspace_bytes=0, stream=0)
_ST = lambda x: {x: P, x + "_stride_tok": 1024, x + "_stride_head": 128}  # noqa: E731
_SL = lambda x: {x: P, x + "_stride_tok": 8, x + "_stride_head": 1}  # noqa: E731

SPEC = {
    "deft_flatten_decode{}_lse": {**_QKV, **_OUT, **_LSE, **_BLOCKS, **_FDIMS, **_SCRATCH},
    "deft_flatten_decode_append{}_lse": {**_QKV, **_OUT, **_LSE, **_BLOCKS, **_FDIMS, **_APPEND, **_SCRATCH},
    "deft_node_decode{}_lse": {**_QKV, **_OUT, **_LSE, **_NODES, **_NDIMS, **_SCRATCH},
    "deft_node_decode_append{}_lse": {**_QKV, **_OUT, **_LSE, **_NODES, **_NDIMS, **_APPEND, **_SCRATCH},
    # (a prefill call has no scratch to refuse: its well-formed default is the empty batch, which returns DEFT_OK without a launch)
    "deft_prefill{}_lse": dict(q=P, q_stride_tok=1024, q_stride_head=128, k=P, k_stride_tok=256, k_stride_head=128, v=P, v_stride_tok=256,
                             v_stride_head=128, **_OUT, **_LSE, b_start_loc=P, b_seq_len=P, batch=0, max_input_len=4, Hq=8, Hkv=2, D=128,
                             scale=0.088, stream=0),
    # (... nor has a merge: n = 0 returns DEFT_OK behind the checks)
    "deft_merge{}_states": {**_ST("o_a"), **_SL("lse_a"), **_ST("o_b"), **_SL("lse_b"), **_ST("out"), **_SL("lse_out"), "n": 0, "Hq": 8,
                          "D": 128, "stream": 0},
}
_NULL_LSE = "null lse (the plain entry point returns no log-sum-exp)"
_MIS_LSE = "lse must be 4-byte aligned"
_FUSED = "fused append needs k_new, v_new and cache_loc"
_MS_NULL = "merge_states: null state pointer (only lse_out may be null)"

# (entry point, overrides of its defaults, return code, deft_last_error()); rows with two faults pin the ORDER of the checks
ROWS = [
    ("deft_flatten_decode{}_lse", dict(), -4, "workspace too small: 0 < 20480"),  # (the plain call's size: workspace sizes do not change)
    ("deft_flatten_decode{}_lse", dict(lse=0), -1, _NULL_LSE),
    ("deft_flatten_decode{}_lse", dict(lse=P + 2), -1, _MIS_LSE),
    ("deft_flatten_decode{}_lse", dict(lse=0, q=0), -1, "null tensor pointer"),
    ("deft_flatten_decode{}_lse", dict(lse=0, o_stride_tok=1023), -1, "out rows must be 4-byte aligned"),
    ("deft_flatten_decode{}_lse", dict(lse=0, workspace=0), -1, _NULL_LSE),
    ("deft_flatten_decode{}_lse", dict(lse=P + 1, NB=-1), -1, _MIS_LSE),
    ("deft_flatten_decode{}_lse", dict(lse_stride_tok=7, lse_stride_head=3), -4, "workspace too small: 0 < 20480"),  # (any strides)
    ("deft_flatten_decode{}_lse", dict(D=64, kv_stride_head=64), -4, "workspace too small: 0 < 18432"),
    ("deft_flatten_decode_append{}_lse", dict(), -4, "workspace too small: 0 < 20480"),
    ("deft_flatten_decode_append{}_lse", dict(lse=0), -1, _NULL_LSE),
    ("deft_flatten_decode_append{}_lse", dict(lse=P + 2), -1, _MIS_LSE),
    ("deft_flatten_decode_append{}_lse", dict(lse=0, k_new=0), -1, _FUSED),
    ("deft_flatten_decode_append{}_lse", dict(lse=0, n_new=-1), -1, _NULL_LSE),
    ("deft_node_decode{}_lse", dict(), -4, "workspace too small: 0 < 33280"),
    ("deft_node_decode{}_lse", dict(lse=0), -1, _NULL_LSE),
    ("deft_node_decode{}_lse", dict(lse=P + 2), -1, _MIS_LSE),
    ("deft_node_decode{}_lse", dict(lse=0, total_kv=-1), -1, _NULL_LSE),
    ("deft_node_decode{}_lse", dict(lse=0, v_base=0), -1, "null tensor pointer"),
    ("deft_node_decode_append{}_lse", dict(), -4, "workspace too small: 0 < 33280"),
    ("deft_node_decode_append{}_lse", dict(lse=0), -1, _NULL_LSE),
    ("deft_node_decode_append{}_lse", dict(lse=P + 2), -1, _MIS_LSE),
    ("deft_node_decode_append{}_lse", dict(lse=0, cache_loc=0), -1, _FUSED),
    ("deft_prefill{}_lse", dict(lse=0), -1, "prefill: " + _NULL_LSE),
    ("deft_prefill{}_lse", dict(lse=P + 2), -1, "prefill: " + _MIS_LSE),
    ("deft_prefill{}_lse", dict(lse=0, batch=1, q=0), -1, "prefill: " + _NULL_LSE),
    ("deft_prefill{}_lse", dict(batch=1, q=0), -1, "bad prefill arguments (batch=1 max_input_len=4 Hq=8 Hkv=2)"),
    ("deft_prefill{}_lse", dict(batch=1, D=48), -2, "prefill: unsupported head_dim 48 (supported: 16, 32, 64, 128)"),
    ("deft_prefill{}_lse", dict(batch=1, out=P + 4), -1, "prefill: q/k/v rows must be 16-byte aligned, out rows 8-byte aligned"),
    ("deft_merge{}_states", dict(o_a=0), -1, _MS_NULL),
    ("deft_merge{}_states", dict(o_b=0), -1, _MS_NULL),
    ("deft_merge{}_states", dict(out=0), -1, _MS_NULL),
    ("deft_merge{}_states", dict(lse_a=0), -1, _MS_NULL),
    ("deft_merge{}_states", dict(lse_b=0, D=48), -1, _MS_NULL),
    ("deft_merge{}_states", dict(D=48), -2, "merge_states: unsupported head_dim 48 (supported: 16, 32, 64, 128)"),
    ("deft_merge{}_states", dict(D=256), -2, "merge_states: unsupported head_dim 256 (supported: 16, 32, 64, 128)"),
    ("deft_merge{}_states", dict(n=-1), -1, "merge_states: bad geometry n=-1 Hq=8"),
    ("deft_merge{}_states", dict(Hq=0), -1, "merge_states: bad geometry n=0 Hq=0"),
    ("deft_merge{}_states", dict(o_b=P + 2), -1, "merge_states: o_a / o_b / out rows must be 4-byte aligned"),
    ("deft_merge{}_states", dict(out_stride_head=127), -1, "merge_states: o_a / o_b / out rows must be 4-byte aligned"),
    ("deft_merge{}_states", dict(lse_out=P + 2), -1, "merge_states: lse pointers must be 4-byte aligned"),
]


def _cases():
    for name, overrides, code, msg in ROWS:
        for fn in (name.format("_f16"), name.format("_bf16")):
            ident = fn + "(" + ", ".join(f"{k}={v:#x}" if v >= P else f"{k}={v}" for k, v in overrides.items()) + ")"
            yield pytest.param(fn, name, overrides, code, msg, id=ident)


@pytest.mark.parametrize("fn, name, overrides, code, msg", _cases())
def test_a_malformed_call_gets_its_code_and_message(fn, name, overrides, code, msg):
    spec = SPEC[name]
    assert code != 0 and not set(overrides) - set(spec), (name, overrides)
    args = {**spec, **overrides}
    assert len(args) == len(getattr(lib, fn).argtypes)
    assert (getattr(lib, fn)(*args.values()), lib.deft_last_error().decode()) == (code, msg)


def test_every_new_entry_point_has_rows_and_the_empty_calls_are_ok():
    assert {name for name, *_ in ROWS} == set(SPEC) == set(NEW)
    for sfx in ("_f16", "_bf16"):  # the well-formed defaults that launch nothing; lse_out may be NULL
        assert getattr(lib, "deft_prefill{}_lse".format(sfx))(*SPEC["deft_prefill{}_lse"].values()) == 0
        assert getattr(lib, "deft_merge{}_states".format(sfx))(*SPEC["deft_merge{}_states"].values()) == 0
        assert getattr(lib, "deft_merge{}_states".format(sfx))(*{**SPEC["deft_merge{}_states"], "lse_out": 0}.values()) == 0


# ---- the Python operators ------------------------------------------------------------------------------------------------------
def _flatten(q, k, v, o, lse):
    i64 = torch.zeros(128, dtype=torch.int64)
    deft_amd.tree_attention_subtree_fwd_lse(q, k, v, o, lse, 128, i64[:1], i64[:1], i64[:1], i64, i64, i64[:1])


def _node(q, k, v, o, lse):
    i64 = torch.zeros(128, dtype=torch.int64)
    deft_amd.tree_attention_fwd_lse(q, k, v, o, lse, i64, i64[:1], i64[:1], i64[:1], i64[:1], i64[:1])


def _flatten_append(q, k, v, o, lse):
    i64 = torch.zeros(128, dtype=torch.int64)
    kv = torch.zeros(8, 2, k.shape[1], k.shape[2], dtype=k.dtype)
    deft_amd.flatten_append_attention_lse(q, kv, o, lse, torch.zeros(1, dtype=torch.int32), k[:1], v[:1], 128, i64[:1], i64[:1], i64[:1],
                                          i64, i64, i64[:1])


def _node_append(q, k, v, o, lse):
    i64 = torch.zeros(128, dtype=torch.int64)
    kv = torch.zeros(8, 2, k.shape[1], k.shape[2], dtype=k.dtype)
    deft_amd.node_append_attention_lse(q, kv, o, lse, torch.zeros(1, dtype=torch.int32), k[:1], v[:1], i64, i64[:1], i64[:1], i64[:1],
                                       i64[:1], i64[:1])


def _prefill(q, k, v, o, lse):
    deft_amd.context_attention_fwd_lse(q, k, v, o, lse, torch.zeros(1, dtype=torch.int32), torch.tensor([q.shape[0]], dtype=torch.int32),
                                       q.shape[0])


@pytest.mark.parametrize("call", [_flatten, _node, _flatten_append, _node_append, _prefill], ids=lambda f: f.__name__[1:])
def test_lse_operators_refuse_a_bad_lse_and_cpu_tensors(call):
    def t(n=1, dtype=F16):
        return torch.zeros(n, 4, 128, dtype=dtype)

    n = 1
    for bad, exc in ((torch.zeros(n, 4, dtype=torch.float64), TypeError), (torch.zeros(n, 4, dtype=F16), TypeError), (None, TypeError),
                     (torch.zeros(n, 5), ValueError), (torch.zeros(n + 1, 4), ValueError), (torch.zeros(n, 4, 1), ValueError),
                     (torch.zeros(n * 4), ValueError)):
        with pytest.raises(exc):
            call(t(), t(8), t(8), t(), bad)
    with pytest.raises(TypeError):  # mixed element types, as in the plain operators
        call(t(), t(8, BF16), t(8, BF16), t(), torch.zeros(n, 4, device="meta"))
    # a sound call on CPU tensors: past every check, stopped because there is no CPU path
    with pytest.raises(deft_amd.DeftLibraryError, match="no CPU path"):
        call(t(), t(8), t(8), t(), torch.zeros(n, 4))
    with pytest.raises(deft_amd.DeftLibraryError, match="no CPU path"):
        call(t(dtype=BF16), t(8, BF16), t(8, BF16), t(dtype=BF16), torch.zeros(8, 4)[::2][:n])  # (any strides)


def test_merge_attention_states_refuses_what_it_must():
    o, l = torch.zeros(3, 4, 64, dtype=F16), torch.zeros(3, 4)
    with pytest.raises(TypeError):
        deft_amd.merge_attention_states(o, l, o.to(BF16), l)
    with pytest.raises(TypeError):
        deft_amd.merge_attention_states(o, l, o, l, out=o.to(BF16))
    with pytest.raises(TypeError):
        deft_amd.merge_attention_states(o.float(), l, o.float(), l)
    with pytest.raises(TypeError):
        deft_amd.merge_attention_states(o, l.double(), o, l)
    with pytest.raises(TypeError):
        deft_amd.merge_attention_states(o, l, o, None)
    with pytest.raises(TypeError):
        deft_amd.merge_attention_states(o, l, o, l, lse_out=l.half())
    with pytest.raises(ValueError):
        deft_amd.merge_attention_states(o, l, o[:2], l[:2])
    with pytest.raises(ValueError):
        deft_amd.merge_attention_states(o, l[:2], o, l)
    with pytest.raises(ValueError):
        deft_amd.merge_attention_states(o, l, o, l, out=o[:2])
    with pytest.raises(ValueError):
        deft_amd.merge_attention_states(o, l, o, l, lse_out=torch.zeros(3, 5))
    with pytest.raises(ValueError):
        deft_amd.merge_attention_states(o[..., :48], l, o[..., :48], l)  # (head_dim 48, and not contiguous)
    with pytest.raises(deft_amd.DeftLibraryError, match="no CPU path"):
        deft_amd.merge_attention_states(o, l, o, l)
    with pytest.raises(deft_amd.DeftLibraryError, match="no CPU path"):
        deft_amd.merge_attention_states(o, l, o, l, out=o)  # in place


# ---- cached_prefix_blocks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots, n_rows, max_q_len", [(1, 1, 32), (128, 32, 32), (129, 33, 32), (300, 70, 32), (300, 70, 16)])
def test_cached_prefix_blocks_against_a_direct_enumeration(n_slots, n_rows, max_q_len):
    slots = [1000 + 3 * i for i in range(n_slots)]  # (distinct, not consecutive)
    bq, cnts, off, masks, kv, lens = (t.tolist() for t in deft_amd.cached_prefix_blocks(slots, n_rows, max_q_len, device="cpu"))
    NB = len(cnts)
    assert len(off) == len(lens) == NB and len(kv) == len(masks) == 128 * NB and len(bq) == sum(cnts)
    n_kv_blocks, n_chunks = -(-n_slots // 128), -(-n_rows // max_q_len)
    assert NB == n_kv_blocks * n_chunks
    seen = {}
    for b in range(NB):
        assert 1 <= cnts[b] <= max_q_len <= 32 and 1 <= lens[b] <= 128
        assert off[b] == sum(cnts[:b])
        rows = bq[off[b] : off[b] + cnts[b]]
        # chunk-major: block b belongs to chunk b // n_kv_blocks and is that chunk's (b % n_kv_blocks)-th piece of the path
        c, piece = divmod(b, n_kv_blocks)
        assert rows == list(range(c * max_q_len, min((c + 1) * max_q_len, n_rows)))
        assert kv[128 * b : 128 * b + lens[b]] == slots[128 * piece : 128 * piece + 128]
        for j in range(128):
            slot, mask = kv[128 * b + j], masks[128 * b + j]
            if j >= lens[b]:
                assert slot == -1 and mask == 0  # pad
                continue
            assert mask == (1 << cnts[b]) - 1  # the chunk's low cnt bits
            for i, r in enumerate(rows):
                if (mask >> i) & 1:
                    seen[(r, slot)] = seen.get((r, slot), 0) + 1
    assert seen == {(r, s): 1 for r in range(n_rows) for s in slots}  # every (row, slot) pair exactly once


def test_cached_prefix_blocks_edges():
    assert [t.numel() for t in deft_amd.cached_prefix_blocks([], 5, device="cpu")] == [0] * 6
    assert [t.numel() for t in deft_amd.cached_prefix_blocks([3, 4], 0, device="cpu")] == [0] * 6
    assert all(t.dtype == torch.int64 for t in deft_amd.cached_prefix_blocks(torch.arange(5, dtype=torch.int32), 2, device="cpu"))
    with pytest.raises(ValueError):
        deft_amd.cached_prefix_blocks([1], 1, max_q_len=33, device="cpu")
