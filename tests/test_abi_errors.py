"""Which code and which deft_last_error() text a malformed call of the C ABI gets, pinned call by call.  No GPU: every call
here is refused before the library touches HIP, so the pointers are plain integers.  The default arguments of every entry point are
a well-formed call of one block / entry at Hq=8, Hkv=2, D=128 whose scratch size (workspace_bytes, plan_bytes, scratch_bytes) is 0
-- the last check in front of the launches -- and a row overrides some of them.  Rows with two faults pin the ORDER of the checks."""
import pytest

import deft_amd
from deft_amd._lib import ELEM_ENTRY_POINTS

lib = deft_amd.lib
P = 0x1000  # a non-null, 16-byte aligned "pointer"
BIG = 1 << 30

_QKV = dict(q=P, q_stride_tok=1024, q_stride_head=128, k_base=P, v_base=P, kv_stride_slot=256, kv_stride_head=128)
_OUT = dict(out=P, o_stride_tok=1024, o_stride_head=128)
_BLOCKS = dict(block_q=P, block_q_cnts=P, block_q_offset=P, block_bitmasks=P, block_kv=P, block_lens=P)
_NODES = dict(node_kv=P, node_kv_offset=P, node_kv_len=P, node_q=P, node_q_offset=P, node_q_len=P)
_FDIMS = dict(NB=1, P=1, nq=1, Hq=8, Hkv=2, D=128, scale=0.088)
_NDIMS = dict(NE=1, P=1, total_kv=128, nq=1, Hq=8, Hkv=2, D=128, scale=0.088)
_SDIMS = dict(plan=P, nq=1, total_tokens=128, Hq=8, Hkv=2, D=128, scale=0.088)
_APPEND = dict(cache_loc=P, k_new=P, v_new=P, new_stride_tok=256, n_new=1)
_ROPE = dict(cos_sin_rows=P, rotary_dim=128, is_neox_style=1)
_SCRATCH = dict(plan=0, workspace=P, workspace_bytes=0, stream=0)
_PLAN_GEOM = dict(Hq=8, Hkv=2, q_stride_tok=1024, q_stride_head=128, kv_stride_slot=256)
_PLAN_APPEND = dict(cache_loc=0, n_new=0, new_stride_tok=256)
_PLAN_OUT = dict(plan=P, plan_bytes=0, stream=0)
_WINDOW = dict(dims=P, nq=1, max_q_len=32, win_tiles=1, win_tab=P)
_TREE = dict(n_nodes=4, nq=1, nqw=1, node_start=P, node_len=P, node_cap=P, refs=P, leaf_node=P, slots=P)
_TREE_MD = dict(max_q_len=32, block_len=128, max_block_len=-1, nbp_cap=4, scratch=P, scratch_bytes=0, md_node_q=P, md_node_kv=P,
                md_node_q_len=P, md_node_kv_len=P, md_node_q_offset=P, md_node_kv_offset=P, **_BLOCKS, advance_loc=P)
_PAGES = dict(page_table=0, page_stride=0, page_rows=0, page_cols=0)

# entry point -> its parameters in ABI order with the default of each
SPEC = {
    "deft_flatten_decode": {**_QKV, **_OUT, **_BLOCKS, **_FDIMS, **_SCRATCH},
    "deft_flatten_decode_append": {**_QKV, **_OUT, **_BLOCKS, **_FDIMS, **_APPEND, **_SCRATCH},
    "deft_flatten_decode_rope_append": {**_QKV, **_OUT, **_BLOCKS, **_FDIMS, **_APPEND, **_ROPE, **_SCRATCH},
    "deft_flatten_stage1": {**_QKV, **_BLOCKS, **_FDIMS, **_SCRATCH},
    "deft_node_decode": {**_QKV, **_OUT, **_NODES, **_NDIMS, **_SCRATCH},
    "deft_node_decode_append": {**_QKV, **_OUT, **_NODES, **_NDIMS, **_APPEND, **_SCRATCH},
    "deft_node_decode_rope_append": {**_QKV, **_OUT, **_NODES, **_NDIMS, **_APPEND, **_ROPE, **_SCRATCH},
    "deft_seq_decode": {**_QKV, **_OUT, **_SDIMS, "workspace": P, "workspace_bytes": 0, "stream": 0},
    "deft_seq_decode_append": {**_QKV, **_OUT, **_SDIMS, **_APPEND, "workspace": P, "workspace_bytes": 0, "stream": 0},
    "deft_kv_append": dict(k_base=P, v_base=P, kv_stride_slot=256, kv_stride_head=128, cache_loc=P, k_new=P, v_new=P,
                           new_stride_tok=256, n=1, Hkv=2, D=128, stream=0),
    "deft_flatten_build_plan": {**_BLOCKS, "NB": 1, "P": 1, **_PLAN_GEOM, **_PLAN_APPEND, **_PLAN_OUT},
    "deft_flatten_build_plan_dims": {**_BLOCKS, "NB": 1, "P": 1, "dims": P, **_PLAN_GEOM, **_PLAN_APPEND, **_PLAN_OUT},
    "deft_flatten_build_plan_window": {**_BLOCKS, "NB": 1, "P": 1, **_WINDOW, **_PLAN_GEOM, **_PLAN_OUT},
    "deft_node_build_plan": {**_NODES, "NE": 1, "P": 1, "total_kv": 128, **_PLAN_GEOM, **_PLAN_APPEND, **_PLAN_OUT},
    "deft_node_build_plan_dims": {**_NODES, "NE": 1, "P": 1, "total_kv": 128, "dims": P, **_PLAN_GEOM, **_PLAN_APPEND, **_PLAN_OUT},
    "deft_node_build_plan_window": {**_NODES, "NE": 1, "P": 1, "total_kv": 128, **_WINDOW, **_PLAN_GEOM, **_PLAN_OUT},
    "deft_seq_build_plan": dict(req_to_token=P, req_stride=128, b_req_idx=P, b_start_loc=P, b_seq_len=P, nq=1, total_tokens=128,
                                **_PLAN_GEOM, **_PLAN_APPEND, **_PLAN_OUT),
    "deft_tree_dev_advance": {**_TREE, "cache_loc": P, "scratch": P, "stream": 0},
    "deft_tree_dev_apply_ops": {**_TREE, "ops": P, "scratch": P, "stream": 0},
    "deft_tree_dev_build_md": {**_TREE, **_TREE_MD, "stream": 0},
    "deft_tree_dev_build_md_ops": {**_TREE, **_TREE_MD, "ops": P, **_PAGES, "stream": 0},
    "deft_window_patch": {**_TREE, "ops": P, "cache_loc": P, **_PAGES, "patch": P, "win_tab": P, "plan": P, "max_q_len": 32,
                          "win_tiles": 1, "Hq": 8, "Hkv": 2, "kv_stride_slot": 256, "new_stride_tok": 256, "scratch": P,
                          "fetch_ring": 0, "fetch_slot_bytes": 0, "fetch_ring_n": 0, "fetch_dst": 0, "fetch_counter": 0, "stream": 0},
}

_NO_APPEND = dict(q=0, k_new=0)  # two faults: the parent answers "fused append"
_FUSED = "fused append needs k_new, v_new and cache_loc"
_FIVE_NODE_ARRAYS = "deft_tree_dev_build_md: the node arrays and the block arrays are each given as a whole or not at all"

# (entry point, overrides of its defaults, return code, deft_last_error()) -- recorded from the library before its host layer was
# consolidated; the Flatten / Node / seq / kv_append rows run for both element types
ROWS = [
    ("deft_flatten_decode", dict(), -4, "workspace too small: 0 < 20480"),
    ("deft_flatten_decode", dict(workspace=0), -1, "null workspace"),
    ("deft_flatten_decode", dict(D=48), -2, "unsupported geometry Hq=8 Hkv=2 D=48 (head_dim must be 16, 32, 64 or 128)"),
    ("deft_flatten_decode", dict(Hkv=3), -1, "bad geometry nq=1 Hq=8 Hkv=3"),
    ("deft_flatten_decode", dict(nq=-1), -1, "bad geometry nq=-1 Hq=8 Hkv=2"),
    ("deft_flatten_decode", dict(out=0), -1, "null tensor pointer"),
    ("deft_flatten_decode", dict(q=P + 2), -1, "q/k/v rows must be 16-byte aligned (pointers and strides multiples of 8 elements)"),
    ("deft_flatten_decode", dict(kv_stride_head=68), -1,
     "q/k/v rows must be 16-byte aligned (pointers and strides multiples of 8 elements)"),
    ("deft_flatten_decode", dict(o_stride_tok=1023), -1, "out rows must be 4-byte aligned"),
    ("deft_flatten_decode", dict(NB=-1), -1, "bad Flatten metadata (NB=-1 P=1)"),
    ("deft_flatten_decode", dict(block_kv=0), -1, "bad Flatten metadata (NB=1 P=1)"),
    ("deft_flatten_decode", dict(workspace=0, NB=-1), -1, "null workspace"),
    ("deft_flatten_decode", dict(workspace=P + 2), -1, "out rows must be 4-byte aligned"),
    ("deft_flatten_decode", dict(D=64, kv_stride_head=64), -4, "workspace too small: 0 < 18432"),
    ("deft_flatten_stage1", dict(), -4, "workspace too small: 0 < 20480"),
    ("deft_flatten_stage1", dict(workspace=0, q=0), -1, "null workspace"),
    ("deft_flatten_stage1", dict(block_q=0), -1, "bad Flatten metadata (NB=1 P=1)"),
    ("deft_flatten_decode_append", dict(), -4, "workspace too small: 0 < 20480"),
    ("deft_flatten_decode_append", dict(k_new=0), -1, _FUSED),
    ("deft_flatten_decode_append", dict(n_new=-1), -1, "bad fused-append arguments (n_new=-1 new_stride=256)"),
    ("deft_flatten_decode_append", dict(k_new=P + 2), -1, "bad fused-append arguments (n_new=1 new_stride=256)"),
    ("deft_flatten_decode_append", dict(new_stride_tok=248), -1, "bad fused-append arguments (n_new=1 new_stride=248)"),
    ("deft_flatten_decode_append", dict(n_new=-1, workspace=0), -1, "bad fused-append arguments (n_new=-1 new_stride=256)"),
    ("deft_flatten_decode_append", dict(n_new=-1, q=0), -1, "null tensor pointer"),
    ("deft_flatten_decode_append", _NO_APPEND, -1, _FUSED),
    ("deft_flatten_decode_rope_append", dict(), -4, "workspace too small: 0 < 20480"),
    ("deft_flatten_decode_rope_append", dict(rotary_dim=100), -2,
     "fused rope: head_dim 128, rotary_dim == head_dim, NeoX pairing (got D=128 rotary_dim=100 neox=1); use deft_rope_qk_f16 + the "
     "append entry point"),
    ("deft_flatten_decode_rope_append", dict(cos_sin_rows=0), -1,
     "bad fused-rope arguments (cos_sin_rows: [n_new][head_dim] fp32, 16-byte aligned)"),
    ("deft_flatten_decode_rope_append", dict(cos_sin_rows=0, rotary_dim=100), -1,
     "bad fused-rope arguments (cos_sin_rows: [n_new][head_dim] fp32, 16-byte aligned)"),
    ("deft_flatten_decode_rope_append", dict(q_stride_tok=512), -2,
     "fused rope needs token-major q (q_stride_tok=512 q_stride_head=128)"),
    ("deft_flatten_decode_rope_append", dict(q=0, rotary_dim=100), -2,
     "fused rope: head_dim 128, rotary_dim == head_dim, NeoX pairing (got D=128 rotary_dim=100 neox=1); use deft_rope_qk_f16 + the "
     "append entry point"),
    ("deft_flatten_decode_rope_append", dict(cos_sin_rows=0, k_new=0), -1, _FUSED),
    ("deft_flatten_decode_rope_append", _NO_APPEND, -1, _FUSED),
    ("deft_node_decode", dict(), -4, "workspace too small: 0 < 33280"),
    ("deft_node_decode", dict(total_kv=-1), -1, "bad Node metadata (NE=1 P=1 total_kv=-1)"),
    ("deft_node_decode", dict(node_q_len=0), -1, "bad Node metadata (NE=1 P=1 total_kv=128)"),
    ("deft_node_decode", dict(workspace=0), -1, "null workspace"),
    ("deft_node_decode", dict(workspace=P + 2), -4, "workspace too small: 0 < 33280"),
    ("deft_node_decode", dict(workspace=0, total_kv=-1), -1, "bad Node metadata (NE=1 P=1 total_kv=-1)"),
    ("deft_node_decode", dict(q=0, total_kv=-1), -1, "null tensor pointer"),
    ("deft_node_decode_append", dict(), -4, "workspace too small: 0 < 33280"),
    ("deft_node_decode_append", dict(n_new=-1), -1, "bad fused-append arguments (n_new=-1 new_stride=256)"),
    ("deft_node_decode_append", dict(n_new=-1, workspace=0), -1, "null workspace"),
    ("deft_node_decode_append", dict(n_new=-1, NE=-1), -1, "bad Node metadata (NE=-1 P=1 total_kv=128)"),
    ("deft_node_decode_append", _NO_APPEND, -1, _FUSED),
    ("deft_node_decode_rope_append", dict(), -4, "workspace too small: 0 < 33280"),
    ("deft_node_decode_rope_append", dict(is_neox_style=0), -2,
     "fused rope: head_dim 128, rotary_dim == head_dim, NeoX pairing (got D=128 rotary_dim=128 neox=0); use deft_rope_qk_f16 + the "
     "append entry point"),
    ("deft_node_decode_rope_append", dict(cos_sin_rows=0, cache_loc=0), -1, _FUSED),
    ("deft_node_decode_rope_append", _NO_APPEND, -1, _FUSED),
    ("deft_seq_decode", dict(), -4, "workspace too small: 0 < 33280"),
    ("deft_seq_decode", dict(plan=0), -1, "bad sequential decode arguments (nq=1 total_tokens=128)"),
    ("deft_seq_decode", dict(plan=0, q=0), -1, "bad sequential decode arguments (nq=1 total_tokens=128)"),
    ("deft_seq_decode", dict(q=0), -1, "null tensor pointer"),
    ("deft_seq_decode", dict(workspace=0), -1, "null workspace"),
    ("deft_seq_decode_append", dict(), -4, "workspace too small: 0 < 33280"),
    ("deft_seq_decode_append", dict(plan=0, v_new=0), -1, _FUSED),
    ("deft_seq_decode_append", dict(n_new=-1), -1, "bad fused-append arguments (n_new=-1 new_stride=256)"),
    ("deft_seq_decode_append", _NO_APPEND, -1, _FUSED),
    ("deft_kv_append", dict(k_new=P + 2), -1, "kv_append rows must be 16-byte aligned"),
    ("deft_kv_append", dict(cache_loc=0), -1, "bad kv_append arguments (n=1 Hkv=2 D=128)"),
    ("deft_flatten_build_plan", dict(), -4, "plan buffer too small: 0 < 15872"),
    ("deft_flatten_build_plan", dict(n_new=-1), -1, "bad plan arguments (NB=1 P=1 Hq=8 Hkv=2)"),
    ("deft_flatten_build_plan", dict(block_lens=0), -1, "bad plan arguments (NB=1 P=1 Hq=8 Hkv=2)"),
    ("deft_flatten_build_plan_dims", dict(), -4, "plan buffer too small: 0 < 15872"),
    ("deft_flatten_build_plan_dims", dict(dims=0), -1, "bad plan arguments (NB=1 P=1 Hq=8 Hkv=2)"),
    ("deft_flatten_build_plan_dims", dict(Hkv=3), -1, "bad plan arguments (NB=1 P=1 Hq=8 Hkv=3)"),
    ("deft_flatten_build_plan_window", dict(), -4, "plan buffer too small: 0 < 15872"),
    ("deft_flatten_build_plan_window", dict(max_q_len=40), -1, "bad window plan arguments (NB=1 P=1 nq=1 max_q_len=40 tiles=1)"),
    ("deft_flatten_build_plan_window", dict(NB=0), -1, "bad window plan arguments (NB=0 P=1 nq=1 max_q_len=32 tiles=1)"),
    ("deft_flatten_build_plan_window", dict(win_tab=0), -1, "bad window plan arguments (NB=1 P=1 nq=1 max_q_len=32 tiles=1)"),
    ("deft_node_build_plan", dict(), -4, "plan buffer too small: 0 < 24320"),
    ("deft_node_build_plan", dict(plan=0), -1, "bad node plan arguments (NE=1 P=1 total_kv=128)"),
    ("deft_node_build_plan", dict(cache_loc=P, n_new=-1, plan_bytes=BIG), -1, "bad node plan append arguments (n_new=-1)"),
    ("deft_node_build_plan", dict(cache_loc=P, n_new=-1), -4, "plan buffer too small: 0 < 24320"),
    ("deft_node_build_plan_dims", dict(), -4, "plan buffer too small: 0 < 24320"),
    ("deft_node_build_plan_dims", dict(dims=0), -1, "deft_node_build_plan_dims: null dims"),
    ("deft_node_build_plan_dims", dict(dims=0, NE=-1), -1, "deft_node_build_plan_dims: null dims"),
    ("deft_node_build_plan_window", dict(), -4, "plan buffer too small: 0 < 24320"),
    ("deft_node_build_plan_window", dict(total_kv=0), -1, "bad window plan arguments (NE=1 P=1 total_kv=0 nq=1)"),
    ("deft_seq_build_plan", dict(), -4, "plan buffer too small: 0 < 26624"),
    ("deft_seq_build_plan", dict(b_seq_len=0), -1, "bad sequential plan arguments (nq=1 total_tokens=128)"),
    ("deft_tree_dev_advance", dict(refs=0), -1, "deft_tree_dev_advance: bad arguments (nodes=4 nq=1)"),
    ("deft_tree_dev_advance", dict(cache_loc=0), -1, "deft_tree_dev_advance: bad arguments (nodes=4 nq=1)"),
    ("deft_tree_dev_advance", dict(nqw=0), -1, "deft_tree_dev_advance: bad arguments (nodes=4 nq=1)"),
    ("deft_tree_dev_apply_ops", dict(node_len=0), -1, "deft_tree_dev_apply_ops: bad arguments (nodes=4 nq=1)"),
    ("deft_tree_dev_apply_ops", dict(ops=0), -1, "deft_tree_dev_apply_ops: bad arguments (nodes=4 nq=1)"),
    ("deft_tree_dev_build_md", dict(), -4, "tree scratch too small: 0 < 2304"),
    ("deft_tree_dev_build_md", dict(slots=0), -1, "deft_tree_dev_build_md: bad arguments (nodes=4 nq=1)"),
    ("deft_tree_dev_build_md", dict(nbp_cap=-1), -1, "deft_tree_dev_build_md: bad arguments (nodes=4 nq=1)"),
    ("deft_tree_dev_build_md", dict(md_node_kv_len=0), -1, _FIVE_NODE_ARRAYS),
    ("deft_tree_dev_build_md", dict(md_node_kv_len=0, leaf_node=0), -1, "deft_tree_dev_build_md: bad arguments (nodes=4 nq=1)"),
    ("deft_tree_dev_build_md", dict(max_q_len=64), -1, "deft_tree_dev_build_md: bad config max_q_len=64 block_len=128 max_block_len=-1"),
    ("deft_tree_dev_build_md_ops", dict(), -4, "tree scratch too small: 0 < 2304"),
    ("deft_tree_dev_build_md_ops", dict(page_table=P), -1,
     "deft_tree_dev_build_md_ops: the page-table write needs advance_loc, rows, cols and a row stride"),
    ("deft_tree_dev_build_md_ops", dict(page_table=P, node_start=0), -1,
     "deft_tree_dev_build_md_ops: the page-table write needs advance_loc, rows, cols and a row stride"),
    ("deft_tree_dev_build_md_ops", dict(node_cap=0), -1, "deft_tree_dev_build_md: bad arguments (nodes=4 nq=1)"),
    ("deft_window_patch", dict(node_start=0), -1, "deft_window_patch: bad arguments (nodes=4 nq=1 tiles=1)"),
    ("deft_window_patch", dict(nq=0), -1, "deft_window_patch: bad arguments (nodes=4 nq=0 tiles=1)"),
    ("deft_window_patch", dict(plan=0), -1, "deft_window_patch: bad arguments (nodes=4 nq=1 tiles=1)"),
    ("deft_window_patch", dict(page_table=P), -1, "deft_window_patch: the page-table write needs rows, cols and a row stride"),
    ("deft_window_patch", dict(page_table=P, refs=0), -1, "deft_window_patch: bad arguments (nodes=4 nq=1 tiles=1)"),
    ("deft_window_patch", dict(fetch_ring=P), -1, "deft_window_patch: bad fetch arguments"),
    ("deft_window_patch", dict(fetch_ring=P, page_table=P), -1,
     "deft_window_patch: the page-table write needs rows, cols and a row stride"),
]


def call(name, overrides):
    spec = SPEC[name]
    assert not set(overrides) - set(spec), (name, overrides)
    args = {**spec, **overrides}
    return lambda fn: (getattr(lib, fn)(*args.values()), lib.deft_last_error().decode())


def _cases():
    for name, overrides, code, msg in ROWS:
        for fn in ([name + "_f16", name + "_bf16"] if name in ELEM_ENTRY_POINTS else [name]):
            ident = fn + "(" + ", ".join(f"{k}={v:#x}" if v >= P else f"{k}={v}" for k, v in overrides.items()) + ")"
            yield pytest.param(fn, name, overrides, code, msg, id=ident)


@pytest.mark.parametrize("fn, name, overrides, code, msg", _cases())
def test_a_malformed_call_gets_its_code_and_message(fn, name, overrides, code, msg):
    assert code != 0  # (no row may be a call that would launch)
    assert call(name, overrides)(fn) == (code, msg)


def test_every_entry_point_with_checks_has_a_row():
    assert {name for name, *_ in ROWS} == set(SPEC)
    assert set(ELEM_ENTRY_POINTS) - set(SPEC) == {"deft_rope_qk", "deft_prefill"}  # (neither is part of the decode host layer)


# Size queries as recorded constants: (Hq, Hkv, D) = (8, 2, 128) with one block / entry, (32, 32, 128) with NB = NE = 100, P = 64,
# total_kv = 5000, nq = 40, and (4, 4, 64) with NB = NE = 7, P = 9, total_kv = 300, nq = 5.
SIZES = [
    ("deft_flatten_workspace_bytes", (1, 1, 1, 8, 2, 128), 20480),
    ("deft_flatten_workspace_bytes", (100, 64, 40, 32, 32, 128), 1280000),
    ("deft_flatten_workspace_bytes", (7, 9, 5, 4, 4, 64), 32256),
    ("deft_flatten_plan_bytes", (1, 1, 8, 2), 15872),
    ("deft_flatten_plan_bytes", (100, 64, 32, 32), 222976),
    ("deft_flatten_plan_bytes", (7, 9, 4, 4), 22528),
    ("deft_node_workspace_bytes", (1, 1, 128, 1, 8, 2, 128), 33280),
    ("deft_node_workspace_bytes", (100, 64, 5000, 40, 32, 32, 128), 74111488),
    ("deft_node_workspace_bytes", (7, 9, 300, 5, 4, 4, 64), 118016),
    ("deft_node_plan_bytes", (1, 1, 128, 8, 2), 24320),
    ("deft_node_plan_bytes", (100, 64, 5000, 32, 32), 638720),
    ("deft_node_plan_bytes", (7, 9, 300, 4, 4), 32256),
    ("deft_seq_plan_bytes", (1, 128, 8, 2), 26624),
    ("deft_seq_plan_bytes", (40, 5000, 32, 32), 222720),
    ("deft_seq_plan_bytes", (5, 300, 4, 4), 26112),
    ("deft_seq_workspace_bytes", (1, 128, 8, 2, 128), 33280),
    ("deft_seq_workspace_bytes", (40, 5000, 32, 32, 128), 1490432),
    ("deft_seq_workspace_bytes", (5, 300, 4, 4, 64), 30464),
    ("deft_tree_dev_scratch_bytes", (4, 1, 4), 2304),
    ("deft_tree_dev_scratch_bytes", (300, 1, 100), 7936),
    ("deft_tree_dev_scratch_bytes", (5000, 3, 4096), 229632),
    ("deft_extend_scratch_bytes", (1, 1), 1792),
    ("deft_extend_scratch_bytes", (40, 100), 3072),
    ("deft_extend_scratch_bytes", (5, 7), 1792),
    # refused shapes: 0
    ("deft_flatten_workspace_bytes", (1, 1, 1, 8, 3, 128), 0),
    ("deft_flatten_plan_bytes", (1, 1, 0, 2), 0),
    ("deft_node_workspace_bytes", (1, 1, 128, 1, 8, 3, 128), 0),
    ("deft_node_plan_bytes", (1, 1, 128, 8, 0), 0),
    ("deft_seq_plan_bytes", (-1, 128, 8, 2), 0),
    ("deft_seq_workspace_bytes", (1, -1, 8, 2, 128), 0),
    ("deft_tree_dev_scratch_bytes", (4, 0, 4), 0),
    ("deft_extend_scratch_bytes", (-1, 1), 0),
]


@pytest.mark.parametrize("fn, args, size", SIZES, ids=[f"{fn}{args}" for fn, args, _ in SIZES])
def test_size_queries_answer_the_recorded_sizes(fn, args, size):
    assert getattr(lib, fn)(*args) == size
