"""Attention states: an operator's output WITH its log-sum-exp, and the merge of two of them.

The state of query row r and head h over a key set S is the pair (o, lse): `o[D]` the normalised attention output in the
call's element type -- exactly what the plain operators write -- and `lse = ln sum_{i in S} exp(scale * q.k_i)` in float32
(natural log, scale included).  The empty set has o = 0, lse = -inf.  Two states over disjoint key sets merge into the state over
their union (`merge_attention_states`), which is what lets one result be combined with attention over any other keys: the two
halves of a split tree, a cached prefix under freshly prefilled tokens (`prefill_with_cached_prefix`), a sink or a window
computed elsewhere.

The `*_lse` operators are their plain siblings (tree_attention.py, context_attention.py) with `lse` behind `output`: the same
kernels with one more 4-byte store per (row, head), so `output` is bit-identical to the plain call's.  `lse` is a float32 CUDA
tensor [n, heads] with any strides.  Backed by libdeft_amd.so like everything else: no PyTorch or CPU fallback.

Not covered: `DecodeSession` captures no *_lse call, and the rope-fused and sequential entry points have no *_lse form (rotate with
`get_rope` first)."""
from __future__ import annotations

import torch

from ._lib import DeftLibraryError, check, entry, same_elem_dtype
from .context_attention import _prefill
from .tree_attention import (_flatten_append, _flatten_append_kv8, _flatten_fwd, _flatten_fwd_kv8, _lse_args, _node_append,
                             _node_append_kv8, _node_fwd, _node_fwd_kv8, _stream_ptr, kv_append)

__all__ = ["tree_attention_subtree_fwd_lse", "tree_attention_fwd_lse", "flatten_append_attention_lse", "node_append_attention_lse",
           "context_attention_fwd_lse", "merge_attention_states", "cached_prefix_blocks", "prefill_with_cached_prefix",
           "tree_attention_subtree_fwd_kv8_lse", "tree_attention_fwd_kv8_lse", "flatten_append_attention_kv8",
           "flatten_append_attention_kv8_lse", "node_append_attention_kv8", "node_append_attention_kv8_lse"]


def _need(lse):
    if lse is None:
        raise TypeError("lse must be a float32 tensor [n, heads]; the plain operator returns no log-sum-exp")
    return lse


@torch.inference_mode()
def tree_attention_subtree_fwd_lse(query_states, key_buffer, value_buffer, output, lse, block_len, block_q, block_q_cnts,
                                   block_q_offset, block_bitmasks, block_kv, block_lens) -> None:
    """`tree_attention_subtree_fwd` (DeFT-Flatten) that also writes lse[q, h].  A query row that no block lists gets (0, -inf)."""
    _flatten_fwd(query_states, key_buffer, value_buffer, output, _need(lse), block_len, block_q, block_q_cnts, block_q_offset,
                 block_bitmasks, block_kv, block_lens)


@torch.inference_mode()
def tree_attention_fwd_lse(query_states, key_buffer, value_buffer, output, lse, KV_indices, KV_indices_offset, KV_len, KVMapQ_List,
                           KVMapQ_List_Offset, KVMapQ_List_Len) -> None:
    """`tree_attention_fwd` (DeFT-Node) that also writes lse[q, h]."""
    _node_fwd(query_states, key_buffer, value_buffer, output, _need(lse), KV_indices, KV_indices_offset, KV_len, KVMapQ_List,
              KVMapQ_List_Offset, KVMapQ_List_Len)


@torch.inference_mode()
def tree_attention_subtree_fwd_kv8_lse(query_states, key_buffer, value_buffer, output, lse, block_len, block_q, block_q_cnts,
                                       block_q_offset, block_bitmasks, block_kv, block_lens, k_scale=None, v_scale=None, scale=None) -> None:
    """`tree_attention_subtree_fwd_kv8` (DeFT-Flatten over an fp8 pool) that also writes lse[q, h]: the state combines with any
    other through `merge_attention_states`."""
    _flatten_fwd_kv8(query_states, key_buffer, value_buffer, output, _need(lse), block_len, block_q, block_q_cnts, block_q_offset,
                     block_bitmasks, block_kv, block_lens, k_scale, v_scale, scale)


@torch.inference_mode()
def tree_attention_fwd_kv8_lse(query_states, key_buffer, value_buffer, output, lse, KV_indices, KV_indices_offset, KV_len, KVMapQ_List,
                               KVMapQ_List_Offset, KVMapQ_List_Len, k_scale=None, v_scale=None, scale=None) -> None:
    """`tree_attention_fwd_kv8` (DeFT-Node over an fp8 pool) that also writes lse[q, h]."""
    _node_fwd_kv8(query_states, key_buffer, value_buffer, output, _need(lse), KV_indices, KV_indices_offset, KV_len, KVMapQ_List,
                  KVMapQ_List_Offset, KVMapQ_List_Len, k_scale, v_scale, scale)


@torch.inference_mode()
def flatten_append_attention_lse(query_states, kv_layer, output, lse, cache_loc, cache_k, cache_v, block_len, block_q, block_q_cnts,
                                 block_q_offset, block_bitmasks, block_kv, block_lens) -> None:
    """`flatten_append_attention` (paged append fused into Flatten attention) that also writes lse[q, h]."""
    _flatten_append(query_states, kv_layer, output, _need(lse), cache_loc, cache_k, cache_v, block_len, block_q, block_q_cnts,
                    block_q_offset, block_bitmasks, block_kv, block_lens)


@torch.inference_mode()
def node_append_attention_lse(query_states, kv_layer, output, lse, cache_loc, cache_k, cache_v, KV_indices, KV_indices_offset, KV_len,
                              KVMapQ_List, KVMapQ_List_Offset, KVMapQ_List_Len) -> None:
    """`node_append_attention` (paged append fused into Node attention) that also writes lse[q, h]."""
    _node_append(query_states, kv_layer, output, _need(lse), cache_loc, cache_k, cache_v, KV_indices, KV_indices_offset, KV_len,
                 KVMapQ_List, KVMapQ_List_Offset, KVMapQ_List_Len)


# ---- fp8 pools: the quantising append fused into the tree decode ------------------------------------------------------------------------
# `flatten_append_attention` / `node_append_attention` over one layer of an fp8 pool ([slots, 2, Hkv, 128] float8_e4m3fn): cache_k /
# cache_v (16-bit, the type of query_states and output) enter slots cache_loc as the codes kv_append_kv8 writes and the attention
# already sees them -- output, lse and every pool byte are bit-identical to kv_append_kv8 followed by the *_kv8 operator, in one
# stage-1 launch less.  k_scale / v_scale: fp32 [Hkv] on the pool's device or None = ones; `scale`: the softmax scale.
@torch.inference_mode()
def flatten_append_attention_kv8(query_states, kv_layer, output, cache_loc, cache_k, cache_v, block_len, block_q, block_q_cnts,
                                 block_q_offset, block_bitmasks, block_kv, block_lens, k_scale=None, v_scale=None, scale=None) -> None:
    """`kv_append_kv8` + `tree_attention_subtree_fwd_kv8` (DeFT-Flatten over an fp8 pool) in one launch sequence."""
    _flatten_append_kv8(query_states, kv_layer, output, None, cache_loc, cache_k, cache_v, block_len, block_q, block_q_cnts,
                        block_q_offset, block_bitmasks, block_kv, block_lens, k_scale, v_scale, scale)


@torch.inference_mode()
def flatten_append_attention_kv8_lse(query_states, kv_layer, output, lse, cache_loc, cache_k, cache_v, block_len, block_q, block_q_cnts,
                                     block_q_offset, block_bitmasks, block_kv, block_lens, k_scale=None, v_scale=None, scale=None) -> None:
    """`flatten_append_attention_kv8` that also writes lse[q, h]."""
    _flatten_append_kv8(query_states, kv_layer, output, _need(lse), cache_loc, cache_k, cache_v, block_len, block_q, block_q_cnts,
                        block_q_offset, block_bitmasks, block_kv, block_lens, k_scale, v_scale, scale)


@torch.inference_mode()
def node_append_attention_kv8(query_states, kv_layer, output, cache_loc, cache_k, cache_v, KV_indices, KV_indices_offset, KV_len,
                              KVMapQ_List, KVMapQ_List_Offset, KVMapQ_List_Len, k_scale=None, v_scale=None, scale=None) -> None:
    """`kv_append_kv8` + `tree_attention_fwd_kv8` (DeFT-Node over an fp8 pool) in one launch sequence."""
    _node_append_kv8(query_states, kv_layer, output, None, cache_loc, cache_k, cache_v, KV_indices, KV_indices_offset, KV_len,
                     KVMapQ_List, KVMapQ_List_Offset, KVMapQ_List_Len, k_scale, v_scale, scale)


@torch.inference_mode()
def node_append_attention_kv8_lse(query_states, kv_layer, output, lse, cache_loc, cache_k, cache_v, KV_indices, KV_indices_offset,
                                  KV_len, KVMapQ_List, KVMapQ_List_Offset, KVMapQ_List_Len, k_scale=None, v_scale=None, scale=None) -> None:
    """`node_append_attention_kv8` that also writes lse[q, h]."""
    _node_append_kv8(query_states, kv_layer, output, _need(lse), cache_loc, cache_k, cache_v, KV_indices, KV_indices_offset, KV_len,
                     KVMapQ_List, KVMapQ_List_Offset, KVMapQ_List_Len, k_scale, v_scale, scale)


@torch.inference_mode()
def context_attention_fwd_lse(q, k, v, o, lse, b_start_loc, b_seq_len, max_input_len) -> None:
    """`context_attention_fwd` (causal prefill) that also writes lse[token, h] over the tokens 0..i of the token's sequence."""
    _prefill(q, k, v, o, _need(lse), b_start_loc, b_seq_len, max_input_len)


def _check_state(o, lse, name: str):
    if o.dim() != 3 or o.stride(2) != 1:
        raise ValueError(f"{name} must be [n, heads, head_dim] with a contiguous head_dim")
    if lse is None:
        raise TypeError(f"the lse of {name} must be a float32 tensor [n, heads]")
    return _lse_args(lse, o, "the lse of " + name)


@torch.inference_mode()
def merge_attention_states(o_a, lse_a, o_b, lse_b, out=None, lse_out=None):
    """(out, lse_out) = the merge of the states (o_a, lse_a) and (o_b, lse_b) over two disjoint key sets: with m = max(lse_a,
    lse_b), w_x = exp(lse_x - m) and s = w_a + w_b, out = (w_a o_a + w_b o_b) / s in fp32 rounded once and lse_out = m + log s;
    (0, -inf) where both are empty.  A side with lse = -inf has weight exactly 0 whatever its o holds, so merging with the empty
    state returns the other one bit for bit.  o_*: [n, heads, head_dim] float16 or bfloat16 (one type), lse_*: [n, heads] float32.
    `out=None` / `lse_out=None` allocate; `out=o_a` (or o_b) merges in place -- any other overlap of out with an input is an error
    the library does not check.  More than two states: fold pairwise."""
    dtype_of = dict(o_a=o_a, o_b=o_b) if out is None else dict(o_a=o_a, o_b=o_b, out=out)
    same_elem_dtype(**dtype_of)
    if o_a.shape != o_b.shape:
        raise ValueError(f"o_a {tuple(o_a.shape)} and o_b {tuple(o_b.shape)} must have one shape")
    a_args, b_args = _check_state(o_a, lse_a, "o_a"), _check_state(o_b, lse_b, "o_b")
    if out is None:
        out = torch.empty(o_a.shape, dtype=o_a.dtype, device=o_a.device)
    elif out.shape != o_a.shape:
        raise ValueError("out must have the shape of o_a")
    if lse_out is None:
        lse_out = torch.empty(o_a.shape[:2], dtype=torch.float32, device=o_a.device)
    out_args = _check_state(out, lse_out, "out")
    n, Hq, D = o_a.shape
    if D not in (16, 32, 64, 128):
        raise ValueError(f"head_dim must be 16, 32, 64 or 128, got {D}")
    for name, t in (("o_a", o_a), ("lse_a", lse_a), ("o_b", o_b), ("lse_b", lse_b), ("out", out), ("lse_out", lse_out)):
        if not t.is_cuda:
            raise DeftLibraryError(f"{name} must be a CUDA (ROCm) tensor; deft_amd has no CPU path")
    fn, fn_name = entry("deft_merge{}_states", o_a.dtype)
    check(fn(o_a.data_ptr(), o_a.stride(0), o_a.stride(1), *a_args, o_b.data_ptr(), o_b.stride(0), o_b.stride(1), *b_args,
             out.data_ptr(), out.stride(0), out.stride(1), *out_args, n, Hq, D, _stream_ptr(o_a)), fn_name)
    return out, lse_out


def cached_prefix_blocks(path_slots, n_rows: int, max_q_len: int = 32, device="cuda"):
    """The six Flatten arrays (block_q, block_q_cnts, block_q_offset, block_bitmasks, block_kv, block_lens) of "`n_rows` query
    rows that all see every slot of `path_slots`" -- new tokens over a cached prefix.  The slots are cut into 128-slot blocks, the rows
    into chunks of at most `max_q_len` (<= 32: a block's bitmask has 32 bits); the blocks are emitted CHUNK-MAJOR -- all blocks of
    chunk 0, then chunk 1, ... -- so that consecutive blocks share their query list and the plan folds them as runs.
    Every live slot's mask is the chunk's low `cnt` bits; pad slots are -1 with mask 0.  So the prefix is read once per chunk."""
    if not 1 <= max_q_len <= 32:
        raise ValueError(f"max_q_len must be 1..32, got {max_q_len}")
    slots = torch.as_tensor(path_slots, dtype=torch.int64).reshape(-1).cpu()
    n_slots, n_rows = int(slots.shape[0]), int(n_rows)
    if n_rows < 0:
        raise ValueError(f"n_rows must be >= 0, got {n_rows}")
    nb = (n_slots + 127) // 128           # blocks per chunk
    nc = (n_rows + max_q_len - 1) // max_q_len if nb else 0  # chunks
    kv = torch.full((nb * 128,), -1, dtype=torch.int64)
    kv[:n_slots] = slots
    lens = torch.full((nb,), 128, dtype=torch.int64)
    if nb:
        lens[-1] = n_slots - 128 * (nb - 1)
    cnts = torch.full((nc,), max_q_len, dtype=torch.int64)
    if nc:
        cnts[-1] = n_rows - max_q_len * (nc - 1)
    live = (kv >= 0).to(torch.int64)                                              # [nb * 128]
    block_q = torch.cat([torch.arange(c * max_q_len, c * max_q_len + int(cnts[c]), dtype=torch.int64).repeat(nb) for c in range(nc)]
                        or [torch.empty(0, dtype=torch.int64)])
    block_q_cnts = cnts.repeat_interleave(nb)
    block_q_offset = torch.cumsum(block_q_cnts, 0) - block_q_cnts
    block_bitmasks = ((torch.bitwise_left_shift(torch.ones_like(cnts), cnts) - 1)[:, None] * live[None, :]).reshape(-1)
    block_kv = kv.repeat(nc)
    block_lens = lens.repeat(nc)
    return tuple(t.to(device) for t in (block_q, block_q_cnts, block_q_offset, block_bitmasks, block_kv, block_lens))


@torch.inference_mode()
def prefill_with_cached_prefix(q, k, v, out, kv_layer, path_slots, new_slots, lse=None) -> None:
    """Prefill the n1 new tokens q / k / v ([n1, heads, head_dim]) of ONE sequence whose prefix is already in the paged pool:
    multi-turn, a fresh branch with a long thought, chunked prefill.  `kv_layer` is one layer of the pool ([size, 2, Hkv, D]),
    `path_slots` the pool slots of the cached prefix in order, `new_slots` the n1 slots the new rows go to.  out[i] = attention of
    new token i over the whole prefix and the new tokens 0..i; `lse` (optional, [n1, heads] float32) receives the log-sum-exp of
    that whole causal row.  No new attention kernel: (1) `context_attention_fwd_lse` causally over the new tokens, (2)
    `tree_attention_subtree_fwd_lse` over `cached_prefix_blocks(path_slots, n1)`, (3) one in-place merge of the two states, (4)
    `kv_append` of the new rows to `new_slots`.  RoPE stays the caller's, as for ForwardMode.PREFILL.

    Cost, plainly: the cached part reads the prefix once per 32-row chunk of new tokens and the block arrays are built on the host
    at every call.  The one measurement there is (profiles/states_cost.txt: 4096 cached tokens, Llama-2-7B heads) has this
    form 3.5 x (256 new tokens) and 8.5 x (1024) SLOWER than a whole-prompt `context_attention_fwd` over all the tokens; against
    anything else it has not been measured.  It saves the prefix's projections, not attention time, and nothing picks it automatically."""
    if kv_layer.dtype == torch.float8_e4m3fn:
        raise NotImplementedError("prefill_with_cached_prefix over an fp8 KV pool is not implemented (fp8 pools serve the tree decode steps and the append of a plain prefill)")
    n1, Hq = q.shape[0], q.shape[1]
    if n1 == 0:
        return
    lse_new = lse if lse is not None else torch.empty((n1, Hq), dtype=torch.float32, device=q.device)
    zero = torch.zeros(1, dtype=torch.int32, device=q.device)
    _prefill(q, k, v, out, lse_new, zero, torch.full((1,), n1, dtype=torch.int32, device=q.device), n1)
    slots = torch.as_tensor(path_slots, dtype=torch.int64).reshape(-1)
    if slots.shape[0]:
        o_c = torch.empty(out.shape, dtype=out.dtype, device=out.device)
        lse_c = torch.empty((n1, Hq), dtype=torch.float32, device=q.device)
        _flatten_fwd(q, kv_layer[:, 0], kv_layer[:, 1], o_c, lse_c, 128, *cached_prefix_blocks(slots, n1, device=q.device))
        merge_attention_states(out, lse_new, o_c, lse_c, out=out, lse_out=lse_new)
    kv_append(kv_layer, torch.as_tensor(new_slots, dtype=torch.int32), k, v)
