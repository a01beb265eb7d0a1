"""The two replaceable operators of the reference, backed by libdeft_amd.so.

Same names, positional signatures, in-place output and argument meaning as
DeFT/deft/layers/attention/tree_attention.py:

  tree_attention_subtree_fwd (:551-667)   DeFT-Flatten
  tree_attention_fwd         (:14-68)     DeFT-Node

so `DeFTAttention.deft_flatten_forward / deft_node_forward`
(DeFT/deft/layers/attention/deft_attention.py:136-148, :94-105) can import them
from here unchanged.  Launches are asynchronous on torch's current stream, the
functions keep no state, and temporaries come from torch's caching allocator —
like the reference (:588-597, :307-312).  `output` is overwritten; the reference
needs it pre-zeroed (:546), which is tolerated.

There is no PyTorch or CPU fallback: tensors must be fp16 or bf16 CUDA tensors (one element type per call) and the
HIP library must be loadable.
"""
from __future__ import annotations

import torch

from ._lib import KV8_DTYPE, DeftLibraryError, check, entry, lib, same_elem_dtype, tensor_version

__all__ = ["tree_attention_subtree_fwd", "tree_attention_fwd", "flatten_append_attention", "kv_append",
           "flatten_stage1_partials", "tree_attention_subtree_fwd_kv8", "tree_attention_fwd_kv8", "kv_append_kv8"]


def _stream_ptr(t: torch.Tensor) -> int:
    """torch's current stream on the tensor's device.  The library keeps per-device facts (CU count, raised LDS limits) under
    HIP's CURRENT device, so the tensors must live on it -- one process per GPU with torch.cuda.set_device(local_rank), or
    `with torch.cuda.device(t.device):` around the call."""
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        raise DeftLibraryError(f"tensors on {t.device} but the current device is cuda:{torch.cuda.current_device()}: "
                               "call inside `with torch.cuda.device(tensor.device):`")
    return torch.cuda.current_stream(t.device).cuda_stream


def _check_qkv(query_states, key_buffer, value_buffer, output):
    same_elem_dtype(query_states=query_states, key_buffer=key_buffer, value_buffer=value_buffer, output=output)
    for name, t in (("query_states", query_states), ("key_buffer", key_buffer), ("value_buffer", value_buffer),
                    ("output", output)):
        if not t.is_cuda:
            raise DeftLibraryError(f"{name} must be a CUDA (ROCm) tensor; deft_amd has no CPU path")
        if t.dim() != 3 or t.stride(2) != 1:
            raise ValueError(f"{name} must be [n, heads, head_dim] with a contiguous head_dim")
    nq, Hq, D = query_states.shape
    Hkv = key_buffer.shape[1]
    assert D in {16, 32, 64, 128}  # tree_attention.py:100, :582
    if key_buffer.shape != value_buffer.shape or key_buffer.stride() != value_buffer.stride():
        raise ValueError("key_buffer and value_buffer must have identical shape and strides")
    if output.shape != query_states.shape:
        raise ValueError("output must have the shape of query_states")
    return nq, Hq, Hkv, D


def _flatten_plan(md, NB: int, P: int, Hq: int, Hkv: int, q_strides, kv_stride_slot: int, stream: int,
                  cache_loc=None, new_stride: int = 0):
    """Device-side repack of the Flatten metadata, built once per decode step.

    The reference builds TreeMetadata once per step and all layers read the same tensor
    objects (tree_cache.py:1021-1037), so the plan is cached ON the block_q tensor, keyed by
    the identity and in-place version of all six arrays, the head counts and the q / pool
    strides.  Fresh
    tensors (or an in-place edit) simply rebuild it; results never depend on the cache."""
    block_q = md[0]
    versions = [tensor_version(t) for t in md] + ([tensor_version(cache_loc)] if cache_loc is not None else [])
    cacheable = min(versions) >= 0  # inference tensors keep no version counter: their plans are never reused
    key = (lib.deft_plan_variant(), kv_stride_slot, NB, P, Hq, Hkv, tuple(q_strides)) + tuple(t.data_ptr() for t in md) + tuple(versions)
    if cache_loc is not None:  # fused-append plans mark this step's new slots
        key += (cache_loc.data_ptr(), cache_loc.shape[0], new_stride)
    cached = getattr(block_q, "_deft_plan", None) if cacheable else None
    if cached is not None and cached[0] == key:
        return cached[1]
    nbytes = lib.deft_flatten_plan_bytes(NB, P, Hq, Hkv)
    plan = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=block_q.device)
    check(lib.deft_flatten_build_plan(*[t.data_ptr() for t in md], NB, P, Hq, Hkv, q_strides[0], q_strides[1],
                                      kv_stride_slot, cache_loc.data_ptr() if cache_loc is not None else None,
                                      cache_loc.shape[0] if cache_loc is not None else 0, new_stride,
                                      plan.data_ptr(), nbytes, stream), "deft_flatten_build_plan")
    if cacheable:
        try:
            block_q._deft_plan = (key, plan)
        except Exception:  # tensors that refuse attributes just do not cache
            pass
    return plan


def _node_plan(md, NE: int, P: int, total_kv: int, Hq: int, Hkv: int, q_strides, kv_stride_slot: int, stream: int,
               cache_loc=None, new_stride: int = 0):
    """Node-mode counterpart of `_flatten_plan`; cached on the KVMapQ_List (node_q) tensor."""
    node_q = md[3]
    versions = [tensor_version(t) for t in md] + ([tensor_version(cache_loc)] if cache_loc is not None else [])
    cacheable = min(versions) >= 0
    key = (lib.deft_plan_variant(), kv_stride_slot, NE, P, total_kv, Hq, Hkv, tuple(q_strides)) + tuple(t.data_ptr() for t in md) + tuple(versions)
    if cache_loc is not None:  # fused-append plans mark this step's new slots
        key += (cache_loc.data_ptr(), cache_loc.shape[0], new_stride)
    cached = getattr(node_q, "_deft_plan", None) if cacheable else None
    if cached is not None and cached[0] == key:
        return cached[1]
    nbytes = lib.deft_node_plan_bytes(NE, P, total_kv, Hq, Hkv)
    plan = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=node_q.device)
    check(lib.deft_node_build_plan(*[t.data_ptr() for t in md], NE, P, total_kv, Hq, Hkv, q_strides[0], q_strides[1],
                                   kv_stride_slot, cache_loc.data_ptr() if cache_loc is not None else None,
                                   cache_loc.shape[0] if cache_loc is not None else 0, new_stride,
                                   plan.data_ptr(), nbytes, stream), "deft_node_build_plan")
    if cacheable:
        try:
            node_q._deft_plan = (key, plan)
        except Exception:
            pass
    return plan


def _lse_args(lse, query_states, what: str = "lse"):
    """The three ABI arguments of a log-sum-exp output (deft_amd/states.py), or none for a plain call; `lse` must be a float32 CUDA
    tensor [n, heads] -- any strides.  Type and shape here, in front of a call's other checks; the device in _lse_on_device."""
    if lse is None:
        return ()
    if not isinstance(lse, torch.Tensor) or lse.dtype != torch.float32:
        raise TypeError(f"{what} must be a float32 tensor, got {getattr(lse, 'dtype', type(lse))}")
    if tuple(lse.shape) != tuple(query_states.shape[:2]):
        raise ValueError(f"{what} must be [n, heads] = {tuple(query_states.shape[:2])}, got {tuple(lse.shape)}")
    return (lse.data_ptr(), lse.stride(0), lse.stride(1))


def _lse_on_device(lse, what: str = "lse"):
    """Behind every type and shape check of a call, like the device check of its other tensors."""
    if lse is not None and not lse.is_cuda:
        raise DeftLibraryError(f"{what} must be a CUDA (ROCm) tensor; deft_amd has no CPU path")


def _i64(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.int64 or not t.is_cuda:
        raise TypeError(f"{name} must be an int64 CUDA tensor (TreeMetadata contract)")
    return t if t.is_contiguous() else t.contiguous()


@torch.inference_mode()
def tree_attention_subtree_fwd(
    query_states: torch.Tensor,  # (query_num, num_heads, head_dim)
    key_buffer: torch.Tensor,  # (-1, num_kv_heads, head_dim)
    value_buffer: torch.Tensor,  # (-1, num_kv_heads, head_dim)
    output: torch.Tensor,  # (query_num, num_heads, head_dim)
    block_len: int,
    block_q: torch.Tensor,  # (partial_q_num)
    block_q_cnts: torch.Tensor,  # (block_num)
    block_q_offset: torch.Tensor,  # (block_num)
    block_bitmasks: torch.Tensor,  # (kv_len)
    block_kv: torch.Tensor,  # (kv_len)
    block_lens: torch.Tensor,  # (block_num)
) -> None:
    _flatten_fwd(query_states, key_buffer, value_buffer, output, None, block_len, block_q, block_q_cnts, block_q_offset,
                 block_bitmasks, block_kv, block_lens)


def _flatten_fwd(query_states, key_buffer, value_buffer, output, lse, block_len, block_q, block_q_cnts, block_q_offset,
                 block_bitmasks, block_kv, block_lens) -> None:
    """The body of tree_attention_subtree_fwd; with `lse` the *_lse entry point, which also writes every row's log-sum-exp."""
    lse_args = _lse_args(lse, query_states)  # (first: refused without a GPU as well)
    nq, Hq, Hkv, D = _check_qkv(query_states, key_buffer, value_buffer, output)
    _lse_on_device(lse)
    if block_len != 128:
        # the reference kernel hard-codes BLOCK_N=128 and ignores this argument (tree_attention.py:655, :922)
        raise ValueError(f"block_len must be 128 (got {block_len})")
    NB = block_q_cnts.shape[0]
    P = block_q.shape[0]
    md = [_i64(t, n) for t, n in ((block_q, "block_q"), (block_q_cnts, "block_q_cnts"),
                                  (block_q_offset, "block_q_offset"), (block_bitmasks, "block_bitmasks"),
                                  (block_kv, "block_kv"), (block_lens, "block_lens"))]
    if block_kv.shape[0] != NB * 128 or block_bitmasks.shape[0] != NB * 128:
        raise ValueError("block_kv / block_bitmasks must hold 128 entries per block")
    ws_bytes = lib.deft_flatten_workspace_bytes(NB, P, nq, Hq, Hkv, D)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=query_states.device)
    scale = 1.0 / (D ** 0.5)  # tree_attention.py:601
    stream = _stream_ptr(query_states)
    plan = _flatten_plan(md, NB, P, Hq, Hkv, (query_states.stride(0), query_states.stride(1)), key_buffer.stride(0), stream)
    fn, fn_name = entry("deft_flatten_decode{}_lse" if lse_args else "deft_flatten_decode", query_states.dtype)
    rc = fn(
        query_states.data_ptr(), query_states.stride(0), query_states.stride(1),
        key_buffer.data_ptr(), value_buffer.data_ptr(), key_buffer.stride(0), key_buffer.stride(1),
        output.data_ptr(), output.stride(0), output.stride(1), *lse_args,
        *[t.data_ptr() for t in md],
        NB, P, nq, Hq, Hkv, D, scale, plan.data_ptr(), ws.data_ptr(), ws_bytes, stream,
    )
    check(rc, fn_name)


@torch.inference_mode()
def flatten_append_attention(query_states, kv_layer, output, cache_loc, cache_k, cache_v, block_len, block_q, block_q_cnts,
                             block_q_offset, block_bitmasks, block_kv, block_lens) -> None:
    """`store_kv_cache` + `tree_attention_subtree_fwd` in ONE launch sequence
    (DeFTAttention.deft_flatten_forward, deft_attention.py:110-151): kv_layer[cache_loc, 0/1] = cache_k / cache_v
    and output = Flatten attention that already sees those rows.  kv_layer is one layer of the pool,
    [size, 2, Hkv, D] fp16 or bf16 (memory_pool.py:61-66)."""
    _flatten_append(query_states, kv_layer, output, None, cache_loc, cache_k, cache_v, block_len, block_q, block_q_cnts,
                    block_q_offset, block_bitmasks, block_kv, block_lens)


def _flatten_append(query_states, kv_layer, output, lse, cache_loc, cache_k, cache_v, block_len, block_q, block_q_cnts,
                    block_q_offset, block_bitmasks, block_kv, block_lens) -> None:
    key_buffer, value_buffer = kv_layer[:, 0], kv_layer[:, 1]
    lse_args = _lse_args(lse, query_states)  # (first: refused without a GPU as well)
    nq, Hq, Hkv, D = _check_qkv(query_states, key_buffer, value_buffer, output)
    _lse_on_device(lse)
    if block_len != 128:
        raise ValueError(f"block_len must be 128 (got {block_len})")
    NB, P = block_q_cnts.shape[0], block_q.shape[0]
    md = [_i64(t, n) for t, n in ((block_q, "block_q"), (block_q_cnts, "block_q_cnts"),
                                  (block_q_offset, "block_q_offset"), (block_bitmasks, "block_bitmasks"),
                                  (block_kv, "block_kv"), (block_lens, "block_lens"))]
    same_elem_dtype(query_states=query_states, cache_k=cache_k, cache_v=cache_v)
    n = cache_loc.shape[0]
    k = cache_k.reshape(n, Hkv, D)
    v = cache_v.reshape(n, Hkv, D)
    if k.stride(2) != 1 or k.stride(1) != D:
        k = k.contiguous()
    if v.stride() != k.stride():
        k, v = k.contiguous(), v.contiguous()
    if cache_loc.dtype != torch.int32 or not cache_loc.is_cuda:
        cache_loc = cache_loc.to(device=query_states.device, dtype=torch.int32)
    ws_bytes = lib.deft_flatten_workspace_bytes(NB, P, nq, Hq, Hkv, D)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=query_states.device)
    stream = _stream_ptr(query_states)
    plan = _flatten_plan(md, NB, P, Hq, Hkv, (query_states.stride(0), query_states.stride(1)), key_buffer.stride(0), stream,
                         cache_loc=cache_loc, new_stride=k.stride(0))
    fn, fn_name = entry("deft_flatten_decode_append{}_lse" if lse_args else "deft_flatten_decode_append", query_states.dtype)
    rc = fn(
        query_states.data_ptr(), query_states.stride(0), query_states.stride(1),
        key_buffer.data_ptr(), value_buffer.data_ptr(), key_buffer.stride(0), key_buffer.stride(1),
        output.data_ptr(), output.stride(0), output.stride(1), *lse_args,
        *[t.data_ptr() for t in md],
        NB, P, nq, Hq, Hkv, D, 1.0 / (D ** 0.5),
        cache_loc.data_ptr(), k.data_ptr(), v.data_ptr(), k.stride(0), n,
        plan.data_ptr(), ws.data_ptr(), ws_bytes, stream,
    )
    check(rc, fn_name)


@torch.inference_mode()
def tree_attention_fwd(
    query_states: torch.Tensor,  # (query_num, num_heads, head_dim)
    key_buffer: torch.Tensor,  # (-1, num_heads, head_dim)
    value_buffer: torch.Tensor,  # (-1, num_heads, head_dim)
    output: torch.Tensor,  # (query_num, num_heads, head_dim)
    KV_indices: torch.Tensor,  # (total_len)
    KV_indices_offset: torch.Tensor,  # (KV_num)
    KV_len: torch.Tensor,  # (KV_num)
    KVMapQ_List: torch.Tensor,  # (parital_num)
    KVMapQ_List_Offset: torch.Tensor,  # (kv_num)
    KVMapQ_List_Len: torch.Tensor,  # (kv_num)
) -> None:
    _node_fwd(query_states, key_buffer, value_buffer, output, None, KV_indices, KV_indices_offset, KV_len, KVMapQ_List,
              KVMapQ_List_Offset, KVMapQ_List_Len)


def _node_fwd(query_states, key_buffer, value_buffer, output, lse, KV_indices, KV_indices_offset, KV_len, KVMapQ_List,
              KVMapQ_List_Offset, KVMapQ_List_Len) -> None:
    """The body of tree_attention_fwd; with `lse` the *_lse entry point."""
    lse_args = _lse_args(lse, query_states)  # (first: refused without a GPU as well)
    nq, Hq, Hkv, D = _check_qkv(query_states, key_buffer, value_buffer, output)
    _lse_on_device(lse)
    NE = KV_indices_offset.shape[0]
    P = KVMapQ_List.shape[0]
    total_kv = KV_indices.shape[0]
    md = [_i64(t, n) for t, n in ((KV_indices, "KV_indices"), (KV_indices_offset, "KV_indices_offset"),
                                  (KV_len, "KV_len"), (KVMapQ_List, "KVMapQ_List"),
                                  (KVMapQ_List_Offset, "KVMapQ_List_Offset"), (KVMapQ_List_Len, "KVMapQ_List_Len"))]
    ws_bytes = lib.deft_node_workspace_bytes(NE, P, total_kv, nq, Hq, Hkv, D)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=query_states.device)
    scale = 1.0 / (D ** 0.5)  # tree_attention.py:102
    stream = _stream_ptr(query_states)
    plan = _node_plan(md, NE, P, total_kv, Hq, Hkv, (query_states.stride(0), query_states.stride(1)),
                      key_buffer.stride(0), stream)
    fn, fn_name = entry("deft_node_decode{}_lse" if lse_args else "deft_node_decode", query_states.dtype)
    rc = fn(
        query_states.data_ptr(), query_states.stride(0), query_states.stride(1),
        key_buffer.data_ptr(), value_buffer.data_ptr(), key_buffer.stride(0), key_buffer.stride(1),
        output.data_ptr(), output.stride(0), output.stride(1), *lse_args,
        *[t.data_ptr() for t in md],
        NE, P, total_kv, nq, Hq, Hkv, D, scale, plan.data_ptr(), ws.data_ptr(), ws_bytes, stream,
    )
    check(rc, fn_name)


@torch.inference_mode()
def node_append_attention(query_states, kv_layer, output, cache_loc, cache_k, cache_v, KV_indices, KV_indices_offset,
                          KV_len, KVMapQ_List, KVMapQ_List_Offset, KVMapQ_List_Len) -> None:
    """`store_kv_cache` + `tree_attention_fwd` in ONE launch sequence (DeFTAttention.deft_node_forward,
    deft_attention.py:72-108): kv_layer[cache_loc, 0/1] = cache_k / cache_v and output = Node attention that
    already sees those rows."""
    _node_append(query_states, kv_layer, output, None, cache_loc, cache_k, cache_v, KV_indices, KV_indices_offset, KV_len,
                 KVMapQ_List, KVMapQ_List_Offset, KVMapQ_List_Len)


def _node_append(query_states, kv_layer, output, lse, cache_loc, cache_k, cache_v, KV_indices, KV_indices_offset, KV_len,
                 KVMapQ_List, KVMapQ_List_Offset, KVMapQ_List_Len) -> None:
    key_buffer, value_buffer = kv_layer[:, 0], kv_layer[:, 1]
    lse_args = _lse_args(lse, query_states)  # (first: refused without a GPU as well)
    nq, Hq, Hkv, D = _check_qkv(query_states, key_buffer, value_buffer, output)
    _lse_on_device(lse)
    NE = KV_indices_offset.shape[0]
    P = KVMapQ_List.shape[0]
    total_kv = KV_indices.shape[0]
    md = [_i64(t, n) for t, n in ((KV_indices, "KV_indices"), (KV_indices_offset, "KV_indices_offset"),
                                  (KV_len, "KV_len"), (KVMapQ_List, "KVMapQ_List"),
                                  (KVMapQ_List_Offset, "KVMapQ_List_Offset"), (KVMapQ_List_Len, "KVMapQ_List_Len"))]
    same_elem_dtype(query_states=query_states, cache_k=cache_k, cache_v=cache_v)
    n = cache_loc.shape[0]
    k = cache_k.reshape(n, Hkv, D)
    v = cache_v.reshape(n, Hkv, D)
    if k.stride(2) != 1 or k.stride(1) != D:
        k = k.contiguous()
    if v.stride() != k.stride():
        k, v = k.contiguous(), v.contiguous()
    if cache_loc.dtype != torch.int32 or not cache_loc.is_cuda:
        cache_loc = cache_loc.to(device=query_states.device, dtype=torch.int32)
    ws_bytes = lib.deft_node_workspace_bytes(NE, P, total_kv, nq, Hq, Hkv, D)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=query_states.device)
    stream = _stream_ptr(query_states)
    plan = _node_plan(md, NE, P, total_kv, Hq, Hkv, (query_states.stride(0), query_states.stride(1)),
                      key_buffer.stride(0), stream, cache_loc=cache_loc, new_stride=k.stride(0))
    fn, fn_name = entry("deft_node_decode_append{}_lse" if lse_args else "deft_node_decode_append", query_states.dtype)
    rc = fn(
        query_states.data_ptr(), query_states.stride(0), query_states.stride(1),
        key_buffer.data_ptr(), value_buffer.data_ptr(), key_buffer.stride(0), key_buffer.stride(1),
        output.data_ptr(), output.stride(0), output.stride(1), *lse_args,
        *[t.data_ptr() for t in md],
        NE, P, total_kv, nq, Hq, Hkv, D, 1.0 / (D ** 0.5),
        cache_loc.data_ptr(), k.data_ptr(), v.data_ptr(), k.stride(0), n,
        plan.data_ptr(), ws.data_ptr(), ws_bytes, stream,
    )
    check(rc, fn_name)


@torch.inference_mode()
def kv_append(kv_layer: torch.Tensor, cache_loc: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor) -> None:
    """kv_layer[cache_loc, 0] = cache_k; kv_layer[cache_loc, 1] = cache_v in one launch.

    kv_layer is one layer of the pool, [size, 2, Hkv, D] fp16 or bf16 (memory_pool.py:61-66);
    semantics of KVCacheUpdater.update, paged branch (tree_cache.py:70-76)."""
    same_elem_dtype(kv_layer=kv_layer, cache_k=cache_k, cache_v=cache_v)
    if not kv_layer.is_cuda:
        raise DeftLibraryError("kv_append needs a CUDA (ROCm) pool; deft_amd has no CPU path")
    size, two, Hkv, D = kv_layer.shape
    assert two == 2 and kv_layer.stride(3) == 1
    n = cache_loc.shape[0]
    k = cache_k.reshape(n, Hkv, D)
    v = cache_v.reshape(n, Hkv, D)
    if k.stride(2) != 1 or k.stride(1) != D:
        k = k.contiguous()
    if v.stride() != k.stride():
        v = v.contiguous()
        k = k.contiguous()
    if cache_loc.dtype != torch.int32:
        cache_loc = cache_loc.to(torch.int32)
    cache_loc = cache_loc.to(kv_layer.device)
    fn, fn_name = entry("deft_kv_append", kv_layer.dtype)
    rc = fn(
        kv_layer[:, 0].data_ptr(), kv_layer[:, 1].data_ptr(), kv_layer.stride(0), kv_layer.stride(2),
        cache_loc.data_ptr(), k.data_ptr(), v.data_ptr(), k.stride(0), n, Hkv, D, _stream_ptr(kv_layer),
    )
    check(rc, fn_name)


@torch.inference_mode()
def flatten_stage1_partials(query_states, key_buffer, value_buffer, block_q, block_q_cnts, block_q_offset,
                            block_bitmasks, block_kv, block_lens):
    """Stage 1 only; returns (partial_o [Hq,P,D] f32, partial_lse [Hq,P] f32) like the
    reference's temporaries (tree_attention.py:588-597).  For tests and profiling."""
    same_elem_dtype(query_states=query_states, key_buffer=key_buffer, value_buffer=value_buffer)
    nq, Hq, D = query_states.shape
    Hkv = key_buffer.shape[1]
    NB, P = block_q_cnts.shape[0], block_q.shape[0]
    ws_bytes = lib.deft_flatten_workspace_bytes(NB, P, nq, Hq, Hkv, D)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=query_states.device)
    st = _stream_ptr(query_states)
    fn, fn_name = entry("deft_flatten_stage1", query_states.dtype)
    rc = fn(
        query_states.data_ptr(), query_states.stride(0), query_states.stride(1),
        key_buffer.data_ptr(), value_buffer.data_ptr(), key_buffer.stride(0), key_buffer.stride(1),
        block_q.data_ptr(), block_q_cnts.data_ptr(), block_q_offset.data_ptr(), block_bitmasks.data_ptr(),
        block_kv.data_ptr(), block_lens.data_ptr(), NB, P, nq, Hq, Hkv, D, 1.0 / (D ** 0.5),
        None, ws.data_ptr(), ws_bytes, st,
    )
    check(rc, fn_name)
    po = torch.empty((Hq, P, D), dtype=torch.float32, device=query_states.device)
    pl = torch.empty((Hq, P), dtype=torch.float32, device=query_states.device)
    check(lib.deft_flatten_read_partials(ws.data_ptr(), ws_bytes, NB, P, nq, Hq, Hkv, D, po.data_ptr(), pl.data_ptr(), st),
          "deft_flatten_read_partials")
    return po, pl


# ---------------------------------------------------------------------------
# fp8 KV pools: OCP e4m3fn codes (torch.float8_e4m3fn) with per-KV-head fp32 scales.  q / output / the new rows keep one 16-bit
# element type; a stored code c of head h means float(c) * scale[h].  kv_append_kv8, then the operator, is two
# stage-1-side launches; the *_append_attention_kv8 operators (deft_amd/states.py, bodies at the end of this file) fuse them.
# ---------------------------------------------------------------------------
def _kv8_scale(scale, name: str, Hkv: int, device):
    """Device pointer of a per-KV-head scale tensor (fp32, `Hkv` elements, on the pool's device), or None = all ones."""
    if scale is None:
        return None
    if not isinstance(scale, torch.Tensor) or scale.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor of {Hkv} per-KV-head scales or None, got {getattr(scale, 'dtype', type(scale))}")
    if scale.numel() != Hkv:
        raise TypeError(f"{name} must hold one scale per KV head ({Hkv}), got {scale.numel()}")
    if scale.device != device:
        raise TypeError(f"{name} is on {scale.device} but the KV pool is on {device}")
    if not scale.is_contiguous():
        scale = scale.contiguous()
    return scale


def _check_qkv_kv8(query_states, key_buffer, value_buffer, output, k_scale, v_scale):
    dtype = same_elem_dtype(query_states=query_states, output=output)
    for name, t in (("key_buffer", key_buffer), ("value_buffer", value_buffer)):
        if t.dtype != KV8_DTYPE:
            raise TypeError(f"{name} must be {KV8_DTYPE} (an fp8 KV pool), got {t.dtype}")
    for name, t in (("query_states", query_states), ("key_buffer", key_buffer), ("value_buffer", value_buffer), ("output", output)):
        if t.dim() != 3 or t.stride(2) != 1:
            raise ValueError(f"{name} must be [n, heads, head_dim] with a contiguous head_dim")
    nq, Hq, D = query_states.shape
    Hkv = key_buffer.shape[1]
    ks = _kv8_scale(k_scale, "k_scale", Hkv, key_buffer.device)
    vs = _kv8_scale(v_scale, "v_scale", Hkv, key_buffer.device)
    for name, t in (("query_states", query_states), ("key_buffer", key_buffer), ("value_buffer", value_buffer), ("output", output)):
        if not t.is_cuda:
            raise DeftLibraryError(f"{name} must be a CUDA (ROCm) tensor; deft_amd has no CPU path")
    if D != 128:
        raise ValueError(f"fp8 KV pools are built for head_dim 128 only, got {D}")
    if key_buffer.shape != value_buffer.shape or key_buffer.stride() != value_buffer.stride():
        raise ValueError("key_buffer and value_buffer must have identical shape and strides")
    if output.shape != query_states.shape:
        raise ValueError("output must have the shape of query_states")
    if key_buffer.stride(0) % 2:
        raise ValueError("the fp8 pool's slot stride must be even")
    return dtype, nq, Hq, Hkv, D, ks, vs


def _ptr(t):
    return None if t is None else t.data_ptr()


@torch.inference_mode()
def tree_attention_subtree_fwd_kv8(query_states, key_buffer, value_buffer, output, block_len, block_q, block_q_cnts, block_q_offset,
                                   block_bitmasks, block_kv, block_lens, k_scale=None, v_scale=None, scale=None) -> None:
    """`tree_attention_subtree_fwd` (DeFT-Flatten) over an fp8 pool: key_buffer / value_buffer are float8_e4m3fn views
    [slots, Hkv, 128], k_scale / v_scale fp32 tensors of Hkv per-head scales on the pool's device (None = ones), query_states and
    output one 16-bit type.  `scale` (default 1/sqrt(head_dim)) is the softmax scale."""
    _flatten_fwd_kv8(query_states, key_buffer, value_buffer, output, None, block_len, block_q, block_q_cnts, block_q_offset,
                     block_bitmasks, block_kv, block_lens, k_scale, v_scale, scale)


def _flatten_fwd_kv8(query_states, key_buffer, value_buffer, output, lse, block_len, block_q, block_q_cnts, block_q_offset,
                     block_bitmasks, block_kv, block_lens, k_scale, v_scale, scale=None) -> None:
    lse_args = _lse_args(lse, query_states)
    dtype, nq, Hq, Hkv, D, ks, vs = _check_qkv_kv8(query_states, key_buffer, value_buffer, output, k_scale, v_scale)
    _lse_on_device(lse)
    if block_len != 128:
        raise ValueError(f"block_len must be 128 (got {block_len})")
    NB = block_q_cnts.shape[0]
    P = block_q.shape[0]
    md = [_i64(t, n) for t, n in ((block_q, "block_q"), (block_q_cnts, "block_q_cnts"),
                                  (block_q_offset, "block_q_offset"), (block_bitmasks, "block_bitmasks"),
                                  (block_kv, "block_kv"), (block_lens, "block_lens"))]
    if block_kv.shape[0] != NB * 128 or block_bitmasks.shape[0] != NB * 128:
        raise ValueError("block_kv / block_bitmasks must hold 128 entries per block")
    ws_bytes = lib.deft_flatten_workspace_bytes(NB, P, nq, Hq, Hkv, D)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=query_states.device)
    stream = _stream_ptr(query_states)
    # the plan addresses pool rows in 2-byte units: half the byte stride (tree_attention._flatten_plan caches per stride)
    plan = _flatten_plan(md, NB, P, Hq, Hkv, (query_states.stride(0), query_states.stride(1)), key_buffer.stride(0) // 2, stream)
    fn, fn_name = entry("deft_flatten_decode{}_kv8_lse" if lse_args else "deft_flatten_decode{}_kv8", dtype)
    rc = fn(
        query_states.data_ptr(), query_states.stride(0), query_states.stride(1),
        key_buffer.data_ptr(), value_buffer.data_ptr(), key_buffer.stride(0), key_buffer.stride(1), _ptr(ks), _ptr(vs),
        output.data_ptr(), output.stride(0), output.stride(1), *lse_args,
        *[t.data_ptr() for t in md],
        NB, P, nq, Hq, Hkv, D, 1.0 / (D ** 0.5) if scale is None else float(scale), plan.data_ptr(), ws.data_ptr(), ws_bytes, stream,
    )
    check(rc, fn_name)


@torch.inference_mode()
def tree_attention_fwd_kv8(query_states, key_buffer, value_buffer, output, KV_indices, KV_indices_offset, KV_len, KVMapQ_List,
                           KVMapQ_List_Offset, KVMapQ_List_Len, k_scale=None, v_scale=None, scale=None) -> None:
    """`tree_attention_fwd` (DeFT-Node) over an fp8 pool; arguments as tree_attention_subtree_fwd_kv8."""
    _node_fwd_kv8(query_states, key_buffer, value_buffer, output, None, KV_indices, KV_indices_offset, KV_len, KVMapQ_List,
                  KVMapQ_List_Offset, KVMapQ_List_Len, k_scale, v_scale, scale)


def _node_fwd_kv8(query_states, key_buffer, value_buffer, output, lse, KV_indices, KV_indices_offset, KV_len, KVMapQ_List,
                  KVMapQ_List_Offset, KVMapQ_List_Len, k_scale, v_scale, scale=None) -> None:
    lse_args = _lse_args(lse, query_states)
    dtype, nq, Hq, Hkv, D, ks, vs = _check_qkv_kv8(query_states, key_buffer, value_buffer, output, k_scale, v_scale)
    _lse_on_device(lse)
    NE = KV_indices_offset.shape[0]
    P = KVMapQ_List.shape[0]
    total_kv = KV_indices.shape[0]
    md = [_i64(t, n) for t, n in ((KV_indices, "KV_indices"), (KV_indices_offset, "KV_indices_offset"),
                                  (KV_len, "KV_len"), (KVMapQ_List, "KVMapQ_List"),
                                  (KVMapQ_List_Offset, "KVMapQ_List_Offset"), (KVMapQ_List_Len, "KVMapQ_List_Len"))]
    ws_bytes = lib.deft_node_workspace_bytes(NE, P, total_kv, nq, Hq, Hkv, D)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=query_states.device)
    stream = _stream_ptr(query_states)
    plan = _node_plan(md, NE, P, total_kv, Hq, Hkv, (query_states.stride(0), query_states.stride(1)),
                      key_buffer.stride(0) // 2, stream)
    fn, fn_name = entry("deft_node_decode{}_kv8_lse" if lse_args else "deft_node_decode{}_kv8", dtype)
    rc = fn(
        query_states.data_ptr(), query_states.stride(0), query_states.stride(1),
        key_buffer.data_ptr(), value_buffer.data_ptr(), key_buffer.stride(0), key_buffer.stride(1), _ptr(ks), _ptr(vs),
        output.data_ptr(), output.stride(0), output.stride(1), *lse_args,
        *[t.data_ptr() for t in md],
        NE, P, total_kv, nq, Hq, Hkv, D, 1.0 / (D ** 0.5) if scale is None else float(scale), plan.data_ptr(), ws.data_ptr(), ws_bytes,
        stream,
    )
    check(rc, fn_name)


@torch.inference_mode()
def kv_append_kv8(kv_layer: torch.Tensor, cache_loc: torch.Tensor, cache_k: torch.Tensor, cache_v: torch.Tensor,
                  k_scale=None, v_scale=None) -> None:
    """Quantising paged append: kv_layer[cache_loc, 0] = e4m3fn(clamp(cache_k / k_scale, -448, 448)) and the same for V, rounded to
    nearest even, in one launch.  kv_layer is one layer of an fp8 pool, [size, 2, Hkv, D] float8_e4m3fn; cache_k / cache_v are the
    new rows in fp16 or bf16 (one type); k_scale / v_scale fp32 [Hkv] on the pool's device, or None = ones."""
    if kv_layer.dtype != KV8_DTYPE:
        raise TypeError(f"kv_layer must be {KV8_DTYPE} (an fp8 KV pool), got {kv_layer.dtype}")
    dtype = same_elem_dtype(cache_k=cache_k, cache_v=cache_v)
    size, two, Hkv, D = kv_layer.shape
    ks = _kv8_scale(k_scale, "k_scale", Hkv, kv_layer.device)
    vs = _kv8_scale(v_scale, "v_scale", Hkv, kv_layer.device)
    if not kv_layer.is_cuda:
        raise DeftLibraryError("kv_append_kv8 needs a CUDA (ROCm) pool; deft_amd has no CPU path")
    assert two == 2 and kv_layer.stride(3) == 1
    n = cache_loc.shape[0]
    k = cache_k.reshape(n, Hkv, D)
    v = cache_v.reshape(n, Hkv, D)
    if k.stride(2) != 1 or k.stride(1) != D:
        k = k.contiguous()
    if v.stride() != k.stride():
        v = v.contiguous()
        k = k.contiguous()
    if cache_loc.dtype != torch.int32:
        cache_loc = cache_loc.to(torch.int32)
    cache_loc = cache_loc.to(kv_layer.device)
    fn, fn_name = entry("deft_kv_append{}_kv8", dtype)
    rc = fn(
        kv_layer[:, 0].data_ptr(), kv_layer[:, 1].data_ptr(), kv_layer.stride(0), kv_layer.stride(2), _ptr(ks), _ptr(vs),
        cache_loc.data_ptr(), k.data_ptr(), v.data_ptr(), k.stride(0), n, Hkv, D, _stream_ptr(kv_layer),
    )
    check(rc, fn_name)


# ---- the fused quantising append: kv_append_kv8 + the kv8 operator in one stage-1 launch (public names in deft_amd/states.py) -------
def _check_append_kv8(query_states, kv_layer, output, cache_loc, cache_k, cache_v, k_scale, v_scale):
    """Types first (a TypeError names the wrong argument), then the device, then shapes; returns what the call needs."""
    if not isinstance(kv_layer, torch.Tensor) or kv_layer.dtype != KV8_DTYPE:
        raise TypeError(f"kv_layer must be {KV8_DTYPE} (one layer of an fp8 KV pool), got {getattr(kv_layer, 'dtype', type(kv_layer))}")
    dtype = same_elem_dtype(query_states=query_states, output=output, cache_k=cache_k, cache_v=cache_v)
    if kv_layer.dim() != 4 or kv_layer.shape[1] != 2 or kv_layer.stride(3) != 1:
        raise ValueError("kv_layer must be [slots, 2, Hkv, head_dim] with a contiguous head_dim")
    Hkv = kv_layer.shape[2]
    ks = _kv8_scale(k_scale, "k_scale", Hkv, kv_layer.device)
    vs = _kv8_scale(v_scale, "v_scale", Hkv, kv_layer.device)
    key_buffer, value_buffer = kv_layer[:, 0], kv_layer[:, 1]
    for name, t in (("query_states", query_states), ("output", output)):
        if t.dim() != 3 or t.stride(2) != 1:
            raise ValueError(f"{name} must be [n, heads, head_dim] with a contiguous head_dim")
    for name, t in (("query_states", query_states), ("kv_layer", kv_layer), ("output", output), ("cache_k", cache_k), ("cache_v", cache_v)):
        if not t.is_cuda:
            raise DeftLibraryError(f"{name} must be a CUDA (ROCm) tensor; deft_amd has no CPU path")
    nq, Hq, D = query_states.shape
    if D != 128 or kv_layer.shape[3] != D:
        raise ValueError(f"fp8 KV pools are built for head_dim 128 only, got {D} (pool: {kv_layer.shape[3]})")
    if output.shape != query_states.shape:
        raise ValueError("output must have the shape of query_states")
    if key_buffer.stride(0) % 2:
        raise ValueError("the fp8 pool's slot stride must be even")
    n = cache_loc.shape[0]
    k = cache_k.reshape(n, Hkv, D)
    v = cache_v.reshape(n, Hkv, D)
    if k.stride(2) != 1 or k.stride(1) != D:
        k = k.contiguous()
    if v.stride() != k.stride():
        k, v = k.contiguous(), v.contiguous()
    if cache_loc.dtype != torch.int32 or not cache_loc.is_cuda:
        cache_loc = cache_loc.to(device=query_states.device, dtype=torch.int32)
    return dtype, nq, Hq, Hkv, D, ks, vs, key_buffer, value_buffer, cache_loc, k, v, n


def _flatten_append_kv8(query_states, kv_layer, output, lse, cache_loc, cache_k, cache_v, block_len, block_q, block_q_cnts,
                        block_q_offset, block_bitmasks, block_kv, block_lens, k_scale, v_scale, scale=None) -> None:
    lse_args = _lse_args(lse, query_states)
    dtype, nq, Hq, Hkv, D, ks, vs, key_buffer, value_buffer, cache_loc, k, v, n = _check_append_kv8(
        query_states, kv_layer, output, cache_loc, cache_k, cache_v, k_scale, v_scale)
    _lse_on_device(lse)
    if block_len != 128:
        raise ValueError(f"block_len must be 128 (got {block_len})")
    NB, P = block_q_cnts.shape[0], block_q.shape[0]
    md = [_i64(t, n_) for t, n_ in ((block_q, "block_q"), (block_q_cnts, "block_q_cnts"),
                                    (block_q_offset, "block_q_offset"), (block_bitmasks, "block_bitmasks"),
                                    (block_kv, "block_kv"), (block_lens, "block_lens"))]
    if block_kv.shape[0] != NB * 128 or block_bitmasks.shape[0] != NB * 128:
        raise ValueError("block_kv / block_bitmasks must hold 128 entries per block")
    ws_bytes = lib.deft_flatten_workspace_bytes(NB, P, nq, Hq, Hkv, D)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=query_states.device)
    stream = _stream_ptr(query_states)
    # the plan addresses pool rows in 2-byte units (half the byte stride) and flags this step's rows: their offsets are bytes of k_new
    plan = _flatten_plan(md, NB, P, Hq, Hkv, (query_states.stride(0), query_states.stride(1)), key_buffer.stride(0) // 2, stream,
                         cache_loc=cache_loc, new_stride=k.stride(0))
    fn, fn_name = entry("deft_flatten_decode_append{}_kv8_lse" if lse_args else "deft_flatten_decode_append{}_kv8", dtype)
    rc = fn(
        query_states.data_ptr(), query_states.stride(0), query_states.stride(1),
        key_buffer.data_ptr(), value_buffer.data_ptr(), key_buffer.stride(0), key_buffer.stride(1), _ptr(ks), _ptr(vs),
        output.data_ptr(), output.stride(0), output.stride(1), *lse_args,
        *[t.data_ptr() for t in md],
        NB, P, nq, Hq, Hkv, D, 1.0 / (D ** 0.5) if scale is None else float(scale),
        cache_loc.data_ptr(), k.data_ptr(), v.data_ptr(), k.stride(0), n,
        plan.data_ptr(), ws.data_ptr(), ws_bytes, stream,
    )
    check(rc, fn_name)


def _node_append_kv8(query_states, kv_layer, output, lse, cache_loc, cache_k, cache_v, KV_indices, KV_indices_offset, KV_len,
                     KVMapQ_List, KVMapQ_List_Offset, KVMapQ_List_Len, k_scale, v_scale, scale=None) -> None:
    lse_args = _lse_args(lse, query_states)
    dtype, nq, Hq, Hkv, D, ks, vs, key_buffer, value_buffer, cache_loc, k, v, n = _check_append_kv8(
        query_states, kv_layer, output, cache_loc, cache_k, cache_v, k_scale, v_scale)
    _lse_on_device(lse)
    NE = KV_indices_offset.shape[0]
    P = KVMapQ_List.shape[0]
    total_kv = KV_indices.shape[0]
    md = [_i64(t, n_) for t, n_ in ((KV_indices, "KV_indices"), (KV_indices_offset, "KV_indices_offset"),
                                    (KV_len, "KV_len"), (KVMapQ_List, "KVMapQ_List"),
                                    (KVMapQ_List_Offset, "KVMapQ_List_Offset"), (KVMapQ_List_Len, "KVMapQ_List_Len"))]
    ws_bytes = lib.deft_node_workspace_bytes(NE, P, total_kv, nq, Hq, Hkv, D)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=query_states.device)
    stream = _stream_ptr(query_states)
    plan = _node_plan(md, NE, P, total_kv, Hq, Hkv, (query_states.stride(0), query_states.stride(1)),
                      key_buffer.stride(0) // 2, stream, cache_loc=cache_loc, new_stride=k.stride(0))
    fn, fn_name = entry("deft_node_decode_append{}_kv8_lse" if lse_args else "deft_node_decode_append{}_kv8", dtype)
    rc = fn(
        query_states.data_ptr(), query_states.stride(0), query_states.stride(1),
        key_buffer.data_ptr(), value_buffer.data_ptr(), key_buffer.stride(0), key_buffer.stride(1), _ptr(ks), _ptr(vs),
        output.data_ptr(), output.stride(0), output.stride(1), *lse_args,
        *[t.data_ptr() for t in md],
        NE, P, total_kv, nq, Hq, Hkv, D, 1.0 / (D ** 0.5) if scale is None else float(scale),
        cache_loc.data_ptr(), k.data_ptr(), v.data_ptr(), k.stride(0), n,
        plan.data_ptr(), ws.data_ptr(), ws_bytes, stream,
    )
    check(rc, fn_name)
