"""Dense tree attention in a chosen precision and the a-priori error bound of the bfloat16 kernels -- shared by the bf16 tests (tests/bf16_util.py) and the fuzzers' --bf16 runs.
On paths without a repeated slot `dense_attention` is tests/truth.py::tree_truth (tests/test_bf16_host.py pins that on the CPU).

With p the fp64 softmax weights of a query row and head, per output element e:

    o_e = sum_i p_i v_ie        A_e = sum_i p_i |v_ie|        tol_e = u A_e + 2 u |o_e| + 2e-5,   u = 2^-8

Scores and exponentials are fp32 (the 2e-5, for |score| up to ~40); each probability is rounded once, to nearest even, to bf16 and the
weights are normalised by the sum of the ROUNDED values (at most u (A_e + |o_e|)); fp32 partials and the log-sum-exp merge add nothing
visible; the one final rounding adds at most u |o_e|.  DESIGN.md, "element types"."""
from __future__ import annotations

from typing import Sequence

import torch

U_BF16 = 2.0 ** -8


def _gather(leaf_paths, dev):
    """(union slots, counts [nq, S]): how often each slot of the union lies on each row's path.  A path is a MULTISET: a
    speculative-decoding merge without its reset (tree_cache.py:300-325) leaves a slot both in the node that took it over and in the
    leaf below it, and the kernels then attend to that key twice -- so does this."""
    nq = len(leaf_paths)
    paths = [torch.as_tensor(list(p), dtype=torch.int64) for p in leaf_paths]
    assert all(p.numel() > 0 for p in paths)
    union, inv = torch.unique(torch.cat(paths), return_inverse=True)
    rows = torch.repeat_interleave(torch.arange(nq), torch.tensor([p.numel() for p in paths]))
    counts = torch.zeros((nq, union.numel()), dtype=torch.float64)
    counts.index_put_((rows, inv), torch.ones(inv.numel(), dtype=torch.float64), accumulate=True)
    return union.to(dev), counts.to(dev)


def dense_attention(q, k_buf, v_buf, leaf_paths: Sequence[Sequence[int]], Hq: int, Hkv: int, scale: float, dtype=torch.float64,
                    with_abs: bool = False):
    """Every query row's softmax attention over the pool slots of its path, in `dtype` (fp64: the truth; fp32: the reference's
    arithmetic before its one rounding); the union of the paths is gathered once.  Optionally with A = sum_i p_i |v_i| alongside:
    one more einsum with v.abs().  Returns [nq, Hq, D] (and A)."""
    nq = len(leaf_paths)
    D = k_buf.shape[-1] if k_buf.dim() == 3 else k_buf.shape[-1] // Hkv
    G = Hq // Hkv
    assert G * Hkv == Hq and q.shape[0] == nq and q.numel() == nq * Hq * D
    union, counts = _gather(leaf_paths, k_buf.device)
    k = k_buf.reshape(k_buf.shape[0], Hkv, D)[union].to(dtype)
    v = v_buf.reshape(v_buf.shape[0], Hkv, D)[union].to(dtype)
    qq = q.reshape(nq, Hkv, G, D).to(device=k.device, dtype=dtype)
    s = torch.einsum("nhgd,shd->nhgs", qq, k) * scale
    s += counts.log().to(dtype)[:, None, None, :]  # a key held c times weighs c exp(s); log 0 = -inf masks what is not on the path
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("nhgs,shd->nhgd", p, v).reshape(nq, Hq, D)
    if not with_abs:
        return o
    return o, torch.einsum("nhgs,shd->nhgd", p, v.abs()).reshape(nq, Hq, D)


def bound_bf16(o: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """tol_e = u A_e + 2 u |o_e| + 2e-5 (module docstring)."""
    return U_BF16 * A + 2.0 * U_BF16 * o.abs() + 2e-5
