"""fp64 model of attention STATES (deft_amd/states.py): the log-sum-exp half of a state over a tree path or a causal row, the state
of a query over any slot list (an empty one included), and the merge of two states as the C header defines it.  Outputs come from
tests/truth.py::tree_truth; this file adds what that has no notion of."""
from __future__ import annotations

from typing import Sequence

import torch


def path_lse(q, k_buf, leaf_paths: Sequence[Sequence[int]], Hq: int, Hkv: int, scale: float) -> torch.Tensor:
    """lse[r, h] = ln sum_{slot in leaf_paths[r]} exp(scale q[r, h] . k[slot, h // G]) in fp64, -inf for an empty path.  [nq, Hq]."""
    dev = k_buf.device
    nq = len(leaf_paths)
    D = k_buf.shape[-1] if k_buf.dim() == 3 else k_buf.shape[-1] // Hkv
    G = Hq // Hkv
    qq = q.reshape(nq, Hkv, G, D).to(device=dev, dtype=torch.float64)
    out = torch.full((nq, Hq), float("-inf"), dtype=torch.float64, device=dev)
    for r, p in enumerate(leaf_paths):
        if len(p) == 0:
            continue
        k = k_buf.reshape(k_buf.shape[0], Hkv, D)[torch.as_tensor(list(p), dtype=torch.int64, device=dev)].to(torch.float64)
        s = torch.einsum("hgd,shd->hgs", qq[r], k) * scale
        out[r] = torch.logsumexp(s, dim=-1).reshape(Hq)
    return out


def causal_lse(q, k, v, start, lens, scale: float) -> torch.Tensor:
    """lse[t, h] of packed causal attention (token i of a sequence over its tokens 0..i), fp64 [T, Hq]."""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    out = torch.empty((T, Hq), dtype=torch.float64, device=q.device)
    for s0, n in zip([int(x) for x in start], [int(x) for x in lens]):
        qq = q[s0 : s0 + n].to(torch.float64).reshape(n, Hkv, G, D)
        s = torch.einsum("ihgd,jhd->hgij", qq, k[s0 : s0 + n].to(torch.float64)) * scale
        s.masked_fill_(torch.ones(n, n, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
        out[s0 : s0 + n] = torch.logsumexp(s, dim=-1).permute(2, 0, 1).reshape(n, Hq)
    return out


def merge_model(o_a, lse_a, o_b, lse_b):
    """The merge of two states in fp64, in the header's order: m = max; (0, -inf) where m = -inf; w = exp(lse - m) with weight exactly
    0 for an empty side WHATEVER its o holds; o = (w_a o_a + w_b o_b) / s; lse = m + log s.  o_*: [n, H, D] any float dtype (read
    exactly), lse_*: [n, H].  Returns (o fp64, lse fp64)."""
    la, lb = lse_a.to(torch.float64), lse_b.to(torch.float64)
    m = torch.maximum(la, lb)
    dead = torch.isinf(m) & (m < 0)
    ms = torch.where(dead, torch.zeros_like(m), m)
    wa, wb = torch.exp(la - ms), torch.exp(lb - ms)  # exp(-inf) = 0
    s = wa + wb
    xa = torch.where((wa > 0)[..., None], o_a.to(torch.float64) * wa[..., None], torch.zeros((), dtype=torch.float64, device=m.device))
    xb = torch.where((wb > 0)[..., None], o_b.to(torch.float64) * wb[..., None], torch.zeros((), dtype=torch.float64, device=m.device))
    o = torch.where(dead[..., None], torch.zeros((), dtype=torch.float64, device=m.device), (xa + xb) / torch.where(dead, torch.ones_like(s), s)[..., None])
    lse = torch.where(dead, m, ms + torch.log(torch.where(dead, torch.ones_like(s), s)))
    return o, lse
