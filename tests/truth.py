"""Dense fp64 truth of tree attention, on the tensors' own device: every query row attends over the pool slots of its root-to-leaf
path.  The union of all paths is gathered ONCE (a shared prefix is read once, not once per leaf), a boolean mask [nq, S] says which
of those slots lie on each row's path, and one masked softmax attention runs over them -- GQA by viewing q as [nq, Hkv, G, D].
At the north-star size (4096-token prefix x 32 branches, 32 KV heads of 128) that is a few hundred MB of fp64 K / V and ~0.1 GB of
scores, so a test can hold every leaf and every head of every step against it."""
from __future__ import annotations

from typing import Sequence

import torch


def tree_truth(q, k_buf, v_buf, leaf_paths: Sequence[Sequence[int]], Hq: int, Hkv: int, scale: float) -> torch.Tensor:
    """q: [nq, Hq, D] or [nq, Hq * D]; k_buf / v_buf: [pool, Hkv, D] (or [pool, Hkv * D]); leaf_paths[r]: the pool slots of query
    row r's root-to-leaf path.  Returns fp64 [nq, Hq, D] on k_buf's device."""
    dev = k_buf.device
    nq = len(leaf_paths)
    D = k_buf.shape[-1] if k_buf.dim() == 3 else k_buf.shape[-1] // Hkv
    G = Hq // Hkv
    assert G * Hkv == Hq and q.shape[0] == nq and q.numel() == nq * Hq * D, (tuple(q.shape), nq, Hq, Hkv, D)
    paths = [torch.as_tensor(list(p), dtype=torch.int64) for p in leaf_paths]
    assert all(p.numel() > 0 for p in paths), "a query row without keys has no attention"
    union, inv = torch.unique(torch.cat(paths), return_inverse=True)
    rows = torch.repeat_interleave(torch.arange(nq), torch.tensor([p.numel() for p in paths]))
    mask = torch.zeros((nq, union.numel()), dtype=torch.bool)
    mask[rows, inv] = True
    mask, union = mask.to(dev), union.to(dev)
    k = k_buf.reshape(k_buf.shape[0], Hkv, D)[union].to(torch.float64)  # [S, Hkv, D]
    v = v_buf.reshape(v_buf.shape[0], Hkv, D)[union].to(torch.float64)
    qq = q.reshape(nq, Hkv, G, D).to(device=dev, dtype=torch.float64)
    s = torch.einsum("nhgd,shd->nhgs", qq, k) * scale
    s.masked_fill_(~mask[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("nhgs,shd->nhgd", p, v).reshape(nq, Hq, D)


def product_leaf_paths(tree):
    """Root-to-leaf pool slots of a deft_amd.TreeCache, by query row (leaves in ascending id: the metadata's query order)."""
    return [tree.leaf_path_slots(tree.leaves[i]) for i in sorted(tree.leaves)]


def max_err(out, truth) -> float:
    """max |out - truth| over every row and head (out of any float dtype; the comparison in fp64)."""
    return float((out.reshape(truth.shape).to(torch.float64) - truth).abs().max())
