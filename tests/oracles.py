"""Oracles that can see ONE key at full size, and inputs that break what random data never breaks.

Visibility inputs: K = 0 on every slot and in k_new, V dyadic (multiples of 2^-9, |v| <= 3, exact in fp16).  Every score is then 0 and
every visible key gets P = 1 exactly, so a query's output is the fp64 MEAN of V over the exact multiset of keys on its path -- a dropped,
doubled or foreign key moves it by ~|v| / N, where N(0,1) logits bury it under the 5e-4 tolerance of the truth checks.  The kernels'
sums are exact too (a partial of n keys sums integers times 2^-9 below 2^15 in fp32 up to ~10k keys), so what is left is:

  * the fp16 rounding of the output: at most half an fp16 ulp of the value;
  * the fp32 normalisation (o / l, one rounding) and the LSE merge (lse = log n, weights exp(lse - max), a weighted sum and a
    division): a handful of fp32 roundings and exp / log approximations, each ~2^-23 relative to values of magnitude <= 3, and the
    merge's weight errors only move the output by (weight error) x |partial - mean|.  Bound: 8 x 2^-23 x 3 ~ 2.9e-6 in the worst case;
    in practice the partials sit within ~0.1 of the mean, ~1e-7.

TOLERANCE = one fp16 ulp of the expected value + FLOOR = 2^-20 (~9.5e-7).  Correct kernels leave well inside it (the GPU tests record
the largest residual); the power check below proves, per shape, that one key more or less moves the expectation by >= 4 x it.

Shaped scores: K[slot, h] = a(slot, h) e0 and Q[r, g] = b(g) e0 (plus small dyadic noise on the other dims), so score(r, g, slot, h) =
a b / sqrt(D) takes the shape a test chooses: a sink, a ramp, a spike at a chosen tile.  The truth of those is tests/truth.py."""
from __future__ import annotations

from typing import Dict, Iterable, Sequence

import torch

FLOOR = 2.0 ** -20


# ---- dyadic data ---------------------------------------------------------------------------------------------------------------
def dyadic_(t: torch.Tensor, generator: torch.Generator) -> torch.Tensor:
    """Fill fp16 `t` in place with deft_amd.utils.synthetic.dyadic_normal's distribution (sum of three uniform integers in
    [-512, 512], times 2^-9: std ~1, |x| <= 3, exact in fp16), drawn on t's device."""
    acc = torch.zeros(t.shape, dtype=torch.int32, device=t.device)
    for _ in range(3):
        acc += torch.randint(-512, 513, t.shape, dtype=torch.int32, device=t.device, generator=generator)
    t.copy_(acc.to(torch.float32) / 512.0)
    return t


def visibility_pool(pool, generator: torch.Generator) -> None:
    """K = 0 on every slot of every layer, V dyadic."""
    st = pool._storage  # [layers, size, 2, Hkv, D]
    st[:, :, 0].zero_()
    for l in range(st.shape[0]):
        dyadic_(st[l, :, 1], generator)


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def check_paths(paths: Sequence[Sequence[int]]) -> None:
    for r, p in enumerate(paths):
        assert len(p) > 0 and len(set(int(s) for s in p)) == len(p), f"path of query {r} is empty or holds a slot twice"


def visible_mean(v_buf: torch.Tensor, paths: Sequence[Sequence[int]], chunk: int = 1 << 14) -> torch.Tensor:
    """fp64 mean of V over every query's path: v_buf [pool, H, D] (or [pool, H * D]) -> [nq, H * D], on v_buf's device.  The union of
    the paths is read once (a shared prefix once, not once per query), in chunks of `chunk` slots."""
    check_paths(paths)
    dev = v_buf.device
    nq = len(paths)
    v2 = v_buf.reshape(v_buf.shape[0], -1)
    lens = torch.tensor([len(p) for p in paths], dtype=torch.float64, device=dev)
    flat = torch.cat([torch.as_tensor(list(p), dtype=torch.int64) for p in paths])
    rows = torch.repeat_interleave(torch.arange(nq), torch.tensor([len(p) for p in paths]))
    union, inv = torch.unique(flat, return_inverse=True)
    out = torch.zeros((nq, v2.shape[1]), dtype=torch.float64, device=dev)
    for c0 in range(0, union.numel(), chunk):
        sel = (inv >= c0) & (inv < c0 + chunk)
        m = torch.zeros((nq, min(chunk, union.numel() - c0)), dtype=torch.float64)
        m[rows[sel], inv[sel] - c0] = 1.0
        out += m.to(dev) @ v2[union[c0 : c0 + chunk].to(dev)].to(torch.float64)
    return out / lens[:, None]


def fp16_ulp(x: torch.Tensor) -> torch.Tensor:
    """One fp16 ulp at |x| (fp64): 2^(e - 10) for |x| in [2^e, 2^(e+1)), 2^-24 for the subnormals and 0."""
    a = x.to(torch.float64).abs().clamp_min(2.0 ** -14)
    _, ex = torch.frexp(a)  # a = m 2^ex, m in [0.5, 1): the binade is 2^(ex - 1)
    return torch.pow(2.0, (ex - 11).to(torch.float64))


def tolerance(expected: torch.Tensor) -> torch.Tensor:
    return fp16_ulp(expected) + FLOOR


def residual(out: torch.Tensor, expected: torch.Tensor) -> Dict[str, float]:
    """{"max_err": max |out - expected|, "ratio": max |out - expected| / tolerance, "over_ulp": max (|out - expected| - ulp)} -- the
    last is what the floor has to cover."""
    e = expected.reshape(expected.shape[0], -1)
    o = out.reshape(e.shape).to(torch.float64)
    err = (o - e).abs()
    return {"max_err": float(err.max()), "ratio": float((err / tolerance(e)).max()), "over_ulp": float((err - fp16_ulp(e)).max())}


def assert_visible_mean(out: torch.Tensor, expected: torch.Tensor, tag=None) -> Dict[str, float]:
    e = expected.reshape(expected.shape[0], -1)
    o = out.reshape(e.shape).to(torch.float64)
    assert bool(torch.isfinite(o).all()), (tag, "non-finite output")
    bad = (o - e).abs() > tolerance(e)
    if bool(bad.any()):
        r, c = (int(i) for i in torch.nonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} elements off the visible mean, first at query {r} element {c}: "
                             f"{float(o[r, c])!r} vs {float(e[r, c])!r} (tolerance {float(tolerance(e[r, c]))!r}); {residual(out, expected)}")
    return residual(out, expected)


def power_check(v_buf: torch.Tensor, paths: Sequence[Sequence[int]], queries: Iterable[int] = (0,), need: float = 4.0) -> float:
    """Without a kernel: for each query given, dropping or doubling one key -- the path's first (prefix) key, the one at the first
    128-slot tile boundary, the leaf's last key -- moves the visible mean by >= `need` x the tolerance in some (head, dim).  Returns
    the weakest factor over the keys tried."""
    v2 = v_buf.reshape(v_buf.shape[0], -1)
    worst = float("inf")
    for r in queries:
        p = [int(s) for s in paths[r]]
        n = len(p)
        idx = torch.as_tensor(p, dtype=torch.int64, device=v2.device)
        total = v2[idx].to(torch.float64).sum(0)
        m = total / n
        for j in sorted({0, min(128, n - 1), n - 1}):
            vj = v2[p[j]].to(torch.float64)
            for moved in ([(total - vj) / (n - 1)] if n > 1 else []) + [(total + vj) / (n + 1)]:
                f = float(((moved - m).abs() / tolerance(m)).max())
                worst = min(worst, f)
    assert worst >= need, f"the oracle cannot see one key at this size: factor {worst:.2f} < {need}"
    return worst


def antithetic_(v_buf: torch.Tensor, paths: Sequence[Sequence[int]]) -> None:
    """For very long paths (~250k keys and more, where one key moves the mean by less than 4 fp16 ulps of a mean of size ~1/sqrt(N)):
    make the V rows of every path pair up as +x / -x, so each path's mean sits at (about) 0, where the fp16 grid is fine.  Pairs are
    taken along the FIRST path; slots of other paths keep their rows."""
    p = [int(s) for s in paths[0]]
    h = len(p) // 2
    a = torch.as_tensor(p[:h], dtype=torch.int64, device=v_buf.device)
    b = torch.as_tensor(p[h : 2 * h], dtype=torch.int64, device=v_buf.device)
    v_buf[b] = -v_buf[a]


def per_query_head(expected: torch.Tensor, Hq: int, Hkv: int) -> torch.Tensor:
    """[nq, Hkv * D] (one value per KV head) -> [nq, Hq * D]: every query head of a GQA group sees its KV head's mean."""
    nq = expected.shape[0]
    D = expected.shape[1] // Hkv
    return expected.reshape(nq, Hkv, 1, D).expand(nq, Hkv, Hq // Hkv, D).reshape(nq, Hq * D)


# ---- the eager decode step, the way bench.py's Bench runs it ------------------------------------------------------------------
def eager_step(tree, pool, mode_name: str, Hq: int, Hkv: int, D: int, q, k_new, v_new, layer: int = 0):
    """One DeFTAttention step of `tree` -- a TreeCache, or a deft_amd.Forest (one operator call over all its trees, as bench.py runs
    forest_8kx8) -- in which each leaf's LAST slot takes k_new / v_new (the fused paged append), in --mode `mode_name` (flatten, node,
    node_chunk, seq).  BLOCK_CONFIG is the mode's while the metadata is built, and restored."""
    import deft_amd

    forest = isinstance(tree, deft_amd.Forest)
    assert not (forest and mode_name == "seq")
    saved = dict(deft_amd.BLOCK_CONFIG)
    try:
        deft_amd.BLOCK_CONFIG["MAX_BLOCK_LEN"] = -1
        mode = deft_amd.forward_mode_from_cli(mode_name)
        trees = tree.trees if forest else [tree]
        leaves = [lf for t in trees for lf in sorted(t.leaves.values(), key=lambda n: n.id)]
        loc = torch.tensor([lf.kv_indices[-1] for lf in leaves], dtype=torch.int32, device=pool.device)
        upd = deft_amd.KVCacheUpdater(True, pool, loc, None, False)
        if mode_name == "seq":
            lens = [len(tree.leaf_path_slots(lf)) for lf in leaves]
            positions = torch.tensor(lens, dtype=torch.int64, device=pool.device) - 1
            meta = deft_amd.InputMetadata.from_tree(tree, tree.req_to_token_pool, pool, mode, positions, upd)
        else:
            deft_amd.register_tree_metadata(tree.metadata() if forest else deft_amd.TreeMetadata.from_tree_cache(tree))
            meta = deft_amd.InputMetadata(mode, upd, pool)
        out = deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, layer)(q, k_new, v_new, meta)
        torch.cuda.synchronize()
        return out
    finally:
        deft_amd.BLOCK_CONFIG.clear()
        deft_amd.BLOCK_CONFIG.update(saved)


def operators(tree, pool, q):
    """The two tree operators (tree_attention_subtree_fwd = Flatten, tree_attention_fwd = Node) on layer 0 of `pool`, q [nq, Hq, D]:
    {"flatten": out, "node": out}, and the metadata they ran on."""
    import deft_amd

    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    kb, vb = pool.get_key_buffer(0), pool.get_value_buffer(0)
    o_flat = torch.full_like(q, float("nan"))
    deft_amd.tree_attention_subtree_fwd(q, kb, vb, o_flat, md.block_len, md.block_q, md.block_q_cnts, md.block_q_offset,
                                        md.block_bitmasks, md.block_kv, md.block_lens)
    o_node = torch.full_like(q, float("nan"))
    deft_amd.tree_attention_fwd(q, kb, vb, o_node, md.node_kv, md.node_kv_offset, md.node_kv_len, md.node_q, md.node_q_offset,
                                md.node_q_len)
    torch.cuda.synchronize()
    return {"flatten": o_flat, "node": o_node}, md


def flatten_leaders(md, pool, Hq: int, Hkv: int, D: int):
    """[(virtual query rows, tiles)] of the chunk leaders of the device-built Flatten plan of metadata `md`, in record order (one KV
    head's worth).  A chunk leaves ONE partial row per query of its rows: a query's merge list is as long as the chunks it is in."""
    from deft_amd._lib import check, lib

    mdl = [md.block_q, md.block_q_cnts, md.block_q_offset, md.block_bitmasks, md.block_kv, md.block_lens]
    NB, P = md.block_q_cnts.shape[0], md.block_q.shape[0]
    nbytes = lib.deft_flatten_plan_bytes(NB, P, Hq, Hkv)
    plan = torch.zeros(nbytes, dtype=torch.uint8, device=pool.device)
    check(lib.deft_flatten_build_plan(*[t.data_ptr() for t in mdl], NB, P, Hq, Hkv, Hq * D, D, pool.kv_data[0].stride(0), None, 0, 0,
                                      plan.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "deft_flatten_build_plan")
    torch.cuda.synchronize()
    hdr = plan[:16].view(torch.int32).cpu()
    assert int(hdr[2]) == 0, "plan error flags"
    NL = int(hdr[1])
    desc = plan[4096 : 4096 + 2048 * NL].view(-1, 2048)[:, 1536:1568].contiguous().view(torch.int32).view(-1, 8).cpu()
    return [(int(r[0]), int(r[4])) for r in desc]


def few_shot_tree(prefix: int, width: int, branch_len: int, Hkv: int, D: int, layers: int = 1, reserve: int = 0, extra: int = 256):
    """build_tree's few_shot shape under any heads; the first `reserve` pool slots are taken before the tree is grown (they are on
    no path).  Returns (tree, pool, reserved slots)."""
    from deft_amd.memory_pool import ReqToTokenPool, TokenToKVPool
    from deft_amd.tree_cache import TreeCache

    size = reserve + prefix + width * branch_len + extra
    req = ReqToTokenPool(max(width, 64) + 8, size + 8, device="cuda")
    pool = TokenToKVPool(size, torch.float16, Hkv, D, layers, device="cuda")
    reserved = pool.alloc(reserve).cpu() if reserve else torch.zeros(0, dtype=torch.int32)
    tree = TreeCache(torch.float16, Hkv, D, layers, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, prefix + 1, dtype=torch.int32))
    tree.branch(tree.root, width)
    for _ in range(branch_len):
        for leaf in list(tree.leaves.values()):
            leaf.append_token(7)
        tree.alloc()
    return tree, pool, reserved


# ---- poisoned pools ----------------------------------------------------------------------------------------------------------
def live_slots(paths: Sequence[Sequence[int]], extra: Iterable[int] = ()) -> torch.Tensor:
    s = set(int(x) for p in paths for x in p)
    s.update(int(x) for x in extra)
    return torch.tensor(sorted(s), dtype=torch.int64)


def poison_pool(pool, live: torch.Tensor, kind: str = "nan") -> int:
    """Every pool row that is NOT in `live` -- K and V, every layer -- := NaN ("nan") or K = +Inf, V = -Inf ("inf").  Data only: no
    index of any table changes.  Returns the number of poisoned slots."""
    st = pool._storage  # [layers, size, 2, Hkv, D]
    size = st.shape[1]
    keep = torch.zeros(size, dtype=torch.bool)
    live = live.cpu()
    assert live.numel() == 0 or (int(live.min()) >= 0 and int(live.max()) < size)
    keep[live] = True
    idx = torch.nonzero(~keep).squeeze(1).to(st.device)
    if idx.numel():
        if kind == "nan":
            st.index_fill_(1, idx, float("nan"))
        else:
            assert kind == "inf", kind
            st[:, idx, 0] = float("inf")
            st[:, idx, 1] = float("-inf")
    return int(idx.numel())


# ---- shaped scores -----------------------------------------------------------------------------------------------------------
def shaped_inputs(k_buf: torch.Tensor, q: torch.Tensor, a: torch.Tensor, b: torch.Tensor, generator: torch.Generator,
                  noise: float = 2.0 ** -6) -> None:
    """K[slot, h] = a[slot, h] e0 + noise on dims 1.. ; Q[r, g] = b[g] e0 (rows r, query heads g) + noise on dims 1.. .  With D = len
    of a head, score = a b / sqrt(D) + O(noise^2 D): the shape a test chooses.  k_buf [pool, Hkv, D], q [nq, Hq, D], fp16; a fp64
    [pool, Hkv], b fp64 [Hq].  `a` and `b` are rounded to fp16 where they land (the truth reads the tensors, not these)."""
    D = k_buf.shape[-1]
    dyadic_(k_buf, generator)
    k_buf.mul_(noise)
    k_buf[:, :, 0] = a.to(device=k_buf.device, dtype=k_buf.dtype)
    dyadic_(q, generator)
    q.mul_(noise)
    q[:, :, 0] = b.to(device=q.device, dtype=q.dtype)[None, :]
    assert D == q.shape[-1]


def running_max_rises_in(scores_along_path: torch.Tensor, lo: int, hi: int) -> bool:
    """Does the running maximum of `scores_along_path` (fp64, path order) rise somewhere in [lo, hi) -- i.e. does a kernel that walks
    the path in that order HAVE to rescale inside that tile?"""
    s = scores_along_path
    before = float(s[:lo].max()) if lo > 0 else float("-inf")
    return float(s[lo:hi].max()) > before
