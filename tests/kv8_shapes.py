"""Shaped scores ON THE e4m3 GRID, for the kv8 operators (tests/test_kv8_sharp.py on the GPU, tests/test_kv8_sharp_model.py without
one), and two deliberately wrong fp64 models of the kv8 kernel's softmax that prove those inputs can fail a kernel.

oracles.shaped_inputs cannot be reused: its a e0 column and its 2^-6 dyadic noise are not e4m3 values, and a linear ramp quantised to
e4m3 has plateaus.  Here dim 0 of K[slot, head] holds a chosen CODE VALUE, dims 1.. hold subnormal codes (m 2^-9, |m| <= 7: exact,
and the kernel's conversion of them is part of the product), Q is 16-bit as shaped_inputs makes it (b e0 + 2^-6 dyadic noise), V comes
from the e4m3-exact list of test_exact_visibility.  A code c of head h means c * k_scale[h], so with Q[., g, 0] = b

    score = c * k_scale[h] * b / sqrt(D)   nats  (+ ~1e-4 of noise);   NPC[h] = k_scale[h] * |b| / sqrt(D) nats per unit of code.

Everything is drawn with a CPU generator and moved afterwards: the inputs are the same tensors on either machine.

  sink       the prompt's first key >= 25 nats above every other key
  staircase  the ramp on the grid: the running max rises by 64 units of code (>= 12.9 nats at the smallest k_scale, 0.57) ONCE per 128-key
             tile of the prefix, at key 5, 37, 69, 101 of successive tiles -- inside wave 0's, 1's, 2's, 3's 32 keys in turn.  That ONE key
             leads: the other 127 keys of tile t stay on level t and tile t + 1 starts on level t + 1, so in every tile the wave that owns the
             rise has a 32-key maximum a whole step above the other three waves'.  One more step inside the leaf, and the leaf's last token
             sits one code (128 -> 144) above everything.  Levels -448, -384, ..., 128: all on the grid.
  spike      >= 15 nats at key 3 of a chosen prefix tile, >= 20 nats at leaf 3's last token
  mixed      KV head h carries MIXED[h % 3]; with GQA the odd query heads of a group have b negated: their staircase descends, the max is
             in the first tile
"""
from __future__ import annotations

import math

import torch

import kv8_model

FP8 = torch.float8_e4m3fn
B = 4.0
D = 128
PATTERNS = ["sink", "staircase", "spike", "mixed"]
MIXED = ("sink", "staircase", "spike")
RISE_AT = (5, 37, 69, 101)  # key of the rise inside prefix tile t: RISE_AT[t % 4], in wave (t % 4)'s 32 keys
STEP = 64.0
BOTTOM = -448.0
LEAF_RISE = 69
# (Hq, Hkv) -> the LAST tile of the first prefix chunk of the device-built Flatten plan of the 1000 x 8 x 150 tree: where the spike goes.
# The plan is built on the GPU; tests/test_kv8_sharp.py asserts these against it (test_sharp_softmax's _prefix_chunk_ends).
SPIKE_TILE = {(4, 4): 0, (8, 2): 0, (3, 3): 0}  # (this tree's prefix goes one tile per chunk; the 32k x 8 case has the long chunks)
V_VALUES = [0, 0.25, -0.25, 0.5, -0.5, 1, -1, 1.5, -1.5, 2, -2, 3, -3]  # exact in e4m3 (tests/test_kv8_gpu.py test_exact_visibility)


def nats_per_code(k_scales) -> list:
    return [float(s) * B / math.sqrt(D) for s in k_scales]


def grid_at_least(x: float) -> float:
    """The smallest positive e4m3 value >= x."""
    vals = kv8_model.code_values()[:127]
    return float(vals[vals >= x].min())


def cpu_few_shot_tree(prefix: int, width: int, branch_len: int, Hkv: int, device: str = "cpu"):
    """oracles.few_shot_tree on any device (the same slots: the allocator does not depend on the device).  (tree, paths, pool size)."""
    import deft_amd
    from truth import product_leaf_paths

    size = prefix + width * branch_len + 256
    req = deft_amd.ReqToTokenPool(max(width, 64) + 8, size + 8, device=device)
    pool = deft_amd.TokenToKVPool(size, torch.float16, Hkv, D, 1, device=device)
    tree = deft_amd.TreeCache(torch.float16, Hkv, D, 1, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, prefix + 1, dtype=torch.int32))
    tree.branch(tree.root, width)
    for _ in range(branch_len):
        for leaf in list(tree.leaves.values()):
            leaf.append_token(7)
        tree.alloc()
    return tree, product_leaf_paths(tree), size


def depths(paths, size: int) -> torch.Tensor:
    d = torch.full((size,), -1, dtype=torch.int64)
    for p in paths:
        d[torch.as_tensor(p)] = torch.arange(len(p))
    return d


def pattern_codes(pattern: str, paths, size: int, prefix: int, k_scales, spike_tile: int):
    """a [size, Hkv] fp64 -- the code VALUE in dim 0 of K, every entry an e4m3 value -- and the pattern each KV head carries."""
    Hkv = len(k_scales)
    npc = nats_per_code(k_scales)
    dep = depths(paths, size)
    n = len(paths[0])
    assert all(len(p) == n for p in paths) and (spike_tile + 1) * 128 <= prefix and prefix % 128 > RISE_AT[3]
    # staircase: level index along the path (dead slots: level 0)
    t = dep.clamp_min(0) // 128
    in_prefix = dep < prefix
    rise = torch.tensor(RISE_AT)[t % 4]
    idx_prefix = t + (dep % 128 == rise).long()  # ONE key leads: the rest of tile t stays on level t, tile t + 1 starts on level t + 1
    top_prefix = (prefix - 1) // 128 + 1  # the level the prefix ends on
    idx_leaf = top_prefix + (dep - prefix >= LEAF_RISE).long()
    stair = BOTTOM + STEP * torch.where(in_prefix, idx_prefix, idx_leaf).to(torch.float64)
    top = BOTTOM + STEP * (top_prefix + 1)
    vals = kv8_model.code_values()[:127]
    last = float(vals[vals > top].min())  # one code above everything
    assert n - prefix > LEAF_RISE + 1 and top == 128.0 and last == 144.0, (top, last)
    stair[torch.tensor([p[-1] for p in paths])] = last
    stair[dep < 0] = BOTTOM
    cols, heads = [], []
    for h in range(Hkv):
        pat = MIXED[h % 3] if pattern == "mixed" else pattern
        heads.append(pat)
        if pat == "staircase":
            assert STEP * npc[h] > 10.0, (h, STEP * npc[h])  # (every step is more than 10 nats on every head)
            cols.append(stair)
            continue
        a = torch.zeros(size, dtype=torch.float64)
        if pat == "sink":
            a[paths[0][0]] = grid_at_least(25.0 / npc[h])
        else:
            a[paths[0][spike_tile * 128 + 3]] = grid_at_least(15.0 / npc[h])
            a[paths[3][-1]] = grid_at_least(20.0 / npc[h])
        cols.append(a)
    return torch.stack(cols, 1), heads


def codes_and_q(a: torch.Tensor, nq: int, Hq: int, b: torch.Tensor, qdtype, seed: int):
    """The pool layer [size, 2, Hkv, D] of e4m3 codes (K: dim 0 = a, dims 1.. subnormal noise; V from V_VALUES) and q [nq, Hq, D] of
    `qdtype` (dim 0 = b[g], dims 1.. 2^-6 dyadic noise, rounded where it lands: the truth reads the tensors).  CPU tensors."""
    size, Hkv = a.shape
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-7, 8, (size, Hkv, D), generator=g).to(torch.float64) * 2.0 ** -9
    k[:, :, 0] = a
    v = torch.tensor(V_VALUES, dtype=torch.float64)[torch.randint(0, len(V_VALUES), (size, Hkv, D), generator=g)]
    codes = torch.stack([k, v], 1).to(torch.float32).to(FP8)
    assert torch.equal(codes.to(torch.float64), torch.stack([k, v], 1)), "an input is not an e4m3 value"
    acc = torch.zeros((nq, Hq, D), dtype=torch.int32)
    for _ in range(3):
        acc += torch.randint(-512, 513, acc.shape, dtype=torch.int32, generator=g)
    q = acc.to(torch.float32) / 512.0 * 2.0 ** -6
    q[:, :, 0] = b.to(torch.float32)[None, :]
    return codes, q.to(qdtype)


def query_b(pattern: str, Hq: int, Hkv: int) -> torch.Tensor:
    b = torch.full((Hq,), B, dtype=torch.float64)
    G = Hq // Hkv
    if pattern == "mixed" and G > 1:
        b[torch.arange(Hq) % G % 2 == 1] = -B
    return b


def shaped_case(pattern: str, paths, size: int, prefix: int, Hq: int, Hkv: int, k_scales, spike_tile: int, qdtype, seed: int = 0):
    """(codes, q, pattern per KV head) of one pattern -- CPU tensors."""
    a, heads = pattern_codes(pattern, paths, size, prefix, k_scales, spike_tile)
    codes, q = codes_and_q(a, len(paths), Hq, query_b(pattern, Hq, Hkv), qdtype, seed + Hq + PATTERNS.index(pattern))
    return codes, q, heads


# ---- what the inputs do to a kernel that walks the path, from the inputs alone ----------------------------------------------------------
def path_scores(q, k64, paths, Hq: int, Hkv: int) -> torch.Tensor:
    """fp64 scores [nq, Hq, n] in nats along every query's path (k64: the DEQUANTISED K, [size, Hkv, D]); all paths one length."""
    nq, n = len(paths), len(paths[0])
    idx = torch.as_tensor(paths, dtype=torch.int64, device=k64.device)  # [nq, n]
    k = k64[idx]  # [nq, n, Hkv, D]
    qq = q.to(device=k64.device, dtype=torch.float64).reshape(nq, Hkv, Hq // Hkv, D)
    return torch.einsum("rhgd,rnhd->rhgn", qq, k).reshape(nq, Hq, n) / math.sqrt(D)


def _rises_in(s: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
    """oracles.running_max_rises_in for every row of s [..., n] at once."""
    before = s[..., :lo].amax(-1) if lo > 0 else torch.full(s.shape[:-1], float("-inf"), dtype=s.dtype, device=s.device)
    return s[..., lo:hi].amax(-1) > before


def assert_branch_taken(pattern: str, heads, s: torch.Tensor, prefix: int, Hq: int, Hkv: int, spike_tile: int) -> float:
    """For EVERY query and every KV head (query head 0 of its group; and the negated heads of a mixed GQA group), from the scores alone:
    the running max rises where the pattern says.  For a staircase head additionally: in every full prefix tile the four waves' 32-key
    maxima differ by more than 10 nats, the rise falling in wave (tile % 4) -- so each of the four wave ranges has at least one such
    tile.  Returns the smallest such difference (nats), inf without a staircase head."""
    G = Hq // Hkv
    nq, _, n = s.shape
    smallest = float("inf")
    for h, pat in enumerate(heads):
        sh = s[:, h * G]  # [nq, n]
        if pat == "sink":
            assert bool((sh[:, 0] > sh[:, 1:].amax(-1) + 20).all()), (pattern, h)
        elif pat == "spike":
            assert bool(_rises_in(sh, spike_tile * 128, (spike_tile + 1) * 128).all()), (pattern, h)
            assert bool(_rises_in(sh[:, : spike_tile * 128 + 4], spike_tile * 128 + 3, spike_tile * 128 + 4).all()), (pattern, h)  # at key 3
            assert bool(_rises_in(sh[3:4], n - 1, n).all()), (pattern, h)
            assert float((sh[:, spike_tile * 128 + 3] - sh[:, : spike_tile * 128 + 3].amax(-1)).min()) > 14.9, (pattern, h)
        else:
            seen = set()
            for t in range(prefix // 128 + 1):
                lo, hi = 128 * t, min(128 * t + 128, prefix)
                assert bool(_rises_in(sh, lo, hi).all()), (pattern, h, t)
                at = lo + RISE_AT[t % 4]
                assert bool(_rises_in(sh[:, : at + 1], at, at + 1).all()), (pattern, h, t)  # (at that key, by a whole step)
                assert float((sh[:, at] - sh[:, :at].amax(-1)).min()) > 10.0, (pattern, h, t)
                if hi - lo == 128:
                    wm = sh[:, lo:hi].reshape(nq, 4, 32).amax(-1)  # the four waves' maxima
                    diff = float((wm.amax(-1) - wm.amin(-1)).min())
                    assert diff > 10.0, (pattern, h, t, diff)
                    smallest = min(smallest, diff)
                    seen.add(t % 4)
            assert seen == {0, 1, 2, 3}, seen
            assert bool(_rises_in(sh, n - 1, n).all()), (pattern, h)
            for j in range(1, G, 2):  # a negated head (mixed, GQA): the staircase descends, the first tile holds the max
                sn = s[:, h * G + j]
                if float(sn[0, 0]) > 0:
                    assert float((sn[:, 0] - sn[:, 128:].amax(-1)).min()) > 10.0 and float(sn[0, 0] - sn[0, RISE_AT[0]]) > 10.0, (pattern, h, j)
    return smallest


# ---- fp64 models of the kernel's softmax: the right one and two wrong ones ---------------------------------------------------------------
def _tiles(s, v64, paths, Hq, Hkv):
    """Scores and V rows along the paths cut into 128-key tiles of four 32-key wave slices (path order; the tail padded with -inf
    scores and zero rows): s [nq, Hq, T, 4, 32], v [nq, Hq, T, 4, 32, D]."""
    nq, _, n = s.shape
    T = (n + 127) // 128
    pad = T * 128 - n
    sp = torch.cat([s, torch.full((nq, Hq, pad), float("-inf"), dtype=s.dtype)], -1).reshape(nq, Hq, T, 4, 32)
    idx = torch.as_tensor(paths, dtype=torch.int64)
    v = v64[idx]  # [nq, n, Hkv, D]
    v = torch.cat([v, torch.zeros((nq, pad, Hkv, D), dtype=v.dtype)], 1)
    v = v.permute(0, 2, 1, 3).repeat_interleave(Hq // Hkv, dim=1).reshape(nq, Hq, T, 4, 32, D)
    return sp, v


def model_outputs(s, v64, paths, Hq: int, Hkv: int) -> dict:
    """{"right", "no_alpha", "no_wave_factors"}: fp64 [nq, Hq, D] each.

      right            per tile, per wave slice (m_w, l_w, O_w); a tile's four combined with exp(m_w - M); the tiles combined by the online
                       recurrence O <- alpha O + O_t.  Equals the dense truth to rounding (the caller asserts it): what is wrong below is the
                       one omission, nothing else.
      no_alpha         the same, but the running O is NOT multiplied by alpha = exp(m_old - m_new) when a tile raises the max (l is).
      no_wave_factors  the same, but a tile's four (l_w, O_w) are summed WITHOUT exp(m_w - M).

    The tiling is the path's own (the kernel's tiles of a leaf follow the plan; the prefix tiles are these): a model of the arithmetic,
    enough to show that the inputs separate right from wrong at the tolerance."""
    sp, v = _tiles(s, v64, paths, Hq, Hkv)
    T = sp.shape[2]
    mw = sp.amax(-1)  # [nq, Hq, T, 4]
    safe = torch.where(torch.isinf(mw), torch.zeros_like(mw), mw)
    p = torch.exp(sp - safe[..., None])  # padded keys: exp(-inf) = 0
    lw = p.sum(-1)
    ow = torch.einsum("rgtwk,rgtwkd->rgtwd", p, v)
    M = mw.amax(-1)  # [nq, Hq, T] (every tile holds a live key)
    out = {}
    for name in ("right", "no_alpha", "no_wave_factors"):
        f = torch.ones_like(mw) if name == "no_wave_factors" else torch.exp(mw - M[..., None])
        f = torch.where(torch.isinf(mw), torch.zeros_like(f), f)
        Lt = (f * lw).sum(-1)
        Ot = (f[..., None] * ow).sum(-2)  # [nq, Hq, T, D]
        m = torch.full(M.shape[:2], float("-inf"), dtype=torch.float64)
        l = torch.zeros_like(m)
        o = torch.zeros(M.shape[:2] + (D,), dtype=torch.float64)
        for t in range(T):
            m_new = torch.maximum(m, M[:, :, t])
            alpha = torch.exp(m - m_new)  # exp(-inf) = 0 at t = 0
            beta = torch.exp(M[:, :, t] - m_new)
            l = l * alpha + beta * Lt[:, :, t]
            o = (o if name == "no_alpha" else o * alpha[..., None]) + beta[..., None] * Ot[:, :, t]
            m = m_new
        out[name] = o / l[..., None]
    return out
