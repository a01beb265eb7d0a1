"""Scores of a chosen SHAPE (tests/oracles.py shaped_inputs: K[slot, h] = a(slot, h) e0, Q[r, g] = b(g) e0, small dyadic noise
elsewhere), so that the data-dependent branches of the kernels fire where a test says: the running-max rescale of stage 1 (per head of
a D = 64 head pair), of prefill and of the merge (partial LSEs tens of nats apart).  With N(0,1) logits the running max settles in the
first tiles and those branches are all but dead.

  sink   the prompt's first token ~25 nats above every other key (the max never moves after the first key)
  ramp   the score rises with depth along the path: the max jumps in every tile, the final max is the leaf's last token
  spike  the max jumps at one prefix tile and at one leaf's last token (a partial ~15-20 nats above the rest)
  mixed  different patterns on different KV heads (the two heads of a D = 64 pair among them) and a sign flip on every other query
         head of a GQA group (its ramp descends: the max is the first key)

Against dense fp64 truth (tests/truth.py) with the prefill rule: 5e-4 + 2^-11 |truth|."""
import math

import numpy as np
import pytest
import torch

import deft_amd
import oracles
from truth import product_leaf_paths, tree_truth

pytestmark = pytest.mark.gpu

B = 4.0
PATTERNS = ["sink", "ramp", "spike", "mixed"]
GEOMS = [(4, 4, 128), (8, 2, 128), (4, 4, 64), (8, 8, 32)]


def _close(out, truth, tag):
    t = truth.reshape(truth.shape[0], -1)
    o = out.reshape(t.shape).to(torch.float64)
    err = (o - t).abs()
    assert bool(torch.isfinite(o).all()) and bool((err <= 5e-4 + 2.0 ** -11 * t.abs()).all()), (tag, float(err.max()))


def _depths(paths, size):
    d = torch.zeros(size, dtype=torch.float64)
    for p in paths:
        d[torch.as_tensor(p)] = torch.arange(len(p), dtype=torch.float64)
    return d


def _prefix_chunk_ends(md, pool, Hq, Hkv, D, nq):
    """Tile index (along the prefix) of the LAST tile of every prefix chunk of the Flatten plan: the prefix's chunks are the leaders
    whose rows hold every query (one partial row per query each), in prefix order."""
    G = Hq // Hkv
    lead = oracles.flatten_leaders(md, pool, Hq, Hkv, D)
    tiles = [t for rows, t in lead if rows == min(32, nq * G)]
    return [int(x) - 1 for x in np.cumsum(tiles)]


def _shape(pattern, paths, size, Hkv, Hq, D, spike_tile=5):
    """a [size, Hkv] and b [Hq] of the pattern (score = a b / sqrt(D)).  The spike: 15 nats at key 3 of tile `spike_tile` of path 0
    (a prefix tile), 20 nats at the last key of path 3."""
    depth = _depths(paths, size)
    k = math.sqrt(D) / B  # a = nats * k
    top = max(len(p) for p in paths)
    ramp = depth * (20.0 / top) * k
    sink = torch.zeros(size, dtype=torch.float64)
    sink[paths[0][0]] = 25.0 * k
    spike = torch.zeros(size, dtype=torch.float64)
    spike[paths[0][spike_tile * 128 + 3]] = 15.0 * k
    spike[paths[3][-1]] = 20.0 * k
    cols = {"sink": sink, "ramp": ramp, "spike": spike}
    b = torch.full((Hq,), B, dtype=torch.float64)
    if pattern != "mixed":
        return cols[pattern][:, None].expand(size, Hkv).clone(), b
    # KV head h: sink, ramp, spike, ... -- the two heads of a D = 64 pair differ, the pair's SECOND head ramps; with GQA the odd query
    # heads of every group see the scores negated (a descending ramp: their max is the first key)
    a = torch.stack([cols[MIXED[h % 3]] for h in range(Hkv)], 1)
    G = Hq // Hkv
    if G > 1:
        b[torch.arange(Hq) % G % 2 == 1] = -B
    return a, b


MIXED = ("sink", "ramp", "spike")


def _scores(k_buf, q, path, r, h, g_head, D):
    return (k_buf[torch.as_tensor(path), h, 0].double() * float(q[r, g_head, 0]) / math.sqrt(D)).cpu()


def _assert_branch_taken(pattern, k_buf, q, paths, D, Hq, Hkv, spike_tile=5):
    """From the inputs alone, for EVERY query and every KV head that carries the pattern (query head 0 of its group): the running max
    rises where the pattern says -- so a kernel that walks the path must rescale there."""
    G = Hq // Hkv
    for h in range(Hkv):
        pat = MIXED[h % 3] if pattern == "mixed" else pattern
        for r, p in enumerate(paths):
            s, n = _scores(k_buf, q, p, r, h, h * G, D), len(p)
            if pat == "ramp":
                assert oracles.running_max_rises_in(s, n - 1, n) and oracles.running_max_rises_in(s, 3 * 128, 4 * 128), (pattern, h, r)
            elif pat == "sink":
                assert float(s[0]) > float(s[1:].max()) + 20, (pattern, h, r)
            else:
                assert oracles.running_max_rises_in(s, spike_tile * 128, (spike_tile + 1) * 128), (pattern, h, r)
                if r == 3:
                    assert oracles.running_max_rises_in(s, n - 1, n), (pattern, h, r)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_shaped_scores_through_flatten_and_node(geom):
    """A 1000-token prefix under 8 two-tile branches; the spike sits in the LAST tile of the prefix's first chunk, and the leaf-3 spike
    in its last token -- which the fused append of an eager DeFTAttention step supplies as the step's new row."""
    Hq, Hkv, D = geom
    tree, pool, _ = oracles.few_shot_tree(1000, 8, 150, Hkv, D)
    paths = product_leaf_paths(tree)
    nq = len(paths)
    kb, vb = pool.get_key_buffer(0), pool.get_value_buffer(0)
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    tile = _prefix_chunk_ends(md, pool, Hq, Hkv, D, nq)[0]
    assert (tile + 1) * 128 <= 1000
    loc = torch.tensor([p[-1] for p in paths], dtype=torch.int64, device="cuda")
    for pattern in PATTERNS:
        g = torch.Generator(device="cuda").manual_seed(D + Hq)
        oracles.dyadic_(vb, g)
        q = torch.empty((nq, Hq, D), dtype=torch.float16, device="cuda")
        a, b = _shape(pattern, paths, kb.shape[0], Hkv, Hq, D, tile)
        oracles.shaped_inputs(kb, q, a, b, g)
        _assert_branch_taken(pattern, kb, q, paths, D, Hq, Hkv, tile)
        truth = tree_truth(q, kb, vb, paths, Hq, Hkv, D ** -0.5)
        outs, _ = oracles.operators(tree, pool, q)
        for mode, out in outs.items():
            _close(out, truth, (geom, pattern, mode))
        k_new, v_new = kb[loc].reshape(nq, -1).clone(), vb[loc].reshape(nq, -1).clone()  # (the append rewrites the same rows)
        out = oracles.eager_step(tree, pool, "flatten", Hq, Hkv, D, q.reshape(nq, -1), k_new, v_new)
        _close(out, truth, (geom, pattern, "fused append"))


@pytest.mark.parametrize("shape", [(8, 2, 32768, 8), (4, 2, 100_000, 48)], ids=["32kx8-coop", "100kx48-scan"])
def test_shaped_scores_through_long_merge_lists(shape):
    """Long merge row lists with partial LSEs tens of nats apart: a 32k prefix under 8 queries at D = 128 (merge_coop_kernel: its four
    waves each fold a quarter of a query's list, then combine) with a sink in one prefix chunk and a spike in the last tile of another,
    and the 100k x 48 shape whose partial rows exceed the per-query lists (the merge scans row_q, several passes)."""
    Hq, Hkv, prefix, width = shape
    D = 128
    tree, pool, _ = oracles.few_shot_tree(prefix, width, 3, Hkv, D)
    paths = product_leaf_paths(tree)
    nq = len(paths)
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    if nq <= 16:
        ends = _prefix_chunk_ends(md, pool, Hq, Hkv, D, nq)
        assert len(ends) > 8, ends  # (every query has more than 8 partial rows: the four-wave path, not the single-wave fallback)
        c_sink, c_spike = len(ends) // 3, (2 * len(ends)) // 3
        sink_tile, spike_tile = ends[c_sink - 1] + 1, ends[c_spike]  # (the first tile of one chunk, the last tile of another)
    else:
        assert md.block_q.shape[0] > 15 * 1024  # (beyond QROWS_MAX: no per-query lists, the merge scans)
        sink_tile, spike_tile = 100, 500
    assert 0 < sink_tile < spike_tile < prefix // 128
    kb, vb = pool.get_key_buffer(0), pool.get_value_buffer(0)
    g = torch.Generator(device="cuda").manual_seed(prefix)
    oracles.dyadic_(vb, g)
    q = torch.empty((nq, Hq, D), dtype=torch.float16, device="cuda")
    kk = math.sqrt(D) / B
    a = torch.zeros((kb.shape[0], Hkv), dtype=torch.float64)
    a[paths[0][sink_tile * 128 + 7], 0] = 25.0 * kk  # KV head 0: a sink inside one chunk
    a[paths[0][spike_tile * 128 + 100], :] = 18.0 * kk  # every head: a spike in another
    a[paths[1][-1], -1] = 30.0 * kk  # the last KV head: query 1's own last token above everything
    oracles.shaped_inputs(kb, q, a, torch.full((Hq,), B, dtype=torch.float64), g)
    s0 = _scores(kb, q, paths[0], 0, 0, 0, D)
    assert oracles.running_max_rises_in(s0, sink_tile * 128, (sink_tile + 1) * 128)
    assert float(s0.max()) - float(s0[: sink_tile * 128].max()) > 20  # (partial LSEs tens of nats apart)
    truth = tree_truth(q, kb, vb, paths, Hq, Hkv, D ** -0.5)
    outs, _ = oracles.operators(tree, pool, q)
    for mode, out in outs.items():
        _close(out, truth, (shape, mode))


@pytest.mark.parametrize("pattern", ["sink", "ramp", "spike"])
def test_shaped_scores_through_prefill(pattern):
    Hq, Hkv, D = 8, 2, 128
    lens = [257, 1500]
    T = sum(lens)
    g = torch.Generator(device="cuda").manual_seed(len(pattern))
    v = oracles.dyadic_(torch.empty((T, Hkv, D), dtype=torch.float16, device="cuda"), g)
    k = torch.empty((T, Hkv, D), dtype=torch.float16, device="cuda")
    q = torch.empty((T, Hq, D), dtype=torch.float16, device="cuda")
    paths = [list(range(0, lens[0])), list(range(lens[0], T))]
    a, b = _shape(pattern, [paths[1], paths[0], paths[0], paths[1]], T, Hkv, Hq, D)  # (the sink / spikes in the long sequence)
    oracles.shaped_inputs(k, q, a, b, g)
    _assert_branch_taken(pattern, k, q, [paths[1]] * 4, D, Hq, Hkv)  # (the last rows of the long sequence)
    start = torch.tensor([0, lens[0]], dtype=torch.int32, device="cuda")
    o = torch.full_like(q, float("nan"))
    deft_amd.context_attention_fwd(q, k, v, o, start, torch.tensor(lens, dtype=torch.int32, device="cuda"), max(lens))
    torch.cuda.synchronize()
    G = Hq // Hkv
    for s0, n in zip((0, lens[0]), lens):
        qq = q[s0 : s0 + n].double().reshape(n, Hkv, G, D)
        kk, vv = k[s0 : s0 + n].double(), v[s0 : s0 + n].double()
        s = torch.einsum("ihgd,jhd->hgij", qq, kk) / math.sqrt(D)
        s.masked_fill_(torch.ones(n, n, dtype=torch.bool, device="cuda").triu(1), float("-inf"))
        truth = torch.einsum("hgij,jhd->ihgd", torch.softmax(s, -1), vv).reshape(n, Hq, D)
        _close(o[s0 : s0 + n], truth, (pattern, n))


def test_sink_through_a_window_session():
    """The prompt's first token 25 nats above everything, through window steps (the step's own rows in overflow tiles)."""
    Hq, Hkv, D = 8, 2, 128
    tree, pool, _ = oracles.few_shot_tree(600, 6, 0, Hkv, D, extra=6 * 40 + 256)
    g = torch.Generator(device="cuda").manual_seed(25)
    kb, vb = pool.get_key_buffer(0), pool.get_value_buffer(0)
    oracles.dyadic_(vb, g)
    q = torch.empty((6, Hq, D), dtype=torch.float16, device="cuda")
    a = torch.zeros((kb.shape[0], Hkv), dtype=torch.float64)
    a[tree.root.kv_indices[0]] = 25.0 * math.sqrt(D) / B
    oracles.shaped_inputs(kb, q, a, torch.full((Hq,), B, dtype=torch.float64), g)
    k_new = (oracles.dyadic_(torch.empty((6, Hkv * D), dtype=torch.float16, device="cuda"), g) * 2.0 ** -6).half()
    v_new = oracles.dyadic_(torch.empty((6, Hkv * D), dtype=torch.float16, device="cuda"), g)
    q2 = q.reshape(6, Hq * D)
    sess = deft_amd.DecodeSession(tree, Hq, Hkv, D, 1, lambda l: (q2, k_new, v_new), mode="flatten", incremental=True)
    for s in range(30):
        for leaf in tree.leaves.values():
            leaf.append_token(7)
        out = sess.step()[0]
        torch.cuda.synchronize()
        truth = tree_truth(q2, kb, vb, product_leaf_paths(tree), Hq, Hkv, D ** -0.5)
        _close(out, truth, s)
    assert sess.step_kinds["patch"] >= 20 and sess.device_errors() == 0, sess.step_kinds
