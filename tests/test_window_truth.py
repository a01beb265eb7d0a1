"""Window plans (csrc/window.h, csrc/window_host.cpp: what DecodeSession(incremental=True) runs by default -- bench.py, tools/replay.py,
TemplateReplay) at full size: the north-star tree (4096-token prefix x 32 branches, Llama-2-7B heads) and configs[1]'s 1k-prefix tree,
through replans, while the plan rules switch under them (leaf groups of three / four, the 7 -> 6 chunk prefix cut, the short prefix's
two-tile chunks).  Every step: the session against the eager path (test_session._agree), both against dense fp64 truth over every
leaf and head (tests/truth.py), pools and page tables bit-equal."""
from collections import Counter

import pytest
import torch

import deft_amd
from deft_amd.utils.workloads import WORKLOADS, Workload, build_tree
from test_plan_rules import _leaders
from test_session import _agree
from truth import max_err, product_leaf_paths, tree_truth

pytestmark = pytest.mark.gpu

Hq = Hkv = 32
D = 128
TOL_EXACT = 5e-4


def _run(workload, mode, start, steps, layers):
    """Decode `steps` steps from `start` tokens per branch, eagerly and through a session; returns (session, {replan step: leaf-group
    histogram of the eager Flatten plan}, {replan step: its 32-row leaders' tiles})."""
    w = Workload(**{**WORKLOADS[workload].__dict__, "branch_len": start})
    g = torch.Generator(device="cuda").manual_seed(start * 7 + steps)
    (te, pe), (ts, ps) = [build_tree(w, layers, "cuda", extra_slots=w.width * steps + 256) for _ in range(2)]
    pe._storage.normal_(generator=g)
    ps._storage.copy_(pe._storage)
    width = w.width
    q = torch.randn((layers, width, Hq * D), dtype=torch.float16, device="cuda", generator=g)
    k = torch.randn((layers, width, Hkv * D), dtype=torch.float16, device="cuda", generator=g)
    v = torch.randn((layers, width, Hkv * D), dtype=torch.float16, device="cuda", generator=g)
    sess = deft_amd.DecodeSession(ts, Hq, Hkv, D, layers, lambda l: (q[l], k[l], v[l]), mode=mode, incremental=True)
    attn = [deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, l) for l in range(layers)]
    fmode = deft_amd.forward_mode_from_cli(mode)
    at_replans, prefix_chunks = {}, {}
    for s in range(steps):
        for tree in (te, ts):
            for leaf in tree.leaves.values():
                leaf.append_token(7)
        upd = te.alloc()
        md = deft_amd.TreeMetadata.from_tree_cache(te)
        deft_amd.register_tree_metadata(md)
        meta = deft_amd.InputMetadata(fmode, upd, pe)
        ref = [attn[l](q[l], k[l], v[l], meta) for l in range(layers)]
        replans = sess.step_kinds["replan"]
        out = sess.step()
        torch.cuda.synchronize()
        paths = product_leaf_paths(te)
        for l in range(layers):
            _agree(out[l], ref[l], True, (s, l))
            truth = tree_truth(q[l], pe.get_key_buffer(l), pe.get_value_buffer(l), paths, Hq, Hkv, D ** -0.5)  # (the step's rows are in)
            e_sess, e_eager = max_err(out[l], truth), max_err(ref[l], truth)
            assert e_sess < TOL_EXACT and e_eager < TOL_EXACT, (s, l, e_sess, e_eager)
        assert torch.equal(pe._storage, ps._storage)
        assert torch.equal(te.req_to_token_pool.req_to_token, ts.req_to_token_pool.req_to_token)
        if sess.step_kinds["replan"] > replans:
            lead = _leaders(te, pe, md=md)
            at_replans[s] = Counter(t for rows, t in lead if rows < 32)
            prefix_chunks[s] = [t for rows, t in lead if rows == 32]
    assert sess.device_errors() == 0
    kinds = sess.step_kinds
    assert kinds["replan"] >= 2 and kinds["patch"] >= steps // 2 and kinds["legacy"] == 0, kinds
    return sess, at_replans, prefix_chunks


@pytest.mark.parametrize("mode", ["flatten", "node"])
def test_north_star_window_steps_through_leaf_groups_of_three_and_four(mode):
    """195 -> 305 tokens per branch: the eager plan's leaf blocks go in threes, then fours (~205-270), then threes again, and the window
    plan is replanned several times on the way."""
    _, at_replans, _ = _run("northstar_4kx32", mode, 195, 110, 1)
    fours = [s for s, gr in at_replans.items() if gr[4]]
    threes = [s for s, gr in at_replans.items() if gr[3] and not gr[4]]
    assert fours and threes and min(threes) < min(fours) < max(threes), at_replans


def test_north_star_window_steps_across_the_prefix_chunk_cut():
    """1 -> 61 tokens per branch: the prefix is cut into 7 chunks per KV head, then 6 (two layers: one plan serves both)."""
    _, _, chunks = _run("northstar_4kx32", "flatten", 1, 60, 2)
    # (test_plan_rules' filter: the prefix's chunks hold 3 tiles or more; at the first steps a 32-row leaf tile -- every leaf's few
    # tokens in one block -- may join one of them)
    counts = {len([t for t in c if t >= 3]) for c in chunks.values()}
    assert {6, 7} <= counts, chunks


def test_short_prefix_window_steps_with_two_tile_chunks():
    """configs[1]'s 1024-token prefix x 32 branches from 1 token per branch: the prefix in 2-tile chunks."""
    _, _, chunks = _run("fewshot_1kx32", "flatten", 1, 60, 1)
    assert [2, 2, 2, 2] in chunks.values(), chunks
