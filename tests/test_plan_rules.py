"""The plan's launch-shape rules that round 6 added, pinned on the shapes they were measured on (profiles/r6_chunk_sweep_short.txt,
profiles/r6_union_len_sweep.txt): what the chunk leaders of a device-built Flatten plan look like -- tiles per leader, by the leader's
query rows -- for the north-star tree at several branch lengths and for configs[1]'s 1k-prefix tree at short branches.  At every
pinned shape the attention itself is held against dense fp64 truth too (tests/truth.py): Flatten and Node, every leaf, every head --
a rule that forms the right shapes but folds them wrongly gives finite, plausible outputs that only truth catches."""
from collections import Counter

import pytest
import torch

import deft_amd
from deft_amd._lib import check, lib
from deft_amd.memory_pool import ReqToTokenPool, TokenToKVPool
from deft_amd.tree_cache import TreeCache
from deft_amd.utils.workloads import WORKLOADS, Workload, build_tree
from truth import max_err, product_leaf_paths, tree_truth

pytestmark = pytest.mark.gpu

Hq = Hkv = 32
D = 128
TOL_EXACT = 5e-4  # (test_gpu_parity.py: fp64 truth, fp32 folds, fp16 output)


def _tree(workload, branch_len):
    w = Workload(**{**WORKLOADS[workload].__dict__, "branch_len": branch_len})
    return build_tree(w, 1, "cuda:0")


def _few_shot_tree(prefix, width, branch_len, hkv, d):
    """build_tree's few_shot shape under heads that utils/workloads.py has no model for (Qwen2-7B: 28 query heads over 4 KV heads)."""
    size = prefix + width * branch_len + 256
    req = ReqToTokenPool(max(width, 64) + 8, size + 8, device="cuda:0")
    pool = TokenToKVPool(size, torch.float16, hkv, d, 1, device="cuda:0")
    tree = TreeCache(torch.float16, hkv, d, 1, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, prefix + 1, dtype=torch.int32))
    tree.branch(tree.root, width)
    for _ in range(branch_len):
        for leaf in list(tree.leaves.values()):
            leaf.append_token(7)
        tree.alloc()
    return tree, pool


def _leaders(tree, pool, hq=Hq, hkv=Hkv, d=D, md=None):
    """[(virtual query rows, tiles)] of the chunk leaders of `tree`'s device-built Flatten plan (one KV head's worth)."""
    md = deft_amd.TreeMetadata.from_tree_cache(tree) if md is None else md
    mdl = [md.block_q, md.block_q_cnts, md.block_q_offset, md.block_bitmasks, md.block_kv, md.block_lens]
    NB, P = md.block_q_cnts.shape[0], md.block_q.shape[0]
    nbytes = lib.deft_flatten_plan_bytes(NB, P, hq, hkv)
    plan = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    check(lib.deft_flatten_build_plan(*[t.data_ptr() for t in mdl], NB, P, hq, hkv, hq * d, d, pool.kv_data[0].stride(0), None, 0, 0,
                                      plan.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "deft_flatten_build_plan")
    torch.cuda.synchronize()
    hdr = plan[:16].view(torch.int32).cpu().numpy()
    assert int(hdr[2]) == 0, "plan error flags"
    NL = int(hdr[1])
    desc = plan[4096 : 4096 + 2048 * NL].view(-1, 2048)[:, 1536:1568].contiguous().view(torch.int32).view(-1, 8).cpu().numpy()
    assert int(desc[:, 4].sum()) == NB  # every block is a tile of exactly one leader's chunk
    return [(int(r[0]), int(r[4])) for r in desc]


def _check_against_truth(tree, pool, hq=Hq, hkv=Hkv, d=D, seed=0):
    """Seeded randn pool and queries; Flatten and Node outputs against fp64 truth over every leaf and head."""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    pool._storage.normal_(generator=g)
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    nq = md.query_num
    q = torch.randn((nq, hq, d), dtype=torch.float16, device="cuda:0", generator=g)
    kb, vb = pool.get_key_buffer(0), pool.get_value_buffer(0)
    o_flat = torch.full_like(q, float("nan"))
    deft_amd.tree_attention_subtree_fwd(q, kb, vb, o_flat, md.block_len, md.block_q, md.block_q_cnts, md.block_q_offset,
                                        md.block_bitmasks, md.block_kv, md.block_lens)
    o_node = torch.full_like(q, float("nan"))
    deft_amd.tree_attention_fwd(q, kb, vb, o_node, md.node_kv, md.node_kv_offset, md.node_kv_len, md.node_q, md.node_q_offset,
                                md.node_q_len)
    truth = tree_truth(q, kb, vb, product_leaf_paths(tree), hq, hkv, d ** -0.5)
    e_flat, e_node = max_err(o_flat, truth), max_err(o_node, truth)
    assert e_flat < TOL_EXACT and e_node < TOL_EXACT, (e_flat, e_node)
    return md


def test_prefix_chunks_of_the_north_star_tree_by_branch_length():
    """A 4096-token prefix under 32 branches (MHA): 8-tile chunks at 200 tokens per branch; while the prefix dominates the tree (short
    branches) it is cut into 7 or 6 chunks per KV head instead of 4."""
    for bl, chunks in ((200, 4), (50, 6), (10, 7)):
        tree, pool = _tree("northstar_4kx32", bl)
        lead = _leaders(tree, pool)
        prefix = [t for rows, t in lead if rows == 32 and t >= 3]
        assert sum(prefix) == 32 and len(prefix) == chunks, (bl, prefix)
        _check_against_truth(tree, pool, seed=bl)


def test_leaf_blocks_in_threes_or_fours_by_list_scheduling():
    """Large MHA launch: leaf blocks go in groups of three -- and of four where threes would finish before the prefix's chunks do
    (~205-270 tokens per branch on this tree: 254 tokens 41.4 -> 37.9 us per layer)."""
    for bl, length in ((150, 3), (200, 3), (230, 4), (254, 4), (300, 3), (400, 3)):
        tree, pool = _tree("northstar_4kx32", bl)
        lead = _leaders(tree, pool)
        groups = Counter(t for rows, t in lead if rows < 32)
        other = 7 - length
        assert groups[length] >= (32 * bl // 128) // length - 1 and groups[other] == 0, (bl, dict(groups))
        _check_against_truth(tree, pool, seed=bl)


def test_leaf_groups_across_both_edges_of_the_fours_band_against_truth():
    """Every 8 tokens from 198 to 278 per branch: the band in which leaf blocks go in fours opens and closes inside the sweep, and the
    attention is truth at every step of it."""
    seen = set()
    for bl in range(198, 279, 8):
        tree, pool = _tree("northstar_4kx32", bl)
        groups = Counter(t for rows, t in _leaders(tree, pool) if rows < 32)
        seen.add(4 if groups[4] else 3 if groups[3] else 0)
        _check_against_truth(tree, pool, seed=bl)
    assert seen == {3, 4}, seen


def test_a_short_prefix_under_single_tile_branches_is_cut_into_two_tile_chunks():
    """configs[1]'s tree (1024-token prefix x 32 branches) at 50 tokens per branch: four 2-tile chunks of the prefix (its 4-tile chain was the
    launch's critical path); at 200 tokens per branch -- more than four times the prefix's tiles beside it -- 4-tile chunks again."""
    (ts, ps), (tl, pl) = _tree("fewshot_1kx32", 50), _tree("fewshot_1kx32", 200)
    short = [t for rows, t in _leaders(ts, ps) if rows == 32]
    long_ = [t for rows, t in _leaders(tl, pl) if rows == 32]
    assert short == [2, 2, 2, 2] and long_ == [4, 4], (short, long_)
    _check_against_truth(ts, ps, seed=50)
    _check_against_truth(tl, pl, seed=200)


@pytest.mark.parametrize("prefix,width,branch_len", [(4096, 32, 200), (8192, 8, 64)])
def test_group_of_seven_query_heads_against_truth(prefix, width, branch_len):
    """Qwen2-7B heads (28 query heads over 4 KV heads, G = 7): a query's seven rows straddle 32-row passes (query 4 of a chunk is
    virtual rows 28..34: four in the first pass, three in the second) -- the north-star tree and the 8192 x 8 x 64 tree, Flatten and Node."""
    tree, pool = _few_shot_tree(prefix, width, branch_len, 4, 128)
    _check_against_truth(tree, pool, 28, 4, 128, seed=prefix + branch_len)
