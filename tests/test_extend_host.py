"""Extend steps, host side: `TreeCache.alloc_extend` / `commit_extend` bookkeeping on a CPU pool against `extend_leaf`, the
refusals, the size query of the C ABI and the agreement of header, export list and library for the new entry points."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import deft_amd
from deft_amd._lib import EXPORTED, LIB_PATH
from extend_model import draft_tree_parents

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("deft_tree_extend_sizes", "deft_extend_scratch_bytes", "deft_extend_dev_build")


def _tree(width=3, private=(5, 130, 0), size=4096):
    req = deft_amd.ReqToTokenPool(64, 2048, device="cpu")
    pool = deft_amd.TokenToKVPool(size, torch.float16, 2, 16, 1, device="cpu")
    tree = deft_amd.TreeCache(torch.float16, 2, 16, 1, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, 201, dtype=torch.int32))
    kids = tree.branch(tree.root, width)
    for kid, n in zip(kids, private):
        if n:
            tree.extend_leaf(kid, torch.arange(100, 100 + n, dtype=torch.int32))
    return tree, kids, pool, req


def _books(tree, kids, pool, req):
    return {
        "slots": [k.kv_indices.tolist() for k in kids],
        "tokens": [list(k.token_ids) for k in kids],
        "positions": [list(k.positions) for k in kids],
        "refcounts": pool.mem_state.copy(),
        "used": pool.used_size(),
        "pages": [req.req_to_token[tree.leaf_to_req[k.id], : k.position_offset + len(k.token_ids)].clone() for k in kids],
        "paths": [tree.leaf_path_slots(k) for k in kids],
    }


def test_chain_commit_equals_extend_leaf():
    toks = {0: [11, 12, 13], 2: [21, 22, 23, 24, 25, 26, 27]}  # (the middle leaf is left out of the step)
    ta, ka, pa, ra = _tree()
    step = ta.alloc_extend({ka[i]: t for i, t in toks.items()})
    assert step.num_rows == 10 and step.is_chain and not step.committed
    assert step.cache_loc.dtype == torch.int32 and step.cache_loc.tolist() == step.slots.tolist()
    assert step.row_leaf.tolist() == [ka[0].id] * 3 + [ka[2].id] * 7  # grouped by leaf, ascending id
    assert step.parents.tolist() == [-1, 0, 1, -1, 3, 4, 5, 6, 7, 8]
    assert step.positions.tolist() == [205, 206, 207] + list(range(200, 207))  # leaf length + depth
    before = _books(ta, ka, pa, ra)
    assert before["used"] == 200 + 135 + 10 and [len(s) for s in before["slots"]] == [5, 130, 0]  # slots taken, tree unchanged
    ta.commit_extend(step)
    assert step.committed
    tb, kb, pb, rb = _tree()
    for i, t in toks.items():
        tb.extend_leaf(kb[i], t)
    a, b = _books(ta, ka, pa, ra), _books(tb, kb, pb, rb)
    for key in ("slots", "tokens", "positions", "paths", "used"):
        assert a[key] == b[key], key
    assert np.array_equal(a["refcounts"], b["refcounts"])
    for x, y in zip(a["pages"], b["pages"]):
        assert torch.equal(x, y)
    with pytest.raises(RuntimeError, match="committed"):
        ta.commit_extend(step)


def test_partial_accept_frees_exactly_the_rejected_slots():
    tree, kids, pool, req = _tree()
    local = draft_tree_parents([1, 2, 4])  # [-1, 0, 0, 1, 1, 2, 2]
    step = tree.alloc_extend({kids[0]: range(7), kids[1]: range(10, 17)}, parents={kids[0]: local, kids[1]: local})
    assert not step.is_chain
    assert step.parents.tolist() == [-1, 0, 0, 1, 1, 2, 2, -1, 7, 7, 8, 8, 9, 9]
    assert step.positions.tolist() == [205, 206, 206, 207, 207, 207, 207, 330, 331, 331, 332, 332, 332, 332]
    with pytest.raises(ValueError, match="chain step"):
        tree.commit_extend(step)  # accepted=None keeps everything: chains only
    with pytest.raises(ValueError, match="not a chain"):
        tree.commit_extend(step, {kids[0]: [0, 3]})  # 3 hangs off 1, not off 0
    with pytest.raises(ValueError, match="not a chain"):
        tree.commit_extend(step, {kids[0]: [1]})  # does not start at the cached path
    used = pool.used_size()
    slots = step.slots.copy()
    tree.commit_extend(step, {kids[0]: [0, 2, 5], kids[1]: []})
    keep = slots[[0, 2, 5]]
    assert kids[0].kv_indices.tolist()[-3:] == keep.tolist() and len(kids[0].kv_indices) == 8
    assert kids[0].token_ids[-3:] == [0, 2, 5] and kids[0].positions[-3:] == [205, 206, 207]
    assert len(kids[1].kv_indices) == 130 and len(kids[1].token_ids) == 130
    assert pool.used_size() == used - 11
    rejected = np.setdiff1d(slots, keep)
    assert (pool.mem_state[rejected] == 0).all() and (pool.mem_state[keep] == 1).all()
    assert req.req_to_token[tree.leaf_to_req[kids[0].id], 205:208].tolist() == keep.tolist()
    assert tree.leaf_path_slots(kids[0])[-3:] == keep.tolist()


def test_refusals():
    tree, kids, pool, req = _tree(size=200 + 135 + 40)
    with pytest.raises(ValueError, match="not a live leaf"):
        tree.alloc_extend({tree.root: [1]})
    with pytest.raises(ValueError, match="at least one token"):
        tree.alloc_extend({})
    with pytest.raises(ValueError, match="at least one token"):
        tree.alloc_extend({kids[0]: []})
    with pytest.raises(ValueError, match="not an earlier"):
        tree.alloc_extend({kids[0]: [1, 2]}, parents={kids[0]: [-1, 1]})  # own index
    with pytest.raises(ValueError, match="not an earlier"):
        tree.alloc_extend({kids[0]: [1, 2]}, parents=[-1, 2])
    with pytest.raises(ValueError, match="another leaf"):
        tree.alloc_extend({kids[0]: [1, 2], kids[1]: [3]}, parents=[-1, 0, 1])
    with pytest.raises(ValueError, match="at most 1024"):
        tree.alloc_extend({kids[0]: range(1025)})
    used = pool.used_size()
    with pytest.raises(RuntimeError, match="free slots"):
        tree.alloc_extend({kids[0]: range(41)})  # the pool has 40 left
    assert pool.used_size() == used  # a refused step takes nothing
    step = tree.alloc_extend({kids[0]: range(40)})
    assert step.num_rows == 40 and pool.used_size() == used + 40


def _sizes(tree, row_leaf, parents, mq=32):
    lib = deft_amd.lib
    lay = np.zeros(5, dtype=np.int64)
    assert lib.deft_tree_layout(tree._native, 256, lay.ctypes.data_as(ctypes.c_void_p)) == 0
    rl, par = np.asarray(row_leaf, dtype=np.int32), np.asarray(parents, dtype=np.int32)
    out = np.zeros(9, dtype=np.int64)
    rc = lib.deft_tree_extend_sizes(tree._native, mq, 128, len(rl), rl.ctypes.data_as(ctypes.c_void_p),
                                    par.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return rc, out.tolist()


def test_size_query_counts_blocks_and_rows():
    """200-token root (two blocks, the second shared with the leaves), leaves of 5 / 130 / 0 tokens: 335 slots in three physical
    blocks with the leaf sets {0,1,2}, {0,1,2}, {1} (the third leaf holds nothing yet).  Sizes = {rows, NB, P, NB and P of the cached
    part, NB and P of the tree's own arrays, physical blocks, slots}."""
    tree, kids, _, _ = _tree()
    chain = lambda n, at: [-1] + list(range(at, at + n - 1))  # noqa: E731
    # 1 / 7 / 33 chain tokens: 41 rows cut the two shared blocks in two; block 2 lists leaf 1's 7 rows; new keys: 1 + 7 pack into one
    # block, the last leaf's 33 rows are a piece of 32 (no room beside the 8 rows) and a piece of one row with 33 keys
    rc, s = _sizes(tree, [0] + [1] * 7 + [2] * 33, chain(1, 0) + chain(7, 1) + chain(33, 8))
    assert rc == 0 and s == [41, 2 * 2 + 1 + 3, 41 * 2 + 7 + 41, 5, 89, 3, 7, 3, 335]
    # a leaf left out of the step contributes no rows; a block nobody of the step lists is dropped
    rc, s = _sizes(tree, [0, 0, 2], [-1, 0, -1])
    assert rc == 0 and s[:5] == [3, 2 + 1, 3 * 2 + 3, 2, 6]
    assert _sizes(tree, [1, 0], [-1, -1])[0] == -1  # not grouped by ascending leaf
    assert _sizes(tree, [0, 3], [-1, -1])[0] == -1  # no such query row
    assert _sizes(tree, [0, 1], [-1, 0])[0] == -1   # a parent on another leaf
    assert _sizes(tree, [0, 0], [-1, 1])[0] == -1   # a parent that is not earlier
    assert b"parent" in deft_amd.lib.deft_last_error()


def _device_needs(counts, mq):
    """What extend_new_kernel keeps in LDS for chains of `counts` tokens per leaf (csrc/extend.h): bit-set words -- one set of
    ceil(M / 64) words per piece of mq rows -- and new-key blocks by the packing rule (a chain's piece j sees its leaf's first
    min(M, (j + 1) mq) tokens)."""
    words, nb, cur_rows, cur_slots, is_open = 0, 0, 0, 0, False
    for M in counts:
        for j in range(-(-M // mq)):
            words += -(-M // 64)
            r, k = min(mq, M - j * mq), min(M, (j + 1) * mq)
            if k > 128:
                nb, is_open = nb + -(-k // 128), False
                continue
            if not (is_open and cur_rows + r <= mq and cur_slots + k <= 128):
                nb, cur_rows, cur_slots, is_open = nb + 1, 0, 0, True
            cur_rows, cur_slots = cur_rows + r, cur_slots + k
    return words, nb


@pytest.mark.parametrize("mq", [1, 2, 4, 8, 16, 32])
def test_a_step_the_size_query_accepts_fits_the_device_kernels(mq):
    """The device build reports a step it cannot hold only through an error word nobody reads without a round trip, so the HOST
    refuses every such step: acceptance by `deft_tree_extend_sizes` implies <= 2048 bit-set words and <= 1024 new-key blocks, at
    every max_q_len -- not only 32, where everything fits.  With max_q_len >= 16 every step of up to 1024 rows is accepted."""
    tree, kids, _, _ = _tree(width=16, private=())
    chain = lambda n, at: [-1] + list(range(at, at + n - 1))  # noqa: E731
    steps = [[64], [300], [512], [700], [900], [1024], [1009] + [1] * 15, [500, 524], [64] * 16, [1] * 16, [33, 200, 7]]
    seen = set()
    for counts in steps:
        rl = [leaf for leaf, M in enumerate(counts) for _ in range(M)]
        par, at = [], 0
        for M in counts:
            par += chain(M, at)
            at += M
        rc, s = _sizes(tree, rl, par, mq=mq)
        words, nb = _device_needs(counts, mq)
        fits = words <= 2048 and nb <= 1024
        assert rc == (0 if fits else -2), (counts, mq, rc, words, nb, deft_amd.lib.deft_last_error())
        if fits:
            assert s[0] == sum(counts) and s[1] - s[3] == nb  # (the host counts new-key blocks by the same rule)
        seen.add(fits)
    assert True in seen and (False in seen) == (mq <= 4), seen
    if mq == 8:  # 128 pieces x 16 words: exactly the limit; one at max_q_len 4 is far over it
        assert _device_needs([1024], 8)[0] == 2048 and _sizes(tree, [0] * 1024, chain(1024, 0), mq=8)[0] == 0
    if mq == 4:
        assert _sizes(tree, [0] * 900, chain(900, 0), mq=4)[0] == -2 and b"words" in deft_amd.lib.deft_last_error()


def test_commit_refuses_a_leaf_that_changed_before_anything_is_committed():
    tree, kids, pool, req = _tree()
    step = tree.alloc_extend({kids[0]: [1, 2], kids[2]: [3, 4, 5]})
    tree.extend_leaf(kids[2], [9])  # the LATER leaf of the step grows behind the step's back
    before = _books(tree, kids, pool, req)
    with pytest.raises(RuntimeError, match="changed between"):
        tree.commit_extend(step)
    after = _books(tree, kids, pool, req)
    assert not step.committed
    for key in ("slots", "tokens", "positions", "paths", "used"):
        assert after[key] == before[key], key  # the earlier leaf was not committed either
    tree.commit_extend(step, {kids[0]: list(step.leaf_rows[kids[0].id])})  # what still fits can be committed; the rest is freed
    assert len(kids[0].kv_indices) == 7 and pool.used_size() == before["used"] - 3


def test_device_build_refuses_bad_arguments_before_any_launch():
    lib = deft_amd.lib
    assert lib.deft_extend_scratch_bytes(3, 3) > 0 and lib.deft_extend_scratch_bytes(-1, 3) == 0
    p = ctypes.c_void_p(0x1000)  # (never dereferenced: the argument checks come first)
    args = lambda rows, mq, sb: ([p] * 6 + [3, 3, p, p, p, rows, mq, 8, 64, p, sb] + [p] * 6 + [None])  # noqa: E731
    assert lib.deft_extend_dev_build(*args(0, 32, 1 << 20)) == -1
    assert lib.deft_extend_dev_build(*args(1025, 32, 1 << 20)) == -1
    assert lib.deft_extend_dev_build(*args(5, 33, 1 << 20)) == -1
    assert lib.deft_extend_dev_build(*args(5, 32, 16)) == -4  # scratch too small
    assert b"scratch" in lib.deft_last_error()


def test_header_export_list_and_library_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "deft_amd.h")).read()
    declared = set(re.findall(r"\b(deft_[a-z0-9_]+)\s*\(", header))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_ENTRY_POINTS:
        assert name in declared and name in defined and name in EXPORTED, name
    assert deft_amd.lib.deft_abi_version() == 2  # additive: the version stays
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_ENTRY_POINTS:
        assert name in table, name


def test_extend_is_a_forward_mode_of_the_module_and_needs_its_metadata():
    assert deft_amd.ExtendStep is not None and hasattr(deft_amd.TreeMetadata, "for_extend")
    assert hasattr(deft_amd.DeFTAttention, "extend_forward")
    tree, kids, pool, _ = _tree()
    step = tree.alloc_extend({kids[0]: [1, 2]})
    with pytest.raises(deft_amd.DeftLibraryError, match="GPU"):
        deft_amd.TreeMetadata.for_extend(tree, step)  # (a CPU pool: there is no host path)
    deft_amd.unregister_tree_metadata()
    attn = deft_amd.DeFTAttention(4, 16, 16 ** -0.5, 2, 0)
    meta = deft_amd.InputMetadata(deft_amd.ForwardMode.EXTEND, step.updater(pool), pool)
    q = torch.zeros((2, 64), dtype=torch.float16)
    with pytest.raises(AssertionError):
        attn(q, q[:, :32], q[:, :32], meta)  # nothing registered
