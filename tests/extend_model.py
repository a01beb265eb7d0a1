"""A numpy model of an extend step (deft_amd.TreeCache.alloc_extend / TreeMetadata.for_extend): what every row must see, how
the six Flatten arrays decode into what every row DOES see, and the invariants of those arrays.  No kernel, no GPU.

Semantics: the tree as it stands, the step's R tokens not yet in it.  Token t is query row t; it sits on leaf `row_leaf[t]`, has
the fresh pool slot `slots[t]` and hangs off `parents[t]` (-1 = the end of the leaf's cached path, else an earlier row of the same
leaf).  Row t attends over exactly  path_slots(leaf[t]) + [slots[u] for u = t and every ancestor of t]."""
from __future__ import annotations

from collections import Counter
from typing import Dict, List, Sequence

import numpy as np

TILE = 128
MAX_ROWS = 32

CHAIN = None  # `parents` of a chain step


def draft_tree_parents(fanout: Sequence[int]) -> List[int]:
    """Local parent indices of a draft tree given by the node count of every level (1 -> 2 -> 4: [1, 2, 4]), level by level: each
    level's nodes are spread evenly under the level above."""
    par, prev, at = [], [-1], 0
    for n in fanout:
        cur = []
        for i in range(n):
            par.append(prev[i * len(prev) // n])
            cur.append(at)
            at += 1
        prev = cur
    return par


def ancestors_or_self(parents: np.ndarray, t: int) -> List[int]:
    out = []
    while t >= 0:
        out.append(int(t))
        t = int(parents[t])
    return out[::-1]


def key_sets(tree, step) -> List[List[int]]:
    """Per row of the step, the pool slots it attends over (cached path first, then its new ancestors, itself last)."""
    paths = {lid: tree.leaf_path_slots(tree.leaves[lid]) for lid in step.leaf_rows}
    return [list(paths[int(step.row_leaf[t])]) + [int(step.slots[u]) for u in ancestors_or_self(step.parents, t)]
            for t in range(step.num_rows)]


def md_arrays(md) -> Dict[str, np.ndarray]:
    return {k: getattr(md, k).cpu().numpy() for k in ("block_q", "block_q_cnts", "block_q_offset", "block_bitmasks", "block_kv",
                                                       "block_lens")}


def decode(arr: Dict[str, np.ndarray], R: int) -> List[Counter]:
    """Per row, the multiset of slots the block arrays make it see."""
    seen = [Counter() for _ in range(R)]
    for b in range(len(arr["block_q_cnts"])):
        cnt, off, ln = int(arr["block_q_cnts"][b]), int(arr["block_q_offset"][b]), int(arr["block_lens"][b])
        rows = arr["block_q"][off : off + cnt]
        for k in range(ln):
            m, slot = int(arr["block_bitmasks"][b * TILE + k]), int(arr["block_kv"][b * TILE + k])
            for j in range(cnt):
                if (m >> j) & 1:
                    seen[int(rows[j])][slot] += 1
    return seen


def check_invariants(arr: Dict[str, np.ndarray], R: int) -> None:
    """Ascending query lists; cnt <= 32 and len <= 128; every live slot has a non-empty mask, and no bit beyond the list; every
    listed row sees a slot of its block; the offsets are the exclusive prefix sums of the counts; the padding reads -1 / 0."""
    NB = len(arr["block_q_cnts"])
    assert NB >= 1 and len(arr["block_lens"]) == NB and len(arr["block_q_offset"]) == NB
    assert len(arr["block_kv"]) == NB * TILE and len(arr["block_bitmasks"]) == NB * TILE
    at = 0
    for b in range(NB):
        cnt, off, ln = int(arr["block_q_cnts"][b]), int(arr["block_q_offset"][b]), int(arr["block_lens"][b])
        assert 1 <= cnt <= MAX_ROWS and 1 <= ln <= TILE, (b, cnt, ln)
        assert off == at, (b, off, at)
        at += cnt
        rows = arr["block_q"][off : off + cnt]
        assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < R, (b, rows)
        masks = arr["block_bitmasks"][b * TILE : b * TILE + ln]
        assert (masks != 0).all(), (b, "a live slot nobody sees")
        assert (masks >> cnt == 0).all(), (b, "a mask bit beyond the query list")
        assert (arr["block_kv"][b * TILE : b * TILE + ln] >= 0).all(), b
        assert (arr["block_kv"][b * TILE + ln : (b + 1) * TILE] == -1).all(), (b, "padding slots")
        assert (arr["block_bitmasks"][b * TILE + ln : (b + 1) * TILE] == 0).all(), (b, "padding masks")
        union = int(np.bitwise_or.reduce(masks))
        assert union == (1 << cnt) - 1, (b, "a listed row that sees nothing of the block")
    assert at == len(arr["block_q"])


def check_against_model(arr: Dict[str, np.ndarray], want: List[List[int]]) -> None:
    """Each (row, slot) pair of the semantics exactly once over all blocks, and nothing else."""
    seen = decode(arr, len(want))
    for t, (s, w) in enumerate(zip(seen, want)):
        assert s == Counter(w), (t, "missing", sorted((Counter(w) - s).elements())[:8], "extra", sorted((s - Counter(w)).elements())[:8])


def new_key_blocks(arr: Dict[str, np.ndarray], step_slots) -> int:
    """Blocks that hold slots of the step (the new-key blocks hold nothing else)."""
    new = set(int(s) for s in step_slots)
    n = 0
    for b in range(len(arr["block_q_cnts"])):
        kv = arr["block_kv"][b * TILE : b * TILE + int(arr["block_lens"][b])]
        isnew = [int(s) in new for s in kv]
        assert all(isnew) or not any(isnew), (b, "a block mixes cached and new keys")
        n += all(isnew)
    return n
