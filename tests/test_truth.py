"""tests/truth.py's dense fp64 tree attention (one masked softmax over the union of all paths) against the oracle's sequential
per-leaf attention (oracle.attention.sequential_truth), on scripted trees: MHA and GQA with a group size (3) that does not divide 32."""
import numpy as np
import pytest
import torch

from helpers import leaf_paths, oracle_metadata, oracle_tree
from oracle import attention as oa
from scenarios import SCENARIOS
from truth import tree_truth


@pytest.mark.parametrize("name,geom", [("multilevel", (4, 4, 64)), ("after_cut", (6, 2, 32))])
def test_tree_truth_equals_the_sequential_oracle(name, geom):
    Hq, Hkv, D = geom
    tree = oracle_tree(name)
    paths = leaf_paths(tree)
    nq = oracle_metadata(name, tree)["query_num"]
    assert nq == len(paths) and nq > 1 and len({tuple(p) for p in paths}) == nq  # (distinct paths over shared nodes)
    rng = np.random.default_rng(sum(map(ord, name)))
    q = rng.standard_normal((nq, Hq, D)).astype(np.float32)
    kv = rng.standard_normal((SCENARIOS[name].pool_size, 2, Hkv, D)).astype(np.float16)
    want = oa.sequential_truth(q, kv, paths)
    kvt = torch.from_numpy(kv)
    got = tree_truth(torch.from_numpy(q), kvt[:, 0], kvt[:, 1], paths, Hq, Hkv, D ** -0.5)
    assert got.dtype == torch.float64 and tuple(got.shape) == (nq, Hq, D)
    assert float(np.abs(got.numpy() - want).max()) < 1e-12
