"""Child process of tests/test_kv8_gpu.py::test_item_loop_of_a_capped_grid: runs against the EXPERIMENTS build
(DEFT_AMD_LIB=deft_amd/lib/libdeft_amd_exp.so), the only one whose launchers read DEFT_NP_GRID / DEFT_NP_MIRROR.

The item loop of stage1_kv8_kernel -- a workgroup of a capped grid takes several work items: next_item in plain (b, b + W, ...) and in
mirrored order (b, 2W - 1 - b, 2W + b, ...), the barrier between two items, Q, partial-row numbers and offsets staged again -- forced to
many rounds by a tiny grid: every item exactly once, the same bits as one workgroup per item, and that run against fp64 truth.

usage: python tests/exp_kv8_items.py Hq Hkv prefix width steps
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import deft_amd  # noqa: E402
import kv8_model  # noqa: E402
import oracles  # noqa: E402
from tools.error_bound import bound_bf16, dense_attention  # noqa: E402
from truth import product_leaf_paths  # noqa: E402

D = 128


def run(shape):
    Hq, Hkv, prefix, width, steps = shape
    tree, pool, _ = oracles.few_shot_tree(prefix, width, steps, Hkv, D)
    paths = product_leaf_paths(tree)
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    g = torch.Generator(device="cuda").manual_seed(13)
    codes = kv8_model.quantize(torch.randn((pool.size, 2, Hkv, D), device="cuda", generator=g).to(torch.float16), 1.0)
    kb, vb = codes[:, 0], codes[:, 1]
    ks = torch.tensor([0.73, 1.9, 1.21, 0.57][:Hkv], dtype=torch.float32, device="cuda")
    vs = torch.tensor([0.61, 0.43, 0.37, 0.53][:Hkv], dtype=torch.float32, device="cuda")
    k64, v64 = kv8_model.dequantize(kb, ks[:, None]), kv8_model.dequantize(vb, vs[:, None])
    flat = (md.block_len, md.block_q, md.block_q_cnts, md.block_q_offset, md.block_bitmasks, md.block_kv, md.block_lens)
    node = (md.node_kv, md.node_kv_offset, md.node_kv_len, md.node_q, md.node_q_offset, md.node_q_len)
    for dtype in (torch.float16, torch.bfloat16):
        q = torch.randn((len(paths), Hq, D), device="cuda", generator=g).to(dtype)
        truth, A = dense_attention(q, k64, v64, paths, Hq, Hkv, D ** -0.5, with_abs=True)
        tol = torch.full_like(truth, 5e-4) if dtype == torch.float16 else bound_bf16(truth, A)
        for fn, args in ((deft_amd.tree_attention_subtree_fwd_kv8, flat), (deft_amd.tree_attention_fwd_kv8, node)):
            def call():
                o = torch.full_like(q, float("nan"))
                fn(q, kb, vb, o, *args, k_scale=ks, v_scale=vs)
                torch.cuda.synchronize()
                return o

            ref = call()
            worst = float(((ref.to(torch.float64) - truth).abs() / tol).max())
            print(f"[kv8] item loop {Hq}x{Hkv} {prefix}x{width}x{steps} {fn.__name__} {dtype}: one item per workgroup, err/tol {worst:.3f}", flush=True)
            assert bool(torch.isfinite(ref).all()) and worst <= 1.0, worst
            for grid, mirror in ((37, 1), (37, 0), (5, 1), (1, 1)):
                os.environ["DEFT_NP_GRID"], os.environ["DEFT_NP_MIRROR"] = str(grid), str(mirror)
                try:
                    o = call()
                finally:
                    del os.environ["DEFT_NP_GRID"], os.environ["DEFT_NP_MIRROR"]
                assert torch.equal(o.view(torch.int16), ref.view(torch.int16)), (fn.__name__, dtype, grid, mirror)


if __name__ == "__main__":
    run(tuple(int(x) for x in sys.argv[1:6]))
    print("items identical")
