#!/usr/bin/env python3
"""fp16 against bf16 on the frozen decode step, one process, alternating: the workload's tree built twice (an fp16 pool and a bf16
pool, N(0,1) data, one distinct KV array per layer), every layer's fused append + attention captured in ONE hipGraph per element type
-- what bench.py times as `attention_latency_us_per_layer` -- and replayed in turns.

   tools/dtype_ab.py [--workload northstar_4kx32] [--layers 32] [--steps 100] [--reps 7]

Prints the per-repetition figures, then median and min-max per element type and the ratio of the medians."""
import argparse, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import deft_amd
from deft_amd.utils.workloads import GEOMETRY, WORKLOADS, build_tree

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="northstar_4kx32")
ap.add_argument("--layers", type=int, default=None)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
w = WORKLOADS[a.workload]
assert w.trees == 1 and w.mode in ("flatten", "node", "node_chunk"), "a single tree in one of the tree modes"
Hq, Hkv, D, model_layers = GEOMETRY[w.model]
layers = a.layers or model_layers
dev = torch.device("cuda", 0)
deft_amd.BLOCK_CONFIG["MAX_BLOCK_LEN"] = 128 if w.mode == "node_chunk" else -1
mode = deft_amd.forward_mode_from_cli(w.mode)


class Step:
    def __init__(self, dtype):
        self.tree, self.pool = build_tree(w, layers, str(dev), dtype=dtype)
        self.md = deft_amd.TreeMetadata.from_tree_cache(self.tree)
        nq = self.md.query_num
        g = torch.Generator(device=dev).manual_seed(0)
        for l in range(layers):
            self.pool._storage[l].normal_(generator=g)
        self.q, self.k, self.v = (torch.randn((layers, nq, h * D), dtype=dtype, device=dev, generator=g) for h in (Hq, Hkv, Hkv))
        leaves = sorted(self.tree.leaves.values(), key=lambda n: n.id)
        loc = torch.tensor([lf.kv_indices[-1] for lf in leaves], dtype=torch.int32, device=dev)
        self.meta = deft_amd.InputMetadata(mode, deft_amd.KVCacheUpdater(True, self.pool, loc, None, False), self.pool)
        self.attn = [deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, l) for l in range(layers)]
        deft_amd.register_tree_metadata(self.md)
        self.eager()
        self.eager()
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            with torch.cuda.graph(self.graph, stream=side):
                self.eager()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph.replay()
        torch.cuda.synchronize(dev)
        assert self.outs[-1].dtype == dtype and bool(torch.isfinite(self.outs[-1]).all())

    def eager(self):
        self.outs = [self.attn[l](self.q[l], self.k[l], self.v[l], self.meta) for l in range(layers)]

    def us_per_layer(self, steps):
        for _ in range(10):
            self.graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            self.graph.replay()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / (steps * layers)


runs = {"fp16": Step(torch.float16), "bf16": Step(torch.bfloat16)}
res = {n: [] for n in runs}
for rep in range(a.reps):
    for n, s in runs.items():
        res[n].append(s.us_per_layer(a.steps))
print(f"{a.workload} ({w.mode}), {layers} layers in one hipGraph, {a.steps} replays x {a.reps} repetitions, alternating; us per layer")
for n, xs in res.items():
    print(f"  {n}: " + " ".join(f"{x:.2f}" for x in xs) + f" | median {np.median(xs):.2f} min {np.min(xs):.2f} max {np.max(xs):.2f}")
print(f"  bf16 / fp16 (medians): {np.median(res['bf16']) / np.median(res['fp16']):.4f}")
