#!/usr/bin/env python3
"""The fp16 decode step against the same step over an fp8 KV pool, one process, alternating: the workload's tree
built twice -- an fp16 pool with N(0,1) data, one distinct KV array per layer, and an fp8 pool that is that pool quantised with unit
scales -- every layer's call captured in ONE hipGraph per pool type and replayed in turns.  The fp16 call is what bench.py times
(fused append + attention, one call per layer); the kv8 call is DeFTAttention.forward on the fp8 pool with the quantising append as a
launch of its own (kv8_fused_append = False: append, kv8 operator); the third arm, "kv8 fused", is the same call with the append inside
the stage-1 launch (kv8_fused_append = True) -- its outputs and pool bytes are asserted equal to the second arm's.  Beside each, `deft_probe_stream_read` over the kv8 launch's K/V bytes: the ceiling of a launch
that only reads them.

   tools/kv8_ab.py [--workloads northstar_4kx32,gqa_4kx32,tot50_4k,medusa64_node] [--layers 32] [--steps 50] [--reps 7] [--out FILE]

Per workload: per-repetition figures, median and min-max of each arm, the ratios of the medians, and the fused arm's median against the
two-launch arm's median plus its min-max spread (the routing rule of DESIGN section 6e)."""
import argparse, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import deft_amd
from deft_amd._lib import check, lib
from deft_amd.utils import workloads as wl
from deft_amd.utils.workloads import GEOMETRY, WORKLOADS, build_tree

ap = argparse.ArgumentParser()
ap.add_argument("--workloads", default="northstar_4kx32,gqa_4kx32,tot50_4k,medusa64_node")
ap.add_argument("--layers", type=int, default=None)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
FP8 = torch.float8_e4m3fn
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def capture(fn):
    fn()
    fn()
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize(dev)
    return graph


def time_graph(graph, steps, layers):
    for _ in range(5):
        graph.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / (steps * layers)


class Step:
    def __init__(self, w, layers, pool_dtype, source=None, fused=None):
        Hq, Hkv, D, _ = GEOMETRY[w.model]
        self.layers = layers
        self.tree, self.pool = build_tree(w, layers, str(dev), dtype=pool_dtype)
        self.md = deft_amd.TreeMetadata.from_tree_cache(self.tree)
        nq = self.md.query_num
        g = torch.Generator(device=dev).manual_seed(0)
        if source is None:
            for l in range(layers):
                self.pool._storage[l].normal_(generator=g)
        else:  # the fp16 pool quantised with unit scales (clamp, then round to nearest even: tests/kv8_model.py)
            for l in range(layers):
                self.pool._storage[l].copy_(torch.clamp(source.pool._storage[l].float(), -448, 448).to(FP8))
        g = torch.Generator(device=dev).manual_seed(1)
        self.q, self.k, self.v = (torch.randn((layers, nq, h * D), dtype=torch.float16, device=dev, generator=g) for h in (Hq, Hkv, Hkv))
        leaves = sorted(self.tree.leaves.values(), key=lambda n: n.id)
        loc = torch.tensor([lf.kv_indices[-1] for lf in leaves], dtype=torch.int32, device=dev)
        mode = deft_amd.forward_mode_from_cli(w.mode)
        self.meta = deft_amd.InputMetadata(mode, deft_amd.KVCacheUpdater(True, self.pool, loc, None, False), self.pool)
        self.attn = [deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, l) for l in range(layers)]
        if fused is not None:  # (an fp8 pool: the quantising append inside the stage-1 launch, or as a launch of its own)
            for at in self.attn:
                at.kv8_fused_append = fused
        self.graph = capture(self.eager)
        assert bool(torch.isfinite(self.outs[-1]).all())

    def eager(self):
        deft_amd.register_tree_metadata(self.md)
        self.outs = [self.attn[l](self.q[l], self.k[l], self.v[l], self.meta) for l in range(self.layers)]


def ceiling(pool, n_kv, layers):
    """One launch per layer that only reads the first n_kv slots of the layer's pool (where the tree's tokens are); best of three grids."""
    nbytes = int(n_kv) * pool.kv_data[0].stride(0) * pool._storage.element_size()
    best = None
    for wgs in (256, 512, 1024):
        def launch_all():
            for l in range(layers):
                check(lib.deft_probe_stream_read(pool.kv_data[l].data_ptr(), nbytes, wgs, torch.cuda.current_stream(dev).cuda_stream),
                      "deft_probe_stream_read")
        us = sorted(time_graph(capture(launch_all), 8, layers) for _ in range(3))[1]
        best = us if best is None or us < best else best
    return best, nbytes


for name in a.workloads.split(","):
    w = WORKLOADS[name]
    assert w.trees == 1 and w.mode in ("flatten", "node", "node_chunk"), "a single tree in one of the tree modes"
    Hq, Hkv, D, model_layers = GEOMETRY[w.model]
    layers = a.layers or model_layers
    deft_amd.BLOCK_CONFIG["MAX_BLOCK_LEN"] = 128 if w.mode == "node_chunk" else -1
    f16 = Step(w, layers, torch.float16)
    kv8 = Step(w, layers, FP8, source=f16, fused=False)
    kv8f = Step(w, layers, FP8, source=f16, fused=True)
    # the two steps compute the same attention up to the quantisation of K / V: a sanity figure, not a tolerance
    diff = float((f16.outs[-1].float() - kv8.outs[-1].float()).abs().max())
    # ... and the fused arm is the two-launch arm bit for bit: the last layer's output and every byte of the two pools
    assert torch.equal(kv8f.outs[-1].view(torch.int16), kv8.outs[-1].view(torch.int16))
    assert torch.equal(kv8f.pool._storage.view(torch.uint8), kv8.pool._storage.view(torch.uint8))
    runs = {"fp16": f16, "kv8": kv8, "kv8 fused": kv8f}
    res = {n: [] for n in runs}
    for rep in range(a.reps):
        for n, s in runs.items():
            res[n].append(time_graph(s.graph, a.steps, layers))
    ceil_us, nbytes = ceiling(kv8.pool, wl.tree_tokens(w), layers)
    say(f"{name} ({w.mode}, {w.model}: Hq {Hq} Hkv {Hkv}), {layers} layers in one hipGraph, {a.steps} replays x {a.reps} repetitions, "
        f"alternating; us per layer")
    for n, xs in res.items():
        say(f"  {n}: " + " ".join(f"{x:.2f}" for x in xs) + f" | median {np.median(xs):.2f} min {np.min(xs):.2f} max {np.max(xs):.2f}")
    m2, mf = np.median(res["kv8"]), np.median(res["kv8 fused"])
    spread = np.max(res["kv8"]) - np.min(res["kv8"])
    say(f"  kv8 fused / kv8 (medians): {mf / m2:.4f}    kv8 fused / fp16: {mf / np.median(res['fp16']):.4f}    fused - two-launch: {mf - m2:+.2f} us, "
        f"the two-launch arm's min-max spread {spread:.2f} us: {'within' if mf - m2 <= spread else 'BEYOND'} it")
    say(f"  kv8 / fp16 (medians): {np.median(res['kv8']) / np.median(res['fp16']):.4f}    "
        f"bare read of the kv8 launch's {nbytes / 1e6:.1f} MB of K/V: {ceil_us:.2f} us    max |fp16 - kv8| of the last layer: {diff:.3e}")
    del f16, kv8, kv8f, runs
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
