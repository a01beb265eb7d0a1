#!/usr/bin/env python3
"""What attention states cost (deft_amd/states.py), one process, same pools:

  ab      the frozen decode step with the plain fused-append entry point against its *_lse sibling: the workload's tree, N(0,1) data,
          every layer's fused append + attention captured in ONE hipGraph per form -- what bench.py times as
          `attention_latency_us_per_layer` -- and replayed in turns.  The yardstick is the plain call of the same library in the same
          run: the *_lse median should lie inside the min-max spread of the plain call's own repetitions.
  merge   merge_attention_states at n x Hq x D = 32 x 32 x 128 (a decode step) and 4096 x 32 x 128 (a 4k prefill) against
          deft_probe_stream_read over the same number of bytes (the bare coalesced read of that size), 20 launches per hipGraph.
  prefix  prefill_with_cached_prefix on a 4096-token cached prefix with 256 / 1024 new tokens (Llama-2-7B heads) against whole-prompt
          context_attention_fwd over all n0 + n1 tokens; eager calls, host work included (the composed form builds its block arrays
          on the host at every call).

   tools/states_ab.py [ab|merge|prefix|all] [--workload northstar_4kx32] [--layers 32] [--steps 100] [--reps 7]"""
import argparse, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import deft_amd
from deft_amd._lib import check, lib
from deft_amd.tree_attention import flatten_append_attention, node_append_attention
from deft_amd.utils.workloads import GEOMETRY, WORKLOADS, build_tree

ap = argparse.ArgumentParser()
ap.add_argument("what", nargs="?", default="all", choices=["ab", "merge", "prefix", "all"])
ap.add_argument("--workload", default="northstar_4kx32")
ap.add_argument("--layers", type=int, default=None)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
dev = torch.device("cuda", 0)
F32 = torch.float32


def captured(fn):
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


def us(run, steps, warm=10):
    for _ in range(warm):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        run()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / steps


def line(name, xs):
    return f"  {name}: " + " ".join(f"{x:.2f}" for x in xs) + f" | median {np.median(xs):.2f} min {np.min(xs):.2f} max {np.max(xs):.2f}"


def ab():
    w = WORKLOADS[a.workload]
    assert w.trees == 1 and w.mode in ("flatten", "node"), "a single tree in Flatten or Node mode"
    Hq, Hkv, D, model_layers = GEOMETRY[w.model]
    layers = a.layers or model_layers
    tree, pool = build_tree(w, layers, str(dev))
    md = deft_amd.TreeMetadata.from_tree_cache(tree)
    nq = md.query_num
    g = torch.Generator(device=dev).manual_seed(0)
    for l in range(layers):
        pool._storage[l].normal_(generator=g)
    q, k, v = (torch.randn((layers, nq, h, D), dtype=torch.float16, device=dev, generator=g) for h in (Hq, Hkv, Hkv))
    leaves = sorted(tree.leaves.values(), key=lambda n: n.id)
    loc = torch.tensor([lf.kv_indices[-1] for lf in leaves], dtype=torch.int32, device=dev)
    outs = torch.empty((2, layers, nq, Hq, D), dtype=torch.float16, device=dev)
    lse = torch.empty((layers, nq, Hq), dtype=F32, device=dev)
    if w.mode == "flatten":
        args = (md.block_len, md.block_q, md.block_q_cnts, md.block_q_offset, md.block_bitmasks, md.block_kv, md.block_lens)
        plain_fn, lse_fn = flatten_append_attention, deft_amd.flatten_append_attention_lse
    else:
        args = (md.node_kv, md.node_kv_offset, md.node_kv_len, md.node_q, md.node_q_offset, md.node_q_len)
        plain_fn, lse_fn = node_append_attention, deft_amd.node_append_attention_lse

    def plain():
        for l in range(layers):
            plain_fn(q[l], pool.kv_data[l], outs[0, l], loc, k[l], v[l], *args)

    def with_lse():
        for l in range(layers):
            lse_fn(q[l], pool.kv_data[l], outs[1, l], lse[l], loc, k[l], v[l], *args)

    graphs = {"plain": captured(plain), "lse": captured(with_lse)}
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(lse).all()), "the *_lse step must write the plain step's outputs"
    res = {n: [] for n in graphs}
    for _ in range(a.reps):
        for n, gr in graphs.items():
            res[n].append(us(gr.replay, a.steps) / layers)
    print(f"{a.workload} ({w.mode}), {layers} layers in one hipGraph, {a.steps} replays x {a.reps} repetitions, alternating; us per layer")
    for n, xs in res.items():
        print(line(n, xs))
    lo, hi, m = np.min(res["plain"]), np.max(res["plain"]), np.median(res["lse"])
    where = "inside" if lo <= m <= hi else f"OUTSIDE by {min(abs(m - lo), abs(m - hi)):.2f} us"
    print(f"  lse / plain (medians): {m / np.median(res['plain']):.4f}; the lse median lies {where} the plain repetitions' spread [{lo:.2f}, {hi:.2f}]")


def merge():
    print("merge_attention_states against a bare coalesced read of the same bytes, 20 launches per hipGraph; us per launch")
    for n, Hq, D in ((32, 32, 128), (4096, 32, 128)):
        g = torch.Generator(device=dev).manual_seed(n)
        o_a, o_b = (torch.randn((n, Hq, D), dtype=torch.float16, device=dev, generator=g) for _ in range(2))
        l_a, l_b = (torch.randn((n, Hq), dtype=F32, device=dev, generator=g) for _ in range(2))
        out, l_o = torch.empty_like(o_a), torch.empty_like(l_a)
        nbytes = 3 * o_a.numel() * 2 + 3 * l_a.numel() * 4  # two states read, one written
        buf = torch.empty(nbytes // 2, dtype=torch.float16, device=dev)
        wgs = min(2048, (n * Hq + 15) // 16)

        def m20():
            for _ in range(20):
                deft_amd.merge_attention_states(o_a, l_a, o_b, l_b, out=out, lse_out=l_o)

        def p20():
            for _ in range(20):
                check(lib.deft_probe_stream_read(buf.data_ptr(), nbytes, wgs, torch.cuda.current_stream(dev).cuda_stream), "probe")

        gm, gp = captured(m20), captured(p20)
        res = {"merge_states": [], "stream read": []}
        for _ in range(a.reps):
            res["merge_states"].append(us(gm.replay, 20) / 20)
            res["stream read"].append(us(gp.replay, 20) / 20)
        print(f" n x Hq x D = {n} x {Hq} x {D} ({nbytes / 1e6:.2f} MB moved, {wgs} workgroups)")
        for name, xs in res.items():
            print(line(name, xs))
        print(f"  merge_states / stream read (medians): {np.median(res['merge_states']) / np.median(res['stream read']):.3f}")


def prefix():
    Hq, Hkv, D = 32, 32, 128
    n0 = 4096
    print("prefill_with_cached_prefix against whole-prompt context_attention_fwd, Llama-2-7B heads, 4096-token cached prefix; eager "
          "calls, host work included; us per call")
    for n1 in (256, 1024):
        N = n0 + n1
        g = torch.Generator(device=dev).manual_seed(n1)
        q, k, v = (torch.randn((N, h, D), dtype=torch.float16, device=dev, generator=g) for h in (Hq, Hkv, Hkv))
        pool = deft_amd.TokenToKVPool(N + 64, torch.float16, Hkv, D, 1, device=str(dev))
        slots = pool.alloc(N).long()
        kv = pool.kv_data[0]
        kv[slots[:n0], 0], kv[slots[:n0], 1] = k[:n0], v[:n0]
        path, new = slots[:n0].tolist(), slots[n0:].tolist()
        whole, out = torch.empty((N, Hq, D), dtype=torch.float16, device=dev), torch.empty((n1, Hq, D), dtype=torch.float16, device=dev)
        start, lens = torch.zeros(1, dtype=torch.int32, device=dev), torch.tensor([N], dtype=torch.int32, device=dev)
        res = {"whole prompt": [], "cached prefix": []}
        for _ in range(a.reps):
            res["whole prompt"].append(us(lambda: deft_amd.context_attention_fwd(q, k, v, whole, start, lens, N), 5, warm=2))
            res["cached prefix"].append(us(lambda: deft_amd.prefill_with_cached_prefix(q[n0:], k[n0:], v[n0:], out, kv, path, new), 5, warm=2))
        err = float((out.float() - whole[n0:].float()).abs().max())
        print(f" {n0} cached + {n1} new tokens (composed vs whole-prompt rows: max |diff| {err:.2e})")
        for name, xs in res.items():
            print(line(name, xs))
        print(f"  cached prefix / whole prompt (medians): {np.median(res['cached prefix']) / np.median(res['whole prompt']):.3f}")


for name, fn in (("ab", ab), ("merge", merge), ("prefix", prefix)):
    if a.what in (name, "all"):
        fn()
