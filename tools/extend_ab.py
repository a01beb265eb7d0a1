#!/usr/bin/env python3
"""One extend step against the decode steps it replaces, on the north-star tree (4096-token prefix x 32 branches x 200 tokens,
Llama-2-7B heads), timed the way bench.py times a step: 32 layers, each on its own KV pool, in one hipGraph.

For n tokens per leaf (default 1, 8, 32; 8 is the condition) the two graphs are replayed ALTERNATELY in one process:

    extend   one DeFTAttention.forward(ForwardMode.EXTEND) per layer over n chain tokens per leaf (32 n query rows)
    decode   one ordinary Flatten decode layer of the same tree; n of them are what the extend layer replaces

and the tool reports, per layer, the medians and the spread (p10 / p90) of both, the ratio extend / (n x decode), the host and
GPU time of the metadata build (`TreeMetadata.for_extend`, against `from_tree_cache` of the same tree) and of the per-step plan,
and with `--long` the same ratio for long extends of ONE leaf (where the decode-kernel form stops paying).

    python tools/extend_ab.py [--tokens 1,8,32] [--reps 40] [--long 64,128,256,512] > profiles/extend_vs_steps.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import deft_amd  # noqa: E402
from deft_amd.utils.workloads import GEOMETRY, WORKLOADS, build_tree  # noqa: E402


def capture(fn, device):
    fn()
    fn()
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream(device).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize(device)
    return graph


def timed_ms(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[len(xs) // 10], xs[(9 * len(xs)) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="1,8,32")
    ap.add_argument("--long", default="64,128,256,512", help="tokens on ONE leaf (empty: skip)")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--layers", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("extend_ab.py measures on the GPU; none found")
    device = torch.device("cuda", torch.cuda.current_device())
    w = WORKLOADS["northstar_4kx32"]
    Hq, Hkv, D, _ = GEOMETRY[w.model]
    L = args.layers
    deft_amd.BLOCK_CONFIG["MAX_BLOCK_LEN"] = -1
    tree, pool = build_tree(w, L, str(device), extra_slots=2048)
    g = torch.Generator(device=device).manual_seed(0)
    for l in range(L):
        pool._storage[l].normal_(generator=g)
    attn = [deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, l) for l in range(L)]
    leaves = [tree.leaves[i] for i in sorted(tree.leaves)]
    nq = len(leaves)
    print(f"# north-star tree: prefix {w.prefix} x {w.width} branches x {w.branch_len} tokens, Hq {Hq} Hkv {Hkv} D {D}, {L} layers "
          f"on {L} pools in one hipGraph; {args.reps} alternating replays per pair; times in us per layer: median (p10 .. p90)")

    # ---- the decode layer, as bench.py freezes it: every leaf's last slot takes the step's K / V
    md_dec = deft_amd.TreeMetadata.from_tree_cache(tree, copy=True)
    loc = torch.tensor([lf.kv_indices[-1] for lf in leaves], dtype=torch.int32, device=device)
    meta_dec = deft_amd.InputMetadata(deft_amd.ForwardMode.TREE_DECODE_FLATTEN, deft_amd.KVCacheUpdater(True, pool, loc, None, False), pool)
    qd = torch.randn((L, nq, Hq * D), dtype=torch.float16, device=device, generator=g)
    kd = torch.randn((L, nq, Hkv * D), dtype=torch.float16, device=device, generator=g)
    vd = torch.randn((L, nq, Hkv * D), dtype=torch.float16, device=device, generator=g)
    deft_amd.register_tree_metadata(md_dec)
    g_dec = capture(lambda: [attn[l](qd[l], kd[l], vd[l], meta_dec) for l in range(L)], device)

    def host_gpu_ms(fn, reps=7):
        host, gpu = [], []
        for _ in range(reps):
            torch.cuda.synchronize(device)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize(device)
            host.append((time.perf_counter() - t0) * 1e3)
            gpu.append(a.elapsed_time(b))
        return out, statistics.median(host[1:]), statistics.median(gpu[1:])

    _, h, gp = host_gpu_ms(lambda: deft_amd.TreeMetadata.from_tree_cache(tree))
    print(f"metadata build, decode step (from_tree_cache): host+GPU {h * 1e3:.0f} us wall, {gp * 1e3:.0f} us between events")

    def case(tokens_by_leaf, label, n_replaced):
        step = tree.alloc_extend(tokens_by_leaf)
        R = step.num_rows
        md, h, gp = host_gpu_ms(lambda: deft_amd.TreeMetadata.for_extend(tree, step))
        NB, P = md.block_q_cnts.shape[0], md.block_q.shape[0]
        meta = deft_amd.InputMetadata(deft_amd.ForwardMode.EXTEND, step.updater(pool), pool)
        q = torch.randn((L, R, Hq * D), dtype=torch.float16, device=device, generator=g)
        k = torch.randn((L, R, Hkv * D), dtype=torch.float16, device=device, generator=g)
        v = torch.randn((L, R, Hkv * D), dtype=torch.float16, device=device, generator=g)
        deft_amd.register_tree_metadata(md)
        torch.cuda.synchronize(device)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        attn[0](q[0], k[0], v[0], meta)  # (the first call of a step builds the plan all layers share)
        b.record()
        b.synchronize()
        first_call_us = a.elapsed_time(b) * 1e3
        g_ext = capture(lambda: [attn[l](q[l], k[l], v[l], meta) for l in range(L)], device)
        te, td = [], []
        for _ in range(args.reps):
            td.append(timed_ms(g_dec) * 1e3 / L)
            te.append(timed_ms(g_ext) * 1e3 / L)
        (me, e10, e90), (mdn, d10, d90) = spread(te), spread(td)
        ratio = me / (n_replaced * mdn)
        print(f"{label}: rows {R}  blocks {NB}  partial rows {P} | extend {me:.1f} ({e10:.1f} .. {e90:.1f}) | decode layer {mdn:.1f} "
              f"({d10:.1f} .. {d90:.1f}) x {n_replaced} = {n_replaced * mdn:.1f} | ratio extend / steps {ratio:.3f} | "
              f"for_extend {h * 1e3:.0f} us wall, {gp * 1e3:.0f} us between events; first layer call with plan build {first_call_us:.0f} us")
        tree.commit_extend(step, {lid: [] for lid in step.leaf_rows})  # nothing kept: the slots go back, the tree stays
        del g_ext
        return ratio

    for n in [int(x) for x in args.tokens.split(",") if x]:
        case({lf: list(range(n)) for lf in leaves}, f"{n:3d} chain tokens per leaf", n)
    for n in [int(x) for x in args.long.split(",") if x]:
        case({leaves[0]: list(range(n))}, f"{n:3d} chain tokens on ONE leaf (long extend; the decode layers it replaces serve all {nq} leaves)", n)
    deft_amd.unregister_tree_metadata()


if __name__ == "__main__":
    main()
