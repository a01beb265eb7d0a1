#!/usr/bin/env python3
"""The captured decode loop over an fp8 KV pool against the 16-bit session and the eager fp8 loop ("In the captured
session"): tools/kv8_ab.py's workloads, one process, the arms alternating, every arm an ADVANCING loop -- every leaf takes a token, then
one step of every layer -- over a tree of its own:

   (a) 16-bit session                 deft_amd.DecodeSession over an fp16 pool (window plans)
   (b) fp8 session, two launches      kv8_fused_append=False, incremental False ("legacy") and True ("window")
   (c) fp8 session, fused             kv8_fused_append=True, the same two settings
   (d) eager fp8 loop                 tree.alloc + TreeMetadata.from_tree_cache + DeFTAttention.forward per layer

   tools/kv8_session_ab.py [--workloads northstar_4kx32,gqa_4kx32,tot50_4k,medusa64_node] [--layers N] [--steps 50] [--reps 7] [--out FILE]

Every arm is warmed up (its epoch uploaded, its graphs captured); a repetition times `steps` steps of one arm between two
synchronisations (wall clock: host and device together, what a serving loop sees), then the next arm's; reported per arm: the
repetitions, their median and min-max, in ms per step.  The trees grow by the same number of tokens in every arm, so the arms stay
comparable inside a repetition, and a later repetition runs on a longer tree than an earlier one (the min-max includes that).
Last per workload: the routing rule of section 6e for each `incremental` setting -- fused only where its median does not exceed the
two-launch median by more than the two-launch arm's own min-max spread; since the raw min-max of an advancing loop also holds the
tree's growth, the spread is taken around the arm's straight-line trend over the repetitions (both are printed)."""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import deft_amd
from deft_amd.utils.workloads import GEOMETRY, WORKLOADS, build_tree

ap = argparse.ArgumentParser()
ap.add_argument("--workloads", default="northstar_4kx32,gqa_4kx32,tot50_4k,medusa64_node")
ap.add_argument("--layers", type=int, default=None)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=12)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.steps >= 50, "an advancing loop of at least 50 steps"
dev = torch.device("cuda", 0)
FP8, F16 = torch.float8_e4m3fn, torch.float16
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


class Arm:
    """One tree, one pool, one way of decoding it."""

    def __init__(self, w, layers, pool_dtype, session, incremental=True, fused=None, source=None):
        Hq, Hkv, D, _ = GEOMETRY[w.model]
        self.layers, self.session = layers, session
        total = a.warmup + a.steps * a.reps + 4
        self.tree, self.pool = build_tree(w, layers, str(dev), extra_slots=256 + total * 64, dtype=pool_dtype)
        nq = len(self.tree.leaves)
        assert nq <= 64
        g = torch.Generator(device=dev).manual_seed(0)
        if source is None:
            for l in range(layers):
                self.pool._storage[l].normal_(generator=g)
        else:  # the fp16 arm's pool quantised with unit scales (clamp, then round to nearest even: tests/kv8_model.py)
            for l in range(layers):
                self.pool._storage[l].copy_(torch.clamp(source.pool._storage[l].float(), -448, 448).to(FP8))
        g = torch.Generator(device=dev).manual_seed(1)
        self.q, self.k, self.v = (torch.randn((layers, nq, h * D), dtype=F16, device=dev, generator=g) for h in (Hq, Hkv, Hkv))
        smode = "node" if w.mode == "node_chunk" else w.mode
        if session:
            kw = dict(elem_dtype=F16, kv8_fused_append=fused) if pool_dtype == FP8 else {}
            self.sess = deft_amd.DecodeSession(self.tree, Hq, Hkv, D, layers, lambda l: (self.q[l], self.k[l], self.v[l]), mode=smode,
                                               incremental=incremental, **kw)
        else:
            self.attn = [deft_amd.DeFTAttention(Hq, D, D ** -0.5, Hkv, l) for l in range(layers)]
            self.fmode = deft_amd.forward_mode_from_cli(w.mode)
        self.run(a.warmup)
        torch.cuda.synchronize(dev)
        assert bool(torch.isfinite(self.out[-1]).all())

    def run(self, steps):
        tree = self.tree
        for _ in range(steps):
            for leaf in tree.leaves.values():
                leaf.append_token(7)
            if self.session:
                self.out = self.sess.step()
            else:
                upd = tree.alloc()
                md = deft_amd.TreeMetadata.from_tree_cache(tree)
                deft_amd.register_tree_metadata(md)
                meta = deft_amd.InputMetadata(self.fmode, upd, self.pool)
                self.out = [self.attn[l](self.q[l], self.k[l], self.v[l], meta) for l in range(self.layers)]

    def timed(self, steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        self.run(steps)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / steps


for name in a.workloads.split(","):
    w = WORKLOADS[name]
    assert w.trees == 1 and w.mode in ("flatten", "node", "node_chunk"), "a single tree in one of the tree modes"
    Hq, Hkv, D, model_layers = GEOMETRY[w.model]
    layers = a.layers or model_layers
    deft_amd.BLOCK_CONFIG["MAX_BLOCK_LEN"] = 128 if w.mode == "node_chunk" else -1
    f16 = Arm(w, layers, F16, True)
    arms = {"(a) 16-bit session": f16,
            "(b) fp8 session, two launches, legacy": Arm(w, layers, FP8, True, False, False, f16),
            "(c) fp8 session, fused, legacy": Arm(w, layers, FP8, True, False, True, f16),
            "(b) fp8 session, two launches, window": Arm(w, layers, FP8, True, True, False, f16),
            "(c) fp8 session, fused, window": Arm(w, layers, FP8, True, True, True, f16),
            "(d) eager fp8 loop": Arm(w, layers, FP8, False, source=f16)}
    res = {n: [] for n in arms}
    for rep in range(a.reps):
        for n, arm in arms.items():
            res[n].append(arm.timed(a.steps))
    say(f"{name} ({w.mode}, {w.model}: Hq {Hq} Hkv {Hkv}), {layers} layers, {len(f16.tree.leaves)} leaves, advancing loops of {a.steps} steps x "
        f"{a.reps} repetitions after {a.warmup} warm-up steps, alternating; ms per step (host and device)")
    for n, xs in res.items():
        kinds = f"  step kinds {arms[n].sess.step_kinds} captures {arms[n].sess.captures}" if arms[n].session else ""
        say(f"  {n}: " + " ".join(f"{x:.3f}" for x in xs) + f" | median {np.median(xs):.3f} ({np.min(xs):.3f}-{np.max(xs):.3f}){kinds}")
    for setting in ("legacy", "window"):
        two, fu = res[f"(b) fp8 session, two launches, {setting}"], res[f"(c) fp8 session, fused, {setting}"]
        m2, mf, spread = np.median(two), np.median(fu), np.max(two) - np.min(two)
        # the tree grows from repetition to repetition, and the raw min-max holds that growth: the spread that decides is the two-launch
        # arm's min-max around its own straight-line fit over the repetitions (what is left is run-to-run noise)
        resid = np.asarray(two) - np.polyval(np.polyfit(np.arange(len(two)), two, 1), np.arange(len(two))) if len(two) > 2 else np.zeros(1)
        noise = float(np.max(resid) - np.min(resid))
        paired = np.asarray(fu) - np.asarray(two)
        say(f"  {setting}: fused - two-launch (medians) {1e3 * (mf - m2):+.1f} us per step (per repetition: median {1e3 * np.median(paired):+.1f}, "
            f"{1e3 * np.min(paired):+.1f} .. {1e3 * np.max(paired):+.1f}); the two-launch arm's min-max spread {1e3 * spread:.1f} us raw, "
            f"{1e3 * noise:.1f} us around its growth trend: {'within' if mf - m2 <= noise else 'BEYOND'} the latter; fused / two-launch {mf / m2:.4f}")
    ma = np.median(res["(a) 16-bit session"])
    say("  medians against (a): " + "; ".join(f"{n} {np.median(xs) / ma:.4f}" for n, xs in res.items() if not n.startswith("(a)")))
    for arm in arms.values():
        if arm.session:
            assert arm.sess.device_errors() == 0
    del arms, f16
    deft_amd.unregister_tree_metadata()
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
