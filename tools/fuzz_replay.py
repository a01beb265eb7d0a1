#!/usr/bin/env python3
"""Randomised replays: random tree templates (widths, node lengths, prompt length), geometries and modes; at every
step the attention output of layer 0 is compared with fp64 per-leaf attention over the leaf's page-table row,
computed with torch on the GPU.  tools/fuzz_replay.py [seconds] [seed] [max replays] [--bf16]
--bf16 (anywhere on the command line): the replays run in bfloat16 and every element is held to the a-priori bound of the bf16
kernels instead (tools/error_bound.py: u A + 2 u |ref| + 2e-5, A = sum_i p_i |v_i|, u = 2^-8)."""
import os, sys, time, random
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from deft_amd import replay as rp

BF16 = "--bf16" in sys.argv
sys.argv = [a for a in sys.argv if a != "--bf16"]
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
t_end = time.time() + budget
max_runs = int(sys.argv[3]) if len(sys.argv) > 3 else 10 ** 9
runs = steps = 0
worst = 0.0
tight = [0, 0]  # elements beyond 5e-4 + half ulp, elements checked
while time.time() < t_end and runs < max_runs:
    Hq, Hkv = rng.choice([(32, 32), (32, 8), (8, 2), (4, 4), (16, 1), (28, 4), (24, 8)])
    D = 64 if Hq <= 8 and rng.random() < 0.3 else 128
    mode = rng.choice(["flatten", "flatten", "node", "node_chunk", "seq"])
    task = rng.choice(["reasoning", "reasoning", "few_shot", "speculative_decoding"])
    if task == "reasoning":
        depth = rng.randint(1, 3)
        tpl = rp.synthetic_reasoning_template(widths=[rng.randint(1, 6) for _ in range(depth)],
                                              lens=[rng.choice([1, 2, 3, 7, 40, 130, 200]) for _ in range(depth)])
        gen = 600
    elif task == "few_shot":
        tpl = rp.synthetic_few_shot_template(rng.choice([1, 2, 5, 33, 40, 64, 70, 100]))
        gen = rng.choice([3, 10, 140])
    else:
        tpl = rp.synthetic_speculative_template(rng.choice([4, 16, 64]), rng.randint(3, 8), (1, rng.randint(1, 4)), rng.randint(0, 999))
        gen = 100
    prompt = rng.choice([1, 5, 127, 128, 129, 300, 1000, 4096, 4096, 20000, 70000] if Hq <= 8 else [1, 5, 127, 128, 129, 300, 1000, 4096])
    if prompt >= 20000:
        gen = min(gen, 30)  # the fp64 check walks every leaf's whole path at every step
    if os.environ.get("FUZZ_VERBOSE"):
        print(runs, Hq, Hkv, D, mode, task, prompt, gen, flush=True)
    r = rp.TemplateReplay(Hq, Hkv, D, layers=1, mode=mode, device="cuda", attention=True, seed=rng.randint(0, 10 ** 6),
                          session=rng.random() < 0.6,  # (the captured session where one exists, the eager calls otherwise)
                          **({"dtype": torch.bfloat16} if BF16 else {}))

    def checked(tree, q, out):
        global steps, worst
        leaves = sorted(tree.leaves.values(), key=lambda n: n.id)
        kv = tree.token_to_kv_pool.kv_data[0].double()
        qd = q.view(-1, Hq, D).double(); od = out.view(-1, Hq, D).double()
        for i, lf in enumerate(leaves):
            path = tree.leaf_path_slots(lf)
            if mode == "seq":  # the comparator reads the PAGE TABLE; the reference's speculative-decoding mock squeezes
                # accepted tokens into the root without rewriting the other leaves' rows (branch_func_example.py:420-437),
                # so there -- and only there -- the table is not the tree path
                req = tree.leaf_to_req[lf.id]
                row = tree.req_to_token_pool.req_to_token[req, : len(path)].tolist()
                if task != "speculative_decoding":
                    assert row == path, (mode, task, i)
                path = row
            slots = torch.tensor(path, device="cuda")
            kk = kv[slots, 0].repeat_interleave(Hq // Hkv, dim=1).transpose(0, 1)  # [Hq, S, D]
            vv = kv[slots, 1].repeat_interleave(Hq // Hkv, dim=1).transpose(0, 1)
            s = torch.einsum("hd,hsd->hs", qd[i], kk) / D ** 0.5
            ref = torch.einsum("hs,hsd->hd", torch.softmax(s, dim=-1), vv)
            err = (od[i] - ref).abs().max().item()
            if BF16:  # per element: the bound of the kernels' arithmetic (module docstring)
                p = torch.softmax(s, dim=-1)
                tol = 2.0 ** -8 * torch.einsum("hs,hsd->hd", p, vv.abs()) + 2.0 ** -7 * ref.abs() + 2e-5
                ratio = ((od[i] - ref).abs() / tol).max().item()
                worst = max(worst, ratio)
                assert ratio <= 1.0, (ratio, err, mode, task, Hq, Hkv, prompt, i, len(slots))
                continue
            worst = max(worst, err)
            # per ELEMENT.  The bar is north_star's 1e-3 (+ half an fp16 ulp of the element: the output's own rounding).  The
            # tighter 5e-4 + half ulp is COUNTED, not asserted: with the probabilities rounded to fp16 for the PV MFMA (relative
            # 2^-11 each) a context of ten or twenty keys leaves an element 3 sigma out once in ~10^6 -- long contexts average it away
            diff = (od[i] - ref).abs()
            bad = (diff > 1e-3 + 2.0 ** -11 * ref.abs()).sum().item()
            tight[0] += int((diff > 5e-4 + 2.0 ** -11 * ref.abs()).sum().item())
            tight[1] += diff.numel()
            assert bad == 0, (bad, err, mode, task, Hq, Hkv, prompt, i, len(slots))
        steps += 1
    r.step_hook = checked
    r.run(tpl, task, prompt, gen, max_rows=512)
    runs += 1
if BF16:
    print(f"fuzz bf16 ok: {runs} replays, {steps} checked steps, every element within the a-priori bound (worst err / bound {worst:.3f})")
    sys.exit(0)
print(f"fuzz ok: {runs} replays, {steps} checked steps, worst |err| {worst:.2e}; {tight[0]} of {tight[1]} elements beyond 5e-4 + half an fp16 ulp (none beyond 1e-3 + half an ulp)")
