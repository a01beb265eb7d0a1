"""What the bfloat16 tests share: the a-priori error bound of the kernels' arithmetic, the reference's arithmetic as a yardstick for the
statistical tripwire, dyadic data that is exact in bf16, and the bf16 forms of the exact-visibility oracle (tests/oracles.py is
fp16-specific: its values are multiples of 2^-9 and its ulp is fp16's).

The bound, per output element e of query row r and head h, with p the fp64 softmax weights of that row and head:

    o_e = sum_i p_i v_ie        A_e = sum_i p_i |v_ie|        tol_e = u A_e + 2 u |o_e| + 2e-5,   u = 2^-8

  * scores and exponentials are fp32: the 2e-5 (covers |score| up to ~40);
  * each probability is rounded ONCE, to nearest even, to bf16 (relative error <= u), and the weights are normalised by the sum of
    the ROUNDED values: the output moves by at most u (A_e + |o_e|);
  * fp32 partials and the LSE merge add nothing visible; the single final rounding adds at most u |o_e|.

It is derived, not tuned: a kernel that exceeds it rounds twice or normalises by the wrong sum.  The tripwire is tighter for the typical
element: the kernel's RMS error against fp64 is at most RMS_FACTOR x that of the reference's arithmetic (fp32 softmax attention over
the same bf16 tensors, rounded once) on the same inputs; a CPU model of the kernel predicts 1.0-1.4."""
from __future__ import annotations

import torch

from tools.error_bound import U_BF16 as U, bound_bf16 as bound, dense_attention  # noqa: F401  (re-exported)
from truth import tree_truth

FLOOR = 2.0 ** -20
RMS_FACTOR = 2.0
BF16 = torch.bfloat16


def report(line: str) -> None:
    """Figures are printed before anything is asserted (`pytest -s` shows them: profiles/bf16_error.txt is made from those lines)."""
    print(line, flush=True)


def check_against_truth(out, q, k_buf, v_buf, leaf_paths, Hq, Hkv, scale, tag, tripwire: bool = True):
    """Every element of `out` (bf16 [nq, Hq * D] or [nq, Hq, D]) within the bound of the fp64 truth over the same bf16 tensors, and
    (randn cases) the RMS tripwire.  Returns (max err / tol, RMS ratio)."""
    assert out.dtype == BF16 and k_buf.dtype == BF16 and q.dtype == BF16, (out.dtype, k_buf.dtype, q.dtype)
    o = tree_truth(q, k_buf, v_buf, leaf_paths, Hq, Hkv, scale)  # the yardstick; A comes with a second evaluation
    o2, A = dense_attention(q, k_buf, v_buf, leaf_paths, Hq, Hkv, scale, torch.float64, with_abs=True)
    assert float((o2 - o).abs().max()) < 1e-12, tag
    got = out.reshape(o.shape).to(torch.float64)
    assert bool(torch.isfinite(got).all()), (tag, "non-finite output")
    err = (got - o).abs()
    worst = float((err / bound(o, A)).max())
    rms = float(err.pow(2).mean().sqrt())
    ratio = float("nan")
    if tripwire:
        ref = dense_attention(q, k_buf, v_buf, leaf_paths, Hq, Hkv, scale, torch.float32).to(BF16).to(torch.float64)
        rms_ref = float((ref - o).abs().pow(2).mean().sqrt())
        ratio = rms / rms_ref
    report(f"bf16 {tag}: max err/tol {worst:.3f}  rms {rms:.3e}  rms / reference arithmetic {ratio:.3f}  ({o.numel()} elements)")
    assert worst <= 1.0, f"{tag}: an element is {worst:.3f} x its a-priori bound"
    if tripwire:
        assert ratio <= RMS_FACTOR, f"{tag}: RMS error {ratio:.3f} x the reference arithmetic's (limit {RMS_FACTOR})"
    return worst, ratio


# ---- trees -------------------------------------------------------------------------------------------------------------------
def few_shot_tree(prefix: int, width: int, branch_len: int, Hkv: int, D: int, layers: int = 1, reserve: int = 0, extra: int = 256,
                  dtype=BF16):
    """oracles.few_shot_tree with a bf16 pool.  Returns (tree, pool, reserved slots)."""
    from deft_amd.memory_pool import ReqToTokenPool, TokenToKVPool
    from deft_amd.tree_cache import TreeCache

    size = reserve + prefix + width * branch_len + extra
    req = ReqToTokenPool(max(width, 64) + 8, size + 8, device="cuda")
    pool = TokenToKVPool(size, dtype, Hkv, D, layers, device="cuda")
    reserved = pool.alloc(reserve).cpu() if reserve else torch.zeros(0, dtype=torch.int32)
    tree = TreeCache(dtype, Hkv, D, layers, req, pool, None, True, False)
    tree.init_prompt(torch.arange(1, prefix + 1, dtype=torch.int32))
    tree.branch(tree.root, width)
    for _ in range(branch_len):
        for leaf in list(tree.leaves.values()):
            leaf.append_token(7)
        tree.alloc()
    return tree, pool, reserved


# ---- exact visibility in bf16 ----------------------------------------------------------------------------------------------------
def dyadic_bf16_(t: torch.Tensor, generator: torch.Generator) -> torch.Tensor:
    """Fill `t` in place with the sum of three uniform integers in [-32, 32] times 2^-5: std ~1, |x| <= 3, multiples of 2^-5 below 8
    -- 8 significant bits, exact in bf16 (oracles.dyadic_'s 2^-9 grid is not)."""
    acc = torch.zeros(t.shape, dtype=torch.int32, device=t.device)
    for _ in range(3):
        acc += torch.randint(-32, 33, t.shape, dtype=torch.int32, device=t.device, generator=generator)
    t.copy_(acc.to(torch.float32) / 32.0)
    assert torch.equal(t.to(torch.float32) * 32.0, acc.to(torch.float32)), "not exact in this dtype"
    return t


def visibility_pool_bf16(pool, generator: torch.Generator) -> None:
    """K = 0 on every slot of every layer, V dyadic on the bf16 grid."""
    st = pool._storage
    st[:, :, 0].zero_()
    for l in range(st.shape[0]):
        dyadic_bf16_(st[l, :, 1], generator)


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp at |x| (fp64): 2^(e - 7) for |x| in [2^e, 2^(e+1)); the smallest normal binade below 2^-126."""
    a = x.to(torch.float64).abs().clamp_min(2.0 ** -126)
    _, ex = torch.frexp(a)  # a = m 2^ex, m in [0.5, 1)
    return torch.pow(2.0, (ex - 8).to(torch.float64))


def tolerance_bf16(expected: torch.Tensor) -> torch.Tensor:
    return bf16_ulp(expected) + FLOOR


def assert_visible_mean_bf16(out: torch.Tensor, expected: torch.Tensor, tag=None) -> float:
    e = expected.reshape(expected.shape[0], -1)
    o = out.reshape(e.shape).to(torch.float64)
    assert bool(torch.isfinite(o).all()), (tag, "non-finite output")
    err = (o - e).abs()
    worst = float((err / tolerance_bf16(e)).max())
    report(f"bf16 visible mean {tag}: max err / (ulp + 2^-20) {worst:.3f}")
    assert worst <= 1.0, f"{tag}: {int((err > tolerance_bf16(e)).sum())} elements off the visible mean by more than one bf16 ulp"
    return worst


def power_check_bf16(v_buf: torch.Tensor, paths, queries=(0,), need: float = 4.0) -> float:
    """oracles.power_check with the bf16 tolerance: dropping or doubling ONE key (the path's first, the one at the first tile boundary,
    the last) moves the visible mean by >= `need` x (one bf16 ulp + floor) in some element.  No kernel involved."""
    v2 = v_buf.reshape(v_buf.shape[0], -1)
    worst = float("inf")
    for r in queries:
        p = [int(s) for s in paths[r]]
        n = len(p)
        idx = torch.as_tensor(p, dtype=torch.int64, device=v2.device)
        total = v2[idx].to(torch.float64).sum(0)
        m = total / n
        for j in sorted({0, min(128, n - 1), n - 1}):
            vj = v2[p[j]].to(torch.float64)
            for moved in ([(total - vj) / (n - 1)] if n > 1 else []) + [(total + vj) / (n + 1)]:
                worst = min(worst, float(((moved - m).abs() / tolerance_bf16(m)).max()))
    assert worst >= need, f"the bf16 oracle cannot see one key at this size: factor {worst:.2f} < {need}"
    return worst
