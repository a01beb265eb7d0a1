"""CPU model of an fp8 KV pool (OCP e4m3fn, torch.float8_e4m3fn): the quantisation rule of the append and the meaning of
a stored code.  torch / numpy only, any device.

    quantize(x, scale)   = RNE_e4m3fn(clamp(float32(x) / scale, -448, +448))   (fp32 division; without the clamp torch's cast gives NaN
                           above 448; NaN stays NaN: torch.clamp passes it and the cast makes 0x7F / 0xFF of it)
    dequantize(c, scale) = float64(c) * float64(scale)

`scale` is a python float or a tensor that broadcasts against x ([Hkv, 1] against [n, Hkv, D])."""
from __future__ import annotations

import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def quantize(x: torch.Tensor, scale=1.0) -> torch.Tensor:
    scale = torch.as_tensor(scale, dtype=torch.float32, device=x.device)
    return torch.clamp(x.to(torch.float32) / scale, -FP8_MAX, FP8_MAX).to(FP8)


def dequantize(codes: torch.Tensor, scale=1.0) -> torch.Tensor:
    assert codes.dtype == FP8, codes.dtype
    scale = torch.as_tensor(scale, device=codes.device).to(torch.float64)
    return codes.to(torch.float64) * scale


def all_codes(device="cpu") -> torch.Tensor:
    """The 256 codes in byte order, as float8_e4m3fn."""
    return torch.arange(256, dtype=torch.int32, device=device).to(torch.uint8).view(FP8)


def is_nan_code(codes: torch.Tensor) -> torch.Tensor:
    return (codes.view(torch.uint8) & 0x7F) == 0x7F


def same_codes(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit for bit, except that any NaN code equals any NaN code."""
    ab, bb = a.view(torch.uint8), b.view(torch.uint8)
    return a.shape == b.shape and bool(((ab == bb) | (is_nan_code(a) & is_nan_code(b))).all())


def code_values() -> torch.Tensor:
    """The 254 finite values by the format's definition (1 sign, 4 exponent bits with bias 7, 3 mantissa bits, subnormals, no
    infinities, NaN = S.1111.111), fp64, in byte order with NaN at 0x7F / 0xFF -- independent of torch's cast."""
    out = torch.empty(256, dtype=torch.float64)
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        out[c] = -v if s else v
    return out


def edge_inputs() -> torch.Tensor:
    """fp32 inputs that pin the quantisation rule (all exact in fp16 except 1e4's neighbours, which only need to clamp): every finite
    code's value, every midpoint between neighbouring codes (ties to even), +-448, +-464, +-1e4, the subnormal range (multiples of
    2^-10 up to 2^-6), +-0 and NaN."""
    vals = code_values()
    pos = vals[:127]  # 0 .. 448 ascending
    mids = (pos[:-1] + pos[1:]) / 2
    sub = torch.arange(0, 17, dtype=torch.float64) * 2.0 ** -10
    extra = torch.tensor([448.0, 464.0, 1e4, 0.0], dtype=torch.float64)
    x = torch.cat([vals[:127], vals[128:255], mids, -mids, sub, -sub, extra, -extra, torch.tensor([float("nan")], dtype=torch.float64)])
    return x.to(torch.float32)


def self_check() -> None:
    codes = all_codes()
    vals = code_values()
    finite = ~is_nan_code(codes)
    assert int(finite.sum()) == 254
    # torch's cast agrees with the format's definition, signed zeros included
    got = codes.to(torch.float64)
    assert torch.equal(got[finite], vals[finite]) and bool(torch.isnan(got[~finite]).all())
    assert bool((torch.signbit(got) == (torch.arange(256) >= 128))[finite].all())
    # all 254 finite codes round-trip, with unit and with other scales
    for scale in (1.0, 0.5, 0.0371, 1.9):
        x = (vals.to(torch.float32) * torch.tensor(scale, dtype=torch.float32))  # one fp32 rounding; the division undoes it or lands within a tie-free distance
        back = quantize(torch.where(finite, x, torch.zeros_like(x)), scale)
        assert same_codes(back[finite], codes[finite]), scale
    # e4m3 -> fp16 / bf16 is exact (3 mantissa bits, the range fits, subnormals included)
    for dt in (torch.float16, torch.bfloat16):
        conv = codes.to(dt).to(torch.float64)
        assert torch.equal(conv[finite], vals[finite]) and bool(torch.isnan(conv[~finite]).all()), dt
    # the rule at its edges: clamp, ties to even, subnormals, zeros, NaN
    q = lambda v: int(quantize(torch.tensor([v], dtype=torch.float32)).view(torch.uint8))  # noqa: E731
    assert q(448.0) == 0x7E and q(464.0) == 0x7E and q(1e4) == 0x7E and q(-1e4) == 0xFE and q(float("inf")) == 0x7E
    assert q(0.0) == 0x00 and q(-0.0) == 0x80 and (q(float("nan")) & 0x7F) == 0x7F
    assert q(2.0 ** -9) == 0x01 and q(2.0 ** -10) == 0x00 and q(3 * 2.0 ** -10) == 0x02  # ties go to the even code
    assert q(1.0625) == 0x38 and q(1.1875) == 0x3A  # 1 + 1/16 -> 1.0 (even), 1 + 3/16 -> 1.25 (even)
