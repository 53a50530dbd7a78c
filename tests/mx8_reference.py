"""CPU oracle of the MXFP8 operand format (compute="mxfp8"; kernels.h 'MXFP8 operands', DESIGN.md §3 'MXFP8 GEMMs').

OCP MX: a block of 32 consecutive K elements shares one E8M0 scale byte s (value 2^(s - 127)); the elements are
e4m3fn. The engine's rule, in integers: amax = the block's largest |v| as fp32 bits, s = clamp(E - 8 + (m > 0x600000),
0, 254) with E / m the exponent / mantissa fields of amax, element = RNE e4m3fn of v 2^(127 - s); a non-finite v gives
0x7F. The elements here go through torch's own float8_e4m3fn conversion, so the library's integer conversion is
checked against an independent one."""

from __future__ import annotations

import math

import torch

E4M3_MAX = 448.0
NAN_BYTE = 0x7F


def scale_byte(amax_bits: torch.Tensor) -> torch.Tensor:
    """The integer rule on fp32 bit patterns of |amax| (int64 tensor)."""
    E = (amax_bits >> 23) & 0xFF
    m = amax_bits & 0x7FFFFF
    return (E - 8 + (m > 0x600000).to(torch.int64)).clamp(0, 254)


def ceil_log2_byte(amax: float) -> int:
    """127 + ceil(log2(amax / 448)) clamped to [0, 254], in exact arithmetic (frexp; amax finite, >= 0)."""
    if amax == 0.0:
        return 0
    fr, ex = math.frexp(amax / E4M3_MAX)  # amax / 448 = fr 2^ex, 0.5 <= fr < 1; the division by 448 = 7 * 64 is NOT
    # exact in binary, so decide the power-of-two boundary on integers instead: amax <= 448 2^k  <=>  amax / 2^k <= 448
    k = ex - 1 if fr == 0.5 else ex
    while math.ldexp(E4M3_MAX, k) < amax:
        k += 1
    while math.ldexp(E4M3_MAX, k - 1) >= amax:
        k -= 1
    return min(max(127 + k, 0), 254)


def quantize(x: torch.Tensor):
    """x [M, K] (any float dtype; the values are taken as fp32), K % 32 == 0 -> (q [M, K] uint8, s [M, K / 32] uint8)."""
    M, K = x.shape
    assert K % 32 == 0
    xf = x.detach().to("cpu", torch.float32).contiguous().view(M, K // 32, 32)
    bits = xf.view(torch.int32).to(torch.int64) & 0x7FFFFFFF
    s = scale_byte(bits.amax(dim=-1))
    mult = torch.ldexp(torch.ones((), dtype=torch.float32), (127 - s).to(torch.int32))[..., None]
    q = (xf * mult).to(torch.float8_e4m3fn).view(torch.uint8)
    q = torch.where(torch.isfinite(xf), q, torch.full_like(q, NAN_BYTE))
    return q.reshape(M, K).contiguous(), s.to(torch.uint8).contiguous()


def dequantize(q: torch.Tensor, s: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """The values the scaled MFMA multiplies: e4m3fn(q) 2^(s - 127), exactly (float64)."""
    M, K = q.shape
    v = q.cpu().contiguous().view(torch.float8_e4m3fn).to(torch.float64).view(M, K // 32, 32)
    sc = torch.ldexp(torch.ones((), dtype=torch.float64), s.cpu().to(torch.int32) - 127)[..., None]
    return (v * sc).reshape(M, K).to(dtype)


def block_cases():
    """Blocks of 32 fp32 values for the rule's sweep: amax = 448 2^k and its next float up over the exponent range,
    fp32 subnormals, a zero block, a NaN and an inf. Every element is a bf16 value (what the quantisers read), except
    where the next float up is wanted (host rule only)."""
    g = torch.Generator().manual_seed(5)
    out = []
    for k in list(range(-134, -118)) + list(range(-40, 41, 5)) + list(range(112, 120)):
        for up in (False, True):
            amax = torch.tensor(math.ldexp(E4M3_MAX, k), dtype=torch.float32)
            if not bool(torch.isfinite(amax)) or float(amax) == 0.0:
                continue
            if up:
                amax = torch.nextafter(amax, torch.tensor(float("inf")))
                if not bool(torch.isfinite(amax)):
                    continue
            blk = (torch.rand(32, generator=g) * 2 - 1) * amax
            blk[int(torch.randint(0, 32, (1,), generator=g))] = amax * (1 if k % 2 else -1)
            out.append(blk.to(torch.float32))
    out.append(torch.zeros(32))
    sub = torch.zeros(32)
    sub[3], sub[17] = 1e-41, -3e-42
    out.append(sub)
    return out
