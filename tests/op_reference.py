"""References for the op-level parity tests (tests/test_gpu_ops.py, tests/test_gpu_fold_ops.py,
tests/test_op_refs.py): plain torch
implementations of the operations behind the conv, norm and GEMM-epilogue kernels, written from the model
definitions (modules.py line numbers below are the reference model's; x_transformers for RMSNorm and the rotary
embedding), not from the kernels. Every function takes `dtype`: torch.float64 gives the reference R64,
torch.float32 the same formula in single precision, R32, whose distance from R64 is the yardstick of the
tolerance (`excess_ratio`). `variant` selects a deliberately wrong form (WRONG_* below): tests/test_op_refs.py
requires each of them to fail the tolerance on the inputs the GPU tests use.

Inputs are the values the kernel reads: what a kernel reads in the operand dtype is rounded by the caller first
(`rnd`). The references never round; the rounding of a stored 16-bit output is the `u_out` term of the tolerance.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

OP_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# unit roundoff of a stored output (round to nearest): half an ulp relative to the value
U_OUT = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
ACC_FACTOR = 8.0  # accumulation-order allowance on max|R32 - R64| (MFMA k-slabs, wave reductions)


def rnd(t, compute):
    """The fp32 values of t after rounding to compute's operand dtype (what a kernel reads from a 16-bit buffer)."""
    return None if t is None else t.to(OP_DTYPE[compute]).float()


def excess_ratio(out, r64, r32, u_out, extra=None):
    """max(|out - R64| - u_out |R64| - extra) / max|R32 - R64|: the elementwise tolerance |out - R64| <= u_out |R64|
    + extra + ACC_FACTOR max|R32 - R64| holds iff this is <= ACC_FACTOR. `extra`: an elementwise allowance derived
    next to the case that uses it (None: 0). A non-finite `out` gives inf; when R32 == R64 exactly (all-zero
    outputs) any positive excess gives inf."""
    out, r64 = out.double(), r64.double()
    if not bool(torch.isfinite(out).all()):
        return math.inf
    acc = float((r32.double() - r64).abs().max())
    exc = (out - r64).abs() - u_out * r64.abs()
    if extra is not None:
        exc = exc - extra.double()
    exc = float(exc.max())
    if acc == 0.0:
        return 0.0 if exc <= 0.0 else math.inf
    return exc / acc


def assert_close(out, r64, r32, u_out, what, factor=ACC_FACTOR, extra=None):
    """Assert the tolerance; `what` = "op/compute/case". Prints the measured ratio before asserting (pytest -s:
    the table in tests/test_gpu_ops.py is the worst of these lines per op and compute mode)."""
    ratio = excess_ratio(out, r64, r32, u_out, extra)
    acc = float((r32.double() - r64.double()).abs().max())
    print(f"[op-parity] {what}: ratio {ratio:.3f} (max|R32-R64| {acc:.3e})")
    assert ratio <= factor, (f"{what}: max(|out - R64| - u_out|R64|) / max|R32 - R64| = {ratio:.4g} > {factor} "
                             f"(max|R32 - R64| = {acc:.3e}, u_out = {u_out:.3e})")
    return ratio


# ---------------------------------------------------------------- ConvPositionEmbedding layer (modules.py:175-201)
WRONG_CONV = ("taps30", "shifted_centre", "keep_ignored_on_input", "halo_from_neighbour", "no_masked_row_zero")


def conv_pos(x, w, bias, keep=None, resid=None, dtype=torch.float64, variant=None):
    """y = mish(where(keep, conv(where(keep, x, 0)) + bias, 0)) [+ resid]: Conv1d(d, d, 31, groups=16, padding=15)
    over time per sequence (modules.py:180), the mask on its input and output (:193, :197), nn.Mish (:181).
    x [S,L,d], w [d, d/16, 31], keep [S,L] bool or None, resid [S,L,d] or None."""
    S, L, d = x.shape
    xx, w, bias = x.to(dtype), w.to(dtype), bias.to(dtype)
    k3 = None if keep is None else keep.bool()[..., None]
    if k3 is not None and variant != "keep_ignored_on_input":
        xx = torch.where(k3, xx, torch.zeros((), dtype=dtype))
    xt = xx.transpose(1, 2)  # [S, d, L]
    if variant == "halo_from_neighbour":  # one long sequence: the 15-row halo crosses the sequence seams
        xt = xx.reshape(1, S * L, d).transpose(1, 2)
    if variant == "taps30":
        y = F.conv1d(xt, w[..., :30], bias, padding=15, groups=16)[..., :xt.shape[-1]]
    elif variant == "shifted_centre":
        y = F.conv1d(F.pad(xt, (16, 14)), w, bias, groups=16)
    else:
        y = F.conv1d(xt, w, bias, padding=15, groups=16)
    y = y.transpose(1, 2).reshape(S, L, d)
    if k3 is not None and variant != "no_masked_row_zero":
        y = torch.where(k3, y, torch.zeros((), dtype=dtype))
    y = F.mish(y)
    return y if resid is None else y + resid.to(dtype)


# ---------------------------------------------------------------- row norms
WRONG_LN = ("eps_1e-5", "unbiased_variance")
WRONG_RMS = ("no_sqrt_d",)


def _layer_norm(x, eps, variant):
    mean = x.mean(-1, keepdim=True)
    var = x.var(-1, keepdim=True, unbiased=(variant == "unbiased_variance"))
    return (x - mean) / torch.sqrt(var + (1e-5 if variant == "eps_1e-5" else eps))


def ln_modulate(h, shift, scale, dtype=torch.float64, variant=None):
    """AdaLayerNorm / AdaLayerNorm_Final (modules.py:319, 325, 340, 346): LayerNorm(d, no affine, eps 1e-6)(h) *
    (1 + scale) + shift. h [M,d]; shift, scale [d]."""
    return _layer_norm(h.to(dtype), 1e-6, variant) * (1 + scale.to(dtype)) + shift.to(dtype)


def rms_norm(h, g, dtype=torch.float64, variant=None):
    """x_transformers RMSNorm: F.normalize(x, dim=-1) * dim ** 0.5 * g, F.normalize dividing by max(|x|_2, 1e-12)."""
    h = h.to(dtype)
    n = h / h.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return n * g.to(dtype) * (1.0 if variant == "no_sqrt_d" else h.shape[-1] ** 0.5)


def dwconv_ln(x, dw_w, dw_b, ln_w, ln_b, dtype=torch.float64, variant=None):
    """ConvNeXtV2Block front half (modules.py:261-264, 272-275): depthwise Conv1d(C, C, 7, padding=3, groups=C) over
    time, then LayerNorm(C, eps 1e-6) with affine. x [S,L,C], dw_w [C,7]."""
    C = x.shape[-1]
    y = F.conv1d(x.to(dtype).transpose(1, 2), dw_w.to(dtype)[:, None, :], dw_b.to(dtype), padding=3, groups=C)
    return _layer_norm(y.transpose(1, 2), 1e-6, variant) * ln_w.to(dtype) + ln_b.to(dtype)


WRONG_GRN = ("norm_over_channels",)


def grn(x, gamma, beta, dtype=torch.float64, variant=None):
    """GRN (modules.py:242-245): Gx = |x|_2 over time (dim 1), Nx = Gx / (mean over channels of Gx + 1e-6),
    gamma (x Nx) + beta + x. x [S,L,C]."""
    x = x.to(dtype)
    if variant == "norm_over_channels":
        Gx = torch.norm(x, p=2, dim=2, keepdim=True)
        Nx = Gx / (Gx.mean(dim=1, keepdim=True) + 1e-6)
    else:
        Gx = torch.norm(x, p=2, dim=1, keepdim=True)
        Nx = Gx / (Gx.mean(dim=-1, keepdim=True) + 1e-6)
    return gamma.to(dtype) * (x * Nx) + beta.to(dtype) + x


# ---------------------------------------------------------------- GEMM epilogues
WRONG_GEMM = {"gelu_tanh": ("gelu_erf_for_tanh",), "resid": ("gate_on_residual",), "resid16": ("gate_on_residual",),
              "resid_fill": ("fill_keeps_c",), "qkv": ("rope_half_split", "rope_on_every_head", "q_unscaled")}


def rope_table(L, dtype=torch.float64):
    """x_transformers RotaryEmbedding(64): inv_freq_j = 10000^(-2j/64), (cos, sin)(n inv_freq_j), [L,32,2]."""
    inv = 1.0 / (10000.0 ** (torch.arange(0, 64, 2, dtype=dtype) / 64.0))
    f = torch.arange(L, dtype=dtype)[:, None] * inv[None, :]
    return torch.stack((torch.cos(f), torch.sin(f)), dim=-1)


def _rope(t, cos, sin, variant):
    """x_transformers apply_rotary_pos_emb with rotate_half on interleaved pairs (x_{2i}, x_{2i+1}): t cos +
    rotate_half(t) sin, the pair's frequency repeated. t [S,L,H,64]; cos, sin [L,32]."""
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    if variant == "rope_half_split":  # pairs (x_i, x_{i+32}) instead
        a, b = t[..., :32], t[..., 32:]
        return torch.cat((a * c - b * s, b * c + a * s), dim=-1)
    a, b = t[..., 0::2], t[..., 1::2]
    return torch.stack((a * c - b * s, b * c + a * s), dim=-1).flatten(-2)


def gemm_epi(epi, A, W, bias=None, C=None, resid=None, gate=None, keep=None, add=None, dual_rows=0, seq_len=0,
             heads=0, rope_heads=0, q_scale=0.0, rope=None, dtype=torch.float64, variant=None, pre=None):
    """acc = A W^T + bias, then the epilogue (kernels.h `Epi`; the model lines they stand for):
    store / store16: acc. silu: SiLU (modules.py:857). gelu_tanh: nn.GELU(approximate="tanh") (:358). gelu_erf /
    gelu_erf_op: nn.GELU() (:266). resid / resid16: x + gate * masked_fill(sub-layer output, ~mask, 0)
    (:551-554, 755-757): where(keep, R + gate acc, R), R = resid if given else C. resid_fill: residual + x then
    masked_fill(~mask, 0) of the ConvNeXt text blocks: where(keep, C + acc, 0). inproj: the split input projection,
    C[m] = acc + add[m] and, with dual_rows, C[m + dual_rows] = acc + add[m + dual_rows]. qkv: to_q / to_k / to_v
    columns [q | k | v], heads of 64; rotary embedding on the first rope_heads heads (0: all) of q and k at position
    m % seq_len from `rope` [L,32,2] (cos, sin), q times q_scale (0: unscaled); returns q, k, v [S,H,L,64].
    pre [M,N]: stands for acc + bias (fold_consumer: the epilogue applied to the normalised pre-activation)."""
    if pre is not None:
        acc = pre.to(dtype)
    else:
        acc = A.to(dtype) @ W.to(dtype).t()
        if bias is not None:
            acc = acc + bias.to(dtype)
    M, N = acc.shape
    kp = None if keep is None else keep.bool()[:, None]
    if epi in ("store", "store16"):
        return acc
    if epi == "silu":
        return F.silu(acc)
    if epi == "gelu_tanh":
        return F.gelu(acc) if variant == "gelu_erf_for_tanh" else F.gelu(acc, approximate="tanh")
    if epi in ("gelu_erf", "gelu_erf_op"):
        return F.gelu(acc)
    if epi in ("resid", "resid16"):
        R = (C if resid is None else resid).to(dtype)
        gt = torch.ones(N, dtype=dtype) if gate is None else gate.to(dtype)
        upd = gt * (R + acc) if variant == "gate_on_residual" else R + gt * acc
        return upd if kp is None else torch.where(kp, upd, R)
    if epi == "resid_fill":
        Cd = C.to(dtype)
        upd = Cd + acc
        if kp is None:
            return upd
        return torch.where(kp, upd, Cd if variant == "fill_keeps_c" else torch.zeros((), dtype=dtype))
    if epi == "inproj":
        ad = add.to(dtype)
        out = acc + ad[:M, :N]
        return out if not dual_rows else torch.cat((out, torch.full((dual_rows - M, N), float("nan"), dtype=dtype),
                                                    acc + ad[dual_rows:dual_rows + M, :N]))
    assert epi == "qkv"
    S, inner = M // seq_len, heads * 64
    q, k, v = (acc[:, i * inner:(i + 1) * inner].reshape(S, seq_len, heads, 64) for i in range(3))
    cos, sin = rope[..., 0].to(dtype), rope[..., 1].to(dtype)
    nrope = heads if (rope_heads == 0 or variant == "rope_on_every_head") else rope_heads
    q = torch.cat((_rope(q[:, :, :nrope], cos, sin, variant), q[:, :, nrope:]), dim=2)
    k = torch.cat((_rope(k[:, :, :nrope], cos, sin, variant), k[:, :, nrope:]), dim=2)
    if q_scale != 0.0 and variant != "q_unscaled":
        q = q * q_scale
    return tuple(t.permute(0, 2, 1, 3).contiguous() for t in (q, k, v))


# ---------------------------------------------------------------- attention
def attention(Q, K, V, kv_len=None, dtype=torch.float64, log2_scores=False):
    """softmax(Q K^T / sqrt(64) + key mask) V, [S,H,N,64] -> [S,N,H*64] (F.scaled_dot_product_attention in the
    AttnProcessor, modules.py:470-555). log2_scores: Q already carries log2(e) / sqrt(64) (the engine's layout), so
    the softmax is 2^s / sum 2^s of s = Q K^T. Returns (O, sqrt(P^2 . V^2), sqrt(sum_k P^2)): the last two are the
    scales of the error that rounding the probabilities P leaves in the numerator and in the row sum."""
    S, H, N, _ = Q.shape
    sc = Q.to(dtype) @ K.to(dtype).transpose(-1, -2)
    if not log2_scores:
        sc = sc / 8.0
    if kv_len is not None:
        dead = torch.arange(N)[None, :] >= kv_len.long()[:, None]
        sc = sc.masked_fill(dead[:, None, None, :], float("-inf"))
    p = torch.exp2(sc - sc.amax(-1, keepdim=True)) if log2_scores else torch.softmax(sc, dim=-1)
    p = p / p.sum(-1, keepdim=True)
    Vd = V.to(dtype)
    fold = lambda t: t.transpose(1, 2).reshape(S, N, H * 64)  # noqa: E731
    return (fold(p @ Vd), fold(torch.sqrt(p.square() @ Vd.square())),
            fold(torch.sqrt(p.square().sum(-1, keepdim=True)).expand(S, H, N, 64)))


# ---------------------------------------------------------------- LayerNorm / RMSNorm fold
# The fold replaces aop = LN(h') (1 + sc) + sh followed by aop W^T + b with algebra inside two GEMMs:
#   producer: hs = round(h' (1 + sc)) and per 64-column strip p of every row the (mean m_p, M2 q_p) of h';
#   consumer: mean = mean_p m_p, M2 = sum_p q_p + 64 sum_p (m_p - mean)^2, rstd = 1 / sqrt(M2 / d + eps),
#             x = rstd (hs W^T - mean u) + v + b with u = sum_k (1 + sc_k) W[n,k], v = sum_k sh_k W[n,k].
# RMSNorm form: strips hold (0, sum of squares), no hs, u = v = 0, W' = round(W diag(g)), eps 1e-30.
def strip_stats(h, dtype=torch.float64, rms=False):
    """[M,d] -> [M, d/64, 2]: (mean, M2 = sum (x - mean)^2) of each 64-column strip, two passes. rms: (0, sum x^2)."""
    M, d = h.shape
    x = h.to(dtype).reshape(M, d // 64, 64)
    mean = torch.zeros(M, d // 64, dtype=dtype) if rms else x.mean(-1)
    return torch.stack((mean, (x - mean[..., None]).square().sum(-1)), dim=-1)


WRONG_HS = ("sc_for_one_plus_sc",)


def fold_hs(hp, scale, compute, variant=None):
    """The producer's hs, to the bit: one fp32 multiply of the stored h' by the fp32 (1 + scale), one rounding."""
    f = scale.float() if variant == "sc_for_one_plus_sc" else 1.0 + scale.float()
    return rnd(hp.float() * f, compute)


WRONG_COMBINE_LN = ("no_between_strip_term", "stale_13th_partial", "unbiased_variance", "eps_1e-5")
WRONG_COMBINE_RMS = ("rms_over_16_strips",)
WRONG_CONSUMER = ("mean_u_dropped", "v_before_rstd")
WRONG_CONSUMER_QKV = ("fold_not_on_v",)


def fold_combine(parts, eps, dtype=torch.float64, variant=None):
    """Strip partials [M,np,2] -> the row's (mean, rstd), [M,1] each, as DESIGN.md §3 states it."""
    p = parts.to(dtype)
    m, q = p[..., 0], p[..., 1]
    M, np_ = m.shape
    d = 64 * np_
    mean = m.mean(-1, keepdim=True)
    m2 = q.sum(-1, keepdim=True)
    if variant != "no_between_strip_term":
        m2 = m2 + 64 * (m - mean).square().sum(-1, keepdim=True)
    if variant == "stale_13th_partial" and np_ == 12:  # the slot after the row's 12: the next row's first partial
        sm, sq = torch.zeros(M, 1, dtype=dtype), torch.zeros(M, 1, dtype=dtype)
        sm[:-1, 0], sq[:-1, 0] = m[1:, 0], q[1:, 0]
        m2 = m2 + sq + 64 * (sm - mean).square()
    div = d - 1 if variant == "unbiased_variance" else (64 * 16 if variant == "rms_over_16_strips" else d)
    return mean, 1.0 / torch.sqrt(m2 / div + (1e-5 if variant == "eps_1e-5" else eps))


def fold_consumer(epi, A, W, bias, parts, u, v, eps, dtype=torch.float64, variant=None, **epi_kw):
    """The fold consumer: x = rstd (A W^T - mean u) + v + bias, then GELU-tanh ("gelu_tanh") or RoPE / q scale /
    scatter ("qkv"; epi_kw as gemm_epi). u, v None: 0 (the RMSNorm form)."""
    acc = A.to(dtype) @ W.to(dtype).t()
    mean, rstd = fold_combine(parts, eps, dtype, variant)
    ud = torch.zeros((), dtype=dtype) if u is None else u.to(dtype)
    vd = torch.zeros((), dtype=dtype) if v is None else v.to(dtype)
    if variant == "mean_u_dropped":
        x = rstd * acc + vd
    elif variant == "v_before_rstd":
        x = rstd * (acc - mean * ud + vd)
    else:
        x = rstd * (acc - mean * ud) + vd
    if variant == "fold_not_on_v":
        n3 = acc.shape[1] // 3
        x = torch.cat((x[:, :2 * n3], acc[:, 2 * n3:]), dim=1)
    return gemm_epi(epi, None, None, pre=x + bias.to(dtype), dtype=dtype, **epi_kw)


WRONG_LNFOLD_UV = ("u_from_sc", "lo_part_dropped", "msa_rows_for_ffn1")


def lnfold_uv(mod, W1, Wqkv, dtype=torch.float64, variant=None, compute=None):
    """mod [nfe, depth, 6, d]: a step's AdaLN rows per layer (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp,
    gate_mlp; modules.py:321-323). W1 [depth,F,d], Wqkv [depth,3d,d] as the kernel reads them (rounded). Returns
    (u1, v1 [nfe,depth,F], u2, v2 [nfe,depth,3d]): u = sum_k (1 + sc_k) W[n,k], v = sum_k sh_k W[n,k], FFN1 from the
    mlp rows and QKV from the msa rows. lo_part_dropped: (1 + sc) and sh rounded to `compute`'s operand dtype."""
    mod = mod.to(dtype)
    sh_ff, sc_ff = (mod[:, :, 0], mod[:, :, 1]) if variant == "msa_rows_for_ffn1" else (mod[:, :, 3], mod[:, :, 4])
    sh_at, sc_at = mod[:, :, 0], mod[:, :, 1]
    one = 0.0 if variant == "u_from_sc" else 1.0
    cut = (lambda t: rnd(t.float(), compute).to(dtype)) if variant == "lo_part_dropped" else (lambda t: t)
    mm = lambda x, w: torch.einsum("sld,lnd->sln", cut(x), w.to(dtype))  # noqa: E731
    return mm(one + sc_ff, W1), mm(sh_ff, W1), mm(one + sc_at, Wqkv), mm(sh_at, Wqkv)


def lnfold_uv_extra(mod, W1, Wqkv, compute):
    """The split allowance of lnfold_uv's outputs (derived in tests/test_gpu_fold_ops.py::test_lnfold_uv), in the
    order of lnfold_uv's results: 6 (u_op^2 / sqrt 3) sqrt(sum_k (x_k W_nk)^2), plus for fp16 the subnormal spacing of
    the lo part 6 (2^-25 / sqrt 3) sqrt(sum_k W_nk^2)."""
    mod = mod.double()
    u_op = U_OUT[compute]
    out = []
    for x, w in ((1.0 + mod[:, :, 4], W1), (mod[:, :, 3], W1), (1.0 + mod[:, :, 1], Wqkv), (mod[:, :, 0], Wqkv)):
        w2 = w.double().square()
        e = 6 * u_op ** 2 / 3 ** 0.5 * torch.sqrt(torch.einsum("sld,lnd->sln", x.square(), w2))
        if compute == "fp16":
            e = e + 6 * 2.0 ** -25 / 3 ** 0.5 * torch.sqrt(w2.sum(-1))[None]
        out.append(e)
    return out


WRONG_SCALE_COLS = ("g_by_row",)


def scale_cols(W_read, g, compute, variant=None):
    """round(W g[None, :]) of the rounded W, to the bit: one fp32 multiply, one rounding."""
    gf = g.float()
    if variant == "g_by_row":
        return rnd(W_read.float() * gf[torch.arange(W_read.shape[0]) % gf.numel()][:, None], compute)
    return rnd(W_read.float() * gf[None, :], compute)


# ================================================================ audio glue, prologue and ODE step kernels
# (tests/test_gpu_glue_ops.py). Two kinds of reference. The gathers and the uncontracted fp32 step arithmetic have a
# float32 torch restatement the kernel must equal bit for bit; tests/test_op_refs.py ties each restatement to an
# independent definition (F.conv1d, torch.stft, the oracle's TextEmbedding, tests/ode_reference.py). The kernels with
# transcendental functions or sums have R64 / R32 forms and WRONG_* variants as above.
def assert_close_special(out, r64, r32, u_out, what):
    """assert_close for references with NaN or +-inf elements: there `out` must hold the same special value; the
    tolerance is asserted over the finite elements (the special ones count as exact zeros on every side)."""
    out, r64, r32 = out.double(), r64.double(), r32.double()
    assert torch.equal(torch.isnan(out), torch.isnan(r64)), f"{what}: NaN where the reference has none, or lost"
    inf = torch.isinf(r64)
    assert torch.equal(out[inf], r64[inf]), f"{what}: +-inf of the reference not reproduced"
    sp = ~torch.isfinite(r64)
    z = lambda t: torch.where(sp, torch.zeros((), dtype=t.dtype), t)  # noqa: E731
    return assert_close(z(out), z(r64), z(r32), u_out, what)


def same_specials(a, b):
    """NaN and +-inf in the same places with the same signs."""
    sa, sb = ~torch.isfinite(a), ~torch.isfinite(b)
    return torch.equal(sa, sb) and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(a[sa & ~torch.isnan(a)].double(), b[sb & ~torch.isnan(b)].double())


# ---------------------------------------------------------------- bitwise restatements: gathers
def mel_frames(wav, n_fft, hop):
    """torch.stft(center=True, pad_mode="reflect")'s framing: wav [B, L] -> [B, 1 + L // hop, n_fft]."""
    padded = F.pad(wav[:, None, :], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
    return padded.unfold(-1, n_fft, hop).contiguous()


def im2col7(mel, Kp, compute="fp32"):
    """Conv1d(k 7, pad 3)'s im2col: mel [B, C, T] -> [B * T, Kp], column 7 c + j = mel[b, c, t + j - 3], zero taps
    outside [0, T) and zero columns from 7 C on; rounded to the operand dtype."""
    B, C, T = mel.shape
    cols = F.pad(mel, (3, 3)).unfold(-1, 7, 1).permute(0, 2, 1, 3).reshape(B * T, C * 7)
    return F.pad(cols, (0, Kp - C * 7)).to(OP_DTYPE[compute])


def text_embed(text, table, N, seq_len=None, freqs=None, freq_rows=0, mask_padding=False):
    """TextEmbedding.forward for both CFG branches (dit.py:86-120; mmdit.py:42-63 for the position clamp): tokens + 1
    (filler 0), cut or padded to N, positions past the sample's seq_len dropped, the filler mask taken before
    drop_text, Embedding, + freqs_cis, masked_fill of filler rows (only with the extra modelling, i.e. with freqs).
    Returns (cond [B,N,td], uncond [B,N,td], keep [2,B,N] uint8: 0 where a filler row was zeroed)."""
    B = text.shape[0]
    tok = F.pad(text[:, :N] + 1, (0, max(0, N - text.shape[1])), value=0)
    valid = torch.ones(B, N, dtype=torch.bool) if seq_len is None else \
        torch.arange(N)[None, :] < torch.as_tensor(seq_len)[:, None]
    tok = tok.masked_fill(~valid, 0)
    fill = tok == 0
    zero = torch.zeros((), dtype=table.dtype)
    ec = torch.where(valid[..., None], table[tok], zero)
    eu = torch.where(valid[..., None], table[torch.zeros_like(tok)], zero)
    zero_row = torch.zeros(B, N, dtype=torch.bool)
    if freqs is not None:
        pos = torch.arange(N)
        if freq_rows:
            pos = pos.clamp(max=freq_rows - 1)
        f = torch.where(valid[..., None], freqs[pos][None], zero)
        ec, eu = ec + f, eu + f
        if mask_padding:
            zero_row = fill
            ec, eu = ec.masked_fill(fill[..., None], 0.0), eu.masked_fill(fill[..., None], 0.0)
    keep = (~zero_row).to(torch.uint8)
    return ec, eu, torch.stack((keep, keep))


def build_ct(cond, cond_mask, text_c, text_u, S, drop_audio=False, drop_text=False, compute="fp32"):
    """InputEmbedding's operand (dit.py:155-156, 347-350): per sequence s and frame [step_cond | 0 .. 128 | text |
    0 .. roundup(td, 64)]; step_cond = where(cond_mask, cond, 0) for the conditional sequences s < B unless
    drop_audio, zeros for the unconditional ones; text = the dropped-text embedding for s >= B or with drop_text."""
    B, N, mel = cond.shape
    td = text_c.shape[-1]
    out = torch.zeros(S, N, 128 + (td + 63) // 64 * 64)
    for s in range(S):
        b = s % B
        if s < B and not drop_audio:
            out[s, :, :mel] = torch.where(cond_mask[b].bool()[:, None], cond[b], torch.zeros(()))
        out[s, :, 128:128 + td] = (text_c if (s < B and not drop_text) else text_u)[b]
    return out.reshape(S * N, -1).to(OP_DTYPE[compute])


def pack_y(y, compute="fp32"):
    return F.pad(y, (0, 128 - y.shape[-1])).to(OP_DTYPE[compute])


def masks(kind, src, S, L=0, off=0):
    """build_rowkeep / build_kvlen from dur [B]; build_textkeep / build_textlen from text [B, nt] (-1 = filler)."""
    B = src.shape[0]
    idx = torch.arange(S) % B
    if kind == "build_rowkeep":
        pos = torch.arange(L)[None, :]
        return ((pos < off) | (pos - off < src[idx].long()[:, None])).to(torch.uint8)
    if kind == "build_kvlen":
        return (src[idx] + off).to(torch.int32)
    real = src[idx] != -1
    if kind == "build_textkeep":
        return real.to(torch.uint8)
    assert kind == "build_textlen"
    last = (real * (torch.arange(src.shape[1]) + 1)[None, :]).amax(-1)
    return last.to(torch.int32)


def final_where_out(cond, cond_mask, y, fault=None):
    """cfm.py:223: where(cond_mask, cond, y); NaN everywhere once the give-up word is set."""
    out = torch.where(cond_mask.bool()[..., None], cond, y)
    return torch.full_like(out, float("nan")) if fault else out


def copy_pred(p, row_off, mel, fault=None):
    out = p[:, row_off:, :mel].contiguous()
    return torch.full_like(out, float("nan")) if fault else out


# ---------------------------------------------------------------- bitwise restatements: CFG + ODE updates
def _f32s(v):
    return torch.tensor(float(v), dtype=torch.float32)


def cfg_slope(p, B, N, mel, row_off, use_cfg, cfg):
    """fn(t, x) = pred + (pred - null_pred) * cfg (cfm.py:190-191), fp32, one rounding per operation."""
    pc = p[:B, row_off:row_off + N, :mel]
    if not use_cfg:
        return pc.clone()
    return pc + (pc - p[B:2 * B, row_off:row_off + N, :mel]) * _f32s(cfg)


def grid_dt(grid, k):
    g = torch.tensor([float(v) for v in grid], dtype=torch.float32)
    return g[k + 1] - g[k]


def euler_update(y, v, dt):
    """torchdiffeq euler: y1 = y0 + dt * f."""
    return y + (_f32s(dt) if not torch.is_tensor(dt) else dt) * v


def rk_stage(method, s, y, v, dt, kbuf=None):
    """One evaluation of torchdiffeq's fixed-grid midpoint / rk4 (3/8 rule) in its written operation order. Returns
    (the next evaluation's input yn, the slopes kept so far): the final stage's yn is y1."""
    if method == "midpoint":
        return (y + v * (_f32s(0.5) * dt) if s == 0 else y + dt * v), kbuf
    c = _f32s(1.0 / 3.0)
    K = None if kbuf is None else kbuf.clone()
    if s == 0:
        yn = y + (dt * v) * c
    elif s == 1:
        yn = y + dt * (v - K[0] * c)
    elif s == 2:
        yn = y + dt * ((K[0] - K[1]) + v)
    else:
        yn = y + (((K[0] + _f32s(3.0) * (K[1] + K[2])) + v) * dt) * _f32s(0.125)
    if s < 3:
        K[s] = v
    return yn, K


def ypad_of(yn, compute):
    """The refreshed operand copy [B N, mel] (round to nearest even); the pad columns are not the update's."""
    return yn.reshape(-1, yn.shape[-1]).to(OP_DTYPE[compute])


# ---------------------------------------------------------------- R64 / R32 references
WRONG_MEL_MAG = ("power2",)
WRONG_MEL_LOG = ("clamp_1e-10", "log10")
WRONG_SPEC = ("no_clip", "sin_cos_swapped")
WRONG_OLA = ("window_not_squared", "first_frame_off_by_one", "no_trim")
WRONG_TIME_SINUS = ("cos_before_sin", "divisor_128", "scale_1")


def mel_mag(spec, bins, ld_mag, dtype=torch.float64, variant=None):
    """torchaudio Spectrogram(power=1): |X_k| of interleaved (re, im) rows; columns [bins, ld_mag) zero."""
    z = spec[:, :2 * bins].to(dtype).reshape(spec.shape[0], bins, 2)
    m = z[..., 0] * z[..., 0] + z[..., 1] * z[..., 1]
    if variant != "power2":
        m = torch.sqrt(m)
    return F.pad(m, (0, ld_mag - bins))


def mel_log(mel, frames, T_out=None, dtype=torch.float64, variant=None):
    """get_vocos_mel_spectrogram's tail (modules.py:107-108): mel.clamp(min=1e-5).log(). mel [sum frames, n_mels].
    T_out None: equal frame counts, returned channel-first [B, n_mels, T] as the reference returns it; else the
    frame-major zero-padded batch [B, T_out, n_mels] CFM.sample takes."""
    x = mel.to(dtype).clamp(min=1e-10 if variant == "clamp_1e-10" else 1e-5)
    x = torch.log10(x) if variant == "log10" else torch.log(x)
    if T_out is None:
        return x.reshape(len(frames), frames[0], -1).transpose(1, 2).contiguous()
    out = torch.zeros(len(frames), T_out, x.shape[-1], dtype=dtype)
    o = 0
    for s, t in enumerate(frames):
        out[s, :t] = x[o:o + t]
        o += t
    return out


def vocos_spec(x, bins, dtype=torch.float64, variant=None):
    """ISTFTHead.forward's pointwise part (vocos heads.py): mag = clip(exp(m), max=1e2), S = mag (cos p + i sin p),
    on columns (2k, 2k+1) = (m, p) of bin k; columns from 2 bins on zero."""
    z = x[:, :2 * bins].to(dtype).reshape(x.shape[0], bins, 2)
    mag = torch.exp(z[..., 0])
    if variant != "no_clip":
        mag = torch.clip(mag, max=1e2)
    c, s = torch.cos(z[..., 1]), torch.sin(z[..., 1])
    if variant == "sin_cos_swapped":
        c, s = s, c
    out = torch.stack((mag * c, mag * s), dim=-1).reshape(x.shape[0], 2 * bins)
    return F.pad(out, (0, x.shape[1] - 2 * bins))


def vocos_ola(frames, win, lens, hop, dtype=torch.float64, variant=None):
    """torch.istft(center=True)'s tail per utterance: overlap-add of the windowed frames over the overlap-added
    squared window, trimmed by n_fft / 2 at the front, (T - 1) hop samples. frames [sum lens, n_fft] packed; returns
    the utterances' samples back to back."""
    n_fft = frames.shape[1]
    fr, w = frames.to(dtype), win.to(dtype)
    wenv = w if variant == "window_not_squared" else w * w
    out, o = [], 0
    for T in lens:
        n = (T - 1) * hop + n_fft
        full, env = torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
        pos = torch.arange(n)
        first = torch.clamp((pos - n_fft + 1 + hop - 1).div(hop, rounding_mode="floor"), min=0)  # first covering frame
        for t in range(T):
            sl = slice(t * hop, t * hop + n_fft)
            use = torch.ones(n_fft, dtype=torch.bool) if variant != "first_frame_off_by_one" else first[sl] != t
            full[sl] += torch.where(use, fr[o + t], torch.zeros((), dtype=dtype))
            env[sl] += torch.where(use, wenv, torch.zeros((), dtype=dtype))
        lo = 0 if variant == "no_trim" else n_fft // 2
        out.append((full / env)[lo:lo + (T - 1) * hop])
        o += T
    return torch.cat(out)


def time_sinus(t, dtype=torch.float64, variant=None):
    """SinusPositionEmbedding(256) with scale 1000 (modules.py:157-169): emb = log(1e4) / (half - 1), x = scale t
    exp(-j emb), [sin x | cos x]."""
    half = 128
    k = math.log(10000) / (half if variant == "divisor_128" else half - 1)
    freq = torch.exp(torch.arange(half).to(dtype) * -k)
    e = (1.0 if variant == "scale_1" else 1000.0) * torch.as_tensor(t).to(dtype)[:, None] * freq[None, :]
    return torch.cat((e.cos(), e.sin()) if variant == "cos_before_sin" else (e.sin(), e.cos()), dim=-1)
