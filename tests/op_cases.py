"""Seeded inputs of the op-level parity tests, shared by tests/test_gpu_ops.py (the kernels against the
references) and tests/test_op_refs.py (wrong variants of the references against the same tolerance on the same
inputs). Shapes are the smallest that reach each launcher branch and edge; every builder returns fp32 CPU tensors
already rounded to the compute mode's operand dtype where the kernel reads that dtype."""

from __future__ import annotations

import functools

import torch

import op_reference as R

COMPUTES = ("fp32", "bf16", "fp16")


def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def wide_bias(n, g):
    """Per-channel bias spanning [-30, 30] in random order: pre-activations of O(1) sums reach Mish's softplus
    threshold at 20, the GELU / SiLU tails and the far negative tail."""
    return torch.linspace(-30.0, 30.0, n)[torch.randperm(n, generator=g)].contiguous()


# ---------------------------------------------------------------- conv_pos
# (d, L, mode, x_as_f32, rowkeep kind, y_row_off); S = 3. rowkeep: None, "random", or per-sequence prefix lengths.
# 16-bit kernel: 256 positions per block (window 286 rows): L 255 / 256 / 257 / 300 are the block seam, 1 / 14 / 16
# sit inside the 15-row halo; prefixes end inside a block (100), on the edge (256), within 15 rows of it (245, 263)
# and at length 1. fp32 kernel: 64 positions per block.
CONV_CASES = {
    "bf16": [
        (128, 1, 0, True, None, 0), (512, 14, 2, False, "random", 1), (768, 16, 1, True, None, 1),
        (1024, 255, 0, False, (255, 1, 241), 0), (128, 256, 2, True, None, 1), (512, 257, 0, True, (257, 100, 1), 0),
        (1024, 300, 1, False, (256, 263, 245), 0), (768, 300, 2, False, "random", 1), (1024, 255, 0, False, None, 0),
        (768, 14, 0, True, (14, 1, 7), 0), (512, 300, 2, True, (300, 256, 1), 1),
    ],
    "fp32": [
        (128, 1, 0, True, None, 0), (512, 63, 1, True, "random", 1), (768, 64, 0, True, (64, 1, 50), 0),
        (1024, 65, 1, False, (64, 65, 60), 0), (1024, 130, 1, True, (128, 70, 1), 1), (128, 130, 0, False, "random", 0),
    ],
}
CONV_CASES["fp16"] = CONV_CASES["bf16"]
CONV_S = 3


@functools.lru_cache(maxsize=None)
def conv_case(compute, idx):
    d, L, mode, x_as_f32, kind, off = CONV_CASES[compute][idx]
    S, cg = CONV_S, d // 16
    g = _gen(1, d, L, mode, idx)
    x = torch.randn(S, L, d, generator=g)
    w = torch.randn(d, cg, 31, generator=g) / (31 * cg) ** 0.5
    bias = wide_bias(d, g)
    resid = torch.randn(S, L, d, generator=g) if mode else None
    if kind is None:
        keep = None
    elif kind == "random":
        keep = torch.rand(S, L, generator=g) < 0.7
    else:
        keep = torch.arange(L)[None, :] < torch.tensor(kind)[:, None]
    # the kernel rounds x itself when it reads fp32 (x_as_f32), so the values that reach the MFMA are rounded
    # either way; the weights are rounded by the packing
    return dict(d=d, L=L, S=S, mode=mode, x_as_f32=x_as_f32, off=off, x=x, w=w, bias=bias, keep=keep, resid=resid,
                x_read=R.rnd(x, compute), w_read=R.rnd(w, compute),
                u_out=R.U_OUT[compute] if mode != 1 else 0.0)


def conv_ref(c, dtype, variant=None):
    return R.conv_pos(c["x_read"], c["w_read"], c["bias"], c["keep"], c["resid"], dtype=dtype, variant=variant)


# ---------------------------------------------------------------- row norms
# d: 1024 / 768 / 512 are the fixed-register kernels (768 only for LayerNorm), 256 / 100 / 2048 the generic one
# (100: a ragged last float4 group; 2048: every register used); M 1, 5, 9: fewer, one more and two blocks more
# than the 4 rows of a block.
NORM_SHAPES = [(1024, 5), (768, 9), (512, 1), (256, 5), (100, 9), (2048, 5)]


@functools.lru_cache(maxsize=None)
def norm_case(compute, kind, d, M, h16):
    g = _gen(2, d, M, kind == "rms")
    h = torch.randn(M, d, generator=g)
    if M > 1:
        h[1] = 100.0 + torch.randn(d, generator=g)      # large mean: cancellation in the variance
        h[2] = 3.0                                       # constant row: zero variance
        h[3] = 1e-3 * torch.randn(d, generator=g)        # variance ~ the 1e-6 epsilon
        h[4] = 0.0 if kind == "rms" else 10.0 * torch.randn(d, generator=g)  # RMS: the 1e-12 clamp, output 0
    p0 = 0.5 * torch.randn(d, generator=g)
    p1 = 0.5 * torch.randn(d, generator=g)
    if kind == "rms":
        p0 = 1.0 + p0
    return dict(h=h, h_read=R.rnd(h, compute) if h16 else h, p0=p0, p1=p1, u_out=R.U_OUT[compute])


def norm_ref(kind, c, dtype, variant=None):
    if kind == "ln":
        return R.ln_modulate(c["h_read"], c["p0"], c["p1"], dtype=dtype, variant=variant)
    return R.rms_norm(c["h_read"], c["p0"], dtype=dtype, variant=variant)


# ---------------------------------------------------------------- dwconv + LayerNorm
# (C, L, flat): L 1 / 2 / 3 are shorter than the 7-tap window's half, 7 the window, 70 many blocks of 4 rows;
# C 100 leaves a ragged last 64-lane group, 1024 fills all 16. flat: sequence 1 is constant along channels after
# the conv (identical taps and bias per channel, inputs on a coarse dyadic grid so every sum is exact): zero variance.
DWCONV_SHAPES = [(64, 1, False), (100, 2, False), (512, 3, False), (1024, 7, False), (100, 70, False),
                 (1024, 70, False), (64, 7, True)]
DWCONV_S = 2


@functools.lru_cache(maxsize=None)
def dwconv_case(compute, C, L, flat):
    g = _gen(3, C, L, flat)
    S = DWCONV_S
    x = torch.randn(S, L, C, generator=g)
    dw_w = torch.randn(C, 7, generator=g) / 7 ** 0.5
    dw_b = torch.randn(C, generator=g)
    if (C, L) == (512, 3):  # conv outputs of scale 1e-3: a row variance comparable to the 1e-6 epsilon
        x, dw_b = 1e-3 * x, 1e-3 * dw_b
    if flat:
        x = (torch.randint(-4, 5, (S, L, 1), generator=g).float() / 2).expand(S, L, C).contiguous()
        dw_w = (torch.randint(-2, 3, (1, 7), generator=g).float() / 4).expand(C, 7).contiguous()
        dw_b = torch.full((C,), 0.5)
    ln_w = 1.0 + 0.5 * torch.randn(C, generator=g)
    ln_b = 0.5 * torch.randn(C, generator=g)
    return dict(x=x, dw_w=dw_w, dw_b=dw_b, ln_w=ln_w, ln_b=ln_b, u_out=R.U_OUT[compute])


def dwconv_ref(c, dtype, variant=None):
    return R.dwconv_ln(c["x"], c["dw_w"], c["dw_b"], c["ln_w"], c["ln_b"], dtype=dtype, variant=variant)


# ---------------------------------------------------------------- GRN
# L 63 / 64 / 65 / 130: the 64-row chunks of the column reduction; C 1100 > the 1024 threads of the normaliser block.
GRN_SHAPES = [(64, 1), (1024, 63), (1100, 64), (64, 65), (1100, 130)]
GRN_S = 2


@functools.lru_cache(maxsize=None)
def grn_case(compute, C, L):
    g = _gen(4, C, L)
    x = torch.randn(GRN_S, L, C, generator=g)
    x[0, :, 3] = 0.0          # an all-zero channel: Gx = 0
    if (C, L) == (1024, 63):
        x[1] = 0.0            # an all-zero sequence: Nx = 0 / (0 + 1e-6)
    gamma = torch.randn(C, generator=g)
    beta = torch.randn(C, generator=g)
    return dict(x=x, gamma=gamma, beta=beta, u_out=R.U_OUT[compute])


def grn_ref(c, dtype, variant=None):
    return R.grn(c["x"], c["gamma"], c["beta"], dtype=dtype, variant=variant)


# ---------------------------------------------------------------- GEMM epilogues
GEMM_SHAPES = [(1, 128, 64), (77, 100, 512), (130, 1024, 64), (900, 256, 128)]
LIVE_LEN, LIVE_SEQ = (300, 0, 37), 300   # M = 900: whole row tiles are dead at every tile height (64 .. 256)
OUT_IS_OPERAND = ("gelu_tanh", "gelu_erf_op", "resid16", "store16", "qkv")
# name -> (epi, options). gate / keep / resid: present or not; live: the pad-row skip (M = 900 only, in place);
# split: which k_split of A2 ("lo" = 64, "hi" = K - 64); dual: INPROJ's second output block
GEMM_CASES = {
    "store": ("store", {}), "silu": ("silu", {}), "gelu_tanh": ("gelu_tanh", {}), "gelu_erf": ("gelu_erf", {}),
    "gelu_erf_op": ("gelu_erf_op", {}), "store16": ("store16", {}),
    "store_a2_lo": ("store", dict(split="lo")), "store16_a2_hi": ("store16", dict(split="hi")),
    "resid_plain": ("resid", {}), "resid_gate_keep_r": ("resid", dict(gate=True, keep=True, resid=True)),
    "resid_gate_keep_live": ("resid", dict(gate=True, keep=True, live=True)),
    "resid16_keep": ("resid16", dict(keep=True)), "resid16_gate_r": ("resid16", dict(gate=True, resid=True)),
    "resid16_gate_keep_live": ("resid16", dict(gate=True, keep=True, live=True)),
    "resid_fill": ("resid_fill", {}), "resid_fill_keep": ("resid_fill", dict(keep=True)),
    "inproj": ("inproj", {}), "inproj_dual": ("inproj", dict(dual=True)),
}


def gemm_shapes_of(name):
    epi, o = GEMM_CASES[name]
    shapes = GEMM_SHAPES
    if epi == "inproj":
        shapes = [s for s in shapes if s[1] % 8 == 0]   # the launcher's contract: 8-column vector rows
    if o.get("split"):
        shapes = [s for s in shapes if s[2] >= 128]
    if o.get("live"):
        shapes = [s for s in shapes if s[0] == 900]
    return shapes


@functools.lru_cache(maxsize=None)
def gemm_case(compute, name, M, N, K):
    epi, o = GEMM_CASES[name]
    g = _gen(5, M, N, K, len(name), sum(map(ord, name)))
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    act = epi in ("silu", "gelu_tanh", "gelu_erf", "gelu_erf_op")
    bias = wide_bias(N, g) if act else torch.randn(N, generator=g)
    c = dict(epi=epi, A=A, W=W, bias=bias, A_read=R.rnd(A, compute), W_read=R.rnd(W, compute))
    op_out = epi in OUT_IS_OPERAND
    c["u_out"] = R.U_OUT[compute] if op_out else 0.0
    if o.get("split"):
        ks = 64 if o["split"] == "lo" else K - 64
        # kernel: A[:, :ks] | A2[:, :K - ks]; the columns it must not read are NaN
        A1 = A.clone()
        A1[:, ks:] = float("nan")
        A2 = torch.full((M, K), float("nan"))
        A2[:, :K - ks] = A[:, ks:]
        c.update(A=A1, A2=A2, k_split=ks)
    if epi in ("resid", "resid16", "resid_fill"):
        C0 = torch.randn(M, N, generator=g)
        c["C"] = C0
        c["C_read"] = R.rnd(C0, compute) if epi == "resid16" else C0
        if o.get("gate"):
            c["gate"] = torch.randn(N, generator=g)
        if o.get("resid"):
            r = torch.randn(M, N, generator=g)
            c["resid"] = r
            c["resid_read"] = R.rnd(r, compute) if epi == "resid16" else r
        if o.get("live"):
            ll = torch.tensor(LIVE_LEN, dtype=torch.int32)
            c["live_len"], c["live_seq"] = ll, LIVE_SEQ
            c["keep"] = (torch.arange(LIVE_SEQ)[None, :] < ll[:, None]).reshape(-1)
        elif o.get("keep"):
            c["keep"] = torch.rand(M, generator=g) < 0.7
    if epi == "inproj":
        c["bias"] = None
        dual = M if o.get("dual") else 0
        c["dual_rows"] = dual
        c["add"] = torch.randn(M + dual, N, generator=g)
    return c


def gemm_ref(c, dtype, variant=None):
    return R.gemm_epi(c["epi"], c["A_read"], c["W_read"], c["bias"], C=c.get("C_read"), resid=c.get("resid_read"),
                      gate=c.get("gate"), keep=c.get("keep"), add=c.get("add"), dual_rows=c.get("dual_rows", 0),
                      dtype=dtype, variant=variant)


# QKV: S = 2 sequences of 70 rows (M = 140: the sequence seam falls inside a 64-row tile, position = m % 70)
QKV_S, QKV_L = 2, 70
Q_SCALE = 0.125 * 1.4426950408889634
QKV_CASES = [(H, rh, qs, K) for H, K in ((2, 64), (4, 512)) for rh in (0, 1) for qs in (0.0, Q_SCALE)]


def rope_table_f32(L):
    """The table as the device builds it (fp32 position x fp32 inverse frequency, fp32 cos / sin): the stand-in
    for the device table where no GPU is present."""
    j = torch.arange(32, dtype=torch.float32)
    inv = 1.0 / torch.pow(torch.tensor(10000.0), 2 * j / 64.0)
    f = torch.arange(L, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.stack((torch.cos(f), torch.sin(f)), dim=-1)


@functools.lru_cache(maxsize=None)
def qkv_case(compute, H, rope_heads, q_scale, K):
    M, N = QKV_S * QKV_L, 3 * H * 64
    g = _gen(6, H, K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    return dict(A=A, W=W, bias=bias, A_read=R.rnd(A, compute), W_read=R.rnd(W, compute), H=H, rope_heads=rope_heads,
                q_scale=q_scale, u_out=R.U_OUT[compute])


def qkv_ref(c, rope, dtype, variant=None):
    return R.gemm_epi("qkv", c["A_read"], c["W_read"], c["bias"], seq_len=QKV_L, heads=c["H"],
                      rope_heads=c["rope_heads"], q_scale=c["q_scale"], rope=rope, dtype=dtype, variant=variant)
