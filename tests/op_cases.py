"""Seeded inputs of the op-level parity tests, shared by tests/test_gpu_ops.py and tests/test_gpu_fold_ops.py (the
kernels against the references) and tests/test_op_refs.py (wrong variants of the references against the same tolerance on the same
inputs). Shapes are the smallest that reach each launcher branch and edge; every builder returns fp32 CPU tensors
already rounded to the compute mode's operand dtype where the kernel reads that dtype."""

from __future__ import annotations

import functools
import math

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


# ---------------------------------------------------------------- LayerNorm / RMSNorm fold
# Strip counts np = d / 64 (the fold's partials per row): 2 = one partial or none per lane of the row's 8, 8 = exactly
# one, 12 = one or two and the once-per-row form's 128-byte fetch runs into the next row's partials, 16 = the
# production shape. M: 1 = a single row, 70 = ragged inside a 64 / 128 / 192-row tile, 300 = a full 256-row tile plus
# a ragged one. Producer K (64: one k tile, 256: several) is independent of d.
FOLD_ROW_KINDS = {1: "mean=100sigma", 2: "sigma=1e-2", 3: "constant", 4: "constant strip", 5: "strip means apart",
                  6: "zero (rms) / ordinary"}
FOLD_PROD_SHAPES = [(1, 128, 64), (70, 128, 256), (300, 512, 64), (70, 768, 256), (300, 768, 64), (1, 1024, 256),
                    (70, 1024, 64), (300, 1024, 256)]                      # (M, N = d, K)
# variant -> what reaches the kernel. The rows of FOLD_ROW_KINDS get A = 0, so their h' is R + gate bias: exactly the
# planted row where the bias is zero (ln "inplace", rms "plain") or the row is masked (rms "keep").
FOLD_PROD_VARIANTS = {"ln": ("gate_resid", "inplace"), "rms": ("plain", "keep")}


def fold_rows(M, d, g, rms):
    """h' rows [M,d] (fp32, not yet rounded): ordinary N(0,1) rows and, from row 1 on when M allows, a row with
    mean = 100 sigma (cancellation), one with sigma = 1e-2 around mean 1 (variance near, above, the 1e-6 epsilon), a
    constant row, a row with one constant strip, a row whose strip means lie far apart (the between-strip term of the
    combine dominates; in the constant row it vanishes) and, for the RMSNorm form, an all-zero row."""
    T = torch.randn(M, d, generator=g)
    if M >= 8:
        T[1] = 100.0 + torch.randn(d, generator=g)
        T[2] = 1.0 + 1e-2 * torch.randn(d, generator=g)
        T[3] = 3.0
        T[4, 64:128] = 0.5
        T[5] = T[5] + 8.0 * torch.randn(d // 64, generator=g).repeat_interleave(64)
        if rms:
            T[6] = 0.0
    return T


def fold_special_rows(M):
    return list(range(1, 7)) if M >= 8 else []


@functools.lru_cache(maxsize=None)
def fold_prod_case(compute, form, variant, M, N, K):
    """An EPI_RESID16 launch whose output rows h' are fold_rows: ordinary rows come from the GEMM, the special rows
    have A = 0 and their residual carries the planted row (less gate bias, so the sum lands near it)."""
    rms = form == "rms"
    g = _gen(7, M, N, K, rms, len(variant))
    T = fold_rows(M, N, g, rms)
    A = torch.randn(M, K, generator=g)
    sp = fold_special_rows(M)
    A[sp] = 0.0
    W = torch.randn(N, K, generator=g) / K ** 0.5
    zero_bias = variant in ("inplace", "plain")
    bias = torch.zeros(N) if zero_bias else torch.randn(N, generator=g)
    gate = None if variant == "inplace" else torch.randn(N, generator=g)
    R0 = T.clone()
    if sp and gate is not None:
        R0[sp] = T[sp] - gate * bias
        if variant == "keep":
            R0[[3, 6]] = T[[3, 6]]                     # masked below: the row itself is the output
    c = dict(epi="resid16", A=A, W=W, bias=bias, A_read=R.rnd(A, compute), W_read=R.rnd(W, compute), gate=gate,
             u_out=R.U_OUT[compute], special=sp, exact=zero_bias, rms=rms)
    if variant in ("gate_resid", "keep"):
        c["C"] = torch.randn(M, N, generator=g)        # overwritten: the residual comes from `resid`
        c["resid"] = R0
        c["resid_read"] = R.rnd(R0, compute)
    else:
        c["C"] = R0
    c["C_read"] = R.rnd(c["C"], compute)
    if variant == "keep":
        keep = torch.rand(M, generator=g) < 0.7
        if sp:
            keep[[3, 6]] = False                       # the constant and the all-zero row stay exactly as planted
            keep[[1, 2, 4, 5]] = True
        c["keep"] = keep
    if not rms:
        c["hs_scale"] = 0.3 * torch.randn(N, generator=g)
    return c


# Consumer: (M, d) with N = 256 (one 256-column tile; two 128-column tiles), and N = 384 once: no whole 256-column
# tile, so a forced 256x256 configuration runs the fold in the 128x128 one.
FOLD_GELU_SHAPES = [(1, 128, 256), (70, 128, 256), (300, 512, 256), (70, 768, 256), (70, 768, 384), (300, 768, 256),
                    (1, 1024, 256), (70, 1024, 256), (300, 1024, 256)]    # (M, d = K, N)
# QKV: heads = 4 (N = 768 = 3 x 256), S = 2 sequences; (seq_len, d, rope_heads, q_scale)
FOLD_QKV_H = 4
FOLD_QKV_CASES = [(70, 128, 0, 0.0), (70, 768, 1, Q_SCALE), (150, 512, 0, Q_SCALE), (150, 768, 0, 0.0),
                  (150, 1024, 1, Q_SCALE), (70, 1024, 0, 0.0)]
FOLD_EPS = {"ln": 1e-6, "rms": 1e-30}   # the two epsilons the engine passes (engine.cpp fold_consumer / rms_consumer)


@functools.lru_cache(maxsize=None)
def fold_cons_case(compute, form, M, d, N):
    """What a consumer reads, every tensor already representable in the type the kernel reads it in: h' rows of
    fold_rows rounded to the operand dtype, their fp64 strip partials rounded to fp32, and for the LayerNorm form
    hs = round(h' (1 + sc)), u and v (fp64 sums rounded to fp32); for the RMSNorm form A = h' and W' = round(W g)."""
    rms = form == "rms"
    g = _gen(8, M, d, N, rms)
    hp = R.rnd(fold_rows(M, d, g, rms), compute)
    W = R.rnd(torch.randn(N, d, generator=g) / d ** 0.5, compute)
    bias = 2.0 * torch.randn(N, generator=g)
    parts = R.strip_stats(hp, torch.float64, rms).float()
    c = dict(hp=hp, parts=parts, bias=bias, eps=FOLD_EPS[form], u_out=R.U_OUT[compute], rms=rms, u=None, v=None)
    if rms:
        gain = 1.0 + 0.5 * torch.randn(d, generator=g)
        c.update(A=hp, W=R.scale_cols(W, gain, compute), gain=gain, W_plain=W)
    else:
        sc, sh = 0.3 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
        c.update(A=R.fold_hs(hp, sc, compute), W=W, sc=sc, sh=sh,
                 u=((1.0 + sc.double()) * W.double()).sum(-1).float(), v=(sh.double() * W.double()).sum(-1).float())
    return c


def fold_gelu_ref(c, dtype, variant=None):
    return R.fold_consumer("gelu_tanh", c["A"], c["W"], c["bias"], c["parts"], c["u"], c["v"], c["eps"], dtype=dtype,
                           variant=variant)


def fold_qkv_ref(c, spec, rope, dtype, variant=None):
    L, _, rh, qs = spec
    return R.fold_consumer("qkv", c["A"], c["W"], c["bias"], c["parts"], c["u"], c["v"], c["eps"], dtype=dtype,
                           variant=variant, seq_len=L, heads=FOLD_QKV_H, rope_heads=rh, q_scale=qs, rope=rope)


# lnfold_uv: (d, F, nfe), depth 2. nfe 1 / 16 / 17 / 35: below, at and past the 16-step group, and a last group whose
# unused lanes read the clamped last row. F = 2d at the production width, 256 otherwise.
LNFOLD_CASES = [(128, 256, 1), (128, 256, 16), (128, 256, 17), (128, 256, 35), (768, 256, 16), (768, 256, 35),
                (1024, 2048, 17)]
LNFOLD_DEPTH, LNFOLD_GAP, LNFOLD_TAIL = 2, 8, 12   # floats between the modulation rows and u / v, and past them


@functools.lru_cache(maxsize=None)
def lnfold_case(compute, d, F, nfe):
    """The AdaLN table [nfe + 1 (a guard row), stride]: modulation rows (scales ~0.3 N(0,1), shifts ~0.1 N(0,1), the
    last step's shifts ~1e-4 N(0,1): in fp16 the lo parts of such shifts are subnormal), then NaN in the u / v
    blocks, out_off > the modulation rows and stride wider than the row; the gap, the tail and the guard row hold
    finite markers that must come back untouched."""
    g = _gen(9, d, F, nfe)
    depth = LNFOLD_DEPTH
    mod = torch.randn(nfe, depth, 6, d, generator=g)
    mod[:, :, (0, 3)] *= 0.1
    mod[:, :, (1, 4)] *= 0.3
    mod[nfe - 1, :, (0, 3)] *= 1e-3
    LW = 2 * F + 6 * d
    out_off = depth * 6 * d + LNFOLD_GAP
    stride = out_off + depth * LW + LNFOLD_TAIL
    table = torch.randn(nfe + 1, stride, generator=g)
    table[:nfe, :depth * 6 * d] = mod.reshape(nfe, -1)
    table[:nfe, out_off:out_off + depth * LW] = float("nan")
    W1 = R.rnd(torch.randn(depth, F, d, generator=g) / d ** 0.5, compute)
    Wqkv = R.rnd(torch.randn(depth, 3 * d, d, generator=g) / d ** 0.5, compute)
    return dict(table=table, mod=mod, W1=W1, Wqkv=Wqkv, out_off=out_off, stride=stride, LW=LW, depth=depth)


def lnfold_blocks(c, table, d, F, nfe):
    """The (u1, v1, u2, v2) blocks of a table, shaped as op_reference.lnfold_uv returns them."""
    t = table[:nfe, c["out_off"]:c["out_off"] + c["depth"] * c["LW"]].reshape(nfe, c["depth"], c["LW"])
    return t[..., :F], t[..., F:2 * F], t[..., 2 * F:2 * F + 3 * d], t[..., 2 * F + 3 * d:]


# scale_cols: 128 x 64 = 1024 8-element groups (four whole blocks of 256 threads), 384 x 768 = 36864 groups (144
# blocks); 130 x 72 = 1170 groups: a ragged last block, and K = 72 is a multiple of 8 only.
SCALE_COLS_SHAPES = [(128, 64), (384, 768), (130, 72)]


@functools.lru_cache(maxsize=None)
def scale_cols_case(compute, rows, K):
    g = _gen(10, rows, K)
    W = torch.randn(rows, K, generator=g)
    return dict(W=W, W_read=R.rnd(W, compute), g=1.0 + 0.5 * torch.randn(K, generator=g))


# ================================================================ audio glue, prologue and ODE step kernels
# (tests/test_gpu_glue_ops.py, and the same inputs in tests/test_op_refs.py)
NAN, INF = float("nan"), float("inf")

# ---------------------------------------------------------------- mel_frames
# (n_fft, hop, L), B = 3 (a read across the batch seam lands in the neighbour's samples). n_fft 64: L 33 is the
# shortest legal wave (L > n_fft/2), its frames reflect at both ends at once; 48 and 64 are multiples of the hop (the
# last frame starts exactly at the last sample's window); 1000 has interior frames without reflection. n_fft 1024 /
# hop 256 (the product's): 513 the shortest, 1300 several blocks.
MEL_FRAMES_CASES = [(64, 16, 33), (64, 16, 48), (64, 16, 64), (64, 16, 1000), (1024, 256, 513), (1024, 256, 1300)]
MEL_FRAMES_B = 3
# one ragged batch: the shortest wave first, the longest next to it, a hop multiple, an odd one; the row stride is
# longer than the longest wave and everything past a wave's length is NaN (never to be read)
MEL_RAGGED = dict(n_fft=64, hop=16, lens=(33, 1000, 64, 257), wav_st=1024)


@functools.lru_cache(maxsize=None)
def mel_frames_case(n_fft, hop, L):
    return torch.randn(MEL_FRAMES_B, L, generator=_gen(20, n_fft, hop, L))


@functools.lru_cache(maxsize=None)
def mel_frames_ragged_case():
    m = MEL_RAGGED
    wav = torch.full((len(m["lens"]), m["wav_st"]), NAN)
    g = _gen(21)
    for s, n in enumerate(m["lens"]):
        wav[s, :n] = torch.randn(n, generator=g)
    return wav


# ---------------------------------------------------------------- mel_mag
# rows 5 x 576 = 2880 outputs: 12 blocks, the last ragged; bins 513 odd; ld_spec 1088 > 2 bins and ld_mag 576 > bins as
# in the product (K padding of the two GEMMs). Magnitudes from 1e-6 to 1e3 (squares 1e-12 .. 1e6), exact zero pairs,
# and NaN in the spec columns past 2 bins, which the kernel must not read; the mag pad columns must come back zero.
MEL_MAG = dict(rows=5, bins=513, ld_spec=1088, ld_mag=576)


@functools.lru_cache(maxsize=None)
def mel_mag_case():
    m = MEL_MAG
    g = _gen(22)
    mag = 10.0 ** (torch.rand(m["rows"], m["bins"], 2, generator=g) * 9.0 - 6.0)
    z = mag * torch.where(torch.rand(m["rows"], m["bins"], 2, generator=g) < 0.5, -1.0, 1.0)
    z[:, ::37] = 0.0       # exact zeros: |0| = 0, not NaN
    z[0, 1, 0] = 0.0       # one component zero
    spec = torch.full((m["rows"], m["ld_spec"]), NAN)
    spec[:, :2 * m["bins"]] = z.reshape(m["rows"], -1)
    return dict(spec=spec, u_out=0.0, **m)


def mel_mag_ref(c, dtype, variant=None):
    return R.mel_mag(c["spec"], c["bins"], c["ld_mag"], dtype=dtype, variant=variant)


# ---------------------------------------------------------------- mel_log
# B = 2, n_mels = 100, T = 1 (the transposition degenerates) and 3; the ragged form with T_s = (1, 3) in T_out = 4.
# Values from 1e-7 to 1e2 around the clamp, and in fixed places 0, 1e-5 and its two float32 neighbours (the clamp's
# edge: below it log(1e-5), above it the value's own log), 1 (log = 0 exactly), +inf (stays +inf) and NaN (stays NaN).
MEL_LOG_T = (1, 3)
MEL_LOG_RAGGED = dict(frames=(1, 3), T_out=4)
MEL_LOG_B, MEL_LOG_NMELS = 2, 100


@functools.lru_cache(maxsize=None)
def mel_log_case(rows):
    g = _gen(23, rows)
    mel = 10.0 ** (torch.rand(rows, MEL_LOG_NMELS, generator=g) * 9.0 - 7.0)
    e = torch.tensor(1e-5, dtype=torch.float32)
    below, above = torch.nextafter(e, torch.tensor(0.0)), torch.nextafter(e, torch.tensor(1.0))
    for r in range(rows):  # every row (every frame of every wave) holds the specials, at row-dependent bins
        mel[r, torch.arange(7) * 13 + r] = torch.stack((torch.tensor(0.0), e, below, above, torch.tensor(1.0),
                                                         torch.tensor(INF), torch.tensor(NAN)))
    return dict(mel=mel, u_out=0.0)


def mel_log_ref(c, frames, T_out, dtype, variant=None):
    return R.mel_log(c["mel"], frames, T_out, dtype=dtype, variant=variant)


# ---------------------------------------------------------------- vocos_im2col
# C = 100 mel bins -> 700 columns, Kp = 704 (the GEMM's K padding: columns 700..703 zero). T 1, 2, 3 are shorter than
# the window's half (every tap but the centre ones is padding), 4 and 7 around the window, 8 longer; B = 2: a tap
# across the batch seam would read the neighbour's frames. Ragged: lengths (1, 2, 9, 4) from [B][N][C] (start > 0) and
# from [B][C][T], with NaN in every source frame outside [start, start + len).
IM2COL = dict(C=100, Kp=704, B=2, Ts=(1, 2, 3, 4, 7, 8))
IM2COL_RAGGED = dict(lens=(1, 2, 9, 4), starts=(3, 1, 2, 5), frames=12)


@functools.lru_cache(maxsize=None)
def im2col_case(T):
    return torch.randn(IM2COL["B"], IM2COL["C"], T, generator=_gen(24, T))


@functools.lru_cache(maxsize=None)
def im2col_ragged_case(layout):
    """(src in `layout` with NaN outside every utterance's frames, [utterance mel [1, C, len]])."""
    m, C = IM2COL_RAGGED, IM2COL["C"]
    g = _gen(25)
    src = torch.full((len(m["lens"]), m["frames"], C), NAN)  # [B][N][C]
    utts = []
    for s, (st, n) in enumerate(zip(m["starts"], m["lens"])):
        x = torch.randn(n, C, generator=g)
        src[s, st:st + n] = x
        utts.append(x.t()[None].contiguous())
    return (src if layout == "BNC" else src.transpose(1, 2).contiguous()), utts


# ---------------------------------------------------------------- vocos_spec
# rows 3 x 544 pairs = 1632 threads (7 blocks, ragged), bins 513 of ld 1088 as in the product. m spans [-20, 10] across
# the clip at log(100) = 4.605 (values on both sides within 1e-3 of it too), m = +inf (magnitude 100) and -inf (0);
# phases near 0 and +-pi (the sign changes of sin / cos) and near 1e2 and 1e4 (argument reduction). NaN in m alone and
# in p alone must both give a NaN pair; the pad pairs start as NaN and must come back zero.
SPEC = dict(rows=3, bins=513, ld=1088)


@functools.lru_cache(maxsize=None)
def spec_case():
    m = SPEC
    g = _gen(26)
    rows, bins = m["rows"], m["bins"]
    mm = torch.rand(rows, bins, generator=g) * 30.0 - 20.0
    mm[:, 10:20] = math.log(100.0) + torch.linspace(-1e-3, 1e-3, 10)
    centre = torch.tensor([0.0, math.pi, -math.pi, 1e2, 1e4])[torch.randint(0, 5, (rows, bins), generator=g)]
    pp = centre + 0.01 * torch.randn(rows, bins, generator=g)
    pp[:, 30:35] = torch.tensor([0.0, math.pi, -math.pi, 1e2, 1e4])
    mm[0, 40], mm[1, 41] = INF, -INF
    mm[0, 5] = NAN   # NaN log-magnitude, finite phase
    pp[1, 7] = NAN   # finite log-magnitude, NaN phase
    x = torch.full((rows, m["ld"]), NAN)
    x[:, :2 * bins] = torch.stack((mm, pp), dim=-1).reshape(rows, -1)
    return dict(x=x, u_out=0.0, **m)


def spec_ref(c, dtype, variant=None):
    return R.vocos_spec(c["x"], c["bins"], dtype=dtype, variant=variant)


# ---------------------------------------------------------------- vocos_ola
# (n_fft, hop): the product's 1024 / 256 and the small 64 / 16, four frames per window both. B = 2. T = 1 has no
# samples (no launch); 2, 3: fewer frames than a window covers; 4: as many; 5, 9: more (interior samples under four
# frames). Ragged: lengths (1, 2, 5, 1, 9) -- one-frame utterances at the start and in the middle contribute nothing
# and shift nobody -- and a batch of one-frame utterances only (no launch).
OLA_FFT = ((1024, 256), (64, 16))
OLA_B = 2
OLA_TS = (2, 3, 4, 5, 9)
OLA_RAGGED_LENS = (1, 2, 5, 1, 9)


@functools.lru_cache(maxsize=None)
def ola_case(n_fft, hop, lens):
    """Packed windowed frames [sum lens, n_fft] and the periodic Hann window."""
    win = torch.hann_window(n_fft, periodic=True)
    fr = torch.randn(sum(lens), n_fft, generator=_gen(27, n_fft, hop, *lens)) * win
    return dict(frames=fr, win=win, lens=lens, hop=hop, u_out=0.0)


def ola_ref(c, dtype, variant=None):
    return R.vocos_ola(c["frames"], c["win"], c["lens"], c["hop"], dtype=dtype, variant=variant)


# ---------------------------------------------------------------- time_sinus
# n = 1, 5 (one block, ragged) and 512 (the launcher's limit, 256 blocks). t = 0 (sin 0, cos 1 exactly), 1e-5 (the
# sway grid's first steps), 0.03125, 0.5 and 1 (arguments up to 1000 rad).
TIME_SINUS_T = {1: (0.03125,), 5: (0.0, 1e-5, 0.03125, 0.5, 1.0), 512: tuple(torch.linspace(0, 1, 512).tolist())}


def time_sinus_case(n):
    return dict(t=torch.tensor(TIME_SINUS_T[n], dtype=torch.float32), u_out=0.0)


def time_sinus_ref(c, dtype, variant=None):
    return R.time_sinus(c["t"], dtype=dtype, variant=variant)


ROPE_LS = (1, 70, 8192)  # one row; a ragged last block; the engine's longest sequence


# ---------------------------------------------------------------- text_embed
# B = 2, nt = 5. Row 0 has a filler in the interior, row 1 fillers at the end. N = 3 cuts the text, 5 = nt, 9 pads it.
# td = 100 leaves a ragged last 64-lane group, 512 fills eight. seq_len None, or per sample (N, N - 2): sample 1's last
# positions are dropped. freqs: None, the full table, or a 4-row table with N = 9 (positions 4..8 read row 3).
TEXT = torch.tensor([[3, -1, 7, 2, 9], [4, 5, 6, -1, -1]])
TEXT_V = 12
TEXT_CASES = [(N, td, per, fr, mp) for N in (3, 5, 9) for td in (100, 512) for per in (False, True)
              for fr in ((None, "full", "rows4") if N == 9 else (None, "full")) for mp in (False, True)]
TEXT_SEG_LENS = (7, 3)  # the ragged form: utterance lengths (one pads its text, one cuts it)


@functools.lru_cache(maxsize=None)
def text_table(td):
    from oracle import ref_cpu

    return torch.randn(TEXT_V, td, generator=_gen(28, td)), ref_cpu.freqs_cis_table(td, 16)


def text_embed_args(N, td, per, fr, mp):
    table, freqs = text_table(td)
    return dict(table=table, N=N, seq_len=(N, max(1, N - 2)) if per else None,
                freqs=None if fr is None else (freqs if fr == "full" else freqs[:4].contiguous()),
                freq_rows=4 if fr == "rows4" else 0, mask_padding=mp)


# ---------------------------------------------------------------- build_ct, pack_y, masks, final_where_out, copy_pred
# build_ct: (S, drop_audio, drop_text) with B = 2: both branches (S = 4) and the single-branch forward (S = 2) under
# the four drop-flag combinations; N = 5; td 100 (text columns 100..127 of the text block are zero padding) and 64 (no
# padding); a cond_mask with kept and dropped frames in both samples.
CT_CASES = [(4, 0, 0), (2, 0, 0), (2, 1, 0), (2, 0, 1), (2, 1, 1)]
CT_TDS = (100, 64)


@functools.lru_cache(maxsize=None)
def ct_case(td):
    g = _gen(29, td)
    B, N = 2, 5
    return dict(cond=torch.randn(B, N, 100, generator=g), cond_mask=torch.tensor([[1, 1, 0, 0, 1], [0, 1, 1, 0, 0]]),
                text_c=torch.randn(B, N, td, generator=g), text_u=torch.randn(B, N, td, generator=g))


PACK_Y = dict(rows=7, mels=(100, 80))  # 896 outputs: 3.5 blocks; mel 100 and 80 leave 28 / 48 zero pad columns
# masks: B = 3, S = 2 B (the unconditional sequences reuse sample s % B); durations below, at and above L; off 0, 1
# (the UNetT time token's row). build_textlen: nt 1, 64 (one pass of the wave), 65 (one lane wraps), 130 (three
# passes); rows: all filler (0), a filler in the interior (fillers do not end the text), the last position valid (nt).
MASK_DUR, MASK_L = (2, 6, 9), 6
TEXTLEN_NTS = (1, 64, 65, 130)


def textlen_case(nt):
    text = torch.arange(3 * nt).reshape(3, nt) % 11
    text[0] = -1
    text[1, nt // 2:] = -1
    text[1, : nt // 4] = -1  # (interior / leading fillers before the last valid position)
    text[2, : nt - 1] = -1   # only the last position valid
    return text


@functools.lru_cache(maxsize=None)
def where_case():
    g = _gen(30)
    B, N, mel = 2, 5, 100
    return dict(cond=torch.randn(B, N, mel, generator=g), y=torch.randn(B, N, mel, generator=g),
                cond_mask=torch.tensor([[1, 1, 0, 0, 1], [0, 0, 1, 0, 0]]))


@functools.lru_cache(maxsize=None)
def copy_pred_case():
    """p [S = 2, L = 6, p_ld = 128] with NaN in the pad columns mel..127 (never copied)."""
    p = torch.randn(2, 6, 128, generator=_gen(31))
    p[..., 100:] = NAN
    return p


# ---------------------------------------------------------------- cfg_euler / cfg_rk
# (B, N, mel): 2 x 1 x 100 = 200 elements, one block; 2 x 166 x 99 = 128 * 256 + 100: the launch is capped at 128
# blocks, so the grid-stride loop wraps for the last 100. p_row_off 1 with p_ld 128 is UNetT's prediction (row 0 the
# time token, pad columns NaN here), p_row_off 0 with p_ld = mel the DiT's.
STEP_SHAPES = ((2, 1, 100), (2, 166, 99))
STEP_P_LAYOUTS = ((1, 128), (0, None))
STEP_GRID = (0.0, 0.0625, 0.21875, 0.5, 1.0)  # nfe 4, unequal steps
STEP_CFG = 2.3


@functools.lru_cache(maxsize=None)
def step_case(B, N, mel, row_off, p_ld, seed=0):
    g = _gen(32, B, N, mel, row_off, seed)
    p = torch.full((2 * B, N + row_off, p_ld or mel), NAN)
    p[:, row_off:, :mel] = torch.randn(2 * B, N, mel, generator=g)
    return dict(y=torch.randn(B, N, mel, generator=g), p=p)


def step_table(n, stride=24):
    """A table of n rows (the AdaLN / time-token rows of the step bookkeeping), row i = i + column / 100."""
    return torch.arange(n)[:, None].float() + torch.arange(stride)[None, :].float() / 100.0
