"""Op-level fp64 parity of the conv, norm and GEMM-epilogue kernels (and attention's q_len path): each kernel alone,
through its production launcher (f5h_op_* in include/f5h.h), on the inputs where it can go wrong, against a float64
reference of the same operation written from the model definition (tests/op_reference.py; inputs in
tests/op_cases.py, which lists the branch or edge every shape is there for).

Tolerance (measured against the reference, not chosen): with R64 the float64 reference and R32 the same formula in
float32 torch on the CPU, elementwise
    |out - R64| <= u_out |R64| + 8 max|R32 - R64|
u_out = the unit roundoff of the stored output type (2^-8 bf16, 2^-11 fp16, 0 fp32); the factor 8 covers a
different accumulation order (MFMA k-slabs, wave reductions). A failure prints
    max(|out - R64| - u_out |R64|) / max|R32 - R64|
tests/test_op_refs.py shows that the wrong variants of every reference miss this bound on the same inputs.

One exception, derived where it is used (test_attention_q_len): the 16-bit attention kernels feed the probabilities
to the P.V MFMA as 16-bit operands, which the bound above has no term for.

Worst measured ratio on the MI355X per op and compute mode (the bound is 8; in the 16-bit modes the output
rounding term u_out |R64| absorbs most of the error of a 16-bit store, so those ratios are small):

    op            fp32    bf16    fp16
    conv_pos      3.05    1.88    1.41    (16-bit: mish_fast's v_exp / v_rcp stay inside the bound)
    ln_modulate   1.97    0.27    0.69
    rms_norm      1.53    0.00    0.01
    dwconv_ln     1.07    0.00    0.03
    grn           1.37    0.03    0.09
    gemm_epi      4.16    1.92    1.53    (16-bit gelu_tanh_fast included)
    gemm_qkv      2.84    0.25    0.19
    attention     2.09    < 0     < 0     (16-bit with the P-rounding term; without it 3477 bf16, 498 fp16)
"""

import pytest
import torch

import op_cases as C
import op_reference as R
from f5_tts_amd.engine import (gemm_force_config, op_attention, op_conv_pos, op_dwconv_ln, op_gemm_epi, op_grn,
                               op_norm)
from test_gpu_parity import GEMM_CONFIGS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------------- conv_pos
CONV_PARAMS = [(cm, i) for cm in C.COMPUTES for i in range(len(C.CONV_CASES[cm]))]


@pytest.mark.parametrize("compute,idx", CONV_PARAMS, ids=[f"{cm}-{C.CONV_CASES[cm][i]}" for cm, i in CONV_PARAMS])
def test_conv_pos(compute, idx):
    """One ConvPositionEmbedding layer: every group width (8 / 32 / 48 / 64 channels), S = 3 (a halo crossing a
    sequence seam would read the neighbour's rows), L around the position block and inside the halo, the three output
    modes, both input types, row masks ending at the block seams, and a bias that drives Mish through its threshold
    at 20 and its negative tail. The torch-layout weight goes through the packing engine creation uses. With
    y_row_off = 1 the output starts as NaN and row 0 of every sequence must stay NaN."""
    _need_gpu()
    c = C.conv_case(compute, idx)
    y = op_conv_pos(_dev(c["x"]), c["w"], c["bias"], rowkeep=_dev(c["keep"]), mode=c["mode"], resid=_dev(c["resid"]),
                    x_as_f32=c["x_as_f32"], y_row_off=c["off"] if c["mode"] else 0, compute=compute).cpu()
    off = c["off"] if c["mode"] else 0
    assert y.shape == (c["S"], c["L"] + off, c["d"])
    if off:
        assert torch.isnan(y[:, :off]).all(), "rows before y_row_off were written"
    R.assert_close(y[:, off:], C.conv_ref(c, F64), C.conv_ref(c, F32), c["u_out"],
                   f"conv_pos/{compute}/{C.CONV_CASES[compute][idx]}")


# ---------------------------------------------------------------- row norms
@pytest.mark.parametrize("compute", C.COMPUTES)
@pytest.mark.parametrize("kind", ["ln", "rms"])
def test_row_norms(compute, kind):
    """ln_modulate / rms_norm_g: every kernel variant (d 1024 / 768 / 512 / generic, fp32 or 16-bit h), M below and
    above the 4 rows of a block, rows with a large mean, zero variance, a variance near the epsilon and (RMSNorm) an
    all-zero row, which must give 0."""
    _need_gpu()
    name = "ln_modulate" if kind == "ln" else "rms_norm"
    for d, M in C.NORM_SHAPES:
        for h16 in ((False, True) if compute != "fp32" else (False,)):
            c = C.norm_case(compute, kind, d, M, h16)
            out = op_norm(kind, _dev(c["h"]), c["p0"], c["p1"], h16=h16, compute=compute).cpu()
            if kind == "rms" and M > 4:
                assert (out[4] == 0).all(), "RMSNorm of an all-zero row"
            R.assert_close(out, C.norm_ref(kind, c, F64), C.norm_ref(kind, c, F32), c["u_out"],
                           f"{name}/{compute}/d{d}-M{M}-h16={int(h16)}")


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_dwconv_ln(compute):
    """Depthwise conv + LayerNorm of the ConvNeXt text blocks: L shorter than the 7-tap window, ragged and full
    channel counts, a variance near the epsilon and rows of zero variance."""
    _need_gpu()
    for Cc, L, flat in C.DWCONV_SHAPES:
        c = C.dwconv_case(compute, Cc, L, flat)
        out = op_dwconv_ln(_dev(c["x"]), c["dw_w"], c["dw_b"], c["ln_w"], c["ln_b"], compute=compute).cpu()
        R.assert_close(out, C.dwconv_ref(c, F64), C.dwconv_ref(c, F32), c["u_out"],
                       f"dwconv_ln/{compute}/C{Cc}-L{L}-flat={int(flat)}")


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_grn(compute):
    """GRN: L around the 64-row chunks of the time reduction, C past the normaliser block's 1024 threads, an
    all-zero channel and an all-zero sequence."""
    _need_gpu()
    for Cc, L in C.GRN_SHAPES:
        c = C.grn_case(compute, Cc, L)
        out = op_grn(_dev(c["x"]), c["gamma"], c["beta"], compute=compute).cpu()
        R.assert_close(out, C.grn_ref(c, F64), C.grn_ref(c, F32), c["u_out"], f"grn/{compute}/C{Cc}-L{L}")


# ---------------------------------------------------------------- GEMM epilogues
def _configs(compute):
    return GEMM_CONFIGS if compute != "fp32" else [-1]  # the fp32 parity mode has one tile configuration


@pytest.mark.parametrize("compute", C.COMPUTES)
@pytest.mark.parametrize("name", list(C.GEMM_CASES))
def test_gemm_epilogue(compute, name):
    """Every GEMM epilogue but the fold forms, under every tile configuration: the fp64 reference is met and all
    configurations agree bit for bit. Shapes: one row, ragged N (the general epilogue), several column tiles, and
    M = 900 with live_len (300, 0, 37): row tiles without a live row are skipped at every tile height and keep C.
    A2: the columns the kernel must not read are NaN."""
    _need_gpu()
    for M, N, K in C.gemm_shapes_of(name):
        c = C.gemm_case(compute, name, M, N, K)
        kw = dict(bias=c["bias"], C=c.get("C"), compute=compute, A2=_dev(c.get("A2")), k_split=c.get("k_split", 0),
                  resid=c.get("resid"), gate=c.get("gate"), rowkeep=c.get("keep"), live_len=c.get("live_len"),
                  live_seq=c.get("live_seq", 0), add=c.get("add"), dual_rows=c.get("dual_rows", 0))
        A, W = _dev(c["A"]), _dev(c["W"])
        outs = []
        try:
            for cfg in _configs(compute):
                gemm_force_config(cfg)
                outs.append(op_gemm_epi(c["epi"], A, W, **kw))
        finally:
            gemm_force_config(-1)
        for cfg, o in zip(_configs(compute), outs):
            assert torch.equal(o, outs[0]), (name, (M, N, K), cfg)
        R.assert_close(outs[0].cpu(), C.gemm_ref(c, F64), C.gemm_ref(c, F32), c["u_out"],
                       f"gemm_epi/{compute}/{name}-{M}x{N}x{K}")


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_gemm_qkv(compute):
    """EPI_QKV: interleaved-pair RoPE on all heads or the first one only, q scaled or not, scattered to q / k / v
    [S,H,L,64], two sequences of 70 rows, under every tile configuration. The reference reads the (cos, sin) table
    the kernel read; the table itself is checked against float64 (fp32 angles: position x inverse frequency carries
    a few ulp of the angle, <= 4 L 2^-24)."""
    _need_gpu()
    for spec in C.QKV_CASES:
        H, rh, qs, K = spec
        c = C.qkv_case(compute, *spec)
        A, W = _dev(c["A"]), _dev(c["W"])
        outs = []
        try:
            for cfg in _configs(compute):
                gemm_force_config(cfg)
                outs.append(op_gemm_epi("qkv", A, W, bias=c["bias"], compute=compute, seq_len=C.QKV_L, heads=H,
                                        rope_heads=rh, q_scale=qs))
        finally:
            gemm_force_config(-1)
        for cfg, o in zip(_configs(compute), outs):
            for t, t0 in zip(o, outs[0]):
                assert torch.equal(t, t0), (spec, cfg)
        q, k, v, rope = (t.cpu() for t in outs[0])
        assert (rope.double() - R.rope_table(C.QKV_L)).abs().max() < 4 * C.QKV_L * 2.0 ** -24 + 1e-6
        r64, r32 = C.qkv_ref(c, rope, F64), C.qkv_ref(c, rope, F32)
        for nm, o, a, b in zip("qkv", (q, k, v), r64, r32):
            R.assert_close(o, a, b, c["u_out"], f"gemm_qkv/{compute}/{nm}-H{H}-rope{rh}-qs{qs:.2f}-K{K}")


# ---------------------------------------------------------------- attention q_len
@pytest.mark.parametrize("compute", C.COMPUTES)
@pytest.mark.parametrize("kv_masked", [False, True])
def test_attention_q_len(compute, kv_masked):
    """The pad skip's q_len: S = 2, H = 2, N = 300, q_len = (300, 70). The skip unit is the 64-row block in the fp32
    kernel and the 32-row wave of the 256-row block in the 16-bit kernels (AttnArgs::q_len, attention.hip). O and
    the 16-bit workspace start as NaN: rows below q_len[s] match the reference, the dead rows of the unit that
    straddles q_len[s] are finite, and units wholly past q_len[s] are left unwritten (still NaN).
    Q carries log2(e)/8 and is rounded beforehand (the engine's layout), so the kernel reads exactly these operands.

    Tolerance exception (16-bit modes): the kernel rounds the probabilities P to the operand dtype for the P.V MFMA
    (attention.hip: 16-bit MFMA operands by design), which the bound has no term for. P~_k = P_k (1 + e_k) with
    |e_k| <= u, the operand dtype's unit roundoff. Taking the e_k as independent and uniform (variance u^2 / 3), the
    numerator sum_k P_k e_k V_k has standard deviation (u / sqrt 3) sqrt(sum_k P_k^2 V_k^2), and a row sum formed
    from the rounded P moves O by a relative (u / sqrt 3) sqrt(sum_k P_k^2). The bound gains six standard deviations
    of the two, elementwise: 6 (u / sqrt 3) (sqrt(P^2 . V^2) + sqrt(sum P^2) |R64|), a sixth of the worst case
    2 u (P . |V|) on these inputs and below the p_k |v_k| ~ 3e-3 that one dropped or extra key would leave. Nothing
    is added in the fp32 mode. The ratio without the term is printed too ("no-P-term")."""
    _need_gpu()
    S, H, N = 2, 2, 300
    q_len = torch.tensor([300, 70], dtype=torch.int32)
    g = torch.Generator(device="cpu").manual_seed(300)
    Q, K, V = (torch.randn(S, H, N, 64, generator=g) for _ in range(3))
    Q, K, V = R.rnd(Q * C.Q_SCALE, compute), R.rnd(K, compute), R.rnd(V, compute)
    kv = q_len if kv_masked else None
    u = R.U_OUT[compute]
    O = op_attention(_dev(Q), _dev(K), _dev(V), kv, compute=compute, q_prescaled=True, poison=True, q_len=q_len).cpu()
    r64, pv2, p2 = R.attention(Q, K, V, kv, F64, log2_scores=True)
    r32 = R.attention(Q, K, V, kv, F32, log2_scores=True)[0]
    extra = 6 * u / 3 ** 0.5 * (pv2 + p2 * r64.abs())
    unit = 64 if compute == "fp32" else 32
    for s in range(S):
        ql = int(q_len[s])
        end = min(N, (ql + unit - 1) // unit * unit)
        what = f"attention/{compute}/kv={int(kv_masked)}-s{s}"
        print(f"[op-parity-info] {what}: no-P-term ratio {R.excess_ratio(O[s, :ql], r64[s, :ql], r32[s, :ql], u):.1f}")
        R.assert_close(O[s, :ql], r64[s, :ql], r32[s, :ql], u, what, extra=extra[s, :ql])
        assert torch.isfinite(O[s, ql:end]).all(), "dead rows of the straddling unit"
        assert torch.isnan(O[s, end:]).all(), "units wholly past q_len were written"
