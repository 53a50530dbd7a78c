"""The MXFP8 kernels on the device (compute="mxfp8"): the quantisers against the CPU oracle bit for bit, the fused
LayerNorm quantiser against its two-launch composition bit for bit, and the MX8 GEMM against the exact integer product,
against an fp64 reference computed from the operands the device itself quantised, and for row independence.

fp64 parity uses the project's bound (op_reference.assert_close): |out - R64| <= u_out |R64| + 8 max|R32 - R64|, with
R64 / R32 the epilogue in float64 / float32 on the DEQUANTISED operands the hook returned, so the quantisation error is
not part of the comparison (it is the format's, and the sampling tests bound its effect).

The accumulation allowance. The bf16 kernels meet the factor 8 on max|R32 - R64| (op_reference.ACC_FACTOR); the
block-scaled MFMA does not: over the cases of this file the worst measured excess on MI355X is 142.655 x max|R32 - R64|
(gemm_mx8/gelu_tanh-257x192x128, where max|R32 - R64| = 1.74e-6: 2.5e-4 beyond the output's rounding, on sums whose
rows are scaled by up to 8; EPI_QKV's q reaches 116.5, so it is not the GELU's slope). The operand and scale maps are
exact (test_gemm_exact_integers is bitwise on 129 x 192 x 640, every tile, wave and K-step) and rows are independent,
so the excess is put down to the instruction's internal sum of its 128 products, which exact small integers do not
exercise; that attribution is an inference, the ratio is the measurement. As the issue provides for that case, this
file (and only this file) uses twice the measured ratio, MX8_ACC_FACTOR = 2 x 142.655; every case prints its ratio
(pytest -s).

Shapes: M in {1, 17, 129, 257} (one row; below, one past and two past the 128-row tile), N in {128, 192, 384} (one tile,
a ragged tile, three tiles), K in {128, 640} (one K-step and five). EPI_QKV scatters whole sequences, so with seq_len 13
its M are the multiples of 13 in the same tile regimes (13, 26, 130, 260), N = 3 * 2 heads * 64; its ragged case is
M = 129 as the segments 1 / 63 / 65."""

import functools

import pytest
import torch

import dit_options_reference as D
import mx8_reference as MX
import op_reference as R
from f5_tts_amd import engine as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
U_BF16 = R.U_OUT["bf16"]
Q_SCALE = 0.125 * 1.4426950408889634
MX8_ACC_FACTOR = 2 * 142.655  # twice the worst measured ratio (module docstring)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rand(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bf(t):
    return t.to(torch.bfloat16).float()


# ---------------------------------------------------------------- quantisers
def _quant_input(M, K, seed):
    """bf16 values whose 32-blocks range over 2^-40 .. 2^40, with zero blocks, blocks whose amax is 448 2^k exactly
    and its next bf16 up (the scale rule's boundary), a block of one value, and negative maxima."""
    g = torch.Generator().manual_seed(seed)
    nb = K // 32
    e = torch.randint(-40, 41, (M, nb), generator=g).float()
    x = torch.randn(M, nb, 32, generator=g) * torch.exp2(e)[..., None]
    x = _bf(x)
    for i in range(M * nb):
        m, b = divmod(i, nb)
        kind = (i * 7 + seed) % 6
        if kind == 0:
            x[m, b] = 0.0
        elif kind in (1, 2):
            amax = 448.0 * 2.0 ** float(e[m, b])
            if kind == 2:
                amax = float(torch.nextafter(torch.tensor(amax, dtype=torch.bfloat16),
                                             torch.tensor(float("inf"), dtype=torch.bfloat16)))
            x[m, b] = _bf(torch.rand(32, generator=g) * amax)
            x[m, b, (i * 5) % 32] = -amax if i % 2 else amax
        elif kind == 3:
            x[m, b] = 0.0
            x[m, b, (i * 3) % 32] = -float(2.0 ** float(e[m, b]))
    return x.reshape(M, K)


@pytest.mark.parametrize("K", [32, 160, 256])
@pytest.mark.parametrize("M", [1, 5, 64, 67])
def test_quant_rows_equals_the_oracle(M, K):
    _need_gpu()
    x = _quant_input(M, K, 3 * M + K)
    q, s = E.op_quant_mx8(x.to(DEV))
    oq, os_ = MX.quantize(x)
    assert torch.equal(s.cpu(), os_), (M, K)
    assert torch.equal(q.cpu(), oq), (M, K)
    assert int((q.cpu() & 0x7F).max()) <= 0x7E


def test_quant_rows_non_finite_inputs():
    _need_gpu()
    x = _quant_input(5, 160, 9)
    x[0, 3], x[1, 40], x[4, 159] = float("nan"), float("inf"), float("-inf")
    q, s = E.op_quant_mx8(x.to(DEV))
    oq, os_ = MX.quantize(x)
    assert torch.equal(q.cpu(), oq) and torch.equal(s.cpu(), os_)
    assert q[0, 3] == q[1, 40] == q[4, 159] == MX.NAN_BYTE


@pytest.mark.parametrize("h16", [False, True])
@pytest.mark.parametrize("d", [1024, 768, 512, 128, 2048])
def test_ln_modulate_mx8_is_the_composition(d, h16):
    """ln_modulate_mx8(h) == quant_rows_mx8(ln_modulate(h)) bit for bit, for every kernel variant (d 1024 / 768 / 512 /
    generic, fp32 or bf16 h) and M below and above the 4 rows of a block; a constant row (zero variance) included."""
    _need_gpu()
    for M in (1, 5, 67):
        h = _rand(d + M, M, d) * 3.0 + 0.5
        if M > 1:
            h[1] = 2.5
        shift, scale = _rand(d + 1, d, scale=0.5), _rand(d + 2, d, scale=0.5)
        q, s = E.op_ln_modulate_mx8(h.to(DEV), shift, scale, h16=h16)
        ln = E.op_norm("ln", h.to(DEV), shift, scale, h16=h16, compute="bf16")
        q2, s2 = E.op_quant_mx8(ln)
        assert torch.equal(s, s2), (d, M, h16)
        assert torch.equal(q, q2), (d, M, h16)
        oq, os_ = MX.quantize(ln.cpu())
        assert torch.equal(q.cpu(), oq) and torch.equal(s.cpu(), os_)


# ---------------------------------------------------------------- GEMM: exact integers
def _int_operand(rows, K, seed):
    """Integers in [-8, 8] times a power of two per 32-block (2^-1, 1, 2, distinct along the row and across rows),
    every block holding +-8: the scale rule puts 8 2^e at 256 2^(s-127), all values are e4m3 numbers, and a product
    of two operands sums exactly in fp32 in any order (|sum| < 2^18, multiples of 2^-2)."""
    g = torch.Generator().manual_seed(seed)
    nb = K // 32
    v = torch.randint(-8, 9, (rows, nb, 32), generator=g).float()
    v[:, :, 0] = 8.0 * (1 - 2 * torch.randint(0, 2, (rows, nb), generator=g).float())
    e = ((torch.arange(rows)[:, None] * 2 + torch.arange(nb)[None, :]) % 3 - 1).float()
    return (v * torch.exp2(e)[..., None]).reshape(rows, K)


@pytest.mark.parametrize("M,N,K", [(16, 128, 128), (129, 192, 640)])
def test_gemm_exact_integers(M, N, K):
    """The operand and scale lane maps of the scaled MFMA: with exact data the product is the integer product, bit
    for bit (a wrong K chunk, a scale taken from another block or row, or swapped rows and columns cannot pass:
    W is asymmetric and every block of every row has its own scale)."""
    _need_gpu()
    A, W = _int_operand(M, K, 1), _int_operand(N, K, 2)
    C0 = torch.zeros(M, N)
    out, (a8, as_, w8, ws) = E.op_gemm_mx8("resid16", A.to(DEV), W.to(DEV), C=C0)
    assert torch.equal(MX.dequantize(a8, as_), A.double()) and torch.equal(MX.dequantize(w8, ws), W.double())
    assert len(torch.unique(as_.cpu())) == 3
    want = (A.double() @ W.double().t()).to(torch.bfloat16).float()
    assert torch.equal(out.cpu(), want)


# ---------------------------------------------------------------- GEMM: fp64 parity
MS, NS, KS = (1, 17, 129, 257), (128, 192, 384), (128, 640)


def _operands(M, N, K, seed):
    A = _rand(seed, M, K) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=torch.Generator().manual_seed(seed)).float())
    W = _rand(seed + 1, N, K, scale=K ** -0.5)
    return A, W, _rand(seed + 2, N, scale=0.2)


def _deq(ops):
    a8, as_, w8, ws = ops
    return MX.dequantize(a8, as_), MX.dequantize(w8, ws)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_gemm_gelu_and_resid16_fp64_parity(M, N, K):
    _need_gpu()
    A, W, bias = _operands(M, N, K, 11 * M + N + K)
    out, ops = E.op_gemm_mx8("gelu_tanh", A.to(DEV), W.to(DEV), bias=bias)
    Ad, Wd = _deq(ops)
    assert torch.equal(ops[0].cpu(), MX.quantize(_bf(A))[0]) and torch.equal(ops[3].cpu(), MX.quantize(_bf(W))[1])
    R.assert_close(out.cpu(), R.gemm_epi("gelu_tanh", Ad, Wd, bias, dtype=F64),
                   R.gemm_epi("gelu_tanh", Ad.float(), Wd.float(), bias, dtype=F32), U_BF16,
                   f"gemm_mx8/gelu_tanh-{M}x{N}x{K}", factor=MX8_ACC_FACTOR)
    C0, gate = _bf(_rand(5, M, N)), _rand(6, N)
    keep = torch.ones(M, dtype=torch.uint8)
    keep[M // 2:: 3] = 0
    out, ops = E.op_gemm_mx8("resid16", A.to(DEV), W.to(DEV), bias=bias, C=C0, gate=gate, rowkeep=keep)
    kw = dict(C=C0, gate=gate, keep=keep)
    R.assert_close(out.cpu(), R.gemm_epi("resid16", Ad, Wd, bias, dtype=F64, **kw),
                   R.gemm_epi("resid16", Ad.float(), Wd.float(), bias, dtype=F32, **kw), U_BF16,
                   f"gemm_mx8/resid16-{M}x{N}x{K}", factor=MX8_ACC_FACTOR)
    dead = keep == 0
    assert torch.equal(out.cpu()[dead], C0[dead]), "masked rows keep their residual"


H, L13 = 2, 13


def _qkv_ref(Ad, Wd, bias, norm, rope, seq_len, dtype):
    pre = R.gemm_epi("store", Ad.to(dtype), Wd.to(dtype), bias, dtype=dtype)
    if norm:
        pre = D.qk_norm_pre(pre, H, norm["q_norm_w"], norm["k_norm_w"], dtype=dtype)
    return R.gemm_epi("qkv", None, None, pre=pre, seq_len=seq_len, heads=H, rope_heads=1, q_scale=Q_SCALE,
                      rope=rope[:seq_len], dtype=dtype)


@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", [13, 26, 130, 260])
def test_gemm_qkv_fp64_parity(M, K, qk_norm):
    _need_gpu()
    N = 3 * H * 64
    A, W, bias = _operands(M, N, K, 7 * M + K)
    norm = dict(q_norm_w=1.0 + 0.3 * _rand(44, 64), k_norm_w=1.0 + 0.3 * _rand(45, 64)) if qk_norm else {}
    (q, k, v, rope), ops = E.op_gemm_mx8("qkv", A.to(DEV), W.to(DEV), bias=bias, seq_len=L13, heads=H, rope_heads=1,
                                         q_scale=Q_SCALE, **norm)
    Ad, Wd = _deq(ops)
    rope = rope.cpu()
    r64, r32 = (_qkv_ref(Ad, Wd, bias, norm, rope, L13, dt) for dt in (F64, F32))
    for nm, o, a, b in zip("qkv", (q, k, v), r64, r32):
        R.assert_close(o.cpu(), a, b, U_BF16, f"gemm_mx8/qkv-{nm}-{M}x{N}x{K}-qkn{int(qk_norm)}",
                       factor=MX8_ACC_FACTOR)


@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("K", KS)
def test_gemm_qkv_ragged_fp64_parity(K, qk_norm):
    """Packed rows of three sequences (1, 63, 65 rows) into padded panels of 65 rows: every sequence against the
    reference on its own rows, rotated from position 0; panel rows past a length stay as the caller left them."""
    _need_gpu()
    off, N = (0, 1, 64, 129), 3 * H * 64
    A, W, bias = _operands(129, N, K, 3 + K)
    norm = dict(q_norm_w=1.0 + 0.3 * _rand(44, 64), k_norm_w=1.0 + 0.3 * _rand(45, 64)) if qk_norm else {}
    (q, k, v, rope), ops = E.op_gemm_mx8("qkv", A.to(DEV), W.to(DEV), bias=bias, heads=H, rope_heads=1, q_scale=Q_SCALE,
                                         qkv_dst_len=65, seg_off=off, **norm)
    Ad, Wd = _deq(ops)
    rope = rope.cpu()
    for s in range(3):
        o, n = off[s], off[s + 1] - off[s]
        r64, r32 = (_qkv_ref(Ad[o: o + n], Wd, bias, norm, rope, n, dt) for dt in (F64, F32))
        for nm, got, a, b in zip("qkv", (q, k, v), r64, r32):
            R.assert_close(got.cpu()[s, :, :n], a[0], b[0], U_BF16,
                           f"gemm_mx8/qkv-ragged-{nm}-s{s}-K{K}-qkn{int(qk_norm)}", factor=MX8_ACC_FACTOR)
            assert torch.isnan(got[s, :, n:]).all()


# ---------------------------------------------------------------- GEMM: row independence
@functools.lru_cache(maxsize=None)
def _big():
    A, W, bias = _operands(257, 384, 640, 99)
    out, _ = E.op_gemm_mx8("gelu_tanh", A.to(DEV), W.to(DEV), bias=bias)
    return A, W, bias, out.cpu()


@pytest.mark.parametrize("rows", [(200,), tuple(range(100, 117)), tuple(range(256, 127, -1)), (0, 256, 128, 127, 1)])
def test_gemm_rows_keep_their_bits_for_any_M_and_position(rows):
    """One tile configuration and a fixed K order: a row's output depends on its own A row only."""
    _need_gpu()
    A, W, bias, big = _big()
    idx = torch.tensor(rows)
    out, _ = E.op_gemm_mx8("gelu_tanh", A[idx].contiguous().to(DEV), W.to(DEV), bias=bias)
    assert torch.equal(out.cpu(), big[idx])
