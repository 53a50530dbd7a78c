"""Op-level checks of the kernels behind isolated batches (use_batch_mask == 2) and MMDiT key masks: attention over
two key ranges against a float64 softmax over the valid keys, and the length-aware GRN / depthwise-conv text kernels
against the plain ops on each sequence alone (bitwise).

Attention bound: the one tests/test_gpu_ops.py::test_attention_q_len uses for f5h_op_attention (R.assert_close,
factor 8 on max|R32 - R64|, the stored output's unit roundoff, and in the 16-bit modes its P-rounding term derived
there), on inputs prepared the same way (Q carries log2(e)/8, all three rounded to the operand dtype beforehand)."""

import pytest
import torch

import op_cases as C
import op_reference as R
from f5_tts_amd.engine import op_attention, op_attention_ranges, op_dwconv_ln, op_grn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ranges_ref(Q, K, V, valid, dtype):
    """R.attention (log2 scores) with an arbitrary key mask valid [S, N]; a sequence without a valid key gives 0."""
    S, H, N, _ = Q.shape
    sc = Q.to(dtype) @ K.to(dtype).transpose(-1, -2)
    sc = sc.masked_fill(~valid[:, None, None, :], float("-inf"))
    mx = sc.amax(-1, keepdim=True)
    p = torch.exp2(sc - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)))
    p = p / p.sum(-1, keepdim=True).clamp_min(torch.finfo(dtype).tiny)
    Vd = V.to(dtype)
    fold = lambda t: t.transpose(1, 2).reshape(S, N, H * 64)  # noqa: E731
    return (fold(p @ Vd), fold(torch.sqrt(p.square() @ Vd.square())),
            fold(torch.sqrt(p.square().sum(-1, keepdim=True)).expand(S, H, N, 64)))


# (L, kv_start2, kv_len, kv_len2): A = the joint shape of golden_cases.B3 (150 audio + 64 text rows) with an
# unaligned second base; B = tile-exact, one-key and empty ranges
RANGE_CASES = {
    "A": (214, 150, [90, 150, 70], [20, 30, 12]),
    "B": (192, 128, [64, 128, 1], [64, 1, 0]),
}


@pytest.mark.parametrize("compute", C.COMPUTES)
@pytest.mark.parametrize("case", sorted(RANGE_CASES))
def test_attention_ranges(compute, case):
    """Valid keys [0, kv_len[s]) and [kv_start2, kv_start2 + kv_len2[s]): every query row against the float64 softmax
    over those keys; then the same call with every K / V row outside the ranges set to NaN must stay finite and
    bitwise equal (rows outside the ranges are never read, and no masked score reaches the P.V product)."""
    _need_gpu()
    L, st2, kv1, kv2 = RANGE_CASES[case]
    S, H = 3, 2
    g = torch.Generator(device="cpu").manual_seed(214)
    Q, K, V = (torch.randn(S, H, L, 64, generator=g) for _ in range(3))
    Q, K, V = R.rnd(Q * C.Q_SCALE, compute), R.rnd(K, compute), R.rnd(V, compute)
    pos = torch.arange(L)[None, :]
    kv1_t, kv2_t = torch.tensor(kv1)[:, None], torch.tensor(kv2)[:, None]
    valid = (pos < kv1_t) | ((pos >= st2) & (pos < st2 + kv2_t))
    u = R.U_OUT[compute]
    O = op_attention_ranges(Q.to(DEV), K.to(DEV), V.to(DEV), kv1, st2, kv2, compute=compute, q_prescaled=True).cpu()
    r64, pv2, p2 = _ranges_ref(Q, K, V, valid, F64)
    r32 = _ranges_ref(Q, K, V, valid, F32)[0]
    extra = 6 * u / 3 ** 0.5 * (pv2 + p2 * r64.abs())
    R.assert_close(O, r64, r32, u, f"attention_ranges/{compute}/{case}", extra=extra)
    dead = ~valid[:, None, :, None].expand(S, H, L, 64)
    Kn, Vn = K.masked_fill(dead, float("nan")), V.masked_fill(dead, float("nan"))
    On = op_attention_ranges(Q.to(DEV), Kn.to(DEV), Vn.to(DEV), kv1, st2, kv2, compute=compute, q_prescaled=True).cpu()
    assert torch.isfinite(On).all(), "a key row outside the ranges was read"
    assert torch.equal(On, O)


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_attention_ranges_without_a_second_range_is_the_qlen_hook(compute):
    """kv_len2 = nullptr: the kernels f5h_op_attention_qlen launches, bit for bit (with and without q_len)."""
    _need_gpu()
    S, H, L = 3, 2, 214
    g = torch.Generator(device="cpu").manual_seed(7)
    Q, K, V = (torch.randn(S, H, L, 64, generator=g).to(DEV) for _ in range(3))
    kv = torch.tensor([90, 150, 70], dtype=torch.int32)
    a = op_attention_ranges(Q, K, V, kv, 150, None, q_len=torch.full((S,), L), compute=compute)
    b = op_attention(Q, K, V, kv, compute=compute, q_len=torch.full((S,), L, dtype=torch.int32))
    assert torch.equal(a, b)
    assert torch.equal(op_attention_ranges(Q, K, V, kv, 0, None, compute=compute),
                       op_attention(Q, K, V, kv, compute=compute))


LEN_CASES = [[90, 150, 70], [64, 65, 1]]  # B3's frames; the 64-row chunk of the GRN partials exactly, one past, one row


def _garbage_past(x, lens):
    """Rows past each sequence's length filled with large finite garbage (what a padded batch may hold there)."""
    x = x.clone()
    for s, n in enumerate(lens):
        x[s, n:] = 1e4 * (1 + torch.arange(x.shape[1] - n)[:, None] % 7) * torch.sign(x[s, n:] + 0.5)
    return x


@pytest.mark.parametrize("compute", C.COMPUTES)
@pytest.mark.parametrize("lens", LEN_CASES, ids=["b3", "chunk"])
def test_grn_len(compute, lens):
    """op_grn with a length per sequence: rows below len[s] equal, bitwise, op_grn of that sequence alone at
    L = len[s], whatever the rows past it hold."""
    _need_gpu()
    S, L, Cc = 3, 150, 128
    g = torch.Generator(device="cpu").manual_seed(128)
    x = _garbage_past(torch.randn(S, L, Cc, generator=g), lens)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    out = op_grn(x.to(DEV), gamma, beta, compute=compute, seq_len=lens).cpu()
    for s, n in enumerate(lens):
        alone = op_grn(x[s:s + 1, :n].contiguous().to(DEV), gamma, beta, compute=compute).cpu()
        assert torch.equal(out[s, :n], alone[0]), (s, n)


@pytest.mark.parametrize("compute", C.COMPUTES)
@pytest.mark.parametrize("lens", LEN_CASES, ids=["b3", "chunk"])
def test_dwconv_ln_len(compute, lens):
    """op_dwconv_ln with a length per sequence as the tap bound: rows below len[s] equal, bitwise, op_dwconv_ln of
    that sequence alone at L = len[s] (the three rows before the end would otherwise read the garbage past it)."""
    _need_gpu()
    S, L, Cc = 3, 150, 64
    g = torch.Generator(device="cpu").manual_seed(64)
    x = _garbage_past(torch.randn(S, L, Cc, generator=g), lens)
    dw_w, dw_b = torch.randn(Cc, 7, generator=g), torch.randn(Cc, generator=g)
    ln_w, ln_b = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    out = op_dwconv_ln(x.to(DEV), dw_w, dw_b, ln_w, ln_b, compute=compute, seq_len=lens).cpu()
    for s, n in enumerate(lens):
        alone = op_dwconv_ln(x[s:s + 1, :n].contiguous().to(DEV), dw_w, dw_b, ln_w, ln_b, compute=compute).cpu()
        assert torch.equal(out[s, :n], alone[0]), (s, n)
