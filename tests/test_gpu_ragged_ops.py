"""The ragged forms of the four ops that reach across rows (ragged sampling): each is compared with the
existing per-sequence op run once per sequence, bit for bit.

Segment lengths (1, 63, 65, 129), R = 258: a one-row sequence, sequences either side of the 64-row boundary (the
attention key tile, the GRN chunk), a GEMM row tile that holds three sequences, attention query blocks and conv
position blocks that straddle a segment boundary. fp32 and bf16. Attention and the conv also run with NaN where a
neighbour stands: a neighbour is never read, so the bits stay those of the clean run."""

import functools

import pytest
import torch

from f5_tts_amd import engine as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENS = (1, 63, 65, 129)
OFF = (0, 1, 64, 129, 258)
R, LMAX, S = 258, 129, 4
COMPUTES = ("fp32", "bf16")
Q_SCALE = 0.125 * 1.4426950408889634


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rand(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _segs():
    return [(s, OFF[s], LENS[s]) for s in range(S)]


# ---------------------------------------------------------------- attention
@functools.lru_cache(maxsize=None)
def _attn_inputs():
    H = 2
    return tuple(_rand(11 + i, S, H, LMAX, 64) for i in range(3))


def _attn_panels(fill):
    """The padded panels with `fill` in every row past a sequence's length."""
    out = []
    for t in _attn_inputs():
        t = t.clone()
        for s, _o, n in _segs():
            t[s, :, n:] = fill
        out.append(t)
    return out


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("compute", COMPUTES)
def test_attention_ragged_equals_per_sequence(compute, prescaled):
    _need_gpu()
    Q, K, V = _attn_panels(float("nan"))  # rows past a length are never read
    O = E.op_attention_ragged(Q, K, V, OFF, compute=compute, q_prescaled=prescaled)
    assert O.shape == (R, 128) and torch.isfinite(O).all()
    for s, o, n in _segs():
        one = E.op_attention(Q[s: s + 1, :, :n].contiguous(), K[s: s + 1, :, :n].contiguous(),
                             V[s: s + 1, :, :n].contiguous(), compute=compute, q_prescaled=prescaled)
        assert torch.equal(O[o: o + n], one[0]), (compute, s)


@pytest.mark.parametrize("compute", COMPUTES)
def test_attention_ragged_never_reads_a_neighbour(compute):
    """Two sequences (63, 65 rows); the second one's panels hold NaN throughout: the first one's bits are the clean
    run's."""
    _need_gpu()
    Q, K, V = (t[1:3].clone() for t in _attn_panels(0.0))
    off = (0, 63, 128)
    clean = E.op_attention_ragged(Q, K, V, off, compute=compute, q_prescaled=True)
    for t in (Q, K, V):
        t[1] = float("nan")
        t[0, :, 63:] = float("nan")
    dirty = E.op_attention_ragged(Q, K, V, off, compute=compute, q_prescaled=True)
    assert torch.isfinite(clean).all()
    assert torch.equal(dirty[:63], clean[:63])


# ---------------------------------------------------------------- conv position embedding
def _conv_inputs(d=128):
    return (_rand(21, R, d), _rand(22, d, d // 16, 31, scale=0.05), _rand(23, d, scale=0.1), _rand(24, R, d))


@pytest.mark.parametrize("compute,mode,x_as_f32", [("fp32", 0, True), ("fp32", 1, True), ("bf16", 0, True),
                                                   ("bf16", 2, False)])
def test_conv_pos_ragged_equals_per_sequence(compute, mode, x_as_f32):
    """The engine's two launches per mode: the first reads the fp32 input embedding (mode 0), the second the first
    one's output and adds the residual (mode 1 in fp32, mode 2 on the 16-bit residual stream)."""
    _need_gpu()
    x, w, b, resid = _conv_inputs()
    y = E.op_conv_pos_ragged(x, w, b, OFF, mode=mode, resid=resid if mode else None, x_as_f32=x_as_f32, compute=compute)
    assert y.shape == (R, 128) and torch.isfinite(y).all()
    for s, o, n in _segs():
        one = E.op_conv_pos(x[None, o: o + n].contiguous(), w, b, mode=mode,
                            resid=resid[None, o: o + n].contiguous() if mode else None, x_as_f32=x_as_f32,
                            compute=compute)
        assert torch.equal(y[o: o + n], one[0]), (compute, mode, s)


@pytest.mark.parametrize("compute,mode,x_as_f32", [("fp32", 1, True), ("bf16", 2, False)])
def test_conv_pos_ragged_never_reads_a_neighbour(compute, mode, x_as_f32):
    _need_gpu()
    x, w, b, resid = (t[:128].clone() if t.shape[0] == R else t for t in _conv_inputs())
    off = (0, 63, 128)
    clean = E.op_conv_pos_ragged(x, w, b, off, mode=mode, resid=resid, x_as_f32=x_as_f32, compute=compute)
    x[63:] = float("nan")
    resid[63:] = float("nan")
    dirty = E.op_conv_pos_ragged(x, w, b, off, mode=mode, resid=resid, x_as_f32=x_as_f32, compute=compute)
    assert torch.isfinite(clean).all()
    assert torch.equal(dirty[:63], clean[:63])


# ---------------------------------------------------------------- GRN
@pytest.mark.parametrize("compute", COMPUTES)
def test_grn_ragged_equals_per_sequence(compute):
    _need_gpu()
    C = 128
    x, gamma, beta = _rand(31, R, C), _rand(32, C), _rand(33, C)
    out = E.op_grn_ragged(x, gamma, beta, OFF, compute=compute)
    assert torch.isfinite(out).all()
    for s, o, n in _segs():
        one = E.op_grn(x[None, o: o + n].contiguous(), gamma, beta, compute=compute)
        assert torch.equal(out[o: o + n], one[0]), (compute, s)


# ---------------------------------------------------------------- QKV epilogue
@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("rope_heads", [0, 1])
@pytest.mark.parametrize("compute", COMPUTES)
def test_qkv_ragged_equals_per_sequence(compute, rope_heads, qk_norm):
    _need_gpu()
    H, K = 2, 128
    A, W, bias = _rand(41, R, K), _rand(42, 3 * H * 64, K, scale=0.1), _rand(43, 3 * H * 64, scale=0.1)
    norm = dict(q_norm_w=_rand(44, 64).abs() + 0.5, k_norm_w=_rand(45, 64).abs() + 0.5) if qk_norm else {}
    q, k, v, _rope = E.op_gemm_epi("qkv", A, W, bias, compute=compute, heads=H, rope_heads=rope_heads, q_scale=Q_SCALE,
                                   qkv_dst_len=LMAX, seg_off=OFF, **norm)
    assert q.shape == (S, H, LMAX, 64)
    for s, o, n in _segs():
        q1, k1, v1, _r = E.op_gemm_epi("qkv", A[o: o + n].contiguous(), W, bias, compute=compute, seq_len=n, heads=H,
                                       rope_heads=rope_heads, q_scale=Q_SCALE, **norm)
        for name, got, want in (("q", q, q1), ("k", k, k1), ("v", v, v1)):
            assert torch.isfinite(want).all()
            assert torch.equal(got[s, :, :n], want[0]), (compute, name, s)
            assert torch.isnan(got[s, :, n:]).all(), "rows past the length stay as the caller left them"


def test_ragged_hooks_refuse_bad_tables():
    _need_gpu()
    x, gamma, beta = _rand(31, 10, 128), _rand(32, 128), _rand(33, 128)
    with pytest.raises(RuntimeError, match="seg"):
        E.op_grn_ragged(x, gamma, beta, (0, 5, 5, 10))  # an empty segment
    with pytest.raises(RuntimeError, match="seg"):
        E.op_grn_ragged(x, gamma, beta, (0, 5, 9))  # does not end at R
