"""Op-level fp64 parity of the LayerNorm / RMSNorm fold (DESIGN.md §3 'LayerNorm fold'): the GEMM epilogue forms the
other op tests leave out (tests/test_gpu_ops.py), each stage alone through its production launcher and then chained.

    producer   EPI_RESID16 with hs / ln_part (LayerNorm form) or ln_rms (RMSNorm form)
    consumer   EPI_GELU_TANH / EPI_QKV with ln_part_in, per chunk row (128-row tiles and below) and once per row
               (256x256 tiles): every output is bitwise equal across the tile configurations, which compares the two
    lnfold_uv  the per-step u / v vectors; scale_cols: W' = W diag(g) of the RMSNorm form

References (tests/op_reference.py) are written from the definitions in DESIGN.md §3; inputs and the reason for every
shape are in tests/op_cases.py; tests/test_op_refs.py shows that the wrong variants of every reference miss the same
bounds on the same inputs. Tolerance as in tests/test_gpu_ops.py: |out - R64| <= u_out |R64| + 8 max|R32 - R64|, with
the extra terms derived where they are used (test_lnfold_uv, test_fold_composition). hs and scale_cols are bitwise
(one fp32 multiply and one rounding); so is every row of a consumer whose neighbour's partials are not finite
(test_fold_consumer_rows_independent).

Worst measured ratio on the MI355X per op and compute mode (the bound is 8):

    op                        bf16    fp16
    producer C                0.27    0.16
    producer strip mean       1.00    1.50
    producer strip M2         2.39    1.67
    consumer GELU             0.56    1.17
    consumer QKV              0.99    1.49
    lnfold_uv                 < 0     1.24    (without the split term 21.7 bf16, 1032 fp16: fp16 keeps subnormal lo parts)
    composition, LayerNorm    < 0     < 0     (without the hs term 1.1e7 bf16, 1.4e6 fp16, on the constant row; the
    composition, RMSNorm      0.00    0.02     largest share of the term an element uses: 0.51 / 0.54 and 0.49 / 0.47)
"""

import pytest
import torch

import op_cases as C
import op_reference as R
from f5_tts_amd import _lib
from f5_tts_amd.engine import gemm_force_config, op_gemm_epi, op_lnfold_uv, op_norm, op_scale_cols
from test_gpu_parity import GEMM_CONFIGS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
MODES = ("bf16", "fp16")  # the fold runs in the 16-bit modes only
G = _lib.OP_GUARD_ROWS


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(t):
    return None if t is None else t.to(DEV)


def _bits_equal(a, b):
    """Bitwise equality that also holds for NaN payloads."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _under_every_config(run):
    """run() under every tile configuration (forced 12 / 13 run the fold as 11 by design): the outputs, as tuples of
    CPU tensors, of the first configuration, after asserting that every other one gives the same bits."""
    outs = []
    try:
        for cfg in GEMM_CONFIGS:
            gemm_force_config(cfg)
            o = run()
            outs.append(tuple(t.cpu() for t in (o if isinstance(o, tuple) else (o,)) if t is not None))
    finally:
        gemm_force_config(-1)
    for cfg, o in zip(GEMM_CONFIGS, outs):
        for i, (t, t0) in enumerate(zip(o, outs[0])):
            assert _bits_equal(t, t0), f"output {i} differs between tile configurations {GEMM_CONFIGS[0]} and {cfg}"
    return outs[0]


# ---------------------------------------------------------------- producer
PROD_PARAMS = [(form, v) for form in ("ln", "rms") for v in C.FOLD_PROD_VARIANTS[form]]


def _check_strip_stats(parts, hp, rms, what):
    """parts [M,np,2] against the fp64 strip statistics of the kernel's own stored h'; exactness on constant strips."""
    r64, r32 = R.strip_stats(hp, F64, rms), R.strip_stats(hp, F32, rms)
    R.assert_close(parts[..., 0], r64[..., 0], r32[..., 0], 0.0, what + "/strip-mean")
    R.assert_close(parts[..., 1], r64[..., 1], r32[..., 1], 0.0, what + "/strip-M2")
    strips = hp.reshape(hp.shape[0], -1, 64)
    const = strips.amax(-1) == strips.amin(-1)
    if rms:
        assert (parts[..., 0] == 0).all(), what + ": the RMSNorm form's strip mean is exactly 0"
        zero = const & (strips[..., 0] == 0)
        assert (parts[..., 1][zero] == 0).all(), what + ": an all-zero strip has sum of squares 0"
    else:
        assert (parts[..., 1][const] == 0).all(), what + ": M2 of a constant strip is exactly 0"
        assert torch.equal(parts[..., 0][const], strips[..., 0][const]), what + ": mean of a constant strip is its value"
    return int(const.sum())


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("form,variant", PROD_PARAMS)
def test_fold_producer(compute, form, variant):
    """EPI_RESID16 as the fold's producer. LayerNorm form (with gate and resid, and in place): C is bitwise the C of
    the same launch without the fold fields and meets the resid16 bound; hs is bitwise round(fp32(h') fp32(1 +
    scale)) of the kernel's own returned h'; the partials are the (mean, M2) of each 64-column strip of that h',
    M2 exactly 0 and the mean exactly the value on a constant strip. RMSNorm form (plain, and with rowkeep over a
    separate residual): the strip "mean" is exactly 0, M2 the strip's sum of squares; a masked row's C is the
    residual unchanged and its statistics are that row's. (The launcher refuses hs in this form, so there is no hs
    buffer to leave untouched.) Guard rows past M stay NaN: the store descriptors end at row M; the live rows start
    as NaN too and none is left."""
    _need_gpu()
    rms = form == "rms"
    for M, N, K in C.FOLD_PROD_SHAPES:
        c = C.fold_prod_case(compute, form, variant, M, N, K)
        A, W = _dev(c["A"]), _dev(c["W"])
        kw = dict(bias=c["bias"], C=c["C"], compute=compute, resid=c.get("resid"), gate=c["gate"],
                  rowkeep=c.get("keep"))
        what = f"fold_producer/{compute}/{form}-{variant}-{M}x{N}x{K}"
        Cf, *rest = _under_every_config(lambda: op_gemm_epi("resid16", A, W, ln_producer=True, ln_rms=rms, poison=True,
                                                            hs_scale=c.get("hs_scale"), **kw))
        plain = op_gemm_epi("resid16", A, W, **kw).cpu()
        assert _bits_equal(Cf, plain), what + ": C differs from the launch without the fold"
        ref = lambda dt: C.gemm_ref(c, dt)  # noqa: E731
        R.assert_close(Cf, ref(F64), ref(F32), c["u_out"], what + "/C")
        if "keep" in c:
            dead = ~c["keep"]
            assert torch.equal(Cf[dead], c["resid_read"][dead]), what + ": a masked row is the residual unchanged"
        if rms:
            (parts,) = rest
        else:
            hs, parts = rest
            assert hs.shape == (M + G, N)
            assert torch.isnan(hs[M:]).all(), what + ": hs guard rows were written"
            assert _bits_equal(hs[:M], R.fold_hs(Cf, c["hs_scale"], compute)), what + ": hs != round(h' (1 + scale))"
        assert parts.shape == (M + G, N // 64, 2)
        assert torch.isnan(parts[M:]).all(), what + ": partials' guard rows were written"
        assert torch.isfinite(parts[:M]).all(), what + ": a strip's partial was left unwritten"
        n_const = _check_strip_stats(parts[:M], Cf, rms, what)
        if c["special"] and (c["exact"] or "keep" in c):
            # the planted constant row arrives exactly (all its strips), and with a zero bias the constant strip too
            assert n_const >= N // 64 + (1 if c["exact"] else 0), what + ": planted constant strips did not arrive"
            if rms:
                assert (Cf[6] == 0).all() and (parts[6] == 0).all(), what + ": the all-zero row"


# ---------------------------------------------------------------- consumer
def _gelu_run(c, compute, parts=None):
    A, W = _dev(c["A"]), _dev(c["W"])
    p = c["parts"] if parts is None else parts
    return lambda: op_gemm_epi("gelu_tanh", A, W, bias=c["bias"], compute=compute, ln_part_in=p, ln_u=c["u"],
                               ln_v=c["v"], ln_rms=c["rms"], ln_eps=c["eps"])


def _qkv_run(c, spec, compute, parts=None):
    L, _, rh, qs = spec
    A, W = _dev(c["A"]), _dev(c["W"])
    p = c["parts"] if parts is None else parts
    return lambda: op_gemm_epi("qkv", A, W, bias=c["bias"], compute=compute, seq_len=L, heads=C.FOLD_QKV_H,
                               rope_heads=rh, q_scale=qs, ln_part_in=p, ln_u=c["u"], ln_v=c["v"], ln_rms=c["rms"],
                               ln_eps=c["eps"])


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("form", ["ln", "rms"])
def test_fold_consumer_gelu(compute, form):
    """EPI_GELU_TANH with ln_part_in alone: hs (or h' for the RMSNorm form), the partials, u and v are supplied
    already representable in the types the kernel reads, so the standard tolerance applies with no extra term.
    Reference: the combine of DESIGN.md §3, x = rstd (hs W^T - mean u) + v + b, GELU-tanh. eps 1e-6 (LayerNorm) and
    1e-30 (RMSNorm, u = v = null), where the all-zero row gives gelu(bias), finite."""
    _need_gpu()
    for M, d, N in C.FOLD_GELU_SHAPES:
        c = C.fold_cons_case(compute, form, M, d, N)
        (out,) = _under_every_config(_gelu_run(c, compute))
        what = f"fold_gelu/{compute}/{form}-{M}x{N}x{d}"
        r64 = C.fold_gelu_ref(c, F64)
        R.assert_close(out, r64, C.fold_gelu_ref(c, F32), c["u_out"], what)
        if form == "rms" and M >= 8:
            act = torch.nn.functional.gelu(c["bias"].double(), approximate="tanh")
            assert torch.equal(r64[6], act), "reference: the all-zero row is gelu(bias)"
            assert torch.isfinite(out[6]).all()


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("form", ["ln", "rms"])
def test_fold_consumer_qkv(compute, form):
    """EPI_QKV with ln_part_in alone: heads = 4 (N = 768 = 3 x 256), two sequences of 70 or 150 rows, RoPE on all
    heads and on the first only, q unscaled and scaled; q, k and v all carry the normalisation. The reference reads
    the (cos, sin) table the kernel read."""
    _need_gpu()
    for spec in C.FOLD_QKV_CASES:
        L, d, rh, qs = spec
        c = C.fold_cons_case(compute, form, 2 * L, d, 3 * C.FOLD_QKV_H * 64)
        q, k, v, rope = _under_every_config(_qkv_run(c, spec, compute))
        r64, r32 = C.fold_qkv_ref(c, spec, rope, F64), C.fold_qkv_ref(c, spec, rope, F32)
        for nm, o, a, b in zip("qkv", (q, k, v), r64, r32):
            R.assert_close(o, a, b, c["u_out"], f"fold_qkv/{compute}/{form}-{nm}-L{L}-d{d}-rope{rh}-qs{qs:.2f}")


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_fold_consumer_rows_independent(compute, bad):
    """A row's statistics come from its own partials only. With np = d / 64 < 16 the once-per-row form fetches 16
    partials (128 bytes) from the row's base, so its tail is the next row's: partials of row r + 1 that are NaN or
    +Inf must leave every other row bitwise as it was, under every tile configuration (d = 768: np = 12, d = 128:
    np = 2; GELU and QKV forms)."""
    _need_gpu()
    for d, bad_row in ((768, 2), (128, 2), (768, 69)):
        c = C.fold_cons_case(compute, "ln", 70, d, 256)
        (base,) = _under_every_config(_gelu_run(c, compute))
        parts = c["parts"].clone()
        parts[bad_row] = bad
        (out,) = _under_every_config(_gelu_run(c, compute, parts))
        rows = torch.arange(70) != bad_row
        assert _bits_equal(out[rows], base[rows]), f"d={d}: a row changed with its neighbour's partials = {bad}"
    for spec in ((70, 768, 1, C.Q_SCALE), (70, 128, 0, 0.0)):
        L, d = spec[:2]
        c = C.fold_cons_case(compute, "ln", 2 * L, d, 3 * C.FOLD_QKV_H * 64)
        base = _under_every_config(_qkv_run(c, spec, compute))
        parts = c["parts"].clone()
        parts[L + 1] = bad                                  # row 1 of the second sequence
        out = _under_every_config(_qkv_run(c, spec, compute, parts))
        pos = torch.arange(L) != 1
        for nm, o, b in zip("qkv", out, base):
            assert _bits_equal(o[0], b[0]) and _bits_equal(o[1][:, pos], b[1][:, pos]), \
                f"d={d}: {nm} rows changed with a neighbour's partials = {bad}"


# ---------------------------------------------------------------- lnfold_uv / scale_cols
@pytest.mark.parametrize("compute", MODES)
def test_lnfold_uv(compute):
    """lnfold_uv: u = sum_k (1 + sc_k) W[n,k], v = sum_k sh_k W[n,k] against fp64 on the rounded W, for FFN1 (mlp rows)
    and QKV (msa rows) of both layers and every step; nfe around the 16-step group.

    Tolerance. The kernel enters each fp32 x (= 1 + sc, or sh) as two 16-bit parts, hi = round(x) and lo = round(x -
    hi), and accumulates hi W + lo W in fp32. |x - hi| <= u_op |x| and rounding that remainder leaves |x - hi - lo|
    <= u_op^2 |x| per term (u_op = 2^-8 bf16, 2^-11 fp16). Taking the residuals as independent and uniform (variance
    (u_op^2 x)^2 / 3), the sum over k has standard deviation (u_op^2 / sqrt 3) sqrt(sum_k (x_k W_nk)^2); the bound
    gains six of them. In fp16 the lo part lies below 2^-14 whenever |x| u_op < 2^-14, where fp16's spacing is the
    fixed 2^-24: its rounding error is then up to 2^-25 whatever x is, which adds 6 (2^-25 / sqrt 3) sqrt(sum_k
    W_nk^2). This holds only if subnormal lo parts survive the conversion and the MFMA: a kernel that flushes them
    misses this bound by two orders of magnitude on the small shifts of the last step (tests/test_op_refs.py).
    All of it on top of 8 max|R32 - R64|; the outputs are fp32, so u_out = 0.

    The modulation rows and every float outside the u / v blocks (the gap before them, the tail of the row, the
    guard row past nfe) come back bitwise; the u / v blocks start as NaN."""
    _need_gpu()
    for d, F, nfe in C.LNFOLD_CASES:
        c = C.lnfold_case(compute, d, F, nfe)
        out = op_lnfold_uv(_dev(c["table"]), _dev(c["W1"]), _dev(c["Wqkv"]), nfe, c["out_off"], compute=compute).cpu()
        lo, hi = c["out_off"], c["out_off"] + c["depth"] * c["LW"]
        assert _bits_equal(out[:, :lo], c["table"][:, :lo]), "modulation rows / gap changed"
        assert _bits_equal(out[:, hi:], c["table"][:, hi:]), "the row's tail changed"
        assert _bits_equal(out[nfe:], c["table"][nfe:]), "a step >= nfe was written"
        r64, r32 = R.lnfold_uv(c["mod"], c["W1"], c["Wqkv"], F64), R.lnfold_uv(c["mod"], c["W1"], c["Wqkv"], F32)
        extra = R.lnfold_uv_extra(c["mod"], c["W1"], c["Wqkv"], compute)
        for nm, o, a, b, e in zip(("u1", "v1", "u2", "v2"), C.lnfold_blocks(c, out, d, F, nfe), r64, r32, extra):
            what = f"lnfold_uv/{compute}/{nm}-d{d}-F{F}-nfe{nfe}"
            print(f"[op-parity-info] {what}: no-split-term ratio {R.excess_ratio(o, a, b, 0.0):.1f}")
            R.assert_close(o, a, b, 0.0, what, extra=e)


@pytest.mark.parametrize("compute", MODES)
def test_scale_cols(compute):
    """scale_cols: bitwise round(fp32(W) g[k]), whole blocks and a ragged last one."""
    _need_gpu()
    for rows, K in C.SCALE_COLS_SHAPES:
        c = C.scale_cols_case(compute, rows, K)
        out = op_scale_cols(_dev(c["W"]), c["g"], compute=compute).cpu()
        assert _bits_equal(out, R.scale_cols(c["W_read"], c["g"], compute)), (rows, K)


# ---------------------------------------------------------------- composition
def _gelu_tanh_lipschitz():
    """max |d/dx gelu_tanh(x)| (~1.129, near x = 1.5), from the derivative on a fine float64 grid."""
    x = torch.linspace(-8.0, 8.0, 160001, dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(torch.nn.functional.gelu(x, approximate="tanh").sum(), x)
    return float(g.abs().max()) * (1 + 1e-6)


def _through_qkv(e, rope, L, heads, q_scale):
    """An elementwise bound e [M, 3 heads 64] on the pre-activation carried through RoPE (all heads) / q scale /
    scatter: a pair (a, b) -> (a cos - b sin, b cos + a sin) moves by at most (|cos| e_a + |sin| e_b, |cos| e_b +
    |sin| e_a); q is then scaled. Returns bounds shaped as q, k, v [S,H,L,64]."""
    M, inner = e.shape[0], heads * 64
    S = M // L
    cos, sin = rope[..., 0].double().abs()[None, :, None, :], rope[..., 1].double().abs()[None, :, None, :]
    outs = []
    for i in range(3):
        t = e[:, i * inner:(i + 1) * inner].reshape(S, L, heads, 64)
        if i < 2:
            a, b = t[..., 0::2], t[..., 1::2]
            t = torch.stack((cos * a + sin * b, cos * b + sin * a), dim=-1).flatten(-2)
        if i == 0 and q_scale != 0.0:
            t = t * q_scale
        outs.append(t.permute(0, 2, 1, 3).contiguous())
    return outs


def _term_used(out, r64, r32, u_out, extra):
    """The largest share of the derived term an element uses: max (|out - R64| - u_out |R64| - 8 max|R32 - R64|) /
    extra."""
    acc = R.ACC_FACTOR * float((r32.double() - r64).abs().max())
    exc = (out.double() - r64).abs() - u_out * r64.abs() - acc
    return float((exc / extra.double().clamp_min(1e-300)).max())


def _report(what, fold, unfolded, r64, M):
    """Per row kind, the largest error of the fold and of the unfolded launches against the same fp64 definition."""
    kinds = {0: "ordinary", **C.FOLD_ROW_KINDS}
    for r, name in kinds.items():
        rows = [i for i in range(M) if i == 0 or i > 6] if r == 0 else [r]
        ef = float((fold[rows].double() - r64[rows]).abs().max())
        eu = float((unfolded[rows].double() - r64[rows]).abs().max())
        print(f"[fold-cost] {what} row kind {name!r}: fold {ef:.3e} unfolded {eu:.3e} (max|R64| "
              f"{float(r64[rows].abs().max()):.2f})")


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("form", ["ln", "rms"])
def test_fold_composition(compute, form):
    """The kernels' own outputs chained, producer -> consumer, with u / v from lnfold_uv (LayerNorm form) or W' from
    scale_cols (RMSNorm form), against the fp64 definition: ln_modulate(h') W^T + b or rms_norm(h', g) W^T + b, then
    GELU-tanh (FFN1, N = 256) or RoPE / q scale / scatter (QKV, N = 3 d); d = 768 and 1024, M = 70, h' the producer's
    own stored output.

    Here the fold's one designed-in deviation shows, and the bound gains a derived term for it, as the attention
    test's does for the rounded probabilities. The consumer's operand is hs_k = h'_k (1 + sc_k) (1 + e_k) with |e_k|
    <= u_op (one rounding to the operand dtype), where the unfolded path rounds the normalised value instead. Taking
    the e_k as independent and uniform (variance u_op^2 / 3) the pre-activation x = rstd (hs W^T - mean u) + v + b moves
    by a sum with standard deviation (u_op / sqrt 3) rstd sqrt(sum_k (h'_k (1 + sc_k) W_nk)^2); the bound gains six of
    them. RMSNorm form: the same with g_k for (1 + sc_k), from rounding W' = W g. To this the u / v allowance of
    test_lnfold_uv is added, times |mean| rstd and rstd, the factors u and v enter x with. The sum e is carried through
    the epilogue by its Lipschitz bound: GELU-tanh has |gelu'| <= 1.129 (_gelu_tanh_lipschitz); RoPE maps a pair's
    (e_a, e_b) to (|cos| e_a + |sin| e_b, |cos| e_b + |sin| e_a), and q is then scaled (_through_qkv).
    The ratio without the term is printed ("no-hs-term"), and per row kind the largest error of the fold and of the
    unfolded launches (op_norm + the plain GEMM) against the same definition: a measurement, recorded in DESIGN.md
    §3; nothing is asserted about the comparison beyond the derived bound."""
    _need_gpu()
    rms = form == "rms"
    M, K0, F, L = 70, 64, 256, 70
    u_op = R.U_OUT[compute]
    lip = _gelu_tanh_lipschitz()
    for d in (768, 1024):
        heads = d // 64
        g = torch.Generator(device="cpu").manual_seed(4200 + d + rms)
        W1 = R.rnd(torch.randn(2, F, d, generator=g) / d ** 0.5, compute)
        Wq = R.rnd(torch.randn(2, 3 * d, d, generator=g) / d ** 0.5, compute)
        b1, bq = 2.0 * torch.randn(F, generator=g), torch.randn(3 * d, generator=g)
        pc = C.fold_prod_case(compute, form, "plain" if rms else "inplace", M, d, K0)
        pkw = dict(bias=pc["bias"], C=pc["C"], compute=compute, gate=pc["gate"], ln_producer=True, ln_rms=rms,
                   poison=True)
        if rms:
            gain = 1.0 + 0.5 * torch.randn(d, generator=g)
            hp, _, parts = op_gemm_epi("resid16", _dev(pc["A"]), _dev(pc["W"]), **pkw)
            hp, parts = hp.cpu(), parts[:M].cpu()
            chains = {"ffn1": dict(A=hp, W=op_scale_cols(_dev(W1[1]), gain, compute=compute), Wd=W1[1], mul=gain),
                      "qkv": dict(A=hp, W=op_scale_cols(_dev(Wq[1]), gain, compute=compute), Wd=Wq[1], mul=gain)}
            ckw = dict(ln_rms=True, ln_eps=C.FOLD_EPS["rms"])
            define = lambda Wd, mul, dt: R.rms_norm(hp, gain, dtype=dt) @ Wd.to(dt).t()  # noqa: E731
            rstd = (d ** 0.5 / hp.double().norm(dim=-1, keepdim=True).clamp_min(1e-12))
            mean = torch.zeros(M, 1, dtype=F64)
        else:
            # step 1 of 2, layer 1 of 2: FFN1 reads the mlp rows (3, 4), QKV the msa rows (0, 1)
            mod = torch.randn(2, 2, 6, d, generator=g)
            mod[:, :, (0, 3)] *= 0.1
            mod[:, :, (1, 4)] *= 0.3
            LW, off = 2 * F + 6 * d, 2 * 6 * d
            table = torch.full((2, off + 2 * LW), float("nan"))
            table[:, :off] = mod.reshape(2, -1)
            tab = op_lnfold_uv(_dev(table), _dev(W1), _dev(Wq), 2, off, compute=compute)
            blk = tab[1, off + LW:off + 2 * LW]
            uv = dict(ffn1=(blk[:F], blk[F:2 * F]), qkv=(blk[2 * F:2 * F + 3 * d], blk[2 * F + 3 * d:]))
            ex = [t[1, 1] for t in R.lnfold_uv_extra(mod, W1, Wq, compute)]
            chains = {}
            for name, Wd, si, ci, (eu, ev) in (("ffn1", W1[1], 3, 4, ex[:2]), ("qkv", Wq[1], 0, 1, ex[2:])):
                sh, sc = mod[1, 1, si], mod[1, 1, ci]
                hp, hs, parts = op_gemm_epi("resid16", _dev(pc["A"]), _dev(pc["W"]), hs_scale=sc, **pkw)
                chains[name] = dict(A=hs[:M], W=_dev(Wd), Wd=Wd, mul=1.0 + sc.double(), sh=sh, sc=sc, eu=eu, ev=ev,
                                    u=uv[name][0], v=uv[name][1])
            hp, parts = hp.cpu(), parts[:M].cpu()   # the same h' and partials in both launches (hs_scale differs)
            ckw = dict(ln_eps=C.FOLD_EPS["ln"])
            define = lambda ch, dt: R.ln_modulate(hp, ch["sh"], ch["sc"], dtype=dt) @ ch["Wd"].to(dt).t()  # noqa: E731
            mean = hp.double().mean(-1, keepdim=True)
            rstd = 1.0 / torch.sqrt(hp.double().var(-1, unbiased=False, keepdim=True) + 1e-6)
        for name, ch in chains.items():
            bias = b1 if name == "ffn1" else bq
            what = f"fold_composition/{compute}/{form}-d{d}-{name}"
            pre = {dt: (define(ch["Wd"], ch["mul"], dt) if rms else define(ch, dt)) + bias.to(dt) for dt in (F64, F32)}
            # the hs (W') rounding term and the u / v term of the pre-activation
            e = 6 * u_op / 3 ** 0.5 * rstd * torch.sqrt(
                (hp.double() * ch["mul"]).square() @ ch["Wd"].double().square().t())
            if not rms:
                e = e + ch["eu"][None] * mean.abs() * rstd + ch["ev"][None] * rstd
            fkw = dict(bias=bias, compute=compute, ln_part_in=parts, ln_u=ch.get("u"), ln_v=ch.get("v"), **ckw)
            if rms:
                normed = op_norm("rms", _dev(hp), gain, h16=True, compute=compute)
            else:
                normed = op_norm("ln", _dev(hp), ch["sh"], ch["sc"], h16=True, compute=compute)
            if name == "ffn1":
                out = op_gemm_epi("gelu_tanh", _dev(ch["A"]), ch["W"], **fkw).cpu()
                unf = op_gemm_epi("gelu_tanh", normed, _dev(ch["Wd"]), bias=bias, compute=compute).cpu()
                r64, r32 = (R.gemm_epi("gelu_tanh", None, None, pre=pre[dt], dtype=dt) for dt in (F64, F32))
                print(f"[op-parity-info] {what}: no-hs-term ratio {R.excess_ratio(out, r64, r32, u_op):.1f}, "
                      f"share of the term used {_term_used(out, r64, r32, u_op, lip * e):.2f}")
                R.assert_close(out, r64, r32, u_op, what, extra=lip * e)
                _report(what, out, unf, r64, M)
            else:
                qkw = dict(seq_len=L, heads=heads, rope_heads=0, q_scale=C.Q_SCALE)
                q, k, v, rope = (t.cpu() for t in op_gemm_epi("qkv", _dev(ch["A"]), ch["W"], **fkw, **qkw))
                unf = [t.cpu() for t in op_gemm_epi("qkv", normed, _dev(ch["Wd"]), bias=bias, compute=compute, **qkw)]
                r64, r32 = (R.gemm_epi("qkv", None, None, pre=pre[dt], dtype=dt, rope=rope, **qkw) for dt in (F64, F32))
                for nm, o, uo, a, b, ee in zip("qkv", (q, k, v), unf, r64, r32, _through_qkv(e, rope, L, heads, C.Q_SCALE)):
                    print(f"[op-parity-info] {what}-{nm}: no-hs-term ratio {R.excess_ratio(o, a, b, u_op):.1f}, "
                          f"share of the term used {_term_used(o, a, b, u_op, ee):.2f}")
                    R.assert_close(o, a, b, u_op, f"{what}-{nm}", extra=ee)
                    # [1,H,L,64] -> rows
                    rows = lambda t: t[0].permute(1, 0, 2).reshape(M, -1)  # noqa: E731
                    _report(f"{what}-{nm}", rows(o), rows(uo), rows(a), M)
