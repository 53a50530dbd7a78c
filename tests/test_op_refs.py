"""The op-level parity tests can tell right from wrong (no GPU): on the inputs tests/test_gpu_ops.py feeds the
kernels, the float32 form R32 of every reference meets the tolerance against the float64 form R64, and every
deliberately wrong float64 variant (op_reference.WRONG_*) misses it on at least one case of every compute mode's
set. A variant that slipped through would mean the inputs are too tame to expose that mistake in a kernel.

Also here: the new op entry points refuse shapes outside their launchers' contracts with F5H_EINVAL before any
device work. The conv weight packing (pack_conv_weight, engine_pack.cpp) runs as a device kernel and cannot be called
on the host; it is covered by the GPU conv tests, which pass the torch-layout weight through it.

The same for tests/test_gpu_glue_ops.py (audio glue, prologue and ODE step kernels), at the end of this module: the
arithmetic references and their wrong variants, NaN / inf propagation of the log and spectrum references, and each
bitwise torch restatement tied to an independent definition (F.conv1d, torch.stft, the oracle's TextEmbedding and
lens_to_mask, tests/ode_reference.py).
"""

import ctypes
import math

import pytest
import torch

import op_cases as C
import op_reference as R

F64, F32 = torch.float64, torch.float32


def _judge(cases, ref, variants):
    """cases: [(label, case)]. R32 must pass every case; returns {variant: worst ratio} over the set."""
    worst = {v: 0.0 for v in variants}
    for label, c in cases:
        r64, r32 = ref(c, F64), ref(c, F32)
        ok = R.excess_ratio(r32, r64, r32, c["u_out"])
        assert ok <= 1.0, (label, ok)  # R32 against its own distance: never above 1
        for v in variants:
            worst[v] = max(worst[v], R.excess_ratio(ref(c, F64, v), r64, r32, c["u_out"]))
    return worst


def _all_rejected(worst, compute):
    for v, ratio in worst.items():
        assert ratio > R.ACC_FACTOR, f"{compute}: wrong variant {v!r} passes the tolerance (worst ratio {ratio:.3g})"


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_conv_pos_wrong_variants_rejected(compute):
    cases = [(i, C.conv_case(compute, i)) for i in range(len(C.CONV_CASES[compute]))]
    _all_rejected(_judge(cases, C.conv_ref, R.WRONG_CONV), compute)


@pytest.mark.parametrize("compute", C.COMPUTES)
@pytest.mark.parametrize("kind", ["ln", "rms"])
def test_norm_wrong_variants_rejected(compute, kind):
    cases = [((d, M, h16), C.norm_case(compute, kind, d, M, h16)) for d, M in C.NORM_SHAPES
             for h16 in ((False, True) if compute != "fp32" else (False,))]
    ref = lambda c, dt, v=None: C.norm_ref(kind, c, dt, v)  # noqa: E731
    _all_rejected(_judge(cases, ref, R.WRONG_LN if kind == "ln" else R.WRONG_RMS), compute)


def test_rms_zero_row_is_zero_not_nan():
    c = C.norm_case("bf16", "rms", 1024, 5, True)
    for dt in (F64, F32):
        out = C.norm_ref("rms", c, dt)
        assert torch.isfinite(out).all() and (out[4] == 0).all()


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_dwconv_ln_wrong_variants_rejected(compute):
    cases = [(s, C.dwconv_case(compute, *s)) for s in C.DWCONV_SHAPES]
    _all_rejected(_judge(cases, C.dwconv_ref, R.WRONG_LN), compute)
    flat = C.dwconv_case(compute, 64, 7, True)
    out = C.dwconv_ref(flat, F64)
    assert torch.equal(out, flat["ln_b"].double().expand_as(out)), "zero-variance rows normalise to the LN bias"


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_grn_wrong_variants_rejected(compute):
    cases = [(s, C.grn_case(compute, *s)) for s in C.GRN_SHAPES]
    _all_rejected(_judge(cases, C.grn_ref, R.WRONG_GRN), compute)


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_gemm_epilogue_wrong_variants_rejected(compute):
    by_epi = {}
    for name, (epi, _) in C.GEMM_CASES.items():
        for shape in C.gemm_shapes_of(name):
            by_epi.setdefault(epi, []).append(((name,) + shape, C.gemm_case(compute, name, *shape)))
    for epi, cases in by_epi.items():
        _all_rejected(_judge(cases, C.gemm_ref, R.WRONG_GEMM.get(epi, ())), compute)


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_qkv_wrong_variants_rejected(compute):
    rope = C.rope_table_f32(C.QKV_L)
    assert (rope.double() - R.rope_table(C.QKV_L)).abs().max() < 4 * C.QKV_L * 2.0 ** -24 + 1e-6
    worst = {v: 0.0 for v in R.WRONG_GEMM["qkv"]}
    for spec in C.QKV_CASES:
        c = C.qkv_case(compute, *spec)
        r64, r32 = C.qkv_ref(c, rope, F64), C.qkv_ref(c, rope, F32)
        for v in worst:
            bad = C.qkv_ref(c, rope, F64, v)
            for o, a, b in zip(bad, r64, r32):
                worst[v] = max(worst[v], R.excess_ratio(o, a, b, c["u_out"]))
        for a, b in zip(r64, r32):
            assert R.excess_ratio(b, a, b, c["u_out"]) <= 1.0
    _all_rejected(worst, compute)


def test_excess_ratio_flags_non_finite_and_exact_zero():
    z = torch.zeros(4)
    assert R.excess_ratio(z, z, z, 0.0) == 0.0
    assert R.excess_ratio(z + 1e-30, z, z, 0.0) == math.inf
    assert R.excess_ratio(torch.tensor([float("nan")]), torch.ones(1), torch.ones(1), 0.0) == math.inf


def test_op_gemm_args_layout_matches_c(tmp_path):
    """The ctypes mirror of f5h_op_gemm_args has the C layout (as test_boundary checks the engine's structs)."""
    import os
    import subprocess

    from f5_tts_amd import _lib

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "f5h.h")
    fields = ("k_split", "A", "C", "live_seq", "q_scale", "add", "dual_rows", "rope_out", "hs_scale", "hs_out",
              "ln_part_out", "ln_part_in", "ln_u", "ln_v", "ln_nparts", "ln_rms", "ln_eps", "poison")
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                    '  printf("%%zu", sizeof(f5h_op_gemm_args));\n%s  return 0;\n}\n'
                    % (header, "".join('  printf(" %%zu", offsetof(f5h_op_gemm_args, %s));\n' % f for f in fields)))
    exe = tmp_path / "layout"
    prog.write_text(prog.read_text().replace("  return 0;", '  printf(" %d", F5H_OP_GUARD_ROWS);\n  return 0;'))
    subprocess.run(["gcc", str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == ([ctypes.sizeof(_lib.OpGemmArgs)] + [getattr(_lib.OpGemmArgs, f).offset for f in fields]
                   + [_lib.OP_GUARD_ROWS])


def test_op_entry_points_refuse_bad_shapes():
    """Shapes outside a launcher's contract: F5H_EINVAL with a message, before any device work (null tensors and
    a null workspace are never touched)."""
    from f5_tts_amd import _lib

    L = _lib.lib()

    def refused(rc, word):
        assert rc == -1, rc
        assert word.encode() in L.f5h_last_error(), L.f5h_last_error()

    for d in (64, 200, 1152):  # d % 128, d > 1024
        refused(L.f5h_op_conv_pos(None, 1, 1, 8, d, None, None, None, None, 0, None, 1, 8, 0, None, None, 0), "d % 128")
    refused(L.f5h_op_conv_pos(None, 0, 1, 8, 128, None, None, None, None, 2, None, 1, 8, 0, None, None, 0), "mode 2")
    refused(L.f5h_op_conv_pos(None, 1, 1, 8, 128, None, None, None, None, 3, None, 1, 8, 0, None, None, 0), "mode")
    for kind in (0, 1):
        for d in (102, 2052, 4096):  # d % 4, d > 2048
            refused(L.f5h_op_norm(None, 1, kind, 0, 4, d, None, None, None, None, None, 0), "d % 4")
    refused(L.f5h_op_norm(None, 0, 0, 1, 4, 256, None, None, None, None, None, 0), "16-bit")
    refused(L.f5h_op_dwconv_ln(None, 1, 2, 8, 1025, None, None, None, None, None, None, None, 0), "C <= 1024")
    refused(L.f5h_op_grn(None, 1, 0, 8, 64, None, None, None, None, None, 0), "bad shape")
    a = _lib.OpGemmArgs()
    a.compute, a.epi, a.M, a.N, a.K = 1, 0, 8, 128, 96
    refused(L.f5h_op_gemm_epi(None, ctypes.byref(a), None, 0), "K % 64")
    a.K, a.epi = 128, 11
    refused(L.f5h_op_gemm_epi(None, ctypes.byref(a), None, 0), "epilogue")
    a.epi, a.N = 6, 100  # INPROJ: 8-column rows
    a.A = a.W = 256  # never dereferenced: validation fails first
    refused(L.f5h_op_gemm_epi(None, ctypes.byref(a), None, 0), "INPROJ")
    a.epi, a.N, a.heads, a.seq_len = 7, 100, 2, 4  # QKV: N = 3 * heads * 64
    refused(L.f5h_op_gemm_epi(None, ctypes.byref(a), None, 0), "QKV")
    a.epi, a.N, a.A2, a.k_split = 0, 128, 256, 32
    refused(L.f5h_op_gemm_epi(None, ctypes.byref(a), None, 0), "k_split")

    # ---- the LayerNorm / RMSNorm fold forms: launch_t's contract (gemm_impl.h)
    P = 256  # a non-null pointer that is never dereferenced

    def fold_args(**kw):
        """A valid LayerNorm-form producer (resid16, N = 256, K = 64), then the overrides."""
        b = _lib.OpGemmArgs()
        b.compute, b.epi, b.M, b.N, b.K = 1, 9, 8, 256, 64
        b.A = b.W = b.C = b.hs_scale = b.hs_out = b.ln_part_out = P
        b.ln_nparts = 4
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def cons_args(**kw):
        """A valid LayerNorm-form consumer (gelu_tanh, N = 256, K = 128), then the overrides."""
        return fold_args(**{**dict(epi=2, K=128, hs_scale=None, hs_out=None, ln_part_out=None, ln_part_in=P, ln_u=P,
                                   ln_v=P, ln_nparts=2, ln_eps=1e-6), **kw})

    for b, word in (
            (fold_args(compute=0), "16-bit"),
            (fold_args(ln_part_in=P), "together"),
            (fold_args(ln_part_out=None), "without ln_part_out"),
            (fold_args(ln_nparts=0), "1..16"), (fold_args(ln_nparts=17), "1..16"),
            (fold_args(N=2048, ln_nparts=32), "1..16"),
            (fold_args(ln_nparts=3), "N / 64"), (cons_args(ln_nparts=4), "K / 64"),
            (fold_args(N=192, ln_nparts=3), "N % 128"), (cons_args(N=192), "N % 128"),
            (fold_args(rowkeep=P, live_len=P, live_seq=8, ln_rms=1, hs_scale=None, hs_out=None), "live_len"),
            (fold_args(rowkeep=P), "rowkeep"),
            (fold_args(hs_scale=None), "hs_scale"), (fold_args(hs_out=None), "hs_scale"),
            (fold_args(ln_rms=1), "hs_scale"), (fold_args(ln_rms=1, hs_out=None), "hs_scale"),
            (fold_args(ln_u=P), "ln_u"), (fold_args(epi=4), "EPI_RESID16"),
            (cons_args(ln_u=None), "ln_u"), (cons_args(ln_v=None), "ln_u"), (cons_args(ln_rms=1), "ln_u"),
            (cons_args(ln_rms=1, ln_v=None), "ln_u"), (cons_args(hs_scale=P), "hs_scale"),
            (cons_args(epi=10), "EPI_GELU_TANH"), (cons_args(ln_rms=2), "ln_rms")):
        refused(L.f5h_op_gemm_epi(None, ctypes.byref(b), None, 0), word)
    # (a valid fold call passes validation and fails only on the missing workspace)
    for b in (fold_args(), fold_args(ln_rms=1, hs_scale=None, hs_out=None, rowkeep=P), cons_args(),
              cons_args(ln_rms=1, ln_u=None, ln_v=None)):
        assert L.f5h_op_gemm_epi(None, ctypes.byref(b), None, 0) == -4 and b"workspace" in L.f5h_last_error()
    refused(L.f5h_op_scale_cols(None, 1, 8, 12, P, P, P, None, 0), "K % 8")
    refused(L.f5h_op_scale_cols(None, 0, 8, 16, P, P, P, None, 0), "16-bit")
    refused(L.f5h_op_lnfold_uv(None, 1, 4, 1, 100, 256, P, 4096, 1024, P, P, None, 0), "d % 64")
    refused(L.f5h_op_lnfold_uv(None, 0, 4, 1, 128, 256, P, 4096, 1024, P, P, None, 0), "16-bit")
    refused(L.f5h_op_lnfold_uv(None, 1, 4, 1, 128, 256, P, 4096, 512, P, P, None, 0), "modulation rows")   # overlaps
    refused(L.f5h_op_lnfold_uv(None, 1, 4, 1, 128, 256, P, 2000, 768, P, P, None, 0), "inside the row")    # too narrow
    refused(L.f5h_op_lnfold_uv(None, 1, 4, 1, 128, 256, P, 4098, 768, P, P, None, 0), "stride % 4")


# ---------------------------------------------------------------- LayerNorm / RMSNorm fold
MODES16 = ("bf16", "fp16")


@pytest.mark.parametrize("compute", MODES16)
@pytest.mark.parametrize("form", ["ln", "rms"])
def test_fold_consumer_wrong_variants_rejected(compute, form):
    """The consumer's references on the inputs of test_gpu_fold_ops: R32 meets the bound, every wrong combine and
    every wrong application misses it."""
    variants = (R.WRONG_COMBINE_LN + R.WRONG_CONSUMER) if form == "ln" else R.WRONG_COMBINE_RMS
    cases = [((M, d, N), C.fold_cons_case(compute, form, M, d, N)) for M, d, N in C.FOLD_GELU_SHAPES]
    worst = _judge(cases, C.fold_gelu_ref, variants)
    worst.update({v: 0.0 for v in R.WRONG_CONSUMER_QKV})
    for spec in C.FOLD_QKV_CASES:
        L, d = spec[:2]
        rope = C.rope_table_f32(L)
        c = C.fold_cons_case(compute, form, 2 * L, d, 3 * C.FOLD_QKV_H * 64)
        r64, r32 = C.fold_qkv_ref(c, spec, rope, F64), C.fold_qkv_ref(c, spec, rope, F32)
        for a, b in zip(r64, r32):
            assert R.excess_ratio(b, a, b, c["u_out"]) <= 1.0
        for v in worst:
            for o, a, b in zip(C.fold_qkv_ref(c, spec, rope, F64, v), r64, r32):
                worst[v] = max(worst[v], R.excess_ratio(o, a, b, c["u_out"]))
    _all_rejected(worst, compute)


def test_fold_rms_zero_row_is_act_of_bias():
    c = C.fold_cons_case("bf16", "rms", 70, 768, 256)
    assert (c["hp"][6] == 0).all() and (c["parts"][6] == 0).all()
    for dt in (F64, F32):
        out = C.fold_gelu_ref(c, dt)
        assert torch.isfinite(out).all()
        assert torch.equal(out[6], torch.nn.functional.gelu(c["bias"].to(dt), approximate="tanh"))


@pytest.mark.parametrize("compute", MODES16)
def test_fold_strip_stats_and_bitwise_refs(compute):
    """Strip statistics: the fp32 two-pass form meets its own bound, constant strips give (value, 0) exactly, and a
    stale or shifted strip does not. hs and scale_cols are compared bitwise on the device: their wrong variants must
    differ in the rounded result."""
    for form in ("ln", "rms"):
        rms = form == "rms"
        c = C.fold_cons_case(compute, form, 70, 768, 256)
        r64, r32 = R.strip_stats(c["hp"], F64, rms), R.strip_stats(c["hp"], F32, rms)
        for i in (0, 1):
            assert R.excess_ratio(r32[..., i], r64[..., i], r32[..., i], 0.0) <= 1.0
        assert (r32[3, :, 1] == (64 * 9.0 if rms else 0.0)).all() and (r32[3, :, 0] == (0.0 if rms else 3.0)).all()
        assert r32[4, 1, 1] == (64 * 0.25 if rms else 0.0)
        # the other form's statistics, and the strips shifted by 8 columns, miss the bound
        for bad in (R.strip_stats(c["hp"], F64, not rms), R.strip_stats(c["hp"].roll(8, 1), F64, rms)):
            assert max(R.excess_ratio(bad[..., i], r64[..., i], r32[..., i], 0.0) for i in (0, 1)) > R.ACC_FACTOR
    c = C.fold_cons_case(compute, "ln", 70, 768, 256)
    for v in R.WRONG_HS:
        assert not torch.equal(R.fold_hs(c["hp"], c["sc"], compute, v), R.fold_hs(c["hp"], c["sc"], compute))
    for rows, K in C.SCALE_COLS_SHAPES:
        s = C.scale_cols_case(compute, rows, K)
        for v in R.WRONG_SCALE_COLS:
            assert not torch.equal(R.scale_cols(s["W_read"], s["g"], compute, v), R.scale_cols(s["W_read"], s["g"], compute))


def _split_sim(mod, W1, Wqkv, compute, flush):
    """lnfold_uv as the kernel forms it, in fp64 sums: x = fp32(1 + sc) or sh, hi = round(x), lo = round(x - hi), each
    rounded to the operand dtype; flush: fp16 lo parts below the smallest normal (2^-14) become 0."""
    def parts(x):
        x = x.float()
        hi = R.rnd(x, compute)
        lo = R.rnd(x - hi, compute)
        if flush:
            lo = torch.where(lo.abs() < 2.0 ** -14, torch.zeros(()), lo)
        return hi.double() + lo.double()
    mm = lambda x, w: torch.einsum("sld,lnd->sln", parts(x), w.double())  # noqa: E731
    m = mod.float()
    return mm(1.0 + m[:, :, 4], W1), mm(m[:, :, 3], W1), mm(1.0 + m[:, :, 1], Wqkv), mm(m[:, :, 0], Wqkv)


@pytest.mark.parametrize("compute", MODES16)
def test_lnfold_uv_wrong_variants_rejected(compute):
    """lnfold_uv's bound (derived in test_gpu_fold_ops.test_lnfold_uv) on the GPU test's inputs: R32 and a simulation
    of the kernel's hi + lo split that keeps subnormal lo parts stay inside it;
    dropping the lo part, flushing subnormal fp16 lo parts, and the wrong-row variants miss it."""
    worst = {v: 0.0 for v in R.WRONG_LNFOLD_UV + (("lo_subnormal_flushed",) if compute == "fp16" else ())}
    for d, F, nfe in C.LNFOLD_CASES:
        c = C.lnfold_case(compute, d, F, nfe)
        args = (c["mod"], c["W1"], c["Wqkv"])
        r64, r32 = R.lnfold_uv(*args, F64), R.lnfold_uv(*args, F32)
        extra = R.lnfold_uv_extra(*args, compute)
        outs = {v: R.lnfold_uv(*args, F64, v, compute) for v in R.WRONG_LNFOLD_UV}
        if compute == "fp16":
            outs["lo_subnormal_flushed"] = _split_sim(*args, compute, True)
        sim = _split_sim(*args, compute, False)
        for i, (a, b, e) in enumerate(zip(r64, r32, extra)):
            assert R.excess_ratio(b, a, b, 0.0, e) <= 1.0
            # the kept-subnormal simulation: inside the split allowance alone
            assert float(((sim[i] - a).abs() / e).max()) <= 1.0, (compute, d, F, nfe, i)
            for v in worst:
                worst[v] = max(worst[v], R.excess_ratio(outs[v][i], a, b, 0.0, e))
    _all_rejected(worst, compute)


# ---------------------------------------------------------------- audio glue, prologue and ODE step kernels
def _ratio_special(out, r64, r32, u_out=0.0):
    """excess_ratio where NaN / +-inf of the reference must be reproduced exactly (else inf) and count as exact."""
    if not R.same_specials(out.double(), r64):
        return math.inf
    sp = ~torch.isfinite(r64)
    z = lambda t: torch.where(sp, torch.zeros((), dtype=torch.float64), t.double())  # noqa: E731
    return R.excess_ratio(z(out), z(r64), z(r32), u_out)


def _judge_special(cases, ref, variants):
    worst = {v: 0.0 for v in variants}
    for label, c in cases:
        r64, r32 = ref(c, F64), ref(c, F32)
        assert _ratio_special(r32, r64, r32) <= 1.0, label
        for v in variants:
            worst[v] = max(worst[v], _ratio_special(ref(c, F64, v), r64, r32))
    return worst


def _ola_cases():
    cases = [((n_fft, hop, T), C.ola_case(n_fft, hop, (T,) * C.OLA_B)) for n_fft, hop in C.OLA_FFT for T in C.OLA_TS]
    return cases + [((n_fft, hop, "ragged"), C.ola_case(n_fft, hop, C.OLA_RAGGED_LENS)) for n_fft, hop in C.OLA_FFT]


def test_glue_arithmetic_refs_wrong_variants_rejected():
    """mel_mag, mel_log, vocos_spec, vocos_ola and time_sinus on the inputs of tests/test_gpu_glue_ops.py: R32 meets
    the bound against R64 on every case, every wrong variant misses it by more than ACC_FACTOR on at least one."""
    _all_rejected(_judge_special([("mag", C.mel_mag_case())], C.mel_mag_ref, R.WRONG_MEL_MAG), "mel_mag")
    B = C.MEL_LOG_B
    log_cases = [((T,), (C.mel_log_case(B * T), [T] * B, None)) for T in C.MEL_LOG_T]
    rg = C.MEL_LOG_RAGGED
    log_cases.append((("ragged",), (C.mel_log_case(sum(rg["frames"])), rg["frames"], rg["T_out"])))
    log_ref = lambda c, dt, v=None: C.mel_log_ref(c[0], c[1], c[2], dt, v)  # noqa: E731
    _all_rejected(_judge_special(log_cases, log_ref, R.WRONG_MEL_LOG), "mel_log")
    _all_rejected(_judge_special([("spec", C.spec_case())], C.spec_ref, R.WRONG_SPEC), "vocos_spec")
    _all_rejected(_judge_special(_ola_cases(), C.ola_ref, R.WRONG_OLA), "vocos_ola")
    ts_cases = [(n, C.time_sinus_case(n)) for n in C.TIME_SINUS_T]
    _all_rejected(_judge_special(ts_cases, C.time_sinus_ref, R.WRONG_TIME_SINUS), "time_sinus")
    for L in C.ROPE_LS:  # the float32 table (as the kernel forms it) meets test_gemm_qkv's bound
        assert (C.rope_table_f32(L).double() - R.rope_table(L)).abs().max() < 4 * L * 2.0 ** -24 + 1e-6


@pytest.mark.parametrize("dtype", [F64, F32])
def test_log_and_spec_refs_propagate_nan_and_inf(dtype):
    """torch's clamp(min).log() and clip(exp, max) keep NaN, in both precisions: the property the kernels must have
    (C fmaxf / fminf would return the other operand). +inf mel stays +inf; m = +inf clips to 100, -inf gives 0."""
    c = C.mel_log_case(2)
    out = C.mel_log_ref(c, [1, 1], None, dtype)
    assert torch.equal(torch.isnan(out.transpose(1, 2).reshape(2, -1)), torch.isnan(c["mel"]))
    assert int(torch.isnan(out).sum()) == 2 and int(torch.isposinf(out).sum()) == 2
    assert (out[0, 0, 0] == math.log(1e-5) or dtype == F32) and out[0, 4 * 13, 0] == 0.0
    s = C.spec_case()
    out = C.spec_ref(s, dtype).reshape(s["rows"], -1, 2)
    nan_pairs = torch.isnan(out).all(-1)
    assert nan_pairs[0, 5] and nan_pairs[1, 7] and int(nan_pairs.sum()) == 2 and int(torch.isnan(out).sum()) == 4
    assert torch.allclose(out[0, 40].norm(), torch.tensor(100.0, dtype=dtype)) and (out[1, 41] == 0).all()
    assert (out[:, s["bins"]:] == 0).all()


def test_im2col_restatement_is_conv1d():
    """im2col followed by the flattened weight is Conv1d(k 7, pad 3): on small integers every sum is exact in fp32,
    so the two agree bit for bit. T below, at and above the window."""
    g = torch.Generator().manual_seed(5)
    for T in C.IM2COL["Ts"]:
        mel = torch.randint(-4, 5, (2, 6, T), generator=g).float()
        w = torch.randint(-3, 4, (5, 6, 7), generator=g).float()
        cols = R.im2col7(mel, 64)
        assert cols.shape == (2 * T, 64) and (cols[:, 42:] == 0).all()
        got = (cols[:, :42] @ w.reshape(5, 42).t()).reshape(2, T, 5).transpose(1, 2)
        assert torch.equal(got, F_conv1d(mel, w))


def F_conv1d(x, w):
    return torch.nn.functional.conv1d(x, w, padding=3)


@pytest.mark.parametrize("n_fft,hop,L", C.MEL_FRAMES_CASES)
def test_framing_restatement_is_torch_stft(n_fft, hop, L):
    """The DFT of the restated frames is torch.stft(center=True, pad_mode="reflect") with a rectangular window."""
    wav = C.mel_frames_case(n_fft, hop, L).double()
    fr = R.mel_frames(wav, n_fft, hop)
    assert fr.shape == (C.MEL_FRAMES_B, 1 + L // hop, n_fft)
    want = torch.stft(wav, n_fft, hop_length=hop, window=torch.ones(n_fft, dtype=F64), center=True,
                      pad_mode="reflect", return_complex=True)
    got = torch.fft.rfft(fr, dim=-1).transpose(1, 2)
    assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())


def _identity_text_block(td, g):
    """Weights of one ConvNeXt text block whose output is its input exactly: pwconv2 is zero, so the block adds 0."""
    p = "text_embed.text_blocks.0."
    return {p + "dwconv.weight": torch.randn(td, 1, 7, generator=g), p + "dwconv.bias": torch.randn(td, generator=g),
            p + "norm.weight": torch.ones(td), p + "norm.bias": torch.zeros(td),
            p + "pwconv1.weight": torch.randn(8, td, generator=g), p + "pwconv1.bias": torch.zeros(8),
            p + "grn.gamma": torch.zeros(1, 1, 8), p + "grn.beta": torch.zeros(1, 1, 8),
            p + "pwconv2.weight": torch.zeros(td, 8), p + "pwconv2.bias": torch.zeros(td)}


def test_text_embed_restatement_is_the_oracles_text_embedding():
    """R.text_embed equals the oracle's TextEmbedding.forward (oracle/ref_cpu.text_embed_dit, the model definition the
    whole-pipeline goldens are built on) for both CFG branches, on every case the GPU test runs except the MMDiT
    position clamp, which the oracle's DiT form does not have. The oracle's ConvNeXt blocks run with a zero last
    layer, i.e. as the identity, so only the embedding is compared."""
    from oracle import ref_cpu

    g = torch.Generator().manual_seed(9)
    for N, td, per, fr, mp in C.TEXT_CASES:
        if fr == "rows4":
            continue
        a = C.text_embed_args(N, td, per, fr, mp)
        ec, eu, keep = R.text_embed(C.TEXT, **a)
        W = {"text_embed.text_embed.weight": a["table"], **_identity_text_block(td, g)}
        arch = dict(conv_layers=0 if fr is None else 1, text_dim=td, text_mask_padding=mp)
        sl = torch.tensor(a["seq_len"]) if per else N
        assert torch.equal(ec, ref_cpu.text_embed_dit(W, arch, C.TEXT, sl, False)), (N, td, per, fr, mp)
        assert torch.equal(eu, ref_cpu.text_embed_dit(W, arch, C.TEXT, sl, True)), (N, td, per, fr, mp)
        zeroed = (ec == 0).all(-1) & (eu == 0).all(-1)
        assert torch.equal(keep[0], keep[1]) and bool((zeroed | keep[0].bool()).all())
    # the clamp against the MMDiT reference's indexing: position n reads row min(n, rows - 1)
    a = C.text_embed_args(9, 100, False, "rows4", False)
    ec, _, _ = R.text_embed(C.TEXT, **a)
    full = R.text_embed(C.TEXT, **{**a, "freqs": C.text_table(100)[1], "freq_rows": 0})[0]
    assert torch.equal(ec[:, :4], full[:, :4]) and not torch.equal(ec[:, 4:], full[:, 4:])
    freqs4 = a["freqs"]
    assert torch.equal(ec[:, 5:], a["table"][0] + freqs4[3].expand(2, 4, 100))  # positions past nt: filler + row 3


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("use_cfg", [False, True])
def test_step_restatements_are_the_ode_reference(method, use_cfg):
    """The per-launch restatements (R.cfg_slope, R.euler_update, R.rk_stage), chained over a grid as the sampler chains
    its launches, give tests/ode_reference.integrate's trajectory bit for bit on a linear vector field, with and
    without the CFG combination (cfm.py:190-191)."""
    import ode_reference

    B, N, mel = 2, 3, 5
    y0 = torch.randn(B, N, mel, generator=torch.Generator().manual_seed(3))
    grid = torch.tensor(C.STEP_GRID, dtype=F32)
    fc = lambda x: -1.7 * x + 0.3  # noqa: E731
    fu = lambda x: 0.4 * x - 0.1   # noqa: E731

    def fn(t, x):
        return fc(x) + (fc(x) - fu(x)) * C.STEP_CFG if use_cfg else fc(x)

    want = ode_reference.integrate(fn, y0, grid, method)
    stages = {"euler": 1, "midpoint": 2, "rk4": 4}[method]
    y, kbuf, traj = y0, torch.zeros(3, B, N, mel), [y0]
    for k in range(grid.numel() - 1):
        dt = R.grid_dt(C.STEP_GRID, k)
        x = y
        for s in range(stages):
            v = R.cfg_slope(torch.cat((fc(x), fu(x))), B, N, mel, 0, use_cfg, C.STEP_CFG)
            if method == "euler":
                x = R.euler_update(y, v, dt)
            else:
                x, kbuf = R.rk_stage(method, s, y, v, dt, kbuf)
        y = x
        traj.append(y)
    assert torch.equal(torch.stack(traj), want)


def test_mask_restatements():
    """The mask builders' restatements against their definitions: lens_to_mask of the oracle (rowkeep), and the
    elementwise text mask whose last set position is textlen."""
    from oracle import ref_cpu

    dur = torch.tensor(C.MASK_DUR, dtype=torch.int32)
    keep = R.masks("build_rowkeep", dur, 6, C.MASK_L, 0)
    assert torch.equal(keep[:3].bool(), ref_cpu.lens_to_mask(dur.long(), C.MASK_L)) and torch.equal(keep[:3], keep[3:])
    keep1 = R.masks("build_rowkeep", dur, 6, C.MASK_L + 1, 1)
    assert keep1[:, 0].all() and torch.equal(keep1[:, 1:], keep)
    assert R.masks("build_kvlen", dur, 6, 0, 1).tolist() == [3, 7, 10, 3, 7, 10]
    for nt in C.TEXTLEN_NTS:
        text = C.textlen_case(nt)
        ln = R.masks("build_textlen", text, 6)
        tk = R.masks("build_textkeep", text, 6)
        assert ln.tolist()[:3] == [0, nt // 2 if nt // 2 > nt // 4 else 0, nt] and ln.tolist()[3:] == ln.tolist()[:3]
        for s in range(6):
            assert int(ln[s]) == (int(tk[s].nonzero().max()) + 1 if tk[s].any() else 0)


def test_op_step_args_layout_matches_c(tmp_path):
    """The ctypes mirror of f5h_op_step_args has the C layout."""
    import os
    import subprocess

    from f5_tts_amd import _lib

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "f5h.h")
    fields = [f for f, _ in _lib.OpStepArgs._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                    '  printf("%%zu", sizeof(f5h_op_step_args));\n%s  return 0;\n}\n'
                    % (header, "".join('  printf(" %%zu", offsetof(f5h_op_step_args, %s));\n' % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.OpStepArgs)] + [getattr(_lib.OpStepArgs, f).offset for f in fields]


def test_glue_op_entry_points_refuse_bad_shapes():
    """The audio-glue, prologue and step hooks: shapes outside a launcher's contract give F5H_EINVAL with a message
    before any device work (P is a non-null pointer that is never dereferenced; the stream is null)."""
    from f5_tts_amd import _lib

    L = _lib.lib()
    P = 256

    def refused(rc, word):
        assert rc == -1, rc
        assert word.encode() in L.f5h_last_error(), L.f5h_last_error()

    refused(L.f5h_op_mel_frames(None, 3, 32, 64, 16, P, P), "L > n_fft / 2")   # L = n_fft / 2: no reflection
    refused(L.f5h_op_mel_frames(None, 3, 512, 1024, 256, P, P), "L > n_fft / 2")
    refused(L.f5h_op_mel_frames(None, 3, 100, 64, 16, None, P), "null")
    refused(L.f5h_op_mel_frames_ragged(None, 4, 3, 64, 16, P, 1024, P, P, P), "bad shape")  # fewer rows than waves
    refused(L.f5h_op_mel_mag(None, 5, 513, 1024, 576, P, P), "ld_spec")    # ld_spec < 2 bins
    refused(L.f5h_op_mel_mag(None, 5, 513, 1089, 576, P, P), "ld_spec")    # odd
    refused(L.f5h_op_mel_mag(None, 5, 513, 1088, 512, P, P), "ld_mag")
    refused(L.f5h_op_mel_log(None, 2, 0, 100, P, P), "bad shape")
    refused(L.f5h_op_mel_log_ragged(None, 2, 0, 100, P, P, P), "bad shape")
    refused(L.f5h_op_vocos_imcol(None, 0, 2, 4, 100, 700, P, P), "Kp")     # Kp % 64
    refused(L.f5h_op_vocos_imcol(None, 0, 2, 4, 100, 640, P, P), "Kp")     # Kp < 7 C
    refused(L.f5h_op_vocos_imcol(None, 2, 2, 4, 100, 704, P, P), "fp32 or bf16")
    refused(L.f5h_op_vocos_imcol_ragged(None, 0, 4, 3, 100, 704, P, 1200, 100, 1, P, P, P), "bad shape")
    refused(L.f5h_op_vocos_imcol_ragged(None, 0, 4, 16, 100, 704, P, 1200, 0, 1, P, P, P), "strides")
    refused(L.f5h_op_vocos_spec(None, 3, 513, 1024, P), "ld")
    refused(L.f5h_op_vocos_spec(None, 3, 513, 1027, P), "ld")
    refused(L.f5h_op_vocos_ola(None, 2, 0, 64, 16, P, P, P), "bad shape")
    refused(L.f5h_op_vocos_ola(None, 2, 4, 64, 24, P, P, P), "n_fft % hop")
    refused(L.f5h_op_vocos_ola_ragged(None, 5, 4, 64, 16, P, P, P, P), "bad shape")
    refused(L.f5h_op_vocos_ola_ragged(None, 5, 18, 64, 24, P, P, P, P), "n_fft % hop")
    for n in (0, 513):
        for dev in (0, 1):
            refused(L.f5h_op_time_sinus(None, dev, n, P, P), "1 <= n <= 512")
    refused(L.f5h_op_rope_table(None, 0, P), "1 <= L")
    refused(L.f5h_op_text_embed(None, 2, 5, 9, 100, P, None, P, None, 4, 0, P, P, None, None), "freq_rows")
    refused(L.f5h_op_text_embed(None, 2, 5, 9, 100, P, P, P, None, 0, 0, P, P, None, P), "seq_len")
    refused(L.f5h_op_text_embed(None, 2, 5, 0, 100, P, None, P, None, 0, 0, P, P, None, None), "bad shape")
    refused(L.f5h_op_build_ct(None, 0, 2, 5, 100, 3, 0, 0, P, P, P, P, P), "S must be")
    refused(L.f5h_op_build_ct(None, 3, 2, 5, 100, 4, 0, 0, P, P, P, P, P), "compute")
    refused(L.f5h_op_pack_y(None, 0, 7, 129, P, P), "mel <= 128")
    refused(L.f5h_op_masks(None, 4, 3, 6, 6, 0, P, P), "kind")
    refused(L.f5h_op_masks(None, 0, 3, 5, 6, 0, P, P), "bad shape")        # S % B
    refused(L.f5h_op_masks(None, 3, 3, 6, 0, 0, P, P), "row length")
    refused(L.f5h_op_masks(None, 2, 3, 6, 6, 1, P, P), "off")
    refused(L.f5h_op_final_where_out(None, 2, 5, 100, P, P, None, P, None), "null")
    refused(L.f5h_op_copy_pred(None, 2, 6, 6, 100, 128, P, P, None), "row_off")
    refused(L.f5h_op_copy_pred(None, 2, 6, 1, 100, 64, P, P, None), "p_ld")

    def step(**kw):
        """A valid host-form Euler call (never launched: every use below breaks one rule), then the overrides."""
        a = _lib.OpStepArgs()
        a.compute, a.method, a.B, a.N, a.mel, a.use_cfg = 0, 0, 2, 1, 100, 1
        a.y = a.p = P
        a.p_seq_stride, a.p_ld, a.p_row_off = 128, 128, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for a, word in ((step(mel=129), "mel <= 128"), (step(p_ld=64), "p_ld >= mel"), (step(p_row_off=1), "p_seq_stride"),
                    (step(method=1), "method"), (step(tgrid=P), "device-indexed"), (step(tick=P), "device-indexed"),
                    (step(kstep=P), "tgrid"), (step(kstep=P, tgrid=P, nfe=4, traj=P), "trajp"),
                    (step(kstep=P, tgrid=P, nfe=4, next_dst=P, next_src=P, next_n=6, next_stride=8), "multiples of 4"),
                    (step(kstep=P, tgrid=P, nfe=4, tick=P), "arrive"), (step(compute=5), "compute")):
        refused(L.f5h_op_cfg_euler(None, ctypes.byref(a)), word)
    rk = dict(method=2, kstep=P, tgrid=P, ypad=P, kbuf=P, nfe=8)
    for a, word in ((step(**{**rk, "method": 0}), "method"), (step(**{**rk, "kbuf": None}), "kbuf"),
                    (step(**{**rk, "ypad": None}), "ypad"), (step(**{**rk, "kstep": None}), "kstep"),
                    (step(**{**rk, "nfe": 0}), "nfe"), (step(**rk, traj=P), "trajp")):
        refused(L.f5h_op_cfg_rk(None, ctypes.byref(a)), word)
    refused(L.f5h_op_cfg_rk(None, None), "null arguments")
