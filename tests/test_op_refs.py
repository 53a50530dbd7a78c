"""The op-level parity tests can tell right from wrong (no GPU): on the inputs tests/test_gpu_ops.py feeds the
kernels, the float32 form R32 of every reference meets the tolerance against the float64 form R64, and every
deliberately wrong float64 variant (op_reference.WRONG_*) misses it on at least one case of every compute mode's
set. A variant that slipped through would mean the inputs are too tame to expose that mistake in a kernel.

Also here: the new op entry points refuse shapes outside their launchers' contracts with F5H_EINVAL before any
device work. The conv weight packing (pack_conv_weight, engine_pack.cpp) runs as a device kernel and cannot be called
on the host; it is covered by the GPU conv tests, which pass the torch-layout weight through it.
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
