"""The op-level parity tests can tell right from wrong (no GPU): on the inputs tests/test_gpu_ops.py feeds the
kernels, the float32 form R32 of every reference meets the tolerance against the float64 form R64, and every
deliberately wrong float64 variant (op_reference.WRONG_*) misses it on at least one case of every compute mode's
set. A variant that slipped through would mean the inputs are too tame to expose that mistake in a kernel.

Also here: the new op entry points refuse shapes outside their launchers' contracts with F5H_EINVAL before any
device work. The conv weight packing (pack_conv_weight, engine.cpp) runs as a device kernel and cannot be called
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
    fields = ("k_split", "A", "C", "live_seq", "q_scale", "add", "dual_rows", "rope_out")
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                    '  printf("%%zu", sizeof(f5h_op_gemm_args));\n%s  return 0;\n}\n'
                    % (header, "".join('  printf(" %%zu", offsetof(f5h_op_gemm_args, %s));\n' % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.OpGemmArgs)] + [getattr(_lib.OpGemmArgs, f).offset for f in fields]


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
