"""compute="mxfp8" on the host side (no GPU): the quantisation rule of the library (the code the device kernels run,
through f5h_debug_mx8_quant_block) against the CPU oracle tests/mx8_reference.py and against ceil(log2(amax / 448)) in
exact arithmetic; the exports and struct sizes; CFM's acceptance of the mode; the refusals, which happen before the
engine is touched; and the MX8 GEMM's generated code."""

from __future__ import annotations

import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import mx8_reference as MX
from f5_tts_amd import _lib, configs
from f5_tts_amd import engine as E
from f5_tts_amd.model import CFM, DiT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "f5-tts_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _f32_bits(x: float) -> int:
    return int(torch.tensor(x, dtype=torch.float32).view(torch.int32)) & 0x7FFFFFFF


def test_scale_rule_is_ceil_log2_of_amax_over_448():
    """clamp(E - 8 + (m > 0x600000), 0, 254) == clamp(127 + ceil(log2(amax / 448)), 0, 254) for 448 2^k and its next
    float up over the whole exponent range, fp32 subnormals and zero."""
    vals = [0.0, 1e-45, 1e-41, 5.8e-39, 1.0, 448.0, 3.0e38]
    for k in range(-149, 120):
        a = torch.tensor(math.ldexp(448.0, k), dtype=torch.float32)
        if float(a) == 0.0 or not bool(torch.isfinite(a)):
            continue
        vals.append(float(a))
        up = torch.nextafter(a, torch.tensor(float("inf")))
        if bool(torch.isfinite(up)):
            vals.append(float(up))
        vals.append(float(torch.nextafter(a, torch.tensor(0.0))))
    for v in vals:
        want = MX.ceil_log2_byte(v)
        got = int(MX.scale_byte(torch.tensor(_f32_bits(v), dtype=torch.int64)))
        assert got == want, (v, got, want)
        # the library's own rule, on a block whose amax is v
        blk = [0.0] * 32
        blk[7] = -v
        _, s = E.mx8_quant_block_host(blk)
        assert s == want, (v, s, want)


def test_library_rule_equals_the_oracle_bit_for_bit():
    """Elements and scale of every sweep block: the library's integer e4m3fn conversion against torch's own."""
    for blk in MX.block_cases():
        q, s = MX.quantize(blk[None, :])
        gq, gs = E.mx8_quant_block_host(blk.tolist())
        assert gs == int(s[0, 0]), (blk, gs, s)
        assert gq == q[0].tolist(), (blk, gq, q[0].tolist())


def test_no_element_exceeds_448_and_nothing_saturates():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(64, 256, generator=g) * torch.exp2(torch.randint(-40, 41, (64, 8), generator=g).float()
                                                        ).repeat_interleave(32, dim=1)
    x = x.to(torch.bfloat16).float()
    q, s = MX.quantize(x)
    mag = q & 0x7F
    assert int(mag.max()) <= 0x7E  # 0x7E = 448, 0x7F = NaN
    deq = MX.dequantize(q, s)
    # an element is within half an e4m3 ulp of its value: relative 2^-4 for normals, absolute 2^-10 2^(s-127) below
    sc = torch.ldexp(torch.ones((), dtype=torch.float64), s.to(torch.int32) - 127).repeat_interleave(32, dim=1)
    assert bool(((deq - x.double()).abs() <= torch.maximum(x.double().abs() * 2.0 ** -4, sc * 2.0 ** -10)).all())
    # the block maximum uses the top binade pair: amax / 2^(s - 127) in (224, 448]
    amax = x.view(64, 8, 32).abs().amax(-1).double()
    top = amax / torch.ldexp(torch.ones((), dtype=torch.float64), s.to(torch.int32) - 127)
    assert bool(((top > 224.0) & (top <= 448.0))[amax > 0].all())


def test_zero_block_and_non_finite_inputs():
    q, s = E.mx8_quant_block_host([0.0] * 32)
    assert s == 0 and q == [0] * 32
    blk = [1.0] * 32
    blk[3], blk[9], blk[20] = float("nan"), float("inf"), float("-inf")
    q, s = E.mx8_quant_block_host(blk)
    assert q[3] == q[9] == q[20] == MX.NAN_BYTE
    oq, os_ = MX.quantize(torch.tensor(blk)[None, :])
    assert q == oq[0].tolist() and s == int(os_[0, 0])


def test_library_exports_the_mx8_entry_points():
    L = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "f5h.h")).read(), flags=re.S)
    for name in _lib.MX8_EXPORTS:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert _lib.has_mx8() is True
    assert _lib.COMPUTE["mxfp8"] == 3 and re.search(r"F5H_MXFP8\s*=\s*3", header)
    assert E.OP_TORCH_DTYPE["mxfp8"] is torch.bfloat16
    assert _lib.MX8_CLASS_BITS == {"qkv": 1, "out": 4, "ffn1": 8, "ffn2": 16}


def test_struct_sizes_match_c(tmp_path):
    """f5h_arch and f5h_op_gemm_args (the MX8 GEMM hook reads the latter) as ctypes mirrors them."""
    prog = tmp_path / "layout.c"
    prog.write_text(f"""
#include <stdio.h>
#include "{os.path.join(REPO, 'include', 'f5h.h')}"
int main(void) {{ printf("%zu %zu %d\\n", sizeof(f5h_arch), sizeof(f5h_op_gemm_args), (int)F5H_MXFP8); return 0; }}""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(prog), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got] == [ctypes.sizeof(_lib.Arch), ctypes.sizeof(_lib.OpGemmArgs), _lib.F5H_MXFP8]


def test_calls_without_a_device_are_refused_by_value():
    L = _lib.lib()
    assert L.f5h_set_mx8_classes(None, 29) == -1
    assert L.f5h_mx8_stats(None, None, None) == -1
    assert L.f5h_op_quant_mx8(None, 4, 48, None, None, None, None, 0) == -1  # K % 32
    assert L.f5h_op_gemm_mx8(None, None, None, None, None, None, None, 0) == -1
    a = _lib.OpGemmArgs()
    a.epi, a.M, a.N, a.K = 2, 4, 128, 192  # K % 128
    assert L.f5h_op_gemm_mx8(None, ctypes.byref(a), None, None, None, None, None, 0) == -1
    assert b"128" in L.f5h_last_error()


def _cfm(cls=DiT, preset="DiT_tiny", **over):
    arch = configs.get_arch(preset, text_num_embeds=64, **over)
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = cls(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    return CFM(transformer=net, num_channels=100, compute="mxfp8")


def test_cfm_accepts_mxfp8_and_auto_never_picks_it():
    m = _cfm()
    assert m.engine_compute() == "mxfp8"
    from f5_tts_amd.model.backbones.base import compute_for_dtype

    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert compute_for_dtype(dt) != "mxfp8"
    with pytest.raises(ValueError, match="mxfp8"):
        CFM(transformer=m.transformer, num_channels=100, compute="fp8")


@pytest.mark.parametrize("preset, over, match", [
    ("UNetT_tiny", {}, "DiT backbone only"),
    ("MMDiT_tiny", {}, "DiT backbone only"),
    ("DiT_tiny", {"dim": 192, "heads": 3}, "multiple of 128"),
    ("DiT_tiny", {"ff_mult": 1.5}, "ff_dim"),
])
def test_refusals_happen_before_the_engine_is_touched(monkeypatch, preset, over, match):
    def boom(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    arch = configs.get_arch(preset, text_num_embeds=64, **over)
    with pytest.raises(NotImplementedError, match=match):
        E.Engine(arch, {}, compute="mxfp8")


def test_older_library_raises_runtime_error(monkeypatch):
    monkeypatch.setattr(_lib, "has_mx8", lambda: False)
    with pytest.raises(RuntimeError, match="older build"):
        E.Engine(configs.get_arch("DiT_tiny", text_num_embeds=64), {}, compute="mxfp8")


def test_gemm_mx8_codegen(tmp_path):
    """gemm_mx8.hip for gfx950: every kernel runs the block-scaled MFMA and uses no scratch memory."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "gemm_mx8.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics",
                    "-ffp-contract=fast-honor-pragmas", "-mllvm", "-disable-promote-alloca-to-lds=1",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "gemm_mx8.hip"), "-o", str(out)], check=True,
                   capture_output=True, timeout=300)
    text = out.read_text()
    kernels = re.findall(r"^(_Z\S*gemm_mx8_kernel\S*):", text, flags=re.M)
    assert len(kernels) == 6, kernels  # QKV x (qk_norm, ragged rows), RESID16, GELU_TANH
    for name in kernels:
        body = text.split(name + ":", 1)[1].split(".Lfunc_end", 1)[0]
        assert len(re.findall(r"\bv_mfma_scale_f32_16x16x128_f8f6f4\b", body)) == 16, name  # 4 x 4 tiles per K-step
        assert "scratch_" not in body, name
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(sizes) == 6 and set(sizes) == {"0"}, sizes
    spills = re.findall(r"\.vgpr_spill_count:\s*(\d+)", text)
    assert set(spills) == {"0"}, spills
