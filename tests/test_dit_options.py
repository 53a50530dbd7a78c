"""qk_norm="rms_norm", long_skip_connection and text_embedding_average_upsampling without a GPU: parameter names and
shapes, the plugin constructors, the arch struct, and that the references of tests/dit_options_reference.py can tell
right from wrong on the inputs tests/test_gpu_dit_options.py uses (wrong variants of the QKV norm miss the op
tolerance; the options move the end-to-end output by well more than the bound the GPU tests hold the engine to)."""

import ctypes

import pytest
import torch

import dit_options_reference as D
import golden_cases as gc
import op_cases as C
import op_reference as R
from f5_tts_amd import _lib, configs
from f5_tts_amd.engine import _arch_struct
from f5_tts_amd.model import DiT, UNetT

F64, F32 = torch.float64, torch.float32
BF16_TOL = 5e-2  # the 16-bit end-to-end bound of tests/test_gpu_dit_options.py


# ---------------------------------------------------------------- names and shapes
def _new_names(tag, **opt):
    base = configs.param_shapes(D.arch_with(tag))
    full = configs.param_shapes(D.arch_with(tag, **opt))
    assert {k: v for k, v in full.items() if k in base} == base, "existing names or shapes changed"
    return {k: v for k, v in full.items() if k not in base}


def test_param_shapes_unchanged_with_the_options_off():
    for tag in ("tiny", "utiny"):
        assert _new_names(tag) == {}
        assert _new_names(tag, qk_norm=None) == {}
    assert _new_names("tiny", long_skip_connection=False, text_embedding_average_upsampling=False) == {}
    s = configs.param_shapes(configs.get_arch("F5TTS_v1_Base"))
    assert not [k for k in s if "q_norm" in k or "k_norm" in k or "long_skip" in k]


def test_param_shapes_with_each_option():
    a = D.arch_with("tiny")
    want = {f"transformer_blocks.{i}.attn.{n}_norm.weight": (64,) for i in range(a["depth"]) for n in "qk"}
    assert _new_names("tiny", qk_norm="rms_norm") == want
    u = D.arch_with("utiny")
    want = {f"layers.{i}.2.{n}_norm.weight": (64,) for i in range(u["depth"]) for n in "qk"}
    assert _new_names("utiny", qk_norm="rms_norm") == want
    assert _new_names("tiny", long_skip_connection=True) == {"long_skip_connection.weight": (a["dim"], 2 * a["dim"])}
    assert _new_names("tiny", text_embedding_average_upsampling=True) == {}


def _plugin(cls, arch):
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim", "skip_connect_type")}
    return cls(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])


def test_plugin_state_dicts_carry_the_new_names():
    for cls, tag, opt in ((DiT, "tiny", dict(qk_norm="rms_norm", long_skip_connection=True,
                                             text_embedding_average_upsampling=True)),
                          (UNetT, "utiny", dict(qk_norm="rms_norm"))):
        plain = set(_plugin(cls, D.arch_with(tag)).state_dict())
        arch = D.arch_with(tag, **opt)
        sd = _plugin(cls, arch).state_dict()
        new = {k: tuple(v.shape) for k, v in sd.items() if k not in plain}
        assert new == _new_names(tag, **opt)
        assert plain <= set(sd)
        W = D.weights_for(arch)
        assert set(W) == set(sd) - {"rotary_embed.inv_freq"}
        for k in new:
            if k.endswith("norm.weight"):
                assert abs(float(W[k].mean()) - 1.0) < 0.1  # a gain around 1 (synthetic._init_scale)


def test_constructor_errors_are_the_reference_s():
    with pytest.raises(ValueError, match="Unimplemented qk_norm: layer_norm"):
        _plugin(DiT, D.arch_with("tiny", qk_norm="layer_norm"))
    with pytest.raises(ValueError, match="Unimplemented qk_norm"):
        _plugin(UNetT, D.arch_with("utiny", qk_norm="layer_norm"))
    with pytest.raises(AssertionError, match="requires text_mask_padding"):
        _plugin(DiT, D.arch_with("tiny", text_embedding_average_upsampling=True, text_mask_padding=False))


def test_arch_struct_fields_and_layout(tmp_path):
    a = _arch_struct(D.arch_with("tiny"), "bf16")
    assert (a.qk_norm, a.long_skip_connection, a.text_average_upsampling) == (0, 0, 0)
    a = _arch_struct(D.arch_with("tiny", qk_norm="rms_norm", long_skip_connection=True,
                                 text_embedding_average_upsampling=True), "fp32")
    assert (a.qk_norm, a.long_skip_connection, a.text_average_upsampling) == (1, 1, 1)
    a = _arch_struct(D.arch_with("utiny", qk_norm="rms_norm"), "fp16")
    assert (a.qk_norm, a.long_skip_connection, a.text_average_upsampling) == (1, 0, 0)
    with pytest.raises(ValueError, match="Unimplemented qk_norm"):
        _arch_struct(D.arch_with("tiny", qk_norm="layer_norm"), "bf16")
    assert _lib.has_dit_options()
    # the appended fields sit where the header puts them
    import os
    import subprocess

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "f5h.h")
    fields = ("compute", "qk_norm", "long_skip_connection", "text_average_upsampling")
    gfields = ("poison", "q_norm_w", "k_norm_w", "qk_norm_eps")
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                    '  printf("%%zu %%zu", sizeof(f5h_arch), sizeof(f5h_op_gemm_args));\n%s%s  return 0;\n}\n'
                    % (header, "".join('  printf(" %%zu", offsetof(f5h_arch, %s));\n' % f for f in fields),
                       "".join('  printf(" %%zu", offsetof(f5h_op_gemm_args, %s));\n' % f for f in gfields)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == ([ctypes.sizeof(_lib.Arch), ctypes.sizeof(_lib.OpGemmArgs)]
                   + [getattr(_lib.Arch, f).offset for f in fields]
                   + [getattr(_lib.OpGemmArgs, f).offset for f in gfields])


def test_bad_option_values_are_refused_before_any_device_work():
    L = _lib.lib()
    h = ctypes.c_void_p()
    base = dict(backbone=0, dim=256, depth=1, heads=4, dim_head=64, ff_dim=512, text_dim=128, text_num_embeds=10,
                mel_dim=100, conv_layers=0, text_mask_padding=1, pe_attn_head=0, attn_mask_enabled=0, compute=1)
    for kw, word in ((dict(qk_norm=2), b"qk_norm"), (dict(long_skip_connection=3), b"must be 0 or 1"),
                     (dict(backbone=1, depth=2, long_skip_connection=1), b"DiT options"),
                     (dict(text_average_upsampling=1, text_mask_padding=0), b"requires text_mask_padding")):
        a = _lib.Arch(**{**base, **kw})
        assert L.f5h_engine_create(ctypes.byref(a), None, 0, 0, ctypes.byref(h)) == -1
        assert word in L.f5h_last_error(), L.f5h_last_error()
    # the GEMM hook: gains go with QKV, and in pairs
    P = 256
    g = _lib.OpGemmArgs()
    g.compute, g.epi, g.M, g.N, g.K, g.A, g.W, g.C, g.q_norm_w, g.k_norm_w = 1, 0, 8, 128, 64, P, P, P, P, P
    assert L.f5h_op_gemm_epi(None, ctypes.byref(g), None, 0) == -1 and b"EPI_QKV" in L.f5h_last_error()
    g.epi, g.N, g.heads, g.seq_len, g.q, g.k, g.v, g.k_norm_w = 7, 384, 2, 4, P, P, P, None
    assert L.f5h_op_gemm_epi(None, ctypes.byref(g), None, 0) == -1 and b"q_norm_w and k_norm_w" in L.f5h_last_error()
    g.k_norm_w = P  # valid: fails only on the missing workspace
    assert L.f5h_op_gemm_epi(None, ctypes.byref(g), None, 0) == -4
    assert L.f5h_op_text_upsample(None, 1, 4, 9000, 64, P, None, P, P + 4) == -1 and b"8192" in L.f5h_last_error()
    assert L.f5h_op_text_upsample(None, 1, 4, 40, 64, P, None, P, P) == -1 and b"aliased" in L.f5h_last_error()


def test_model_cfg_with_the_options_constructs(tmp_path):
    """load_model with a model_cfg carrying the options: the plugin grows the extra parameters and a checkpoint
    that holds them loads strictly (checkpoint.load_model, the path api.F5TTS takes)."""
    from f5_tts_amd.checkpoint import load_model
    from f5_tts_amd.model import CFM
    from f5_tts_amd.model.utils import get_tokenizer

    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join([" ", "a", "b", "c", "d"]) + "\n")
    _, vocab_size = get_tokenizer(str(vocab))
    cfg = dict(dim=128, depth=2, heads=2, ff_mult=2, text_dim=64, conv_layers=1, qk_norm="rms_norm",
               long_skip_connection=True, text_embedding_average_upsampling=True)
    src = CFM(transformer=DiT(**cfg, text_num_embeds=vocab_size, mel_dim=100))
    with torch.no_grad():
        params = dict(src.transformer.named_parameters())
        params["long_skip_connection.weight"].fill_(0.25)
        params["transformer_blocks.1.attn.k_norm.weight"].fill_(1.5)
    ckpt = tmp_path / "model.pt"
    torch.save({"model_state_dict": src.state_dict()}, str(ckpt))
    m = load_model(DiT, cfg, str(ckpt), vocab_file=str(vocab), use_ema=False, device="cpu")
    sd = m.transformer.state_dict()
    assert (sd["long_skip_connection.weight"] == 0.25).all() and sd["long_skip_connection.weight"].shape == (128, 256)
    assert (sd["transformer_blocks.1.attn.k_norm.weight"] == 1.5).all()
    assert m.transformer.arch["qk_norm"] == "rms_norm"
    assert m.transformer.arch["text_embedding_average_upsampling"] is True
    # a checkpoint without the gains does not load into a model that has them
    plain = CFM(transformer=DiT(**{**cfg, "qk_norm": None}, text_num_embeds=vocab_size, mel_dim=100))
    torch.save({"model_state_dict": plain.state_dict()}, str(ckpt))
    with pytest.raises(RuntimeError, match="q_norm.weight"):
        load_model(DiT, cfg, str(ckpt), vocab_file=str(vocab), use_ema=False, device="cpu")


# ---------------------------------------------------------------- the references tell right from wrong
@pytest.mark.parametrize("compute", C.COMPUTES)
def test_qk_norm_wrong_variants_rejected(compute):
    """On the GPU op test's inputs: R32 meets the op tolerance against R64, each deliberately wrong form misses it."""
    rope = C.rope_table_f32(C.QKV_L)
    worst = {v: 0.0 for v in D.WRONG_QKN}
    for spec in D.QKN_CASES:
        c = D.qkn_case(compute, *spec)
        r64, r32 = D.qkn_ref(c, rope, F64), D.qkn_ref(c, rope, F32)
        for a, b in zip(r64, r32):
            assert R.excess_ratio(b, a, b, c["u_out"]) <= 1.0
        for v in worst:
            for o, a, b in zip(D.qkn_ref(c, rope, F64, v), r64, r32):
                worst[v] = max(worst[v], R.excess_ratio(o, a, b, c["u_out"]))
    for v, ratio in worst.items():
        assert ratio > R.ACC_FACTOR, f"{compute}: wrong variant {v!r} passes the tolerance (worst ratio {ratio:.3g})"


def test_qk_norm_special_rows():
    c = D.qkn_case("bf16", 2, 2, False)
    rope = C.rope_table_f32(C.QKV_L)
    q, k, v = D.qkn_ref(c, rope, F64)
    z = D.ROW_ZERO
    assert (q[0, :, z] == 0).all() and (k[0, :, z] == 0).all() and torch.isfinite(q).all() and torch.isfinite(k).all()
    pre = R.gemm_epi("store", c["A_read"], c["W_read"], None, dtype=F64)
    ms = pre[:, :2 * 128].reshape(-1, 4, 64).square().mean(-1)
    assert 1e-7 < float(ms[D.ROW_SMALL].mean()) < 1e-5, "the small row's mean square sits at the epsilon"
    assert float(ms[D.ROW_LARGE].mean()) > 1e3
    # the epsilon matters on the small row only
    bad = D.qkn_ref(c, rope, F64, "eps_1e-5")[0]
    d = (bad - q).abs().amax(dim=(0, 1, 3))
    assert d[D.ROW_SMALL] > 0.1 and d[D.ROW_LARGE] < 1e-4


def test_upsample_restatement():
    c = D.upsample_case()
    out = D.upsample_ref(c)
    te = c["te"]
    # sequence 0: valid slots 0, 1, 3, 4, 5 over 40 frames, 8 each
    for j, slot in enumerate((0, 1, 3, 4, 5)):
        assert torch.equal(out[0, 8 * j:8 * j + 8], te[0, slot].expand(8, -1))
    assert torch.equal(out[1, :23], te[1, :23]) and (out[1, 23:] == 0).all()   # T = audio_len: the identity
    assert (out[2] == 0).all()                                                  # no valid token
    o39 = D.upsample_ref(c, torch.tensor([39, 22, 7]))
    # 39 = 7 + 8 x 4: the first token 7 times, the last four 8 times; frame 39 zero
    assert torch.equal(o39[0, :7], te[0, 0].expand(7, -1)) and torch.equal(o39[0, 7:15], te[0, 1].expand(8, -1))
    assert torch.equal(o39[0, 31:39], te[0, 5].expand(8, -1)) and (o39[0, 39] == 0).all()


@pytest.mark.parametrize("spec_name", ["B1", "B3"])
def test_options_move_the_output_by_more_than_the_16bit_bound(spec_name):
    """The end-to-end GPU tests can tell an engine that ignores an option from one that applies it only if the
    option moves the reference by well more than the bound. qk_norm on the synthetic tiny DiT does not (it moves
    the fp32 sample by under 2e-2), so its 16-bit cases multiply to_q / to_k by QK_SCALE: asserted here to separate
    by at least twice the bound. Long skip and upsampling separate on the plain weights."""
    spec = getattr(gc, spec_name)
    plain = D.case("tiny", spec, {})
    plain4 = D.case("tiny", spec, {}, qk_scale=D.QK_SCALE)
    seps = {
        "qk_norm (unscaled)": gc.rel_err(D.case("tiny", spec, dict(qk_norm="rms_norm"))["out"], plain["out"]),
        "qk_norm": gc.rel_err(D.case("tiny", spec, dict(qk_norm="rms_norm"), qk_scale=D.QK_SCALE)["out"], plain4["out"]),
        "long_skip": gc.rel_err(D.case("tiny", spec, dict(long_skip_connection=True))["out"], plain["out"]),
        "upsampling": gc.rel_err(D.case("tiny", spec, dict(text_embedding_average_upsampling=True))["out"],
                                 plain["out"]),
    }
    print(spec_name, {k: f"{v:.3e}" for k, v in seps.items()})
    assert seps["qk_norm (unscaled)"] > 1e-3, "even unscaled it clears the fp32 bound"
    for k in ("qk_norm", "long_skip", "upsampling"):
        assert seps[k] >= 2 * BF16_TOL, (k, seps[k])
