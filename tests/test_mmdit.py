"""MMDiT without a GPU: parameter names against the reference's state dict, the CPU restatement
(tests/mmdit_reference.py) against every fp32 fixture the reference produced, the deviations that restatement must be
able to tell from the model, and the refusals that happen before any device work."""

import hashlib
import json
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
import mmdit_reference as mr
from f5_tts_amd import _lib, configs, synthetic
from f5_tts_amd.engine import _arch_struct
from f5_tts_amd.model import CFM, MMDiT
from f5_tts_amd.model.backbones import MMDiT as MMDiT2

SAMPLE_TOL = 2e-5   # test_oracle_golden.py: the restatement runs the reference's torch ops
WRONG_TOL = 3e-3    # 3 x the fp32 GPU bound: a deviation this large cannot hide inside the engine's contract

# sha256 of json.dumps([[name, shape], ...]) of param_shapes(get_arch(preset)), computed on the commit before MMDiT
PARENT_SHAPES = {
    "DiT_tiny": "0c5b686f60fb1aeb",
    "E2TTS_Base": "bf9f4b70c4890aee",
    "F5TTS_Base": "0a421775f93815ef",
    "F5TTS_v1_Base": "0a421775f93815ef",
    "F5TTS_v1_Small": "e5218f07b2bac15c",
    "F5TTS_v1_Small_4L": "d9ba6855c10143b4",
    "UNetT_tiny": "cb727e72aa8325d7",
}


def _state_dict_fixture():
    with open(os.path.join(gc.GOLDEN, "mmdit_state_dict.json")) as f:
        return json.load(f)


def _plugin(arch):
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    return MMDiT(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])


@pytest.mark.parametrize("tag", ["tiny", "tiny_qkn"])
def test_param_shapes_equal_the_reference_state_dict(tag):
    want = [(k, tuple(s)) for k, s in _state_dict_fixture()[tag]]
    have = list(configs.param_shapes(mr.arch_of(tag)).items())
    assert have == want  # names, shapes and order


def test_existing_presets_keep_their_param_shapes():
    assert set(PARENT_SHAPES) == set(configs.PRESETS) - {"MMDiT_tiny"}
    for name, want in PARENT_SHAPES.items():
        s = configs.param_shapes(configs.get_arch(name))
        have = hashlib.sha256(json.dumps([[k, list(v)] for k, v in s.items()]).encode()).hexdigest()[:16]
        assert have == want, name


@pytest.mark.parametrize("tag", ["tiny", "tiny_qkn"])
def test_plugin_state_dict_names(tag):
    assert MMDiT2 is MMDiT
    net = _plugin(mr.arch_of(tag))
    sd = {k: tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith("inv_freq")}
    assert list(sd.items()) == [(k, tuple(s)) for k, s in _state_dict_fixture()[tag]]
    assert net.dim == 128 and net.depth == 3
    missing, unexpected = net.load_state_dict(synthetic.make_weights_torch(mr.arch_of(tag)), strict=False)
    assert not unexpected and all(m.endswith("inv_freq") for m in missing)


def test_unknown_qk_norm_raises_the_reference_error():
    with pytest.raises(ValueError, match="Unimplemented qk_norm"):
        MMDiT(dim=128, depth=2, heads=2, qk_norm="layer_norm")


def test_registered_in_the_api():
    from f5_tts_amd import api

    assert api._BACKBONES["MMDiT"] is MMDiT
    assert configs.get_arch("MMDiT_tiny")["depth"] == 3
    assert configs.get_arch(dict(backbone="MMDiT", dim=256))["ff_mult"] == 4  # MMDiT's defaults, not DiT's


def test_checkpoint_with_reference_names_loads(tmp_path):
    """checkpoint.load_model (utils_infer.py:238-275) on an MMDiT config: an EMA checkpoint under the reference's
    state-dict names (`ema_model.transformer.*`, the rotary buffer included) loads strictly."""
    from f5_tts_amd import api, checkpoint

    arch = configs.get_arch("MMDiT_tiny", qk_norm="rms_norm")
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join([" "] + [chr(97 + i) for i in range(26)]) + "\n")
    arch["text_num_embeds"] = 27
    W = synthetic.make_weights_torch(arch)
    sd = {"ema_model.transformer." + k: v for k, v in W.items()}
    sd["ema_model.transformer.rotary_embed.inv_freq"] = _plugin(arch).rotary_embed.inv_freq.clone()
    sd["initted"], sd["step"] = torch.tensor(True), torch.tensor(1)
    path = tmp_path / "model.pt"
    torch.save({"ema_model_state_dict": sd}, path)
    cfg = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    m = checkpoint.load_model(api._BACKBONES["MMDiT"], cfg, str(path), vocab_file=str(vocab), device="cpu")
    assert isinstance(m.transformer, MMDiT)
    name = "transformer_blocks.1.attn.c_k_norm.weight"
    assert torch.equal(m.transformer.state_dict()[name], W[name])


# ---------------------------------------------------------------- the restatement against the reference
@pytest.mark.parametrize("name", mr.FP32_SAMPLES)
def test_restatement_matches_sample_fixture(name, torch_threads):
    fx = gc.load(name)
    assert fx is not None, name
    out = mr.run_sample_case(name).numpy()
    err = gc.max_rel(out, fx["out"])
    print(f"{name}: max-rel {err:.3e}")
    assert err < SAMPLE_TOL


@pytest.mark.parametrize("name", list(mr.FORWARD_CASES))
def test_restatement_matches_forward_fixture(name, torch_threads):
    fx = gc.load(name)
    assert fx is not None, name
    err = gc.max_rel(mr.run_forward_case(name).numpy(), fx["out"])
    print(f"{name}: max-rel {err:.3e}")
    assert err < SAMPLE_TOL


@pytest.mark.parametrize("variant", mr.VARIANTS)
def test_wrong_variant_misses_the_fixture(variant, torch_threads):
    """Each deviation from the model moves the output by more than WRONG_TOL. The position clamp is checked on the
    1400-token forward: with the 1030 tokens of mmdit_tiny_fwd_b1_longtext only 7 positions lie past the clamp and its
    absence moves the output by 1.2e-3 with the synthetic weights (4.8e-2 at 1400 tokens)."""
    if variant == "no_pos_clamp":
        name = "mmdit_tiny_fwd_b1_longtext1400"
        out = mr.run_forward_case(name, variant).numpy()
    else:
        name = "mmdit_tiny_sample_b3"
        out = mr.run_sample_case(name, variant).numpy()
    err = gc.max_rel(out, gc.load(name)["out"])
    print(f"{variant}: max-rel {err:.3e}")
    assert err > WRONG_TOL


# ---------------------------------------------------------------- the arch struct and the refusals
def test_arch_struct_fills_the_mmdit_backbone():
    a = _arch_struct(mr.arch_of("tiny_qkn"), "bf16")
    assert a.backbone == 2 == _lib.F5H_MMDIT
    assert (a.dim, a.depth, a.heads, a.dim_head, a.ff_dim, a.text_dim) == (128, 3, 2, 64, 256, 128)
    assert (a.conv_layers, a.pe_attn_head, a.long_skip_connection, a.text_average_upsampling) == (0, 0, 0, 0)
    assert a.qk_norm == 1 and a.text_mask_padding == 1 and a.attn_mask_enabled == 0
    assert _lib.has_mmdit()


@pytest.mark.parametrize("field,value", [("text_dim", 64), ("conv_layers", 2), ("pe_attn_head", 1),
                                         ("long_skip_connection", True)])
def test_bad_fields_are_refused_by_name(field, value):
    arch = dict(mr.arch_of("tiny"), **{field: value})
    with pytest.raises(ValueError, match=field):
        _arch_struct(arch, "fp32")


@pytest.mark.parametrize("field,value", [("text_dim", 64), ("conv_layers", 2), ("pe_attn_head", 1),
                                         ("long_skip_connection", 1), ("text_average_upsampling", 1), ("depth", 0)])
def test_library_refuses_bad_fields_by_name(field, value):
    """The C side's own check (f5h_engine_create_views validates the arch before it touches a device): an Arch
    struct filled by hand, past the Python checks."""
    import ctypes

    a = _arch_struct(mr.arch_of("tiny"), "fp32")
    setattr(a, field, value)
    h = ctypes.c_void_p()
    L = _lib.lib()
    rc = L.f5h_engine_create_views(ctypes.byref(a), None, 0, 0, ctypes.byref(h))
    msg = L.f5h_last_error().decode()
    assert rc == -1 and not h.value  # F5H_EINVAL
    assert msg.startswith("MMDiT: ") and field in msg, msg


def test_attn_mask_with_a_batch_is_refused_before_device_work():
    arch = configs.get_arch("MMDiT_tiny", text_num_embeds=64, attn_mask_enabled=True)
    net = _plugin(arch)
    m = CFM(transformer=net, num_channels=100, compute="fp32")  # on the CPU: any device work would fail differently
    inp = synthetic.make_case(**gc.B3)
    with pytest.raises(NotImplementedError, match="attn_mask_enabled"):
        m.sample(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=2)
    fi = mr.forward_inputs(gc.B3)
    with pytest.raises(NotImplementedError, match="prefix"):
        net(fi["x"], fi["cond"], fi["text"], torch.tensor(0.3), mask=fi["mask"], cfg_infer=True)
