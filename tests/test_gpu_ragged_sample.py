"""Ragged sampling (CFM.sample(ragged=True), f5h_sample_ragged) on the GPU: the utterances of a batch as packed rows,
no pad frames, every utterance bit for bit its own B = 1 call and hence the isolate=True batch.

The recipe of tests/test_gpu_isolate.py: tiny DiT models with synthetic weights, NFE 4, seed 7, cfg 2.0, sway -1,
utterance i built by make_case(B=1, seed=100 + its total frames), the LayerNorm fold off in the 16-bit single calls
(a ragged call never folds, and the fold is not bitwise the separate launches). All comparisons are torch.equal over
rows [0, duration); rows past a duration are exact zeros."""

import functools

import numpy as np
import pytest
import torch

from f5_tts_amd import configs, infer, synthetic
from f5_tts_amd.model import CFM, DiT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NFE, SEED, CFG, SWAY = 4, 7, 2.0, -1.0
ARCHS = {
    "dit": {},
    "dit_nopad": {"text_mask_padding": False},
    # F5TTS_Base's options: ConvNeXt text blocks, RoPE on the first head only, no text mask padding
    "base": {"conv_layers": 2, "pe_attn_head": 1, "text_mask_padding": False},
    "opts": {"qk_norm": "rms_norm", "long_skip_connection": True},
}
# (total frames, prompt frames, text tokens); "tile": on, two past and one past the 64-key tile / 64-row GRN chunk
CASES = {
    "b3": ((90, 40, 20), (150, 60, 30), (70, 25, 12)),
    "tile": ((64, 30, 15), (129, 50, 25), (65, 20, 10)),
}
B3_PERMUTED = ((70, 25, 12), (150, 60, 30), (90, 40, 20))  # the same (B, R, Lmax) as b3, other lengths per slot
OTHER = (80, 33, 16)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _model(arch_key, compute, method="euler"):
    arch = configs.get_arch("DiT_tiny", text_num_embeds=64, **ARCHS[arch_key])
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=64, mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    m = CFM(transformer=net, num_channels=100, compute=compute, odeint_kwargs=dict(method=method)).to(DEV)
    if compute != "fp32":
        m.transformer.get_engine(compute, m.device).set_ln_fold(False)
    return m


def _utt(spec):
    total, ref, nt = spec
    return synthetic.make_case(B=1, ref_frames=ref, total_frames=total, n_text=nt, seed=100 + total, vocab=64)


def _stack(utts):
    Rf, T = max(u["cond"].shape[1] for u in utts), max(u["text"].shape[1] for u in utts)
    cond = torch.zeros(len(utts), Rf, 100)
    text = torch.full((len(utts), T), -1, dtype=torch.long)
    for i, u in enumerate(utts):
        cond[i, : u["cond"].shape[1]] = u["cond"][0]
        text[i, : u["text"].shape[1]] = u["text"][0]
    return dict(cond=cond, text=text, lens=torch.cat([u["lens"] for u in utts]),
                duration=torch.cat([u["duration"] for u in utts]))


def _sample(m, inp, traj=False, **kw):
    out, tr = m.sample(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=inp["duration"], lens=inp["lens"],
                       steps=NFE, cfg_strength=CFG, sway_sampling_coef=SWAY, seed=SEED, keep_trajectory=traj, **kw)
    torch.cuda.synchronize()
    return (out.float().cpu(), tr.float().cpu()) if traj else out.float().cpu()


@functools.lru_cache(maxsize=None)
def _singles(arch_key, compute, specs, method="euler"):
    m = _model(arch_key, compute, method)
    return tuple(_sample(m, _utt(s))[0] for s in specs)


@functools.lru_cache(maxsize=None)
def _batch(arch_key, compute, specs, mode, method="euler"):
    m = _model(arch_key, compute, method)
    return _sample(m, _stack([_utt(s) for s in specs]), **{mode: True})


def _check_against_singles(batch, singles, specs, tag):
    assert torch.isfinite(batch).all()
    assert batch.shape[1] == max(s[0] for s in specs)
    for i, s in enumerate(specs):
        assert singles[i].shape[0] == s[0]
        assert torch.equal(batch[i, : s[0]], singles[i]), (tag, i)
        assert not batch[i, s[0]:].any(), (tag, i, "rows past the duration are exact zeros")


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("arch_key", sorted(ARCHS))
def test_ragged_equals_single_calls_and_isolated_batch(arch_key, case, compute):
    _need_gpu()
    specs = CASES[case]
    rag = _batch(arch_key, compute, specs, "ragged")
    _check_against_singles(rag, _singles(arch_key, compute, specs), specs, (arch_key, case, compute))
    iso = _batch(arch_key, compute, specs, "isolate")
    for i, s in enumerate(specs):
        assert torch.equal(rag[i, : s[0]], iso[i, : s[0]]), (arch_key, case, compute, i)


@pytest.mark.parametrize("arch_key", sorted(ARCHS))
def test_ragged_fp16(arch_key):
    _need_gpu()
    specs = CASES["b3"]
    _check_against_singles(_batch(arch_key, "fp16", specs, "ragged"), _singles(arch_key, "fp16", specs), specs,
                           (arch_key, "fp16"))


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_ragged_midpoint(compute):
    _need_gpu()
    specs = CASES["b3"]
    singles = _singles("dit", compute, specs, "midpoint")
    _check_against_singles(_batch("dit", compute, specs, "ragged", "midpoint"), singles, specs, ("midpoint", compute))
    assert not torch.equal(singles[1], _singles("dit", compute, specs)[1]), "the solver had no effect"


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_ragged_trajectory_equals_single_calls(compute):
    _need_gpu()
    m, specs = _model("dit", compute), CASES["b3"]
    out, traj = _sample(m, _stack([_utt(s) for s in specs]), traj=True, ragged=True)
    assert traj.shape == (NFE + 1, 3, 150, 100)
    for i, s in enumerate(specs):
        o1, t1 = _sample(m, _utt(s), traj=True)
        assert torch.equal(traj[:, i, : s[0]], t1[:, 0]), i
        assert torch.equal(out[i, : s[0]], o1[0]), i
        assert not traj[:, i, s[0]:].any()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_equal_shape_other_lengths_replays_one_graph(compute):
    """Two calls with equal (B, R, Lmax) and different lengths share one captured step graph; the lengths live in the
    workspace's segment tables. A length baked into a captured launch would make the second call wrong."""
    _need_gpu()
    m = _model("base", compute)
    eng = m.transformer.get_engine(compute, m.device)
    first = _sample(m, _stack([_utt(s) for s in CASES["b3"]]), ragged=True)
    cap = eng.graph_stats()["captures"]
    second = _sample(m, _stack([_utt(s) for s in B3_PERMUTED]), ragged=True)
    assert eng.graph_stats()["captures"] == cap, "the second call captured a graph of its own"
    _check_against_singles(first, _singles("base", compute, CASES["b3"]), CASES["b3"], "first")
    _check_against_singles(second, _singles("base", compute, B3_PERMUTED), B3_PERMUTED, "second")


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_neighbour_does_not_change_the_others(compute):
    _need_gpu()
    other = CASES["b3"][:2] + (OTHER,)
    a, b = _batch("dit", compute, CASES["b3"], "ragged"), _batch("dit", compute, other, "ragged")
    for i in (0, 1):
        n = CASES["b3"][i][0]
        assert torch.equal(a[i, :n], b[i, :n]), (compute, i)
    assert not torch.equal(a[2, :70], b[2, :70])


def test_ragged_is_the_plain_call_for_one_utterance():
    _need_gpu()
    m, u = _model("dit", "bf16"), _utt(CASES["b3"][0])
    assert torch.equal(_sample(m, u, ragged=True), _sample(m, u))


def test_replayed_call_equals_the_first():
    _need_gpu()
    m = _model("base", "bf16")
    inp = _stack([_utt(s) for s in CASES["tile"]])
    outs = [_sample(m, inp, ragged=True) for _ in range(3)]
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])


def test_workspace_is_smaller_than_the_padded_batch():
    _need_gpu()
    m = _model("dit", "bf16")
    eng = m.transformer.get_engine("bf16", m.device)
    dur = [s[0] for s in CASES["tile"]]
    nt = max(s[2] for s in CASES["tile"])
    ragged = eng.workspace_bytes_ragged(dur, nt, NFE)
    padded = eng.workspace_bytes(len(dur), max(dur), nt, NFE)
    print(f"workspace tile case: ragged {ragged} B, padded {padded} B")
    assert 0 < ragged < padded


def test_infer_batch_ragged_waveforms_equal_isolated():
    """infer_batch(ragged=True) against infer_batch(isolate=True): the same waveforms, bit for bit."""
    _need_gpu()
    from f5_tts_amd.vocos import Vocos, make_weights

    arch = configs.get_arch("DiT_tiny", text_num_embeds=256)
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=256, mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    model = CFM(transformer=net, num_channels=100, compute="fp32",
                vocab_char_map={chr(i): i for i in range(256)}).to(DEV)
    voc = Vocos(compute="fp32")
    voc.load_state_dict(make_weights())
    voc = voc.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    items = [((torch.randn(1, n, generator=g) * 0.05, 24000), ref, gen) for n, ref, gen in (
        (9000, "Some call me nature.", "Others call me mother nature."),
        (6000, "A short one.", "Hi there."),
        (12000, "The longest reference of the three, by far.", "And a rather longer sentence to generate."),
        (7000, "Number four.", "The fourth utterance goes to the second batch."))]
    kw = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3, max_batch=3)
    iso = infer.infer_batch(items, model, voc, isolate=True, **kw)
    rag = infer.infer_batch(items, model, voc, ragged=True, **kw)
    assert len(iso) == len(rag) == 4
    for (w0, sr0), (w1, sr1) in zip(iso, rag):
        assert sr0 == sr1 == 24000 and np.isfinite(w0).all()
        assert w0.shape == w1.shape and np.array_equal(w0, w1)
