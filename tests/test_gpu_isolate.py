"""Isolated batches (CFM.sample(isolate=True), use_batch_mask == 2) on the GPU: every utterance of a padded batch is
computed as if it were sampled alone.

DiT and UNetT: bitwise equal, over each utterance's own frames, to the three B = 1 calls (fp32 and bf16, 4 NFE steps,
seed 7, the per-utterance noise of cfm.py:196-201). In bf16 the engine's LayerNorm / RMSNorm fold is off for the whole
comparison: a masked DiT batch never folds, and the fold is not bitwise the separate launches. The same batch without
isolation must differ from the single calls by more than 1e-3 (the reference differs by more than 1e-2 there): this
is the check that fails without the feature. All backbones, MMDiT included: replacing a shorter neighbour leaves the
other utterances' bits unchanged. MMDiT against its single calls is not bitwise (the text keys' tile partition differs
between a batch and a single call): fp32 within the project's parity bound 1e-3, and the unisolated batch at least
10 x further away.

Measured on MI355X (max-abs over max-abs against the B = 1 calls, worst utterance; DESIGN.md §3 'Isolated batches'):
isolated DiT / UNetT 0 (bitwise), MMDiT fp32 3.8e-7; unisolated DiT 9.0e-2, text_mask_padding=False 5.3e-2, UNetT
4.0e-1, MMDiT 1.0e-1."""

import functools
import threading

import numpy as np
import pytest
import torch

from f5_tts_amd import configs, infer, synthetic
from f5_tts_amd.model import CFM, DiT, MMDiT, UNetT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NFE, SEED, CFG, SWAY = 4, 7, 2.0, -1.0
ARCHS = {
    "dit": ("DiT_tiny", {}),
    "dit_nopad": ("DiT_tiny", {"text_mask_padding": False}),
    "unett": ("UNetT_tiny", {}),
    "mmdit": ("MMDiT_tiny", {}),
}
# (total frames, prompt frames, text tokens) per utterance. "b3": golden_cases.B3's lengths; "tile": the 64-key tile and
# the 64-row GRN chunk exactly, one past two of them, one past one
CASES = {
    "b3": [(90, 40, 20), (150, 60, 30), (70, 25, 12)],
    "tile": [(64, 30, 15), (129, 50, 25), (65, 20, 10)],
}
OTHER = (80, 33, 16)  # the neighbour that replaces the last utterance in the invariance test


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _model(arch_key, compute, method="euler"):
    name, over = ARCHS[arch_key]
    arch = configs.get_arch(name, text_num_embeds=64, **over)
    cls = {"DiT": DiT, "UNetT": UNetT, "MMDiT": MMDiT}[arch["backbone"]]
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = cls(**kw, text_num_embeds=64, mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    m = CFM(transformer=net, num_channels=100, compute=compute, odeint_kwargs=dict(method=method)).to(DEV)
    if compute != "fp32":
        m.transformer.get_engine(compute, m.device).set_ln_fold(False)
    return m


def _utt(spec, seed):
    """One utterance as its own B = 1 case (a row of make_case(B=3) is not its B = 1 case: the generator runs on)."""
    total, ref, nt = spec
    return synthetic.make_case(B=1, ref_frames=ref, total_frames=total, n_text=nt, seed=seed, vocab=64)


def _stack(utts):
    R, T = max(u["cond"].shape[1] for u in utts), max(u["text"].shape[1] for u in utts)
    cond = torch.zeros(len(utts), R, 100)
    text = torch.full((len(utts), T), -1, dtype=torch.long)
    for i, u in enumerate(utts):
        cond[i, : u["cond"].shape[1]] = u["cond"][0]
        text[i, : u["text"].shape[1]] = u["text"][0]
    return dict(cond=cond, text=text, lens=torch.cat([u["lens"] for u in utts]),
                duration=torch.cat([u["duration"] for u in utts]))


def _sample(m, inp, isolate):
    out, _ = m.sample(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=inp["duration"], lens=inp["lens"],
                      steps=NFE, cfg_strength=CFG, sway_sampling_coef=SWAY, seed=SEED, keep_trajectory=False,
                      isolate=isolate)
    torch.cuda.synchronize()
    return out.float().cpu()


def _specs(case):
    return CASES[case] if isinstance(case, str) else list(case)


@functools.lru_cache(maxsize=None)
def _singles(arch_key, compute, case, method="euler"):
    """The B = 1 calls of a case's utterances (utterance i: make_case seed 100 + its total frames)."""
    m = _model(arch_key, compute, method)
    return tuple(_sample(m, _utt(s, 100 + s[0]), False)[0] for s in _specs(case))


@functools.lru_cache(maxsize=None)
def _batch(arch_key, compute, case, isolate, method="euler"):
    m = _model(arch_key, compute, method)
    return _sample(m, _stack([_utt(s, 100 + s[0]) for s in _specs(case)]), isolate)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _worst(batch, singles, case):
    return max(_rel(batch[i, : s[0]], singles[i]) for i, s in enumerate(_specs(case)))


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("arch_key", ["dit", "dit_nopad", "unett"])
def test_isolated_batch_equals_single_calls_bitwise(arch_key, case, compute):
    _need_gpu()
    singles, batch = _singles(arch_key, compute, case), _batch(arch_key, compute, case, True)
    assert torch.isfinite(batch).all()
    for i, s in enumerate(_specs(case)):
        assert singles[i].shape[0] == s[0]
        print(f"isolate {arch_key}/{compute}/{case} utterance {i}: max-rel {_rel(batch[i, : s[0]], singles[i]):.3e}")
        assert torch.equal(batch[i, : s[0]], singles[i]), (arch_key, compute, case, i)


@pytest.mark.parametrize("arch_key", ["dit", "unett"])
def test_isolated_midpoint_equals_single_calls_bitwise(arch_key):
    _need_gpu()
    singles, batch = _singles(arch_key, "fp32", "b3", "midpoint"), _batch(arch_key, "fp32", "b3", True, "midpoint")
    for i, s in enumerate(CASES["b3"]):
        assert torch.equal(batch[i, : s[0]], singles[i]), i
    assert not torch.equal(singles[1], _singles(arch_key, "fp32", "b3")[1]), "the solver had no effect"


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("arch_key", ["dit", "dit_nopad", "unett"])
def test_unisolated_batch_leaks(arch_key, compute):
    """The padded batch as the reference computes it: an utterance's mel depends on its neighbours (pad keys, GRN
    over the padded axis, unmasked conv position embedding). The reference's own figures on this batch (CPU, fp32,
    utterance 0): DiT 6.6e-2, UNetT 2.7e-1."""
    _need_gpu()
    d = _worst(_batch(arch_key, compute, "b3", False), _singles(arch_key, compute, "b3"), "b3")
    print(f"leak {arch_key}/{compute}: unisolated batch vs single calls, worst utterance max-rel {d:.3e}")
    assert d > 1e-3


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("arch_key", sorted(ARCHS))
def test_neighbour_does_not_change_the_others(arch_key, compute):
    """The longest utterance stays; the last one is replaced by another utterance of another length."""
    _need_gpu()
    other = tuple(CASES["b3"][:2]) + (OTHER,)
    a, b = _batch(arch_key, compute, "b3", True), _batch(arch_key, compute, other, True)
    for i in (0, 1):
        n = CASES["b3"][i][0]
        assert torch.equal(a[i, :n], b[i, :n]), (arch_key, compute, i)
    assert not torch.equal(a[2, :70], b[2, :70])


def test_mmdit_isolated_batch_matches_single_calls():
    _need_gpu()
    singles = _singles("mmdit", "fp32", "b3")
    iso = _worst(_batch("mmdit", "fp32", "b3", True), singles, "b3")
    leak = _worst(_batch("mmdit", "fp32", "b3", False), singles, "b3")
    print(f"mmdit/fp32: isolated batch vs single calls max-rel {iso:.3e}; unisolated {leak:.3e}")
    assert iso <= 1e-3
    assert leak >= 10 * iso


@pytest.mark.parametrize("arch_key", sorted(ARCHS))
def test_isolate_is_the_plain_call_for_one_utterance(arch_key):
    _need_gpu()
    m, u = _model(arch_key, "bf16"), _utt(CASES["b3"][0], 190)
    assert torch.equal(_sample(m, u, True), _sample(m, u, False))


@pytest.mark.parametrize("arch_key", ["dit", "unett", "mmdit"])
def test_replayed_call_equals_the_first(arch_key):
    _need_gpu()
    m = _model(arch_key, "bf16")
    inp = _stack([_utt(s, 100 + s[0]) for s in CASES["tile"]])
    outs = [_sample(m, inp, True) for _ in range(3)]  # eager / captured, then replays
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])


@pytest.mark.parametrize("arch_key", ["dit", "unett"])
def test_plugin_forward_isolated(arch_key):
    """The backbone plugin's forward(isolate=True): bitwise the single forwards over each sample's own rows, and the
    slope of the engine's first Euler evaluation (one-step trajectory of the isolated sample call, fp32)."""
    _need_gpu()
    from f5_tts_amd.model.utils import lens_to_mask, time_grid

    m = _model(arch_key, "fp32")
    net = m.transformer
    utts = [_utt(s, 100 + s[0]) for s in CASES["b3"]]
    inp = _stack(utts)
    dur, lens = inp["duration"], inp["lens"]
    N = int(dur.max())
    y0 = synthetic.reference_noise(dur.tolist(), SEED)
    cmask = lens_to_mask(lens, length=N)[..., None]
    cond = torch.nn.functional.pad(inp["cond"], (0, 0, 0, N - inp["cond"].shape[1]))
    step_cond = torch.where(cmask, cond, torch.zeros_like(cond))
    t = time_grid(1, SWAY, True, device="cpu", dtype=torch.float32)
    pc = net(y0.to(DEV), step_cond.to(DEV), inp["text"].to(DEV), t[0].to(DEV), mask=lens_to_mask(dur).to(DEV),
             cfg_infer=True, isolate=True).cpu()
    for i, u in enumerate(utts):
        n, r = int(dur[i]), int(lens[i])
        c1 = torch.zeros(1, n, 100)
        c1[0, :r] = u["cond"][0]
        one = net(y0[i: i + 1, :n].to(DEV), c1.to(DEV), u["text"].to(DEV), t[0].to(DEV), mask=None,
                  cfg_infer=True).cpu()
        assert torch.equal(pc[i, :n], one[0]) and torch.equal(pc[3 + i, :n], one[1]), i
    _, traj = m.sample(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=dur, lens=lens, steps=1,
                       cfg_strength=CFG, sway_sampling_coef=SWAY, y0=y0.to(DEV), isolate=True)
    f = pc[:3] + (pc[:3] - pc[3:]) * CFG
    y1 = y0 + float(t[1] - t[0]) * f
    for i in range(3):
        n = int(dur[i])
        assert _rel(traj[1][i, :n].float().cpu(), y1[i, :n]) < 1e-5, i


def test_batched_chunks_equal_the_thread_pool_path():
    """infer_batch_process(batch_chunks=True): a 3-chunk text as one isolated batch (one log-mel, one sample, one
    decode_ragged) gives the wave and the spectrogram of the per-chunk calls, bit for bit."""
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
    g = torch.Generator().manual_seed(9)
    audio = torch.randn(1, 9000, generator=g) * 0.05  # below target_rms: boosted, and undone on every wave
    chunks = ["Others call me mother nature.", "Hi.", "And a rather longer sentence to generate, here it is."]

    class Seeded:
        """The model with a fixed noise seed. CFM.sample seeds the device generator and draws per utterance; the lock
        keeps one thread-pool call's seed-and-draw from interleaving with another's."""

        device, mel_spec, lock = model.device, model.mel_spec, threading.Lock()

        def sample(self, **kw):
            with self.lock:
                return model.sample(seed=3, **kw)

    kw = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0)
    w0, sr0, s0 = next(infer.infer_batch_process((audio, 24000), "Some call me nature.", chunks, Seeded(), voc, **kw))
    w1, sr1, s1 = next(infer.infer_batch_process((audio, 24000), "Some call me nature.", chunks, Seeded(), voc,
                                                 batch_chunks=True, **kw))
    assert sr0 == sr1 == 24000 and np.isfinite(w0).all()
    assert w0.shape == w1.shape and np.array_equal(w0, w1)
    assert s0.shape == s1.shape and np.array_equal(s0, s1)
