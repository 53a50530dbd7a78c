"""Isolated batches on the host side (no GPU): the flag's way from `CFM.sample` / `infer` down to the engine call, the
old-library refusal and the orchestration of `infer_batch_process(batch_chunks=True)` on stand-ins."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import golden_cases as gc
import ragged_fakes as rf
from f5_tts_amd import _lib, configs, infer, synthetic
from f5_tts_amd import engine as E
from f5_tts_amd.model import CFM, DiT
from infer_fakes import ref_audios


class _Engine:
    """Records what CFM.sample hands to Engine.sample."""

    def __init__(self):
        self.modes = []

    def sample(self, cond, cond_mask, text, duration, y0, t_grid, cfg_strength, use_batch_mask, **kw):
        self.modes.append(use_batch_mask)
        return torch.zeros_like(cond), None


def _cfm(monkeypatch):
    arch = configs.get_arch("DiT_tiny", text_num_embeds=64)
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=64, mel_dim=arch["mel_dim"])
    eng = _Engine()
    monkeypatch.setattr(net, "get_engine", lambda compute, device: eng)
    return CFM(transformer=net, num_channels=100, compute="fp32"), eng


def test_sample_hands_the_mode_to_the_engine(monkeypatch):
    m, eng = _cfm(monkeypatch)
    b3, b1 = synthetic.make_case(**gc.B3), synthetic.make_case(**gc.B1)
    for inp, isolate in ((b3, True), (b3, False), (b1, True), (b1, False)):
        m.sample(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=2,
                 isolate=isolate, keep_trajectory=False)
    assert [int(v) for v in eng.modes] == [2, 1, 0, 0]  # B = 1: the plain single call
    assert eng.modes[0] is not True


def test_mask_mode_values():
    arch = configs.get_arch("DiT_tiny", text_num_embeds=64)
    assert [E._mask_mode(arch, v) for v in (False, True, 0, 1, 2)] == [0, 1, 0, 1, 2]


def test_old_library_refuses_isolation(monkeypatch):
    """A library without f5h_op_attention_ranges: isolate=True raises, the plain batch runs as before."""
    monkeypatch.setattr(_lib, "has_isolate", lambda: False)
    m, eng = _cfm(monkeypatch)
    inp = synthetic.make_case(**gc.B3)
    with pytest.raises(NotImplementedError, match="f5h_op_attention_ranges"):
        m.sample(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=2, isolate=True)
    m.sample(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=2)
    assert [int(v) for v in eng.modes] == [1]  # the plain masked batch still runs


def test_mmdit_masked_batch_stays_refused_unless_isolated():
    """attn_mask_enabled with a plain batch mask keeps its refusal; the isolated call masks both key ranges itself."""
    masked = configs.get_arch("MMDiT_tiny", text_num_embeds=64, attn_mask_enabled=True)
    with pytest.raises(NotImplementedError, match="prefix"):
        E._refuse_mmdit_masked(masked, True)
    E._refuse_mmdit_masked(masked, False)
    E._refuse_mmdit_masked(masked, 2)
    E._refuse_mmdit_masked(configs.get_arch("MMDiT_tiny", text_num_embeds=64), True)


# ---------------------------------------------------------------- infer
class _Mel:
    def __init__(self):
        self.calls = 0

    def __call__(self, wav):  # [1, n] -> [1, 100, 1 + n // hop], a function of the wave
        self.calls += 1
        T = 1 + wav.shape[-1] // rf.HOP
        t = torch.arange(T, dtype=torch.float64)[None, :]
        return (float(wav.double().abs().mean()) * 10 + 0.01 * t + 0.001 * torch.arange(100)[:, None]).float()[None]

    def forward_ragged(self, *a, **k):
        raise AssertionError("batch_chunks takes the prompt's log-mel once, not forward_ragged")


class _Model:
    """A stand-in for CFM on which every utterance is a function of its own prompt, text and lengths: the raw-wave
    single call of the thread-pool path and a row of the batched call give the same frames."""

    device = torch.device("cpu")

    def __init__(self):
        self.mel_spec = _Mel()
        self.calls = []

    def sample(self, cond, text, duration, *, lens=None, steps, cfg_strength, sway_sampling_coef, isolate=False,
               seed=None):
        self.calls.append(dict(B=len(text), isolate=isolate, seed=seed,
                               duration=duration.tolist() if torch.is_tensor(duration) else duration,
                               lens=None if lens is None else lens.tolist(),
                               host=(not torch.is_tensor(duration)) or duration.device.type == "cpu"))
        if cond.ndim == 2:
            cond = self.mel_spec(cond).permute(0, 2, 1)
        B, F = cond.shape[0], cond.shape[1]
        dur = [int(duration)] * B if not torch.is_tensor(duration) else [int(v) for v in duration]
        dur = [max(max(len(t), F) + 1, d) for t, d in zip(text, dur)]
        out = torch.full((B, max(dur), 100), 7.0)
        for b in range(B):
            sig = float(cond[b].double().sum()) * 1e-3 + 0.01 * len(text[b]) + 1e-3 * steps + 0.1 * cfg_strength
            t = torch.arange(dur[b], dtype=torch.float64)[:, None]
            out[b, : dur[b]] = torch.sin(0.013 * t * (torch.arange(100)[None] + 1) + sig).float()
        return out, None


class _Vocoder(rf.FakeVocoder):
    def decode(self, mel):  # [1, 100, T]: the per-utterance form of decode_ragged
        return torch.stack(rf.FakeVocoder.decode_ragged(self, mel.permute(0, 2, 1), [0], [mel.shape[-1]]))


CHUNKS = ["I don't really care what you call me.", "I've been a silent spectator, watching species evolve.", "Hi."]


@pytest.mark.parametrize("amp", [0.05, 0.3])  # below target_rms (boosted, undone per wave) and above
def test_batch_chunks_is_one_batch_and_equals_the_thread_pool_path(amp):
    audio = ref_audios([amp])[0]
    kw = dict(nfe_step=8, cfg_strength=2.0, sway_sampling_coef=-1.0, device="cpu")
    ref_text = "Some call me nature, others call me mother nature."
    pool_m, pool_v = _Model(), _Vocoder()
    wav0, sr0, spec0 = next(infer.infer_batch_process((audio, 24000), ref_text, CHUNKS, pool_m, pool_v, **kw))
    assert [c["B"] for c in pool_m.calls] == [1, 1, 1] and not any(c["isolate"] for c in pool_m.calls)
    m, v = _Model(), _Vocoder()
    wav1, sr1, spec1 = next(infer.infer_batch_process((audio, 24000), ref_text, CHUNKS, m, v, batch_chunks=True, **kw))
    assert m.mel_spec.calls == 1 and len(m.calls) == 1 and len(v.calls) == 1
    call = m.calls[0]
    assert call["B"] == 3 and call["isolate"] is True and call["host"]
    frames = 1 + audio.shape[-1] // 256
    assert call["lens"] == [frames] * 3
    assert sorted(call["duration"]) == sorted(c["duration"] for c in pool_m.calls)  # (the pool's order is free)
    assert v.calls[0][0] == [audio.shape[-1] // 256] * 3
    assert sr0 == sr1 == 24000
    assert np.array_equal(wav0, wav1) and np.array_equal(spec0, spec1)
    s0 = list(infer.infer_batch_process((audio, 24000), ref_text, CHUNKS, _Model(), _Vocoder(), streaming=True,
                                        chunk_size=3000, **kw))
    s1 = list(infer.infer_batch_process((audio, 24000), ref_text, CHUNKS, _Model(), _Vocoder(), streaming=True,
                                        chunk_size=3000, batch_chunks=True, **kw))
    assert len(s0) == len(s1) and all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(s0, s1))


def test_batch_chunks_with_one_chunk_is_the_single_call():
    audio = ref_audios([0.3])[0]
    m = _Model()
    next(infer.infer_batch_process((audio, 24000), "ref text.", ["only one chunk"], m, _Vocoder(), nfe_step=4,
                                   device="cpu", batch_chunks=True))
    assert len(m.calls) == 1 and m.calls[0]["isolate"] is False and m.mel_spec.calls == 1  # (inside the single call)


class _RaggedModel(rf.FakeModel):
    def sample(self, cond, text, duration, *, isolate=False, **kw):
        out = super().sample(cond, text, duration, **kw)
        self.calls[-1]["isolate"] = isolate
        return out


def test_infer_batch_forwards_isolate():
    g = torch.Generator().manual_seed(3)
    items = [((torch.randn(1, n, generator=g) * 0.3, 24000), "a prompt here", "and something to say")
             for n in (6000, 9000, 7000)]
    for isolate in (False, True):
        m = _RaggedModel()
        infer.infer_batch(items, m, rf.FakeVocoder(), nfe_step=4, isolate=isolate)
        assert m.calls and all(c["isolate"] is isolate for c in m.calls)
    plain = rf.FakeModel()  # a model without the keyword keeps working while the flag is off
    infer.infer_batch(items, plain, rf.FakeVocoder(), nfe_step=4)
    assert plain.calls
