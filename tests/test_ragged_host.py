"""Ragged sampling on the host side (no GPU): the exports, the old-library and backbone refusals, the packing that
`CFM.sample(ragged=True)` hands to the engine and the unpacking of what comes back, and `infer_batch`'s batching."""

from __future__ import annotations

import ctypes
import types

import pytest
import torch

import golden_cases as gc
import ragged_fakes as rf
from f5_tts_amd import _lib, configs, infer, parallel, synthetic
from f5_tts_amd import engine as E
from f5_tts_amd.model import CFM, DiT, MMDiT, UNetT

RAGGED_EXPORTS = ("f5h_sample_ragged", "f5h_workspace_size_ragged", "f5h_op_attention_ragged",
                  "f5h_op_conv_pos_ragged", "f5h_op_grn_ragged")


def test_library_exports_the_ragged_entry_points():
    L = _lib.lib()
    for name in RAGGED_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert _lib.has_ragged_sampler() is True
    # the appended fields of the GEMM op hook and the call's argument struct, as include/f5h.h lays them out
    assert _lib.OpGemmArgs.seg_off.offset == _lib.OpGemmArgs.qkv_dst_len.offset + 4
    assert _lib.OpGemmArgs.n_seq.offset == _lib.OpGemmArgs.seg_off.offset + 8
    assert _lib.RaggedArgs.R.offset == 16 and ctypes.sizeof(_lib.RaggedArgs) == 96


def test_ragged_calls_without_a_device_are_refused_by_value():
    """The C entry points validate before any device work: null arguments and a workspace query without an engine."""
    L = _lib.lib()
    assert L.f5h_workspace_size_ragged(None, 3, 310, 150, 30, 4, 1, 0) == 0
    assert L.f5h_sample_ragged(None, None, None, 0, None, 0) == -1


class _Engine:
    """Records what CFM.sample hands to the engine and returns a known packed result."""

    def __init__(self):
        self.ragged, self.padded = [], []

    def sample(self, cond, cond_mask, text, duration, y0, t_grid, cfg_strength, use_batch_mask, **kw):
        self.padded.append(dict(cond=cond, cond_mask=cond_mask, y0=y0, mode=use_batch_mask))
        return torch.zeros_like(cond), None

    def sample_ragged(self, cond, cond_mask, text, durations, y0, t_grid, cfg_strength, keep_trajectory=True, **kw):
        self.ragged.append(dict(cond=cond, cond_mask=cond_mask, y0=y0, text=text, durations=list(durations)))
        R, nfe = cond.shape[0], len(t_grid) - 1
        out = torch.arange(R * 100, dtype=torch.float32).reshape(R, 100) + 1.0
        traj = torch.stack([out * (k + 1) for k in range(nfe + 1)]) if keep_trajectory else None
        return out, traj


def _cfm(monkeypatch, cls=DiT, preset="DiT_tiny", **over):
    arch = configs.get_arch(preset, text_num_embeds=64, **over)
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = cls(**kw, text_num_embeds=64, mel_dim=arch["mel_dim"])
    eng = _Engine()
    monkeypatch.setattr(net, "get_engine", lambda compute, device: eng)
    return CFM(transformer=net, num_channels=100, compute="fp32"), eng


def _pack(x, dur):
    return torch.cat([x[b, :d] for b, d in enumerate(dur)], dim=0)


@pytest.mark.parametrize("variant", ["plain", "edit_mask", "duplicate_test", "no_ref_audio"])
def test_sample_packs_the_padded_batch(monkeypatch, variant):
    """The packed cond / cond_mask / y0 are the padded batch's valid rows, concatenated; the result keeps the padded
    shapes with exact zeros past every duration."""
    m, eng = _cfm(monkeypatch)
    inp = synthetic.make_case(**gc.B3)
    kw = dict(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=4, seed=7)
    if variant == "edit_mask":
        em = torch.ones(3, inp["cond"].shape[1], dtype=torch.bool)
        em[:, 5:9] = False
        kw["edit_mask"] = em
    elif variant != "plain":
        kw[variant] = True
    m.sample(isolate=True, **kw)
    out, traj = m.sample(ragged=True, **kw)
    assert len(eng.padded) == 1 and len(eng.ragged) == 1
    pad, rag = eng.padded[0], eng.ragged[0]
    assert int(pad["mode"]) == 2
    dur = rag["durations"]
    assert dur == [int(d) for d in inp["duration"]] and all(isinstance(d, int) for d in dur)
    R = sum(dur)
    assert rag["cond"].shape == (R, 100) and rag["y0"].shape == (R, 100) and rag["cond_mask"].shape == (R,)
    assert torch.equal(rag["cond"], _pack(pad["cond"], dur))
    assert torch.equal(rag["cond_mask"], _pack(pad["cond_mask"], dur))
    assert torch.equal(rag["y0"], _pack(pad["y0"], dur))
    assert rag["text"].shape[0] == 3
    # unpacking: the engine's packed rows land at [b, :dur[b]], everything else is zero
    N = max(dur)
    assert out.shape == (3, N, 100) and traj.shape[1:] == (3, N, 100)
    known = torch.arange(R * 100, dtype=torch.float32).reshape(R, 100) + 1.0
    r = 0
    for b, d in enumerate(dur):
        assert torch.equal(out[b, :d], known[r: r + d]) and not out[b, d:].any()
        for k in range(traj.shape[0]):
            assert torch.equal(traj[k, b, :d], known[r: r + d] * (k + 1)) and not traj[k, b, d:].any()
        r += d


def test_one_utterance_is_the_plain_call(monkeypatch):
    m, eng = _cfm(monkeypatch)
    inp = synthetic.make_case(**gc.B1)
    m.sample(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=2, ragged=True)
    assert not eng.ragged and [int(p["mode"]) for p in eng.padded] == [0]


@pytest.mark.parametrize("cls,preset", [(UNetT, "UNetT_tiny"), (MMDiT, "MMDiT_tiny")])
def test_other_backbones_refuse_ragged(monkeypatch, cls, preset):
    m, eng = _cfm(monkeypatch, cls, preset)
    inp = synthetic.make_case(**gc.B3)
    with pytest.raises(NotImplementedError, match="DiT backbone only"):
        m.sample(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=2, ragged=True)
    assert not eng.ragged and not eng.padded  # refused before touching the engine


def test_text_average_upsampling_refuses_ragged():
    arch = configs.get_arch("DiT_tiny", text_num_embeds=64, text_embedding_average_upsampling=True)
    with pytest.raises(NotImplementedError, match="average_upsampling"):
        E._refuse_ragged(arch)
    E._refuse_ragged(configs.get_arch("DiT_tiny", text_num_embeds=64))


def test_old_library_refuses_ragged(monkeypatch):
    """A library object without f5h_sample_ragged (an older build through F5H_LIB): RuntimeError, nothing runs."""
    real = _lib.lib()
    old = types.SimpleNamespace(**{n: getattr(real, n) for n in _lib.EXPORTS
                                   if n not in RAGGED_EXPORTS and hasattr(real, n)})
    monkeypatch.setattr(_lib, "_lib", old)
    assert _lib.has_ragged_sampler() is False
    m, eng = _cfm(monkeypatch)
    inp = synthetic.make_case(**gc.B3)
    with pytest.raises(RuntimeError, match="f5h_sample_ragged"):
        m.sample(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=2, ragged=True)
    assert not eng.ragged and not eng.padded
    m.sample(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=2, isolate=True)
    assert len(eng.padded) == 1  # the isolated batch still runs


class _RaggedModel(rf.FakeModel):
    def sample(self, cond, text, duration, *, isolate=False, ragged=False, **kw):
        out = super().sample(cond, text, duration, **kw)
        self.calls[-1].update(isolate=isolate, ragged=ragged)
        return out


def test_infer_batch_ragged_sends_input_order_batches():
    """ragged=True: batches of max_batch in input order, no length buckets; the waves are those of isolate=True."""
    g = torch.Generator().manual_seed(3)
    sizes = (6000, 12000, 7000, 15000, 6500, 9000, 8000)
    gens = ("short", "a considerably longer text to say, with more bytes in it", "mid length text here",
            "and another long one that stretches the total frames a lot", "tiny", "something to say", "the last")
    items = [((torch.randn(1, n, generator=g) * 0.3, 24000), "a prompt here", t) for n, t in zip(sizes, gens)]
    m, v = _RaggedModel(), rf.FakeVocoder()
    rag = infer.infer_batch(items, m, v, nfe_step=4, max_batch=3, ragged=True)
    assert [len(c["duration"]) for c in m.calls] == [3, 3, 1]
    assert all(c["ragged"] is True and c["isolate"] is False for c in m.calls)
    assert [n for c in m.mel_spec.calls for n in c] == list(sizes)  # input order, whatever the lengths
    m2 = _RaggedModel()
    iso = infer.infer_batch(items, m2, rf.FakeVocoder(), nfe_step=4, max_batch=3, isolate=True)
    assert all(c["isolate"] is True and c["ragged"] is False for c in m2.calls)
    assert sorted(n for c in m2.mel_spec.calls for n in c) == sorted(sizes)
    for (w0, _), (w1, _) in zip(iso, rag):
        assert w0.shape == w1.shape and (w0 == w1).all()
    plain = rf.FakeModel()  # a model without the keyword keeps working while the flag is off
    infer.infer_batch(items, plain, rf.FakeVocoder(), nfe_step=4)
    assert plain.calls


def test_run_sharded_passes_ragged():
    seen = []

    def fn(cond, text, duration, lens, ragged=False):
        seen.append(ragged)
        return rf.sample_fn(cond, text, duration, lens)

    utts = rf.job(5)
    a = parallel.run_sharded(utts, fn, rank=0, world=1, max_batch=2, ragged=True)
    assert seen and all(seen)
    b = parallel.run_sharded(utts, rf.sample_fn, rank=0, world=1, max_batch=2)
    assert all(torch.equal(a[i], b[i]) for i in a)
