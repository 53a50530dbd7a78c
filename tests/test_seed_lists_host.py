"""Per-utterance seeds on the host side (no GPU): `CFM.sample(seed=[...])` draws utterance b's noise from seed[b] in
every mode, and `infer_batch`'s per-item dicts override `speed` and `seed` for their item."""

from __future__ import annotations

import pytest
import torch

import golden_cases as gc
import ragged_fakes as rf
from f5_tts_amd import configs, infer, synthetic
from f5_tts_amd.model import CFM, DiT


class _Engine:
    """Records the noise CFM.sample hands to the engine."""

    def __init__(self):
        self.ragged, self.padded = [], []

    def sample(self, cond, cond_mask, text, duration, y0, t_grid, cfg_strength, use_batch_mask, **kw):
        self.padded.append(dict(y0=y0, mode=use_batch_mask))
        return torch.zeros_like(cond), None

    def sample_ragged(self, cond, cond_mask, text, durations, y0, t_grid, cfg_strength, keep_trajectory=True, **kw):
        self.ragged.append(dict(y0=y0, durations=list(durations)))
        return torch.zeros(cond.shape[0], 100), None


def _cfm(monkeypatch):
    arch = configs.get_arch("DiT_tiny", text_num_embeds=64)
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=64, mel_dim=arch["mel_dim"])
    eng = _Engine()
    monkeypatch.setattr(net, "get_engine", lambda compute, device: eng)
    return CFM(transformer=net, num_channels=100, compute="fp32"), eng


def _call(m, inp, **kw):
    return m.sample(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=4,
                    keep_trajectory=False, **kw)


@pytest.mark.parametrize("mode", [dict(), dict(isolate=True), dict(ragged=True)])
@pytest.mark.parametrize("seeds", [[11, 5, 11], (3, None, 4), torch.tensor([8, 9, 10])])
def test_seed_lists_give_every_utterance_its_own_noise(monkeypatch, mode, seeds):
    m, eng = _cfm(monkeypatch)
    inp = synthetic.make_case(**gc.B3)
    _call(m, inp, seed=seeds, **mode)
    call = (eng.ragged or eng.padded)[0]
    assert bool(eng.ragged) == bool(mode.get("ragged"))
    dur = [int(d) for d in inp["duration"]]
    vals = seeds.tolist() if torch.is_tensor(seeds) else list(seeds)
    torch.manual_seed(1234)  # the state a None entry draws from: whatever the previous draw left
    r = 0
    for b, d in enumerate(dur):
        if vals[b] is not None:
            torch.manual_seed(vals[b])
        want = torch.randn(d, 100)
        got = call["y0"][r: r + d] if call["y0"].ndim == 2 else call["y0"][b, :d]
        if vals[b] is not None or b > 0:
            assert torch.equal(got, want), (mode, b)
        r += d
    if call["y0"].ndim == 3:
        for b, d in enumerate(dur):
            assert not call["y0"][b, d:].any()


def test_an_int_seeds_every_utterance_alike(monkeypatch):
    m, eng = _cfm(monkeypatch)
    inp = synthetic.make_case(**gc.B3)
    _call(m, inp, seed=11)
    _call(m, inp, seed=[11, 11, 11])
    dur = [int(d) for d in inp["duration"]]
    a, b = eng.padded[0]["y0"], eng.padded[1]["y0"]
    assert torch.equal(a, b)
    for i, d in enumerate(dur):
        torch.manual_seed(11)
        assert torch.equal(a[i, :d], torch.randn(d, 100))


def test_one_utterance_takes_a_list_of_one(monkeypatch):
    m, eng = _cfm(monkeypatch)
    inp = synthetic.make_case(**gc.B1)
    _call(m, inp, seed=[6])
    torch.manual_seed(6)
    d = int(inp["duration"][0])
    assert torch.equal(eng.padded[0]["y0"][0, :d], torch.randn(d, 100))


@pytest.mark.parametrize("seeds", [[1, 2], (1, 2, 3, 4), torch.tensor([1])])
def test_wrong_length_raises_before_the_engine(monkeypatch, seeds):
    m, eng = _cfm(monkeypatch)
    inp = synthetic.make_case(**gc.B3)
    with pytest.raises(ValueError, match="entries for 3 utterances"):
        _call(m, inp, seed=seeds, ragged=True)
    assert not eng.ragged and not eng.padded


# ---------------------------------------------------------------- infer_batch with per-item dicts
class _Model(rf.FakeModel):
    def sample(self, cond, text, duration, *, lens, steps, cfg_strength, sway_sampling_coef, seed=None, **kw):
        out = super().sample(cond, text, duration, lens=lens, steps=steps, cfg_strength=cfg_strength,
                             sway_sampling_coef=sway_sampling_coef, seed=seed)
        self.calls[-1].update(kw=kw)
        return out


def _items():
    g = torch.Generator().manual_seed(3)
    sizes, gens = (6000, 12000, 7000, 15000), ("short text", "a considerably longer text to say", "mid length", "last")
    return [((torch.randn(1, n, generator=g) * 0.3, 24000), "a prompt here", t) for n, t in zip(sizes, gens)]


def test_infer_batch_hands_per_item_seeds_as_a_list():
    items = _items()
    items[0] += ({"seed": 9},)
    items[2] += ({},)
    m = _Model()
    infer.infer_batch(items, m, rf.FakeVocoder(), nfe_step=4, seed=3, max_batch=3, ragged=True)
    first, second = m.calls
    assert first["seed"] == [9, 3, 3] and first["steps"] == 4 and first["kw"] == {"ragged": True}
    assert second["seed"] == 3 and second["kw"] == {"ragged": True}  # a batch without overrides: the call it always was
    plain = _Model()
    infer.infer_batch(_items(), plain, rf.FakeVocoder(), nfe_step=4, seed=3, max_batch=3, ragged=True)
    assert [c["duration"] for c in plain.calls] == [first["duration"], second["duration"]]


@pytest.mark.parametrize("mode", [dict(), dict(isolate=True), dict(ragged=True)])
def test_infer_batch_per_item_speed(mode):
    """Twice the speed for one item: half its generated frames, the other items and their waves as they were."""
    base, fast = _items(), _items()
    fast[1] += ({"speed": 2.0, "seed": 5},)
    m0, m1 = _Model(), _Model()
    w0 = infer.infer_batch(base, m0, rf.FakeVocoder(), nfe_step=4, seed=3, max_batch=8, **mode)
    w1 = infer.infer_batch(fast, m1, rf.FakeVocoder(), nfe_step=4, seed=3, max_batch=8, **mode)
    (c0,), (c1,) = m0.calls, m1.calls
    assert c0["seed"] == 3 and sorted(c1["seed"]) == [3, 3, 3, 5]
    d0, d1 = sorted(c0["duration"]), sorted(c1["duration"])
    assert len(d1) == 4 and sum(d1) < sum(d0) and len(set(d0) & set(d1)) == 3
    ref = 1 + 12000 // 256  # item 1: its prompt's frames, and the duration rule at both speeds
    nb, gb = len("a prompt here ".encode()), len("a considerably longer text to say".encode())
    assert ref + int(ref / nb * gb / 1.0) in d0 and ref + int(ref / nb * gb / 2.0) in d1
    assert len(w1[1][0]) < len(w0[1][0])
    for i in (0, 2, 3):
        assert (w0[i][0] == w1[i][0]).all()


def test_infer_batch_refuses_other_per_item_settings():
    for key in ("nfe_step", "cfg_strength", "sway_sampling_coef", "nfe"):
        items = _items()
        items[2] += ({key: 2},)
        m = _Model()
        with pytest.raises(ValueError, match="item 2"):
            infer.infer_batch(items, m, rf.FakeVocoder(), nfe_step=4, ragged=True)
        assert not m.calls and not m.mel_spec.calls
