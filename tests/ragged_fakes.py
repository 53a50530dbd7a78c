"""Pure-torch stand-ins for `model_obj` (with its `mel_spec`) and `vocoder` with the ragged batch surface
(`forward_ragged`, `sample(..., lens=)`, `decode_ragged`), used to pin the host orchestration of
`infer.infer_batch` and `parallel.run_sharded(vocoder=...)` without a GPU. Every utterance's result is a function
of its own inputs only, so a single-utterance call is the expected value of any batch, and the calls are recorded."""

from __future__ import annotations

import torch

HOP = 256


class FakeMel:
    n_fft, hop_length, n_mel_channels = 1024, HOP, 100

    def __init__(self):
        self.calls = []

    def forward_ragged(self, wavs, lens=None, length=None):
        self.calls.append([int(w.shape[-1]) for w in wavs])
        frames = [1 + int(w.shape[-1]) // HOP for w in wavs]
        cond = torch.zeros(len(wavs), max(frames) if length is None else length, 100)
        for i, w in enumerate(wavs):
            w = w.reshape(-1).double()
            t = torch.arange(frames[i], dtype=torch.float64)[:, None]
            cond[i, : frames[i]] = (w.abs().mean() * 10 + 0.01 * t + 0.001 * torch.arange(100)[None]).float()
        return cond, frames


class FakeModel:
    device = torch.device("cpu")

    def __init__(self):
        self.mel_spec = FakeMel()
        self.calls = []

    def sample(self, cond, text, duration, *, lens, steps, cfg_strength, sway_sampling_coef, seed=None):
        assert duration.device.type == "cpu" and lens.device.type == "cpu"  # host lengths: no hidden sync
        self.calls.append(dict(text=["".join(t) for t in text], duration=duration.tolist(), lens=lens.tolist(),
                               steps=steps, cfg=cfg_strength, sway=sway_sampling_coef, seed=seed))
        out = torch.zeros(cond.shape[0], int(duration.max()), 100)
        for b in range(cond.shape[0]):
            n, r = int(duration[b]), int(lens[b])
            sig = float(cond[b, :r].double().sum()) * 1e-3 + 0.01 * len(text[b]) + 1e-3 * steps + 0.1 * cfg_strength
            t = torch.arange(n, dtype=torch.float64)[:, None]
            out[b, :n] = torch.sin(0.013 * t * (torch.arange(100)[None] + 1) + sig).float()
            out[b, n:] = 7.0  # what lies past an utterance's end must not reach its wave
        return out, None


class FakeVocoder:
    hop_length = HOP

    def __init__(self):
        self.calls = []

    def decode_ragged(self, feats, starts, lens, channels_last=True):
        starts = [int(v) for v in (starts.tolist() if torch.is_tensor(starts) else starts)]
        lens = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
        self.calls.append((starts, lens))
        out = []
        for i, (s, n) in enumerate(zip(starts, lens)):
            m = feats[i, s: s + n].double().mean(1)[:-1].repeat_interleave(HOP)
            out.append((0.3 * torch.tanh(m) + 0.05 * torch.sin(0.02 * torch.arange(m.shape[0]))).float())
        return out


def sample_fn(cond, text, duration, lens):
    """`run_sharded`'s sampler stand-in: row n of utterance b depends on its own prompt, tokens and lengths."""
    B, N = cond.shape[0], int(duration.max())
    out = torch.full((B, N, 100), 7.0)
    for b in range(B):
        n = int(duration[b])
        base = float(cond[b, : int(lens[b])].sum()) + float(text[b][text[b] >= 0].sum()) + 10.0 * n
        out[b, :n] = 1e-3 * base + torch.arange(n)[:, None] * 0.5 + 0.01 * torch.arange(100)[None]
    return out


def job(n=7):
    g = torch.Generator().manual_seed(11)
    utts = []
    for _ in range(n):
        total = int(torch.randint(20, 90, (1,), generator=g))
        ref = total // 3
        utts.append(dict(cond=torch.randn(ref, 100, generator=g), ref=ref, total=total,
                         text=torch.randint(0, 50, (ref // 4 + 1,), generator=g)))
    utts[2]["total"] = utts[2]["ref"] + 1  # one generated frame: an empty wave
    return utts


def expected_wave(u):
    out = sample_fn(u["cond"][None], u["text"][None], torch.tensor([u["total"]]), torch.tensor([u["ref"]]))
    return FakeVocoder().decode_ragged(out, [u["ref"]], [u["total"] - u["ref"]])[0]
