"""Per-utterance seeds on the GPU: in an isolated or ragged batch, utterance b sampled with seed[b] is bit for bit
its own B = 1 call with that seed. The recipe of tests/test_gpu_ragged_sample.py (DiT_tiny, synthetic weights, NFE 4,
cfg 2.0, sway -1, the LayerNorm fold off in the 16-bit single calls)."""

import functools

import pytest
import torch

from f5_tts_amd import configs, synthetic
from f5_tts_amd.model import CFM, DiT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPECS = ((64, 30, 15), (129, 50, 25), (65, 20, 10))  # (total frames, prompt frames, text tokens)
SEEDS = (11, 5, 11)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _model(compute):
    arch = configs.get_arch("DiT_tiny", text_num_embeds=64)
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=64, mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    m = CFM(transformer=net, num_channels=100, compute=compute).to(DEV)
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


def _sample(m, inp, seed, **kw):
    out, _ = m.sample(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=inp["duration"], lens=inp["lens"],
                      steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=seed, keep_trajectory=False, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


@functools.lru_cache(maxsize=None)
def _single(compute, spec, seed):
    return _sample(_model(compute), _utt(spec), seed)[0]


@pytest.mark.parametrize("mode", ["isolate", "ragged"])
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_every_utterance_has_the_noise_of_its_own_seed(compute, mode):
    _need_gpu()
    batch = _sample(_model(compute), _stack([_utt(s) for s in SPECS]), list(SEEDS), **{mode: True})
    assert torch.isfinite(batch).all()
    for i, s in enumerate(SPECS):
        assert torch.equal(batch[i, : s[0]], _single(compute, s, SEEDS[i])), (compute, mode, i)
    # the seed matters: utterance 1 with utterance 0's seed is another result
    assert not torch.equal(batch[1, :129], _single(compute, SPECS[1], SEEDS[0]))
