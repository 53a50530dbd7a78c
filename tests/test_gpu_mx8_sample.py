"""compute="mxfp8" end to end on the GPU: CFM.sample on the reference's fp32 fixtures, the launch count, the error
against the bf16 engine's, the ragged / isolate / single-call identity and the identity of mask 0 with compute="bf16".

Error bound (rel-L2 over the generated frames against the reference's fp32 output, the metric of
tests/test_gpu_envelope.py): the mode must lose precision against bf16 (its GEMM operands carry 3 mantissa bits
instead of 7), and by no more than 16 x 1.5 x the bf16 engine's error in the same test: 16 = the ratio of the unit
roundoffs 2^-4 / 2^-8, 1.5 = the envelope test's margin. MEASURED holds each case's value on MI355X (the kernels are
deterministic); a case must stay within its value + 25 %."""

import functools

import numpy as np
import pytest
import torch

import golden_cases as gc
from f5_tts_amd import synthetic
from f5_tts_amd.model import CFM, DiT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROUNDOFF_RATIO, MARGIN = 16.0, 1.5
CASES = ["dit_tiny_sample_b1", "dit_tiny_sample_b3", "dit_tiny_sample_b3_masked", "c1_sample_fp32"]
# case -> (mxfp8 error, bf16 engine error) as measured on MI355X, all four classes on MX8 operands
MEASURED = {
    "dit_tiny_sample_b1": (0.0194021, 0.00618248),
    "dit_tiny_sample_b3": (0.0230245, 0.00729594),
    "dit_tiny_sample_b3_masked": (0.0227291, 0.00725535),
    "c1_sample_fp32": (0.0404928, 0.00801705),
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(arch, compute):
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    return CFM(transformer=net, num_channels=100, compute=compute).to(DEV)


def _gen_frames(x, lens, dur):
    return np.concatenate([x[i, int(lens[i]):int(dur[i])] for i in range(x.shape[0])], axis=0)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    tag, spec, nfe, sway, cfg = gc.SAMPLE_CASES[case]
    inp = synthetic.make_case(**spec)
    dur = torch.maximum(torch.maximum((inp["text"] != -1).sum(-1), inp["lens"]) + 1, inp["duration"])
    return inp, dur, synthetic.reference_noise(dur, gc.SEED)


def _sample(case, compute, mask=None):
    """(out [B,N,100] fp32 numpy, MX8 GEMM launches the call ran, the model's depth, nfe)."""
    tag, spec, nfe, sway, cfg = gc.SAMPLE_CASES[case]
    arch = gc.arch_of(tag)
    m = _model(arch, compute)
    eng = m.transformer.get_engine(compute, m.device)
    if mask is not None:
        eng.set_mx8_classes(mask)
    inp, dur, y0 = _inputs(case)
    torch.cuda.synchronize()
    n0 = eng.mx8_stats()[1] if compute == "mxfp8" else 0
    out, _ = m.sample(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=inp["duration"].to(DEV),
                      lens=inp["lens"].to(DEV), steps=nfe, cfg_strength=cfg, sway_sampling_coef=sway, y0=y0.to(DEV),
                      keep_trajectory=False)
    torch.cuda.synchronize()
    n1 = eng.mx8_stats()[1] if compute == "mxfp8" else 0
    return out.float().cpu().numpy(), n1 - n0, arch["depth"], nfe


def _err(case, out):
    f32 = gc.load(case)
    assert f32 is not None, case
    inp, dur, _ = _inputs(case)
    assert out.shape == f32["out"].shape
    ref = _gen_frames(f32["out"], inp["lens"], dur)
    return gc.rel_err(_gen_frames(out, inp["lens"], dur), ref)


@pytest.mark.parametrize("case", CASES)
def test_sample_error_and_launch_count(case):
    _need_gpu()
    out, launches, depth, nfe = _sample(case, "mxfp8")
    assert np.isfinite(out).all()
    assert launches == 4 * depth * nfe, (launches, depth, nfe)
    e_mx = _err(case, out)
    e_bf = _err(case, _sample(case, "bf16")[0])
    print(f"mx8 {case}: e_mxfp8={e_mx:.6g} e_bf16={e_bf:.6g} ratio={e_mx / e_bf:.3f}")
    assert e_mx > e_bf, (e_mx, e_bf)
    assert e_mx <= ROUNDOFF_RATIO * MARGIN * e_bf, (e_mx, e_bf)
    measured = MEASURED.get(case)
    assert measured is not None, f"record the measured e_mxfp8={e_mx:.6g}, e_bf16={e_bf:.6g} of {case} in MEASURED"
    assert e_mx <= 1.25 * measured[0], (e_mx, measured)


@pytest.mark.parametrize("case", ["dit_tiny_sample_b1", "dit_tiny_sample_b3_masked"])
def test_mask_0_is_the_bf16_mode_bit_for_bit(case):
    _need_gpu()
    out, launches, _, _ = _sample(case, "mxfp8", mask=0)
    assert launches == 0
    assert np.array_equal(out, _sample(case, "bf16")[0])


@pytest.mark.parametrize("mask, per_layer", [(1, 1), (4 | 16, 2), (8, 1)])
def test_class_mask_selects_the_launches(mask, per_layer):
    _need_gpu()
    out, launches, depth, nfe = _sample("dit_tiny_sample_b1", "mxfp8", mask=mask)
    assert np.isfinite(out).all()
    assert launches == per_layer * depth * nfe


# ---------------------------------------------------------------- ragged == isolate == single calls
NFE, SEED, CFG, SWAY = 4, 7, 2.0, -1.0
SPECS = ((90, 40, 20), (150, 60, 30), (70, 25, 12))  # (total frames, prompt frames, text tokens)


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


def _run(m, inp, **kw):
    out, _ = m.sample(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=inp["duration"], lens=inp["lens"],
                      steps=NFE, cfg_strength=CFG, sway_sampling_coef=SWAY, seed=SEED, keep_trajectory=False, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


def test_ragged_batch_equals_isolated_batch_and_single_calls():
    """The MX8 GEMM has one tile configuration and a fixed K order, and the quantisers work on one row's blocks: an
    utterance has the bits of its own B = 1 call in the ragged batch and in the isolated padded batch."""
    _need_gpu()
    m = _model(gc.arch_of("tiny"), "mxfp8")
    eng = m.transformer.get_engine("mxfp8", m.device)
    singles = [_run(m, _utt(s))[0] for s in SPECS]
    batch = _stack([_utt(s) for s in SPECS])
    n0 = eng.mx8_stats()[1]
    rag = _run(m, batch, ragged=True)
    assert eng.mx8_stats()[1] - n0 == 4 * 2 * NFE
    iso = _run(m, batch, isolate=True)
    assert torch.isfinite(rag).all()
    for i, s in enumerate(SPECS):
        assert torch.equal(rag[i, : s[0]], singles[i]), i
        assert torch.equal(iso[i, : s[0]], singles[i]), i
        assert not rag[i, s[0]:].any()
