"""Ragged batches on the GPU: `Vocos.decode_ragged` and `MelSpec.forward_ragged` against the CPU oracles and,
bit for bit, against today's per-utterance path (`Vocos.decode`, `MelSpec.forward`), which is the invariant the
project already holds for equal-length batches (tests/test_vocos.py: fixed per-element reduction order in every
kernel); then `infer.infer_batch` end to end against the hand-assembled per-utterance pipeline.

Bounds (the issue's, which are the per-utterance tests' own): fp32 Vocos vs oracle max|diff| / max|ref| <= 1e-3
(test_vocos_fp32_matches_oracle); log-mel vs oracle linear max-rel <= 1e-4 and log max|diff| <= 2e-3 above 1e-3
(test_mel_hip_matches_oracle); everything else is exact equality.

Shapes: lens [29, 1, 70, 2, 3, 7, 131] put segments shorter than the +-3 tap reach between long ones, with the
segment edges (29, 30, 100, 102, 105, 112, 243) off the 4-row dwconv_ln blocks and off the 64- and 128-row GEMM
tiles; a 1-frame segment gives an empty wave."""

import ctypes

import numpy as np
import pytest
import torch

from oracle import mel_cpu, vocos_cpu
from test_mel import _wav
from test_vocos import _maxrel, _mel

DEV = "cuda:0"
LENS = [29, 1, 70, 2, 3, 7, 131]
STARTS = [0, 5, 3, 0, 11, 2, 1]
WAVE_LENS = [513, 768, 1000, 5000, 1300]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_VOC = {}


def _vocos(compute):
    from f5_tts_amd.vocos import Vocos, make_weights

    if compute not in _VOC:
        W = make_weights()
        v = Vocos(compute=compute)
        v.load_state_dict(W)
        _VOC[compute] = (v.to(DEV).eval(), W)
    return _VOC[compute]


def _src():
    """[7, 140, 100] channel-last (the sampler's output layout), values as test_vocos._mel"""
    return _mel(7, 140, seed=7140).permute(0, 2, 1).contiguous()


@pytest.fixture(scope="module")
def oracle_waves():
    """`vocos_cpu.decode` of every utterance's own slice, computed once (torch.istft refuses a single frame: that
    utterance's wave is empty by its length (T - 1) * hop)."""
    _gpu()
    from f5_tts_amd.vocos import make_weights

    W, src = make_weights(), _src()
    return [vocos_cpu.decode(W, vocos_cpu.VOCOS_MEL_24KHZ, src[i, s: s + n].T[None])[0] if n > 1 else torch.zeros(0)
            for i, (s, n) in enumerate(zip(STARTS, LENS))]


def _single(v, src, i):
    return v.decode(src[i, STARTS[i]: STARTS[i] + LENS[i]].T[None])[0]


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.gpu
def test_decode_ragged_fp32_matches_oracle(oracle_waves):
    _gpu()
    v, _ = _vocos("fp32")
    out = v.decode_ragged(_src().to(DEV), STARTS, LENS)
    assert len(out) == 7
    for i, (o, ref) in enumerate(zip(out, oracle_waves)):
        assert o.shape == ref.shape == ((LENS[i] - 1) * 256,) and o.dtype == torch.float32
        if LENS[i] == 1:
            continue
        o = o.cpu()
        assert torch.isfinite(o).all()
        print(f"utterance {i} ({LENS[i]} frames): max-rel vs oracle {_maxrel(o, ref):.3e}")
        assert _maxrel(o, ref) <= 1e-3, (i, _maxrel(o, ref))


# ---------------------------------------------------------------- 2. bitwise against today's path
@pytest.mark.gpu
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_decode_ragged_equals_per_utterance_decode_bitwise(compute):
    _gpu()
    v, _ = _vocos(compute)
    src = _src().to(DEV)
    out = v.decode_ragged(src, STARTS, LENS)
    for i in range(7):
        assert torch.equal(out[i], _single(v, src, i)), (compute, i)
    # one packed buffer, utterance i at sum_{j<i} (len_j - 1) * hop
    assert out[0].data_ptr() + 4 * sum((n - 1) * 256 for n in LENS[:6]) == out[6].data_ptr()
    # the same bits from vocos' channel-first layout [B, 100, T], read through its own strides
    cf = src.permute(0, 2, 1).contiguous()
    for a, b in zip(out, v.decode_ragged(cf, STARTS, LENS, channels_last=False)):
        assert torch.equal(a, b)
    # a single segment of 256 rows is the equal-length decode
    mel = _mel(1, 256, seed=256).to(DEV)
    assert torch.equal(v.decode_ragged(mel, 0, 256, channels_last=False)[0], v.decode(mel)[0])


# ---------------------------------------------------------------- 3. nothing leaks across a boundary
@pytest.mark.gpu
def test_decode_ragged_never_reads_outside_the_segments():
    _gpu()
    v, _ = _vocos("bf16")
    keep = torch.zeros(7, 140, 1, dtype=torch.bool)
    for i, (s, n) in enumerate(zip(STARTS, LENS)):
        keep[i, s: s + n] = True
    outs = []
    for fill in (float("nan"), 1e30, 0.0):
        src = torch.where(keep, _src(), torch.tensor(fill)).to(DEV)
        outs.append(torch.cat(v.decode_ragged(src, STARTS, LENS)))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0], torch.cat(v.decode_ragged(_src().to(DEV), STARTS, LENS)))


# ---------------------------------------------------------------- 4. replays and staging (the C ABI itself)
@pytest.mark.gpu
def test_decode_ragged_calls_queue_without_sync_and_own_their_staging():
    """Shape A, shape B (another batch size and other lengths), A again, enqueued back to back through the C
    entry point with the host `starts` / `lens` arrays overwritten the moment each call returns: the library has
    consumed them by then, so the third result equals the first bit for bit (and the per-utterance decodes)."""
    _gpu()
    from f5_tts_amd import _lib

    v, _ = _vocos("bf16")
    L, h = _lib.lib(), v._engine()
    src = _src().to(DEV)
    shape_a = (7, STARTS, LENS)
    shape_b = (3, [4, 0, 9], [50, 9, 33])
    need = max(int(L.f5h_vocos_ragged_workspace_size(h, B, sum(n))) for B, _, n in (shape_a, shape_b))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = _lib.stream_handle(torch.device(DEV))
    i32p = ctypes.POINTER(ctypes.c_int32)
    outs = []
    for B, starts, lens in (shape_a, shape_b, shape_a):
        st, ln = np.array(starts, np.int32), np.array(lens, np.int32)
        audio = torch.empty((sum(lens) - B) * 256, dtype=torch.float32, device=DEV)
        rc = L.f5h_vocos_decode_ragged(h, stream, B, src.data_ptr(), *src.stride(), st.ctypes.data_as(i32p),
                                       ln.ctypes.data_as(i32p), audio.data_ptr(), ws.data_ptr(), ws.numel())
        st[:] = 100  # would read past every row of the source
        ln[:] = 1
        assert rc == 0, L.f5h_last_error()
        outs.append(audio)
    assert torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0], torch.cat([_single(v, src, i) for i in range(7)]))
    assert torch.equal(outs[1], torch.cat([v.decode(src[i, s: s + n].T[None])[0]
                                           for i, (s, n) in enumerate(zip(*shape_b[1:]))]))


@pytest.mark.gpu
def test_c_abi_names_the_offending_row():
    _gpu()
    from f5_tts_amd import _lib

    v, _ = _vocos("bf16")
    L, h = _lib.lib(), v._engine()
    buf = torch.zeros(4096, device=DEV)
    i32 = ctypes.c_int32 * 3
    args = (buf.data_ptr(), buf.data_ptr(), 4096 * 4)
    assert L.f5h_vocos_decode_ragged(h, None, 3, buf.data_ptr(), 0, 100, 1, i32(0, 0, 0), i32(2, 0, 2), *args) == -1
    assert b"row 1" in L.f5h_last_error()
    assert L.f5h_vocos_decode_ragged(h, None, 3, buf.data_ptr(), 0, 100, 1, i32(0, 0, -4), i32(2, 2, 2), *args) == -1
    assert b"row 2" in L.f5h_last_error() and b"negative start" in L.f5h_last_error()
    assert L.f5h_vocos_decode_ragged(h, None, 3, buf.data_ptr(), 0, 100, 1, i32(0, 0, 0), i32(2, 1 << 24, 2),
                                     *args) == -1
    assert b"2^24" in L.f5h_last_error() and b"row 1" in L.f5h_last_error()
    from f5_tts_amd.mel import MelSpec

    m = MelSpec()
    mh = m._engine(torch.device(DEV))
    assert L.f5h_mel_forward_ragged(mh, None, 3, buf.data_ptr(), 1000, i32(600, 512, 600), 8, *args) == -1
    assert b"wave 1" in L.f5h_last_error() and b"n_fft/2" in L.f5h_last_error()
    assert L.f5h_mel_forward_ragged(mh, None, 3, buf.data_ptr(), 1000, i32(600, 600, 1000), 3, *args) == -1
    assert b"wave 2" in L.f5h_last_error() and b"T_out" in L.f5h_last_error()


# ---------------------------------------------------------------- 5. log-mel
@pytest.mark.gpu
def test_forward_ragged_equals_per_wave_mel_and_matches_oracle():
    _gpu()
    from f5_tts_amd.mel import MelSpec

    m = MelSpec()
    waves = [_wav(1, n, seed=n)[0] for n in WAVE_LENS]
    cond, frames = m.forward_ragged([w.to(DEV) for w in waves])
    assert frames == [1 + n // 256 for n in WAVE_LENS] and cond.shape == (5, max(frames), 100)
    for i, w in enumerate(waves):
        T = frames[i]
        assert torch.equal(cond[i, :T], m(w[None].to(DEV))[0].T), i
        assert (cond[i, T:] == 0).all()
        out, ref = cond[i, :T].T.cpu(), mel_cpu.log_mel(w[None])[0]
        lin_err = float((out.exp() - ref.exp()).abs().max() / ref.exp().abs().max())
        log_err = float((out - ref)[ref > np.log(1e-3)].abs().max())
        print(f"wave {i} ({WAVE_LENS[i]} samples): linear max-rel {lin_err:.3e}, log max-abs {log_err:.3e}")
        assert lin_err <= 1e-4, (i, lin_err)
        assert log_err <= 2e-3, (i, log_err)
    # the padded-input form: what lies beyond lens[i] is never read, and `length` pads with exact zeros
    padded = torch.full((5, max(WAVE_LENS) + 7), float("nan"))
    for i, w in enumerate(waves):
        padded[i, : WAVE_LENS[i]] = w
    cond2, frames2 = m.forward_ragged(padded.to(DEV), lens=torch.tensor(WAVE_LENS), length=max(frames) + 3)
    assert frames2 == frames and cond2.shape == (5, max(frames) + 3, 100)
    assert torch.equal(cond2[:, : max(frames)], cond) and (cond2[:, max(frames):] == 0).all()


# ---------------------------------------------------------------- 6. end to end
@pytest.mark.gpu
def test_infer_batch_equals_the_hand_assembled_pipeline_bitwise():
    _gpu()
    from f5_tts_amd import configs, infer, parallel, synthetic
    from f5_tts_amd.model import CFM, DiT

    arch = configs.get_arch("DiT_tiny", text_num_embeds=256)
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=256, mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    model = CFM(transformer=net, num_channels=100, compute="bf16",
                vocab_char_map={chr(i): i for i in range(256)}).to(DEV)
    voc, _ = _vocos("bf16")
    audio = [_wav(1, n, seed=n) * a for n, a in ((9000, 1.0), (14000, 0.1), (6000, 1.0))]  # the second is boosted
    items = [((audio[0], 24000), "Some call me nature.", "Others call me mother nature."),
             ((audio[1], 24000), "a quiet prompt", "and a rather longer sentence to generate, here"),
             ((audio[2], 24000), "Short?", "Yes.")]
    opts = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    got = infer.infer_batch(items, model, voc, **opts)
    again = infer.infer_batch(items, model, voc, **opts)

    # by hand: per-utterance MelSpec, padded_mel_batch, the same batched sample, per-utterance decode, RMS undo
    rms, text, ref, total = [], [], [], []
    for (a, _), rt, gt in items:
        r = torch.sqrt(torch.mean(torch.square(a)))
        rms.append(r)
        if len(rt[-1].encode()) == 1:
            rt += " "
        text.append(infer.convert_char_to_pinyin([rt + gt])[0])
        ref.append(1 + a.shape[-1] // 256)
        total.append(ref[-1] + int(ref[-1] / len(rt.encode()) * len(gt.encode()) / 1.0))
    assert [bool(r < 0.1) for r in rms] == [False, True, False]
    order = parallel.bucket(range(3), total, 32)[0]
    mels = []
    for i in order:
        a = audio[i] * 0.1 / rms[i] if rms[i] < 0.1 else audio[i]
        mels.append(model.mel_spec(a.to(DEV))[0].T)
        assert mels[-1].shape[0] == ref[i]
    out, _ = model.sample(cond=parallel.padded_mel_batch(mels), text=[text[i] for i in order],
                          duration=torch.tensor([total[i] for i in order]), lens=torch.tensor([ref[i] for i in order]),
                          steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    for j, i in enumerate(order):
        wav = voc.decode(out[j, ref[i]: total[i]].to(torch.float32).T[None])[0]
        if rms[i] < 0.1:
            wav = wav * rms[i] / 0.1
        wav = wav.cpu().numpy()
        assert got[i][1] == 24000 and got[i][0].shape == wav.shape == ((total[i] - ref[i] - 1) * 256,)
        assert np.isfinite(wav).all() and np.array_equal(got[i][0], wav), i
        assert np.array_equal(got[i][0], again[i][0]), i
