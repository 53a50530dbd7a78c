"""Ragged batches to waveforms, the host side (no GPU): the C-ABI boundary of the ragged entry points, the
argument checks of `Vocos.decode_ragged` / `MelSpec.forward_ragged` (they run before any device work), and the
orchestration of `infer.infer_batch` and `parallel.run_sharded(vocoder=...)` with pure-torch stand-ins
(tests/ragged_fakes.py), each utterance checked against its single-utterance result."""

import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ragged_fakes as rf
from f5_tts_amd import infer, parallel
from test_parallel import _expected, _fake_sample, _free_port, _job

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ("f5h_vocos_ragged_workspace_size", "f5h_vocos_decode_ragged", "f5h_mel_ragged_workspace_size",
          "f5h_mel_forward_ragged")


# ---------------------------------------------------------------- C ABI
def test_library_has_the_ragged_entry_points():
    from f5_tts_amd import _lib

    assert _lib.has_ragged()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "f5h.h")).read(), flags=re.S)
    for name in RAGGED:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)


def test_c_abi_refuses_null_objects_before_any_device_work():
    """The size functions answer 0 and the calls F5H_EINVAL for a null object (nothing is dereferenced)."""
    from f5_tts_amd import _lib

    L = _lib.lib()
    assert L.f5h_vocos_ragged_workspace_size(None, 2, 10) == 0
    assert L.f5h_mel_ragged_workspace_size(None, 2, 10) == 0
    assert L.f5h_vocos_decode_ragged(None, None, 1, None, 0, 0, 0, None, None, None, None, 0) == -1
    assert L.f5h_mel_forward_ragged(None, None, 1, None, 0, None, 1, None, None, 0) == -1


# ---------------------------------------------------------------- argument checks (before any device work)
def _voc():
    from f5_tts_amd.vocos import Vocos

    return Vocos()


@pytest.mark.parametrize("starts,lens,msg", [
    ([0, 0], [5, 5, 5], "entries for 3"),          # count mismatch
    ([0, 0, 0, 0], [5, 5, 5], "entries for 3"),
    ([0, 0, 0], [5, 0, 5], "utterance 1: length 0"),
    ([0, 0, 0], [5, 5, -2], "utterance 2: length -2"),
    ([0, 36, 0], [5, 5, 5], "utterance 1: frames \\[36, 41\\)"),  # start + len beyond the 40 frames
    ([0, -1, 0], [5, 5, 5], "utterance 1"),
    ([0, 0, 0], torch.empty(3, dtype=torch.int32, device="meta"), "host values"),  # device-resident lengths
    (torch.empty(3, dtype=torch.int64, device="meta"), [5, 5, 5], "host values"),
])
def test_decode_ragged_argument_checks(starts, lens, msg):
    with pytest.raises(ValueError, match=msg):
        _voc().decode_ragged(torch.zeros(3, 40, 100), starts, lens)


def test_decode_ragged_checks_follow_the_layout():
    v = _voc()
    with pytest.raises(ValueError, match="mel channels"):
        v.decode_ragged(torch.zeros(3, 100, 40), 0, 5)  # channel-first data declared channel-last
    with pytest.raises(ValueError, match=r"frames \[36, 41\)"):
        v.decode_ragged(torch.zeros(3, 100, 40), 36, 5, channels_last=False)
    # valid arguments get past the checks and stop at the missing weights (no device was touched)
    with pytest.raises(RuntimeError, match="load_state_dict"):
        v.decode_ragged(torch.zeros(3, 100, 40), [0, 35, 3], [40, 5, 1], channels_last=False)


def test_forward_ragged_argument_checks():
    from f5_tts_amd.mel import MelSpec

    m = MelSpec()
    w = torch.zeros(3, 2000)
    with pytest.raises(ValueError, match="entries for 3"):
        m.forward_ragged(w, lens=[2000, 1000])
    with pytest.raises(ValueError, match="wave 1: 512 samples"):
        m.forward_ragged(w, lens=[2000, 512, 2000])  # L_i <= n_fft/2: no reflect padding
    with pytest.raises(ValueError, match="wave 0: 300 samples"):
        m.forward_ragged([torch.zeros(300), torch.zeros(1, 900)])
    with pytest.raises(ValueError, match="wave 2: length 2001"):
        m.forward_ragged(w, lens=[2000, 1000, 2001])
    with pytest.raises(ValueError, match="host values"):
        m.forward_ragged(w, lens=torch.empty(3, dtype=torch.int64, device="meta"))
    with pytest.raises(ValueError, match="length 7 is shorter"):
        m.forward_ragged(w, lens=[2000, 1000, 600], length=7)  # 2000 samples are 8 frames
    with pytest.raises(ValueError, match="lens differ"):
        m.forward_ragged([torch.zeros(600), torch.zeros(900)], lens=[600, 800])
    # valid arguments get past the checks and stop at the device (the HIP front end has no CPU path)
    with pytest.raises(RuntimeError, match="GPU device"):
        m.forward_ragged(w, lens=[2000, 513, 600], length=8)


# ---------------------------------------------------------------- infer_batch
def _items():
    g = torch.Generator().manual_seed(9)
    amp = [0.5, 0.01, 0.5, 0.02, 0.5]           # items 1 and 3 are quieter than target_rms: boosted
    n = [9000, 7000, 12000, 5000, 8000]
    audio = [(torch.randn(2 if i == 2 else 1, n[i], generator=g) * amp[i], 24000) for i in range(5)]
    ref_text = ["Some call me nature.", "others call me mother", "Quiet caf\u00e9", "A b c?", "the prompt "]
    gen_text = ["I don't really care what you call me.", "short one", "A somewhat longer sentence to say, here.",
                "Hello there!", "x"]
    return list(zip(audio, ref_text, gen_text))


def _single(item, **kw):
    """The recipe of one utterance, written out (eval/utils_eval.py:109-148, eval_infer_batch.py:188-212)."""
    (audio, sr), ref_text, gen_text = item
    audio = audio.mean(0, keepdim=True) if audio.shape[0] > 1 else audio
    rms = torch.sqrt(torch.mean(torch.square(audio)))
    if rms < 0.1:
        audio = audio * 0.1 / rms
    if len(ref_text[-1].encode()) == 1:
        ref_text += " "
    ref = 1 + audio.shape[-1] // 256
    total = ref + int(ref / len(ref_text.encode()) * len(gen_text.encode()) / kw.get("speed", 1.0))
    model, voc = rf.FakeModel(), rf.FakeVocoder()
    cond, _ = model.mel_spec.forward_ragged([audio[0]])
    out, _ = model.sample(cond, infer.convert_char_to_pinyin([ref_text + gen_text]), torch.tensor([total]),
                          lens=torch.tensor([ref]), steps=8, cfg_strength=2.0, sway_sampling_coef=-1.0)
    wav = voc.decode_ragged(out, [ref], [total - ref])[0]
    if rms < 0.1:
        wav = wav * rms / 0.1
    return wav.numpy(), ref, total, "".join(infer.convert_char_to_pinyin([ref_text + gen_text])[0]), bool(rms < 0.1)


@pytest.mark.parametrize("speed", [1.0, 0.7])
def test_infer_batch_recipe_buckets_and_order(speed):
    items = _items()
    model, voc = rf.FakeModel(), rf.FakeVocoder()
    got = infer.infer_batch(items, model, voc, nfe_step=8, cfg_strength=2.0, sway_sampling_coef=-1.0, speed=speed,
                            seed=5, max_batch=2)
    want = [_single(it, speed=speed) for it in items]
    assert [w[4] for w in want] == [False, True, False, True, False]  # the RMS undo has both cases to show
    assert len(got) == 5
    for (wave, sr), (w, ref, total, _, _) in zip(got, want):  # input order, [ref:total] slices, RMS undo
        assert sr == 24000 and wave.dtype == w.dtype and wave.shape == ((total - ref - 1) * 256,)
        assert (wave == w).all()
    # duration formula and trailing-space rule as the sampler saw them; buckets of neighbours in total length
    order = sorted(range(5), key=lambda i: want[i][2])
    buckets = [order[0:2], order[2:4], order[4:5]]
    assert [c["duration"] for c in model.calls] == [[want[i][2] for i in b] for b in buckets]
    assert [c["lens"] for c in model.calls] == [[want[i][1] for i in b] for b in buckets]
    assert [c["text"] for c in model.calls] == [[want[i][3] for i in b] for b in buckets]
    raw = ["Some call me nature. I don't really care what you call me.", "others call me mother short one",
           "Quiet caf\u00e9A somewhat longer sentence to say, here.", "A b c? Hello there!", "the prompt  x"]
    assert [w[3] for w in want] == ["".join(infer.convert_char_to_pinyin([t])[0]) for t in raw]
    assert all(c["seed"] == 5 and c["steps"] == 8 for c in model.calls)
    assert voc.calls == [([want[i][1] for i in b], [want[i][2] - want[i][1] for i in b]) for b in buckets]
    assert model.mel_spec.calls == [[items[i][0][0].shape[-1] for i in b] for b in buckets]  # one intake per bucket


def test_infer_batch_refuses_an_item_with_nothing_to_generate():
    with pytest.raises(ValueError, match="item 1"):
        infer.infer_batch([_items()[0], (_items()[1][0], "a prompt", "")], rf.FakeModel(), rf.FakeVocoder(),
                          nfe_step=8, cfg_strength=2.0, sway_sampling_coef=-1.0)


# ---------------------------------------------------------------- run_sharded(vocoder=...)
def test_run_sharded_vocoder_world1_waves():
    utts = rf.job()
    voc = rf.FakeVocoder()
    got = parallel.run_sharded(utts, rf.sample_fn, rank=0, world=1, max_batch=3, vocoder=voc)
    assert sorted(got) == list(range(len(utts)))
    for i, u in enumerate(utts):
        assert got[i].shape == ((u["total"] - u["ref"] - 1) * rf.HOP,)
        assert torch.equal(got[i], rf.expected_wave(u))
    assert got[2].numel() == 0
    assert sum(len(c[1]) for c in voc.calls) == len(utts) and max(len(c[1]) for c in voc.calls) <= 3


def test_run_sharded_without_vocoder_is_unchanged():
    utts = _job(5)
    got = parallel.run_sharded(utts, _fake_sample, rank=0, world=1, max_batch=2, vocoder=None)
    assert sorted(got) == list(range(5))
    for i, u in enumerate(utts):
        assert got[i].shape == (u["total"] - u["ref"], 100) and torch.equal(got[i], _expected(u))


def _wave_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    utts = rf.job()
    voc = rf.FakeVocoder()
    got = parallel.run_sharded(utts, rf.sample_fn, rank=rank, world=world, max_batch=3, vocoder=voc)
    ok = sorted(got) == list(range(len(utts))) and all(torch.equal(got[i], rf.expected_wave(u))
                                                       for i, u in enumerate(utts))
    q.put((rank, ok, sum(len(c[1]) for c in voc.calls)))
    dist.barrier()
    dist.destroy_process_group()


def test_run_sharded_vocoder_world2_gloo_every_wave_on_every_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_wave_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _ in res), res
    assert sum(n for _, _, n in res) == len(rf.job())  # the two ranks decoded every utterance exactly once
    assert all(p.exitcode == 0 for p in procs)
