"""The request batcher (`f5_tts_amd.serve.BatchingSynthesizer`) on the GPU: a request's wave is bit for bit the wave
of its own single run, whatever travels with it.

The recipe of `test_gpu_ragged_sample.py::test_infer_batch_ragged_waveforms_equal_isolated`: `DiT_tiny` (and
`UNetT_tiny`) with `text_num_embeds=256`, a byte vocab, synthetic Vocos weights, NFE 4 or 6, prompts of 6000-12000
samples, totals of about 50-130 frames. The expected value of a request is `infer_batch` of that one item with
`isolate=True` (one utterance: the plain call), its seed and speed as per-item settings and its group's sampler
settings; on a 16-bit DiT the LayerNorm fold is off while the expected values are computed and only then (the plain
call folds by default, a batch never does, and the fold is not bitwise the separate launches). The synthesizer always
runs under the engine's default settings.

The own-run test also decides the noise question: the synthesizer draws each request's noise from a private
`torch.Generator` seeded with the request's seed, `infer_batch` from the global generator after
`torch.manual_seed(seed)`; the waves are equal only if the two draw the same bits."""

import functools
import threading

import numpy as np
import pytest
import torch

from f5_tts_amd import configs, infer, serve, synthetic
from f5_tts_amd.model import CFM, DiT, UNetT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GROUPS = {"a": dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0),
          "b": dict(nfe_step=6, cfg_strength=1.5, sway_sampling_coef=-1.0)}
# (samples, sample rate, amplitude, ref_text, gen_text, group, speed)
SPEC = (
    (9000, 24000, 0.3, "Some call me nature.", "Others call me mother nature.", "a", 1.0),
    (6000, 16000, 0.3, "A short one.", "Hi there, friend.", "b", 1.0),  # resampled to 24 kHz
    (12000, 24000, 0.02, "The longest reference of them, by far.", "A rather longer sentence to say.", "a", 1.0),  # quiet
    (7000, 24000, 0.3, "Number four.", "The fourth utterance is here.", "b", 1.5),  # its own speed
    (6000, 24000, 0.3, "Five.", "Short.", "a", 1.0),
    (8000, 24000, 0.02, "Six is quiet too.", "And it has a longer text to go with it.", "b", 1.0),  # quiet
)
# the graph-reuse rounds: requests (samples, gen_text) on one ref_text, one settings group
GRAPH_REF = "One reference text."
GRAPH_SPEC = ((6000, "Twenty characters it is here."), (7000, "And some thirty characters of text."),
              (8000, "This one has the most text of all the seven."), (6500, "A few words to say."),
              (7500, "The last but one of the requests, long."), (6200, "Words."), (7800, "Some more words for this one."))
GRAPH_ROUNDS = ((0, 1), (2,), (3, 4, 5))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _requests():
    g = torch.Generator().manual_seed(5)
    return [dict(item=((torch.randn(1, n, generator=g) * amp, sr), ref, gen), group=grp, speed=spd, seed=20 + k)
            for k, (n, sr, amp, ref, gen, grp, spd) in enumerate(SPEC)]


def _graph_requests():
    g = torch.Generator().manual_seed(6)
    return [dict(item=((torch.randn(1, n, generator=g) * 0.3, 24000), GRAPH_REF, gen), group="a", speed=1.0,
                 seed=70 + k) for k, (n, gen) in enumerate(GRAPH_SPEC)]


REQS = _requests()


def _shape(reqs):
    """(B, R, Lmax, nt) of the requests as one call's live utterances, from the host intake alone."""
    dur, ntok = [], []
    for r in reqs:
        it = infer.prepare_item(infer.prepare_prompt(*r["item"][:2]), r["item"][2], r["speed"])
        ntok.append(len(it["text"]))
        dur.append(min(max(max(ntok[-1], it["ref"]) + 1, it["total"]), 65536))
    return len(reqs), sum(dur), max(dur), max(ntok)


def _build(cls, preset, compute):
    arch = configs.get_arch(preset, text_num_embeds=256)
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = cls(**kw, text_num_embeds=256, mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    return CFM(transformer=net, num_channels=100, compute=compute,
               vocab_char_map={chr(i): i for i in range(256)}).to(DEV)


@functools.lru_cache(maxsize=None)
def _model(kind, compute):
    return _build(*{"dit": (DiT, "DiT_tiny"), "unett": (UNetT, "UNetT_tiny")}[kind], compute)


@functools.lru_cache(maxsize=None)
def _vocoder():
    from f5_tts_amd.vocos import Vocos, make_weights

    voc = Vocos(compute="fp32")
    voc.load_state_dict(make_weights())
    return voc.to(DEV).eval()


def _engine(m, compute):
    return m.transformer.get_engine(compute, m.device)


def _own_run(m, r):
    return infer.infer_batch([r["item"] + ({"seed": r["seed"], "speed": r["speed"]},)], m, _vocoder(), isolate=True,
                             **GROUPS[r["group"]])[0][0]


@functools.lru_cache(maxsize=None)
def _expected(kind, compute):
    """Every request's own single run, computed once; the fold is off for these calls only (16-bit DiT)."""
    m = _model(kind, compute)
    fold_off = compute != "fp32"
    if fold_off:
        _engine(m, compute).set_ln_fold(False)
    try:
        waves = tuple(_own_run(m, r) for r in REQS)
        torch.cuda.synchronize()
    finally:
        if fold_off:
            _engine(m, compute).set_ln_fold(True)  # the engine's default
    return waves


def _submit(s, r):
    return s.submit(*r["item"], speed=r["speed"], seed=r["seed"], **GROUPS[r["group"]])


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_each_request_equals_its_own_run(compute):
    _need_gpu()
    m, exp = _model("dit", compute), _expected("dit", compute)
    with serve.BatchingSynthesizer(m, _vocoder()) as s:
        with s.hold():
            futs = [_submit(s, r) for r in REQS]
        got = [f.result(timeout=120) for f in futs]
        st = s.stats()
    assert st["calls"] == 2 and [c["live"][0] for c in st["calls_detail"]] == [3, 3]  # the two settings groups
    for k, (w, sr) in enumerate(got):
        assert sr == 24000 and w.dtype == np.float32 and w.ndim == 1 and np.isfinite(w).all() and np.abs(w).max() > 0
        assert w.shape == exp[k].shape and np.array_equal(w, exp[k]), (compute, k)
    assert not np.array_equal(got[0][0][:1000], got[4][0][:1000])


def test_traffic_does_not_change_a_request_under_default_engine_settings():
    """bf16, the fold left on: a request served alone and the same request served with company get the same bits.
    A lone request sent as a one-utterance call would take the plain path, which folds, and differ."""
    _need_gpu()
    m = _model("dit", "bf16")
    x, others = REQS[0], [REQS[2], REQS[4], dict(REQS[2], seed=99)]  # its settings group
    with serve.BatchingSynthesizer(m, _vocoder()) as s:
        alone = _submit(s, x).result(timeout=120)[0]
        assert s.stats()["calls_detail"][0]["live"][0] == 1
        with s.hold():
            futs = [_submit(s, r) for r in others[:2]] + [_submit(s, x), _submit(s, others[2])]
        crowd = futs[2].result(timeout=120)[0]
        assert s.stats()["calls_detail"][1]["live"][0] == 4
    assert np.isfinite(alone).all() and np.array_equal(alone, crowd)
    assert np.array_equal(alone, _expected("dit", "bf16")[0])
    # the trap is there at this shape: the plain one-utterance call under the same default settings folds and differs
    # (measured: 8e-3 of the wave's peak), so a lone request sent down that path would not have passed the lines above
    assert not np.array_equal(_own_run(m, x), alone)


def test_unett_requests_equal_their_own_runs():
    _need_gpu()
    m, exp = _model("unett", "fp32"), _expected("unett", "fp32")
    with serve.BatchingSynthesizer(m, _vocoder()) as s:
        with s.hold():
            futs = {k: _submit(s, REQS[k]) for k in (0, 2, 4)}
        got = {k: f.result(timeout=120)[0] for k, f in futs.items()}
        (call,) = s.stats()["calls_detail"]
    assert call["live"][0] == 3 and call["cap"][0] == 4
    for k, w in got.items():
        assert np.isfinite(w).all() and np.array_equal(w, exp[k]), k


def test_bucketed_rounds_replay_one_step_graph():
    """Three held rounds of different requests whose capacities agree: one step graph captured in round one, none
    after; with row_bucket=1 (no bucketing) every round captures its own."""
    _need_gpu()
    reqs = _graph_requests()
    rounds = [[reqs[k] for k in rd] for rd in GRAPH_ROUNDS]
    shapes = [_shape(rd) for rd in rounds]
    caps = [serve.capacity(b + 1, r + 1, l, nt, 256) for b, r, l, nt in shapes]
    assert caps[0] == caps[1] == caps[2] and len({sh[1] for sh in shapes}) == 3, (shapes, caps)
    raw = [serve.capacity(b + 1, r + 1, l, nt, 1) for b, r, l, nt in shapes]
    assert len({c[:3] for c in raw}) == 3, raw
    m = _build(DiT, "DiT_tiny", "bf16")  # an engine of its own: nothing captured yet
    eng = _engine(m, "bf16")
    waves = {}
    for rb, want in ((256, [1, 0, 0]), (1, [1, 1, 1])):
        with serve.BatchingSynthesizer(m, _vocoder(), row_bucket=rb) as s:
            for i, rd in enumerate(rounds):
                before = eng.graph_stats()["captures"]
                with s.hold():
                    futs = [_submit(s, r) for r in rd]
                waves[rb, i] = [f.result(timeout=120)[0] for f in futs]
                assert eng.graph_stats()["captures"] - before == want[i], (rb, i)
            st = s.stats()
            assert st["calls"] == 3 and st["graph_captures"] == eng.graph_stats()["captures"]
            assert [c["cap"] for c in st["calls_detail"]] == (caps if rb == 256 else raw)
    for i in range(3):  # and the bucket does not enter the result
        for a, b in zip(waves[256, i], waves[1, i]):
            assert np.isfinite(a).all() and np.array_equal(a, b)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_ragged_lmax_does_not_change_the_result(compute):
    _need_gpu()
    import test_gpu_ragged_sample as rs

    m = rs._model("dit", compute)
    inp = rs._stack([rs._utt(sp) for sp in rs.CASES["b3"]])
    base = rs._sample(m, inp, ragged=True)
    wide = rs._sample(m, inp, ragged=True, ragged_lmax=192)
    assert torch.isfinite(base).all() and torch.equal(base, wide)
    with pytest.raises(ValueError, match="ragged_lmax"):
        rs._sample(m, inp, ragged=True, ragged_lmax=149)


def test_concurrent_submitters():
    """12 requests from 4 threads, no hold: all resolve, each equals its own run, and the counters add up."""
    _need_gpu()
    m, exp = _model("dit", "fp32"), _expected("dit", "fp32")
    got, errs = {}, []
    with serve.BatchingSynthesizer(m, _vocoder(), max_wait_ms=2.0) as s:
        def worker(t):
            try:
                for j in range(3):
                    k = (t + 2 * j) % len(REQS)
                    got[t, j] = (k, _submit(s, REQS[k]))
            except BaseException as e:  # pragma: no cover
                errs.append(e)

        th = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs and len(got) == 12
        res = {key: (k, f.result(timeout=120)[0]) for key, (k, f) in got.items()}
        st = s.stats()
    for key, (k, w) in res.items():
        assert np.array_equal(w, exp[k]), (key, k)
    assert st["requests"] == 12 and st["queued"] == 0 and st["inflight"] == 0 and st["failed_calls"] == 0
    assert st["calls"] == len(st["calls_detail"]) and sum(c["live"][0] for c in st["calls_detail"]) == 12
    assert st["rows_live"] == sum(c["live"][1] for c in st["calls_detail"])
    assert st["rows_filler"] == sum(c["cap"][1] - c["live"][1] for c in st["calls_detail"])
    for c in st["calls_detail"]:
        assert c["cap"] == serve.capacity(c["live"][0] + 1, c["live"][1] + 1, c["live"][2], c["live"][3], 256)
        assert 1 <= c["cap"][0] - c["live"][0] and c["cap"][1] - c["live"][1] <= 256 + c["cap"][0]
