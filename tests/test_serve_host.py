"""The request batcher (`f5_tts_amd.serve.BatchingSynthesizer`) on the host side, no GPU: the dispatch policy, the
capacities and fillers, the invariance of every result against its own single run, errors, shutdown, threads and
the `ragged_lmax` passthrough of `CFM.sample`. The model below makes each utterance a function of its own inputs
(prompt frames, text ids, noise, settings), so `infer_batch` of one item is the expected value of any traffic."""

from __future__ import annotations

import threading
import time

import numpy as np
import pytest
import torch

import golden_cases as gc
import ragged_fakes as rf
from f5_tts_amd import configs, infer, serve, synthetic
from f5_tts_amd.model import CFM, DiT

SETTINGS = {"a": dict(nfe_step=4, cfg_strength=2.0), "b": dict(nfe_step=6, cfg_strength=1.5),
            "c": dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=None)}


class Model:
    """`model_obj` stand-in taking what both `infer_batch` (text lists, `seed=`) and the synthesizer (padded ids,
    `y0=`) send. Utterance b's frames depend on its own prompt, ids, noise and the settings only."""

    device = torch.device("cpu")
    num_channels = 100
    vocab_char_map = {chr(i): i for i in range(256)}

    def __init__(self, route="ragged", fail_steps=None):
        self.mel_spec = rf.FakeMel()
        self.serve_route = route
        self.fail_steps = fail_steps
        self.calls = []

    def sample(self, cond, text, duration, *, lens, steps, cfg_strength, sway_sampling_coef, seed=None, y0=None,
               keep_trajectory=True, isolate=False, ragged=False, ragged_lmax=None):
        assert duration.device.type == "cpu" and lens.device.type == "cpu"  # host lengths: no hidden sync
        if steps == self.fail_steps:
            raise RuntimeError("this batch fails")
        B = cond.shape[0]
        if isinstance(text, list):
            ids = [torch.tensor([self.vocab_char_map.get(c, 0) for c in t]) for t in text]
            nt = max(len(i) for i in ids)
        else:
            ids, nt = [row[row >= 0] for row in text], text.shape[1]
        dur = [min(max(max(len(i), int(l)) + 1, int(d)), 65536) for i, l, d in zip(ids, lens, duration)]
        if y0 is None:
            seeds = seed if isinstance(seed, (list, tuple)) else [seed] * B
            y0 = torch.zeros(B, max(dur), 100)
            for b in range(B):
                torch.manual_seed(seeds[b])
                y0[b, : dur[b]] = torch.randn(dur[b], 100)
        self.calls.append(dict(B=B, dur=dur, lens=[int(l) for l in lens], nt=nt, steps=steps, cfg=cfg_strength,
                               sway=sway_sampling_coef, isolate=isolate, ragged=ragged, lmax=ragged_lmax,
                               ntok=[len(i) for i in ids]))
        out = torch.zeros(B, max(dur), 100)
        for b in range(B):
            n, r = dur[b], int(lens[b])
            sig = (float(cond[b, :r].double().sum()) * 1e-3 + 0.01 * float(ids[b].sum()) + 1e-3 * steps
                   + 0.1 * cfg_strength + (0.0 if sway_sampling_coef is None else 0.05 * sway_sampling_coef))
            t = torch.arange(n, dtype=torch.float64)[:, None]
            out[b, :n] = torch.sin(0.013 * t * (torch.arange(100)[None] + 1) + sig).float() + 0.1 * y0[b, :n].float()
            out[b, n:] = 7.0  # what lies past an utterance's end must not reach its wave
        return out, None


def _requests():
    g = torch.Generator().manual_seed(9)
    spec = [(9000, 24000, 0.3, "Some call me nature.", "Others call me mother nature.", "a", 1.0),
            (4000, 16000, 0.3, "A short one.", "Hi there, friend.", "b", 1.0),  # resampled
            (12000, 24000, 0.01, "The longest reference of them, by far.", "A rather longer sentence to say.", "a", 1.0),
            (7000, 24000, 0.3, "Number four.", "The fourth utterance is here.", "c", 1.5),
            (6000, 24000, 0.3, "Five.", "Short.", "a", 1.0),
            (8000, 24000, 0.02, "Six is quiet too.", "And it has a longer text to go with it.", "b", 0.8),
            (10000, 24000, 0.3, "Seven here.", "Seventh of the lot, with its own words.", "a", 1.0)]
    return [dict(item=((torch.randn(1, n, generator=g) * amp, sr), ref, gen), group=grp, speed=spd, seed=40 + k)
            for k, (n, sr, amp, ref, gen, grp, spd) in enumerate(spec)]


REQS = _requests()


def _expected(k):
    r = REQS[k]
    return infer.infer_batch([r["item"] + ({"seed": r["seed"], "speed": r["speed"]},)], Model(), rf.FakeVocoder(),
                             isolate=True, **{"sway_sampling_coef": -1.0, **SETTINGS[r["group"]]})[0][0]


EXPECTED = [_expected(k) for k in range(len(REQS))]


def _dur(k):
    r = REQS[k]
    it = infer.prepare_item(infer.prepare_prompt(*r["item"][:2]), r["item"][2], r["speed"])
    return min(max(max(len(it["text"]), it["ref"]) + 1, it["total"]), 65536)


def _submit(s, k):
    r = REQS[k]
    return s.submit(*r["item"], speed=r["speed"], seed=r["seed"], **SETTINGS[r["group"]])


def _synth(model=None, **kw):
    model = model or Model()
    return serve.BatchingSynthesizer(model, rf.FakeVocoder(), **kw), model


def _wait_for(cond, seconds=5.0):
    end = time.monotonic() + seconds
    while not cond():
        assert time.monotonic() < end, "timed out"
        time.sleep(0.001)


# ------------------------------------------------------------------ capacity
def test_capacity_rounds_up_and_is_idempotent_and_monotone():
    rng = np.random.default_rng(0)
    for rb in (1, 64, 100, 256):
        for _ in range(300):
            B = int(rng.integers(1, 40))
            R = B + int(rng.integers(0, 3000))
            L, nt = int(rng.integers(1, 2000)), int(rng.integers(0, 300))
            c = serve.capacity(B, R, L, nt, rb)
            assert c[0] % 4 == 0 and c[1] % rb == 0 and c[2] % 64 == 0 and c[3] % 16 == 0
            assert c[0] >= B and c[1] >= R + (c[0] - B) and c[2] >= max(L, rb) and c[3] >= nt
            assert c[0] < B + 4 and c[1] < R + (c[0] - B) + rb and c[3] < max(nt, 1) + 16
            assert c[2] == max(-(-L // 64) * 64, -(-rb // 64) * 64)
            assert serve.capacity(*c, rb) == c  # idempotent
            # monotone: growing R, Lmax or nt never shrinks a capacity; growing B never shrinks B_cap, Lmax_cap, nt_cap
            for d in ((0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 7, 5, 3)):
                c2 = serve.capacity(B + d[0], R + d[1], L + d[2], nt + d[3], rb)
                assert all(x <= y for x, y in zip(c, c2)), (B, R, L, nt, rb, d)
            c3 = serve.capacity(B + 1, R + 1, L, nt, rb)
            assert c3[0] >= c[0] and c3[2] >= c[2] and c3[3] >= c[3]
    assert serve.capacity(2, 101, 90, 37, 256) == (4, 256, 256, 48)
    assert serve.capacity(2, 101, 90, 37, 1) == (4, 103, 128, 48)
    assert serve.capacity(5, 254, 64, 1, 256)[1] == 512 and serve.capacity(8, 254, 64, 1, 256)[1] == 256  # documented
    with pytest.raises(ValueError):
        serve.capacity(0, 10, 10, 1, 256)
    with pytest.raises(ValueError):
        serve.capacity(3, 2, 10, 1, 256)
    assert serve.filler_lengths(3, 11) == [4, 4, 3] and serve.filler_lengths(1, 5) == [5]


# ------------------------------------------------------------------ dispatch policy
def _live(model):
    """Per call: the requests it carried, as indices into REQS (matched by their token counts and durations)."""
    sig = {(len(infer.prepare_item(infer.prepare_prompt(*r["item"][:2]), r["item"][2], r["speed"])["text"]), _dur(k)): k
           for k, r in enumerate(REQS)}
    return [[sig[(n, d)] for n, d, l in zip(c["ntok"], c["dur"], c["lens"]) if l > 0] for c in model.calls]


def test_groups_are_served_oldest_first_fifo_within():
    s, m = _synth(max_batch=3)
    with s:
        with s.hold():
            futs = [_submit(s, k) for k in range(7)]  # groups: a b a c a b a
            time.sleep(0.003)
            assert not m.calls and s.stats()["queued"] == 7  # held: nothing starts
        for k, f in enumerate(futs):
            assert np.array_equal(f.result(timeout=10)[0], EXPECTED[k])
    # a: 0 2 4 | 6, b: 1 5, c: 3; heads by age after the first call: b (1), c (3), a (6)
    assert _live(m) == [[0, 2, 4], [1, 5], [3], [6]]
    assert [(c["steps"], c["cfg"], c["sway"]) for c in m.calls] == [(4, 2.0, -1.0), (6, 1.5, -1.0), (4, 2.0, None),
                                                                    (4, 2.0, -1.0)]
    st = s.stats()
    assert st["requests"] == 7 and st["calls"] == 4 and st["queued"] == 0 and st["inflight"] == 0


def test_max_rows_splits_a_group_and_an_oversize_request_goes_alone():
    order = [4, 0, 6, 2]  # group a
    d = {k: _dur(k) for k in order}
    limit = 140
    assert d[4] + d[0] <= limit < d[4] + d[0] + d[6] and d[6] > limit and d[2] <= limit
    s, m = _synth(max_batch=8, max_rows=limit)
    with s:
        with s.hold():
            futs = [_submit(s, k) for k in order]
        for k, f in zip(order, futs):
            assert np.array_equal(f.result(timeout=10)[0], EXPECTED[k])
    assert _live(m) == [[4, 0], [6], [2]]  # the split, then the oversize request alone, then the rest


def test_every_call_carries_filler_at_its_capacity():
    for rb, mb in ((256, 3), (64, 2), (1, 8)):
        s, m = _synth(max_batch=mb, row_bucket=rb)
        with s:
            with s.hold():
                futs = [_submit(s, k) for k in range(7)]
            [f.result(timeout=10) for f in futs]
        st = s.stats()
        assert len(st["calls_detail"]) == len(m.calls) == st["calls"]
        live_rows = filler_rows = 0
        for c, rec in zip(m.calls, st["calls_detail"]):
            n = sum(1 for l in c["lens"] if l > 0)
            live = (n, sum(c["dur"][:n]), max(c["dur"][:n]), max(c["ntok"][:n]))
            cap = serve.capacity(n + 1, live[1] + 1, live[2], live[3], rb)
            assert rec["live"] == live and rec["cap"] == cap
            # what the sampler saw is the capacity: B, R, the lmax handed through, the text width
            assert (c["B"], sum(c["dur"]), c["lmax"], c["nt"]) == cap and c["ragged"] and not c["isolate"]
            fill = c["dur"][n:]
            assert len(fill) >= 1 and all(1 <= f <= cap[2] for f in fill)
            assert all(l == 0 for l in c["lens"][n:]) and all(t == 0 for t in c["ntok"][n:])
            assert sum(fill) <= rb + cap[0]
            live_rows, filler_rows = live_rows + live[1], filler_rows + sum(fill)
        assert (st["rows_live"], st["rows_filler"]) == (live_rows, filler_rows)


def test_isolate_route_pads_to_the_capacity():
    s, m = _synth(Model(route="isolate"), max_batch=3)
    with s:
        with s.hold():
            futs = [_submit(s, k) for k in (0, 2, 4)]
        for k, f in zip((0, 2, 4), futs):
            assert np.array_equal(f.result(timeout=10)[0], EXPECTED[k])
    (c,) = m.calls
    live = (3, sum(c["dur"][:3]), max(c["dur"][:3]), max(c["ntok"][:3]))
    cap = serve.capacity(4, live[1] + 1, live[2], live[3], 1)
    assert c["isolate"] and not c["ragged"] and c["lmax"] is None
    assert (c["B"], max(c["dur"]), c["nt"]) == (cap[0], cap[2], cap[3])


@pytest.mark.parametrize("max_batch", [1, 2, 3, 32])
def test_results_equal_the_single_run_for_any_order(max_batch):
    for order in ((0, 1, 2, 3, 4, 5, 6), (6, 5, 4, 3, 2, 1, 0), (3, 0, 5, 2, 6, 1, 4)):
        s, _ = _synth(max_batch=max_batch, row_bucket=64 if max_batch == 2 else 256)
        with s:
            with s.hold():
                futs = {k: _submit(s, k) for k in order}
            for k, f in futs.items():
                w, sr = f.result(timeout=10)
                assert sr == 24000 and w.dtype == np.float32 and w.ndim == 1
                assert np.array_equal(w, EXPECTED[k]), (max_batch, order, k)


def test_registered_voice_equals_the_prompt_given_each_time():
    s, _ = _synth()
    with s:
        s.register_voice("v", *REQS[2]["item"][:2])
        f = s.submit(voice="v", gen_text=REQS[2]["item"][2], seed=REQS[2]["seed"], **SETTINGS["a"])
        assert np.array_equal(f.result(timeout=10)[0], EXPECTED[2])
        with pytest.raises(ValueError, match="not registered"):
            s.submit(voice="w", gen_text="hello there")


def test_submit_refuses_what_infer_batch_refuses():
    s, m = _synth()
    with s:
        audio = (torch.randn(1, 6000) * 0.3, 24000)
        for bad in ((audio, "A long enough reference text to divide by.", ""),):
            with pytest.raises(ValueError, match="nothing to generate") as e1:
                infer.infer_batch([bad], Model(), rf.FakeVocoder())
            with pytest.raises(ValueError, match="nothing to generate") as e2:
                s.submit(*bad)
            assert str(e1.value).split(": ", 1)[1] == str(e2.value).split(": ", 1)[1]
        with pytest.raises(ValueError, match="nothing to generate"):
            s.submit(audio, "Some words.", "More words to say.", fix_duration=0.1)
        st = s.stats()
        assert st["requests"] == 0 and st["queued"] == 0 and not m.calls


def test_a_failed_batch_fails_only_its_futures():
    s, m = _synth(Model(fail_steps=6), max_batch=4)
    with s:
        with s.hold():
            futs = [_submit(s, k) for k in range(7)]
        for k, f in enumerate(futs):
            if REQS[k]["group"] == "b":
                with pytest.raises(RuntimeError, match="this batch fails"):
                    f.result(timeout=10)
            else:
                assert np.array_equal(f.result(timeout=10)[0], EXPECTED[k])
        assert np.array_equal(_submit(s, 0).result(timeout=10)[0], EXPECTED[0])  # it goes on serving
        st = s.stats()
        assert st["failed_calls"] == 1 and st["inflight"] == 0


def test_close_cancels_or_drains():
    s, m = _synth()
    h = s.hold()
    h.__enter__()
    futs = [_submit(s, k) for k in range(3)]
    s.close(wait=False)
    assert all(f.cancelled() for f in futs) and not m.calls
    with pytest.raises(RuntimeError, match="closed"):
        _submit(s, 0)
    s, m = _synth()
    h = s.hold()
    h.__enter__()
    futs = [_submit(s, k) for k in range(3)]
    s.close()  # drains, hold or not
    assert all(f.done() and not f.cancelled() for f in futs)
    for k, f in enumerate(futs):
        assert np.array_equal(f.result()[0], EXPECTED[k])
    s.close()  # idempotent


def test_submissions_from_eight_threads_all_resolve():
    s, m = _synth(max_batch=4, max_wait_ms=1.0)
    got, errs = {}, []

    def worker(t):
        try:
            for j in range(3):
                k = (t + 3 * j) % len(REQS)
                got[(t, j)] = (k, _submit(s, k))
        except BaseException as e:  # pragma: no cover
            errs.append(e)

    with s:
        th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs and len(got) == 24
        for k, f in got.values():
            assert np.array_equal(f.result(timeout=20)[0], EXPECTED[k])
        st = s.stats()
    assert st["requests"] == 24 and st["queued"] == 0 and st["inflight"] == 0
    assert sum(c["live"][0] for c in st["calls_detail"]) == 24 and st["calls"] == len(m.calls)


class _Gate:
    """A completion event that stays pending until the test opens it: the device is busy for that long."""

    def __init__(self):
        self.ev = threading.Event()

    def synchronize(self):
        assert self.ev.wait(10)


def test_wait_and_idle_device_rules_with_an_injected_clock():
    now = [100.0]
    s, m = _synth(max_batch=4, max_wait_ms=5.0, max_inflight=2, clock=lambda: now[0])
    gates = []

    def new_event():
        gates.append(_Gate())
        return gates[-1]

    s._new_event = new_event
    try:
        f0 = _submit(s, 0)  # an idle device never waits: the clock stands still and the call starts
        _wait_for(lambda: len(m.calls) == 1)
        f6 = _submit(s, 6)  # one batch in flight, max_inflight is 2: still no waiting
        _wait_for(lambda: len(m.calls) == 2)
        f2 = _submit(s, 2)  # the device is busy (two in flight), the group is not full, nobody has waited
        time.sleep(0.012)  # several of the dispatcher's wake-ups
        assert len(m.calls) == 2 and s.stats()["queued"] == 1 and not f0.done()
        now[0] += 0.004
        time.sleep(0.006)
        assert len(m.calls) == 2  # 4 ms waited, max_wait_ms is 5
        f4 = _submit(s, 4)
        now[0] += 0.0011  # the oldest has now waited 5.1 ms: it goes, with whatever shares its group
        _wait_for(lambda: len(m.calls) == 3)
        assert _live(m) == [[0], [6], [2, 4]]
        for k in (6, 0, 2, 4):  # a full group goes at once, busy device and fresh requests notwithstanding
            fs = _submit(s, k)
        _wait_for(lambda: len(m.calls) == 4)
        assert _live(m)[3] == [6, 0, 2, 4]
    finally:
        s._new_event = lambda: serve._Done()
        _wait_for(lambda: len(gates) >= 1)
        for g in gates:
            g.ev.set()
    assert np.array_equal(f0.result(timeout=10)[0], EXPECTED[0])
    assert np.array_equal(f2.result(timeout=10)[0], EXPECTED[2])
    assert np.array_equal(f6.result(timeout=10)[0], EXPECTED[6])
    assert np.array_equal(f4.result(timeout=10)[0], EXPECTED[4])
    assert np.array_equal(fs.result(timeout=10)[0], EXPECTED[4])
    s.close()


# ------------------------------------------------------------------ CFM.sample(ragged_lmax=...)
class _Engine:
    def __init__(self):
        self.ragged, self.padded = [], []

    def sample(self, cond, cond_mask, text, duration, y0, t_grid, cfg_strength, use_batch_mask, **kw):
        self.padded.append(kw)
        return torch.zeros_like(cond), None

    def sample_ragged(self, cond, cond_mask, text, durations, y0, t_grid, cfg_strength, keep_trajectory=True, **kw):
        self.ragged.append(dict(kw, durations=list(durations)))
        return torch.zeros(cond.shape[0], 100), None


def test_cfm_sample_passes_ragged_lmax(monkeypatch):
    arch = configs.get_arch("DiT_tiny", text_num_embeds=64)
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=64, mel_dim=arch["mel_dim"])
    eng = _Engine()
    monkeypatch.setattr(net, "get_engine", lambda compute, device: eng)
    m = CFM(transformer=net, num_channels=100, compute="fp32")
    inp = synthetic.make_case(**gc.B3)
    args = dict(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"], steps=2, seed=1,
                keep_trajectory=False)
    longest = int(inp["duration"].max())
    m.sample(ragged=True, **args)
    assert "lmax" not in eng.ragged[0]  # the default stays the engine's own: max(durations)
    out, _ = m.sample(ragged=True, ragged_lmax=longest + 40, **args)
    assert eng.ragged[1]["lmax"] == longest + 40 and out.shape[1] == longest
    m.sample(ragged=True, ragged_lmax=longest, **args)
    assert eng.ragged[2]["lmax"] == longest
    with pytest.raises(ValueError, match="ragged_lmax"):
        m.sample(ragged=True, ragged_lmax=longest - 1, **args)
    assert len(eng.ragged) == 3 and not eng.padded  # refused before the engine
    m.sample(isolate=True, ragged_lmax=1, **args)  # ignored unless the call is ragged
    assert len(eng.padded) == 1 and "lmax" not in eng.padded[0]
    one = synthetic.make_case(**gc.B1)
    m.sample(cond=one["cond"], text=one["text"], duration=one["duration"], lens=one["lens"], steps=2, ragged=True,
             ragged_lmax=1)  # one utterance is the plain call: not ragged, ignored
    assert len(eng.padded) == 2


def test_package_exports_the_synthesizer():
    import f5_tts_amd

    assert f5_tts_amd.BatchingSynthesizer is serve.BatchingSynthesizer
