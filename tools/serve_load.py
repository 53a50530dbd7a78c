#!/usr/bin/env python3
"""Load test of the request batcher (`f5_tts_amd.serve.BatchingSynthesizer`) on one GPU: a seeded synthetic request
trace (prompt lengths, text lengths, a settings mix, Poisson arrival times) against `infer.infer_batch`.

    python tools/serve_load.py --preset F5TTS_v1_Base --compute bf16 --nfe 16 --requests 64 --out profiles/x.json

Three steps, each a child process under its own `timeout`; the tool stops at the first that fails:

* closed: all requests at once. `rounds` interleaved rounds of (synthesizer: submit all under `hold()`, wait for all)
  and (baseline: `infer_batch(items, ragged=True, max_batch=M)` per settings group, per-item seeds), after one
  untimed round of each. Wall seconds per round, requests/s, the baseline's round-to-round spread, the filler share.
* open: Poisson arrivals at `--rate` requests/s through the synthesizer (p50 / p95 latency, calls per request, step
  graph captures and the engine's capture + instantiate host ms per call), then the same arrivals served one at a
  time by single-item `infer_batch` calls.
* open_rb1: the synthesizer again on the same arrivals with `row_bucket=1` (no bucketing), for the capture cost.

Prints one JSON line (and writes it to `--out`)."""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "f5-tts_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

WORDS = ("some call me nature others mother and the wind goes over hills where rivers run slowly down to a sea of "
         "glass while people talk about weather trains bread music light years stones").split()


def make_trace(n, seed, nfe, rate):
    """n requests: prompt 3-9 s of noise at 24 kHz (one in four at 16 kHz, one in four quiet), ~14 bytes of ref_text
    per second, 30-150 bytes of gen_text, settings (nfe, 2.0) 60 % / (nfe, 1.5) 25 % / (nfe / 2, 2.0) 15 %, sway -1,
    speed 1.0 (one in eight 1.3), exponential inter-arrival times at `rate` per second."""
    import numpy as np
    import torch

    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)

    def text(nbytes):
        out = []
        while sum(len(w) + 1 for w in out) < nbytes:
            out.append(WORDS[int(rng.integers(len(WORDS)))])
        return " ".join(out).capitalize() + "."

    reqs, t = [], 0.0
    for k in range(n):
        secs = float(rng.uniform(3.0, 9.0))
        sr = 16000 if rng.random() < 0.25 else 24000
        amp = 0.02 if rng.random() < 0.25 else 0.3
        u = rng.random()
        key = (nfe, 2.0, -1.0) if u < 0.6 else (nfe, 1.5, -1.0) if u < 0.85 else (max(nfe // 2, 1), 2.0, -1.0)
        t += float(rng.exponential(1.0 / rate))
        reqs.append(dict(item=((torch.randn(1, int(secs * sr), generator=g) * amp, sr), text(int(14 * secs)),
                               text(int(rng.integers(30, 151)))),
                         key=key, speed=1.3 if rng.random() < 0.125 else 1.0, seed=1000 + k, arrival=t))
    return reqs


def build(preset, compute):
    import torch

    from f5_tts_amd import configs, infer, synthetic
    from f5_tts_amd.model import CFM, DiT, UNetT

    arch = configs.get_arch(preset)
    cls = DiT if arch["backbone"] == "DiT" else UNetT
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = cls(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    model = CFM(transformer=net, num_channels=100, compute=compute,
                vocab_char_map={chr(i): i for i in range(256)}).to("cuda:0")
    voc = infer.load_vocoder(is_local=True, local_path="synthetic", device="cuda:0")
    torch.cuda.synchronize()
    return model, voc


def _kw(key):
    return dict(nfe_step=key[0], cfg_strength=key[1], sway_sampling_coef=key[2])


def _submit(s, r):
    return s.submit(*r["item"], speed=r["speed"], seed=r["seed"], **_kw(r["key"]))


def _pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(p / 100.0 * (len(xs) - 1))))]


def _call_summary(st):
    cap_ms = [c["host_ms"]["capture"] + c["host_ms"]["instantiate"] for c in st["calls_detail"] if c.get("host_ms")]
    tot_ms = [c["host_ms"]["total"] for c in st["calls_detail"] if c.get("host_ms")]
    return dict(calls=st["calls"], calls_per_request=round(st["calls"] / max(st["requests"], 1), 4),
                rows_live=st["rows_live"], rows_filler=st["rows_filler"], filler_share=round(st["filler_share"], 4),
                graph_captures=st["graph_captures"], shapes=len({tuple(c["cap"]) + tuple(c["key"]) for c in st["calls_detail"]}),
                capture_instantiate_ms_per_call=round(sum(cap_ms) / max(len(cap_ms), 1), 3),
                capture_instantiate_ms_total=round(sum(cap_ms), 2),
                sample_host_ms_per_call=round(sum(tot_ms) / max(len(tot_ms), 1), 3))


def step_closed(a, reqs):
    import torch

    from f5_tts_amd import infer, serve

    model, voc = build(a.preset, a.compute)
    eng = model.transformer.get_engine(model.engine_compute(), model.device)
    groups = {}
    for r in reqs:
        groups.setdefault(r["key"], []).append(r)

    def baseline():
        t0 = time.perf_counter()
        for key, rs in groups.items():
            infer.infer_batch([r["item"] + ({"seed": r["seed"], "speed": r["speed"]},) for r in rs], model, voc,
                              ragged=True, max_batch=a.max_batch, **_kw(key))
        return time.perf_counter() - t0

    s = serve.BatchingSynthesizer(model, voc, max_batch=a.max_batch, row_bucket=a.row_bucket)

    def batcher():
        t0 = time.perf_counter()
        with s.hold():
            futs = [_submit(s, r) for r in reqs]
        for f in futs:
            f.result(timeout=600)
        return time.perf_counter() - t0

    warm = dict(batcher=round(batcher(), 4), baseline=round(baseline(), 4))
    cap0, st0 = eng.graph_stats()["captures"], s.stats()
    tb, ts = [], []
    for _ in range(a.rounds):
        ts.append(batcher())
        tb.append(baseline())
    st = s.stats()
    s.close()
    torch.cuda.synchronize()
    mean = lambda xs: sum(xs) / len(xs)  # noqa: E731
    timed = [c for c in st["calls_detail"]][st0["calls"]:]
    host = [c["host_ms"]["total"] for c in timed if c.get("host_ms")]
    return dict(requests=len(reqs), rounds=a.rounds, warmup_s=warm,
                batcher_s=[round(x, 4) for x in ts], baseline_s=[round(x, 4) for x in tb],
                batcher_mean_s=round(mean(ts), 4), baseline_mean_s=round(mean(tb), 4),
                batcher_req_per_s=round(len(reqs) / mean(ts), 2), baseline_req_per_s=round(len(reqs) / mean(tb), 2),
                ratio=round(mean(ts) / mean(tb), 4), baseline_spread_s=round(max(tb) - min(tb), 4),
                baseline_spread_rel=round((max(tb) - min(tb)) / mean(tb), 4),
                filler_share=round(st["filler_share"], 4), calls_per_round=(st["calls"] - st0["calls"]) / a.rounds,
                captures_in_timed_rounds=eng.graph_stats()["captures"] - cap0,
                batcher_sample_host_ms_per_call=round(mean(host), 3) if host else None,
                call_shapes=[dict(live=c["live"], cap=c["cap"]) for c in timed[: len(timed) // a.rounds]])


def _open_batcher(a, reqs, model, voc, row_bucket):
    from f5_tts_amd import serve

    lat = [None] * len(reqs)
    with serve.BatchingSynthesizer(model, voc, max_batch=a.max_batch, row_bucket=row_bucket) as s:
        t0 = time.perf_counter()
        futs = []
        for k, r in enumerate(reqs):
            d = r["arrival"] - (time.perf_counter() - t0)
            if d > 0:
                time.sleep(d)
            f = _submit(s, r)
            f.add_done_callback(lambda _f, k=k, at=r["arrival"]: lat.__setitem__(k, time.perf_counter() - t0 - at))
            futs.append(f)
        for f in futs:
            f.result(timeout=600)
        wall = time.perf_counter() - t0
        st = s.stats()
    out = dict(row_bucket=row_bucket, wall_s=round(wall, 3), p50_s=round(_pct(lat, 50), 4), p95_s=round(_pct(lat, 95), 4),
               max_s=round(max(lat), 4))
    out.update(_call_summary(st))
    return out


def step_open(a, reqs):
    from f5_tts_amd import infer

    model, voc = build(a.preset, a.compute)
    w = reqs[0]  # one untimed single call: library start-up is not traffic
    infer.infer_batch([w["item"]], model, voc, ragged=True, **_kw(w["key"]))
    res = dict(rate_per_s=a.rate, batcher=_open_batcher(a, reqs, model, voc, a.row_bucket))
    eng = model.transformer.get_engine(model.engine_compute(), model.device)
    cap0 = eng.graph_stats()["captures"]
    lat, cap_ms, t0 = [], [], time.perf_counter()
    for r in reqs:  # the same arrivals, one single-item call at a time
        d = r["arrival"] - (time.perf_counter() - t0)
        if d > 0:
            time.sleep(d)
        infer.infer_batch([r["item"] + ({"seed": r["seed"], "speed": r["speed"]},)], model, voc, ragged=True,
                          **_kw(r["key"]))
        lat.append(time.perf_counter() - t0 - r["arrival"])
        h = eng.last_call_host_ms()
        cap_ms.append(h["capture"] + h["instantiate"])
    res["sequential"] = dict(wall_s=round(time.perf_counter() - t0, 3), p50_s=round(_pct(lat, 50), 4),
                             p95_s=round(_pct(lat, 95), 4), max_s=round(max(lat), 4), calls=len(reqs),
                             calls_per_request=1.0, graph_captures=eng.graph_stats()["captures"] - cap0,
                             capture_instantiate_ms_per_call=round(sum(cap_ms) / len(cap_ms), 3),
                             capture_instantiate_ms_total=round(sum(cap_ms), 2))
    return res


def step_open_rb1(a, reqs):
    from f5_tts_amd import infer

    model, voc = build(a.preset, a.compute)
    w = reqs[0]
    infer.infer_batch([w["item"]], model, voc, ragged=True, **_kw(w["key"]))
    return _open_batcher(a, reqs, model, voc, 1)


STEPS = {"closed": step_closed, "open": step_open, "open_rb1": step_open_rb1}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--preset", default="F5TTS_v1_Base")
    ap.add_argument("--compute", default="bf16")
    ap.add_argument("--nfe", type=int, default=16)
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--row-bucket", type=int, default=256)
    ap.add_argument("--rate", type=float, default=4.0, help="open loop: mean arrivals per second")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds per step")
    ap.add_argument("--steps", default="closed,open,open_rb1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)  # a child: run this step, JSON to --out
    a = ap.parse_args(argv)
    if a.step:
        res = STEPS[a.step](a, make_trace(a.requests, a.seed, a.nfe, a.rate))
        with open(a.out, "w") as f:
            json.dump(res, f)
        return 0
    result = dict(tool="serve_load", preset=a.preset, compute=a.compute, nfe=a.nfe, requests=a.requests, seed=a.seed,
                  max_batch=a.max_batch, row_bucket=a.row_bucket)
    tr = make_trace(a.requests, a.seed, a.nfe, a.rate)
    result["trace"] = dict(groups={str(k): sum(1 for r in tr if r["key"] == k) for k in sorted({r["key"] for r in tr})},
                           prompt_s=[round(min(r["item"][0][0].shape[-1] / r["item"][0][1] for r in tr), 2),
                                     round(max(r["item"][0][0].shape[-1] / r["item"][0][1] for r in tr), 2)],
                           last_arrival_s=round(tr[-1]["arrival"], 2))
    rc = 0
    for step in a.steps.split(","):
        with tempfile.NamedTemporaryFile(suffix=".json", delete=False) as tf:
            path = tf.name
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
               "--out", path] + [x for k in ("preset", "compute", "nfe", "requests", "seed", "rounds", "max_batch",
                                             "row_bucket", "rate")
                                 for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        t0 = time.perf_counter()
        rc = subprocess.run(cmd).returncode
        if rc != 0:  # a fault, an abort, a time limit: nothing more starts on the GPU
            result["failed"] = dict(step=step, returncode=rc)
            break
        with open(path) as f:
            result[step] = json.load(f)
        result[step]["step_wall_s"] = round(time.perf_counter() - t0, 1)
        os.unlink(path)
    line = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
