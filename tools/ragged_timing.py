"""Ragged batch to waveforms against the per-utterance loop, on C3's mix: 32 utterances whose
generated lengths span 282..938 frames.

  decode:  Vocos.decode_ragged(out, ref, total - ref) on the sampler's [32, N, 100] output, against the loop of 32
           Vocos.decode(out[i, ref_i:total_i].T[None]) calls (slice, permute, contiguous, ~30 launches each);
  mel:     MelSpec.forward_ragged(waves) against the loop of 32 MelSpec()(w[None]) calls.

The loop runs the per-utterance entry points (`f5h_vocos_decode`, `f5h_mel_forward`) and is the yardstick. Device
events, every shape warmed up first, the two variants alternated in one process, each window longer than
--window seconds; prints per variant the median window (ms per batch of 32) and the spread (max - min)/median.

  python tools/ragged_timing.py [--compute fp32|bf16] [--windows 7] [--window 0.5]
"""

import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "f5-tts_amd")]

from f5_tts_amd import synthetic  # noqa: E402
from f5_tts_amd.mel import MelSpec  # noqa: E402
from f5_tts_amd.vocos import Vocos, make_weights  # noqa: E402

DEV = "cuda:0"


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(name, variants, windows, min_s):
    reps = {}
    for k, fn in variants.items():  # warm-up of every shape, then the repetitions a window needs
        fn()
        ms = window(fn, 3)
        reps[k] = max(3, int(min_s * 1e3 / ms) + 1)
    times = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():  # alternated
            times[k].append(window(fn, reps[k]))
    out = {}
    for k, t in times.items():
        med = statistics.median(t)
        out[k] = dict(ms=round(med, 4), spread=round((max(t) - min(t)) / med, 4), reps=reps[k])
    print(json.dumps({"what": name, **out, "ragged_over_loop": round(out["ragged"]["ms"] / out["loop"]["ms"], 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compute", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    c3 = synthetic.c3_case()
    ref, total = c3["ref"], c3["total"]
    gen = [t - r for t, r in zip(total, ref)]
    assert (min(gen), max(gen), len(gen)) == (282, 938, 32)
    g = torch.Generator().manual_seed(0)
    out = (torch.randn(32, max(total), 100, generator=g) * 2.0 - 4.0).to(DEV)  # the sampler's output layout
    voc = Vocos(compute=a.compute)
    voc.load_state_dict(make_weights())
    voc.to(DEV)

    def dec_loop():
        return [voc.decode(out[i, ref[i]: total[i]].permute(1, 0)[None]) for i in range(32)]

    def dec_ragged():
        return voc.decode_ragged(out, ref, gen)

    for w, s in zip(dec_ragged(), dec_loop()):
        assert torch.equal(w, s[0])
    compare(f"vocos decode {a.compute}, 32 utterances, {sum(gen)} frames", dict(loop=dec_loop, ragged=dec_ragged),
            a.windows, a.window)

    mel = MelSpec()
    waves = [(0.1 * torch.randn(r * 256, generator=g)).to(DEV) for r in ref]  # the prompts: ref_i * hop samples

    def mel_loop():
        return [mel(w[None]) for w in waves]

    def mel_ragged():
        return mel.forward_ragged(waves)

    cond, frames = mel_ragged()
    for i, m in enumerate(mel_loop()):
        assert torch.equal(cond[i, : frames[i]], m[0].T)
    compare(f"log-mel, 32 waves, {sum(frames)} frames", dict(loop=mel_loop, ragged=mel_ragged), a.windows, a.window)


if __name__ == "__main__":
    main()
