"""Ragged sampling against the isolated padded batch (DESIGN §5 'Ragged sampling').

  sample:  one CFM.sample call at C3's shape (B = 32, 564..1876 frames, NFE 32, F5TTS_v1_Base with synthetic weights),
           host clock around a synchronised call, --calls alternating calls per arm: isolate=True, ragged=True.
           --probe adds, per arm, the device time of every kernel class over one more call (f5h_probe_enable).
  chunks:  a six-sentence text through infer_batch_process(batch_chunks=True), with and without ragged=True: wall time
           of the whole call (F5TTS_v1_Base and Vocos with synthetic weights, an 8 s prompt, NFE 32).

Prints one JSON line per figure with every value and the medians.

  python tools/ragged_sample_timing.py [--compute bf16] [--calls 5] [--what sample,chunks] [--probe] [--small]
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "f5-tts_amd")]

from f5_tts_amd import _lib, configs, infer, synthetic  # noqa: E402
from f5_tts_amd.model import CFM, DiT  # noqa: E402

DEV = "cuda:0"
SENTENCES = [
    "Some call me nature, others call me mother nature, and a few do not call me at all.",
    "I have been here for over four and a half billion years, twenty two thousand five hundred times longer than you.",
    "I do not really need people, but people need me, every single one of them.",
    "Your future depends on me: when I thrive you thrive, and when I falter you falter, or worse.",
    "I have fed species greater than you, and I have starved species greater than you.",
    "My oceans, my soil, my flowing streams and my forests can all take you, or leave you.",
]


def build(preset, compute, vocab_map=None, **over):
    arch = configs.get_arch(preset, **over)
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    return CFM(transformer=net, num_channels=100, compute=compute, vocab_char_map=vocab_map).to(DEV)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def report(what, arms, extra=None):
    out = {"what": what}
    for k, v in arms.items():
        out[k] = dict(median_ms=round(statistics.median(v), 2), ms=[round(x, 2) for x in v])
    a, b = (statistics.median(arms[k]) for k in list(arms)[:2])
    out["second_over_first"] = round(b / a, 4)
    if extra:
        out.update(extra)
    print(json.dumps(out), flush=True)


def sample_figure(args):
    case = synthetic.c3_case()
    if args.small:  # a quick shape for checking the script itself
        case.update(B=4, ref=case["ref"][::8], total=case["total"][::8], nt=case["nt"][::8], nfe=4)
    m = build(case["preset"], args.compute)
    inp = synthetic.make_case(B=case["B"], ref_frames=case["ref"], total_frames=case["total"], n_text=case["nt"])
    cond, text = inp["cond"].to(DEV), inp["text"].to(DEV)

    def call(**kw):
        m.sample(cond=cond, text=text, duration=inp["duration"], lens=inp["lens"], steps=case["nfe"],
                 cfg_strength=case["cfg"], sway_sampling_coef=case["sway"], seed=0, keep_trajectory=False, **kw)

    arms = {"isolate": dict(isolate=True), "ragged": dict(ragged=True)}
    for kw in arms.values():  # the first call of a shape captures its graph
        call(**kw)
        call(**kw)
    times = {k: [] for k in arms}
    for _ in range(args.calls):
        for k, kw in arms.items():  # alternated
            times[k].append(timed(lambda: call(**kw)))
    tot = case["total"]
    extra = dict(B=case["B"], rows_padded=case["B"] * max(tot), rows_live=sum(tot), nfe=case["nfe"],
                 compute=args.compute)
    if args.probe:
        eng = m.transformer.get_engine(args.compute, m.device)
        classes = {}
        for kc in _lib.KCLASS:
            if kc == "chain":
                continue
            classes[kc] = {}
            for k, kw in arms.items():
                eng.probe(kc)
                call(**kw)
                torch.cuda.synchronize()
                n, ms = eng.probe_read()
                classes[kc][k] = dict(launches=n, ms=round(ms, 3))
            eng.probe(None)
        extra["probe_sampled_ms"] = classes
    report("sample_c3_shape", times, extra)


def chunks_figure(args):
    from f5_tts_amd.vocos import Vocos, make_weights

    m = build("F5TTS_v1_Base", args.compute, vocab_map={chr(i): i for i in range(256)}, text_num_embeds=256)
    voc = Vocos(compute=args.compute if args.compute != "fp16" else "bf16")
    voc.load_state_dict(make_weights())
    voc = voc.to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    audio = torch.randn(1, 8 * 24000, generator=g) * 0.3
    ref_text = "Some call me nature, others call me mother nature."
    nfe = 4 if args.small else 32

    def call(**kw):
        return next(infer.infer_batch_process((audio, 24000), ref_text, SENTENCES, m, voc, nfe_step=nfe,
                                              batch_chunks=True, **kw))

    arms = {"batch_chunks": {}, "batch_chunks_ragged": dict(ragged=True)}
    for kw in arms.values():
        call(**kw)
        call(**kw)
    times = {k: [] for k in arms}
    for _ in range(max(args.calls, 4)):
        for k, kw in arms.items():
            times[k].append(timed(lambda: call(**kw)))
    report("six_chunk_infer_batch_process", times, dict(nfe=nfe, compute=args.compute))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compute", default="bf16", choices=("bf16", "fp16", "fp32"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--what", default="sample,chunks")
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    for w in args.what.split(","):
        {"sample": sample_figure, "chunks": chunks_figure}[w](args)


if __name__ == "__main__":
    main()
