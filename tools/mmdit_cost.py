"""Per-call and per-class cost of one MMDiT configuration (the reference ships no MMDiT config, so this is a record,
not a comparison): dim 1024, depth 8, heads 16, ff_mult 4, bf16, the C2 inputs (B = 1, 938 + 938 frames, 300 tokens),
NFE 16, CFG 2. Per-call milliseconds over interleaved rounds, then every kernel class by its in-kernel stamps (every
4th step is sampled; the text-side launches count in their class).

    python tools/mmdit_cost.py [OUT.json] [--rounds 5] [--calls 5]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "f5-tts_amd")]

import torch  # noqa: E402

from f5_tts_amd import _lib, configs, synthetic  # noqa: E402
from f5_tts_amd.model import CFM, MMDiT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    arch = configs.get_arch(dict(backbone="MMDiT", dim=1024, depth=8, heads=16, ff_mult=4))
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = MMDiT(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    m = CFM(transformer=net, num_channels=100, compute="bf16").to(dev)
    case = synthetic.c2_case()
    inp = synthetic.make_case(B=1, ref_frames=case["ref"], total_frames=case["total"], n_text=case["nt"])
    skw = dict(cond=inp["cond"].to(dev), text=inp["text"].to(dev), duration=inp["duration"], lens=inp["lens"],
               steps=case["nfe"], cfg_strength=case["cfg"], sway_sampling_coef=case["sway"], seed=0,
               keep_trajectory=False)
    eng = m.transformer.get_engine("bf16", dev)

    def step():
        return m.sample(**skw)[0]

    for _ in range(3):
        out = step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    rounds = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            step()
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e3 / a.calls)
    classes = {}
    for kc in _lib.KCLASS:
        if kc == "chain":
            continue
        eng.probe(kc)
        step()
        step()
        torch.cuda.synchronize()
        n, ms = eng.probe_read()
        eng.probe(None)
        if n:
            classes[kc] = dict(sampled_launches=n, avg_us=round(ms / n * 1e3, 2))
    wt, plain = eng.store_policy_stats()
    res = dict(config=dict(arch=arch, compute="bf16", B=1, frames=case["total"], nt=case["nt"], nfe=case["nfe"],
                           cfg=case["cfg"]),
               ms_per_call=dict(median=round(sorted(rounds)[len(rounds) // 2], 3), min=round(min(rounds), 3),
                                max=round(max(rounds), 3), rounds=[round(r, 3) for r in rounds]),
               classes=classes, store_policy=dict(write_through=wt, plain=plain),
               note="avg_us per launch over audio-side and text-side launches of a class together")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
