"""compute="mxfp8" against compute="bf16" in one build and one process: `CFM.sample` wall time in interleaved rounds and
the in-kernel launch-probe time of the four per-layer GEMM classes, at the C2 (B = 1) and C3 (batch) shapes.

    python tools/mx8_ab.py [--configs c2,c3] [--rounds 5] [--calls 3] [--classes qkv,out,ffn1,ffn2] [--json OUT]

What the numbers are (measuring-on-mi355x): the wall time is a host clock around `calls` sample calls that end in a
device synchronise, after a warm call per arm (graph capture), arms alternating inside every round; median, minimum and
the spread of the per-round means are printed, and a difference counts only beyond twice the bf16 arm's spread. The
class times are the engine's launch probe (first workgroup start to last wave end of every launch of the class in
every 4th ODE step, s_memrealtime stamps inside the kernels), taken in calls of their own after the timed rounds. The
probe covers the GEMM launch only: the mxfp8 arm's quantiser launches ahead of the out-projection and FFN2 are in its
wall time, not in its class times. The mxfp8 arm's error against the bf16 arm (rel-L2 of the outputs) is printed
beside the times; it is a different compute mode, not a bitwise-equal one. Needs a GPU; fails without one."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "f5-tts_amd")]

import torch  # noqa: E402

import bench  # noqa: E402
from f5_tts_amd import synthetic  # noqa: E402

ARMS = ("bf16", "mxfp8")


def run_config(config, rounds, calls, classes):
    dev = torch.device("cuda", 0)
    case = {"c1": synthetic.c1_case, "c2": synthetic.c2_case, "c3": synthetic.c3_case, "c4": synthetic.c4_case}[config]()
    B = case["B"]
    refs = case["ref"] if isinstance(case["ref"], list) else [case["ref"]] * B
    tots = case["total"] if isinstance(case["total"], list) else [case["total"]] * B
    inp = synthetic.make_case(B=B, ref_frames=refs, total_frames=tots, n_text=case["nt"])
    kw = dict(cond=inp["cond"].to(dev), text=inp["text"].to(dev), duration=inp["duration"].to(dev),
              lens=inp["lens"].to(dev), steps=case["nfe"], cfg_strength=case["cfg"], sway_sampling_coef=case["sway"],
              seed=0, keep_trajectory=False)
    models = {arm: bench.build_model(case["preset"], arm, dev)[0] for arm in ARMS}
    engines = {arm: m.transformer.get_engine(arm, dev) for arm, m in models.items()}
    outs = {arm: models[arm].sample(**kw)[0].float().clone() for arm in ARMS}  # warm: graph capture
    torch.cuda.synchronize()
    times = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            models[arm].sample(**kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                models[arm].sample(**kw)
            torch.cuda.synchronize()
            times[arm].append((time.perf_counter() - t0) / calls * 1e3)
    res = {"config": config, "preset": case["preset"], "B": B, "nfe": case["nfe"], "sample_ms": {}, "class_us": {}}
    for arm in ARMS:
        t = sorted(times[arm])
        res["sample_ms"][arm] = {"median": round(t[len(t) // 2], 3), "min": round(t[0], 3),
                                 "spread": round(t[-1] - t[0], 3)}
    res["rel_l2_mxfp8_vs_bf16"] = float((outs["mxfp8"] - outs["bf16"]).norm() / outs["bf16"].norm())
    res["mx8_launches_per_call"] = None
    n0 = engines["mxfp8"].mx8_stats()[1]
    models["mxfp8"].sample(**kw)
    torch.cuda.synchronize()
    res["mx8_launches_per_call"] = engines["mxfp8"].mx8_stats()[1] - n0
    for kc in classes:
        res["class_us"][kc] = {}
        for arm in ARMS:
            eng = engines[arm]
            eng.probe(kc)
            models[arm].sample(**kw)  # captures the probed step graph (the probe is part of the graph key)
            models[arm].sample(**kw)
            torch.cuda.synchronize()
            n, ms = eng.probe_read()
            eng.probe(None)
            res["class_us"][kc][arm] = round(ms / n * 1e3, 3) if n else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--classes", default="qkv,out,ffn1,ffn2")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/mx8_ab.py measures on the GPU: no device found")
    results = []
    for config in a.configs.split(","):
        r = run_config(config, a.rounds, a.calls, a.classes.split(","))
        results.append(r)
        print(f"== {config} ({r['preset']}, B = {r['B']}, NFE {r['nfe']}): mxfp8 vs bf16 rel-L2 "
              f"{r['rel_l2_mxfp8_vs_bf16']:.3e}, {r['mx8_launches_per_call']} MX8 GEMM launches per call", flush=True)
        for arm in ARMS:
            s = r["sample_ms"][arm]
            print(f"  sample {arm:6s} median {s['median']:9.3f} ms  min {s['min']:9.3f} ms  spread {s['spread']:7.3f} ms")
        for kc, v in r["class_us"].items():
            b, m = v["bf16"], v["mxfp8"]
            ratio = f"{m / b:.3f}" if b and m else "n/a"
            print(f"  class {kc:5s} bf16 {b} us  mxfp8 {m} us per launch  (mxfp8 / bf16 = {ratio})", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
