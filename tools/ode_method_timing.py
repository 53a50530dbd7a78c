"""One-box A/B of the fixed-grid ODE solvers at the C2 shape (F5TTS_v1_Base, 938 + 938 frames, bf16, CFG 2,
EPSS + sway -1): HIP events around CFM.sample, warm-up calls first, then --calls timed calls.

Variants, interleaved round after round, each in a process of its own (one variant after the other, never two
at a time):
  parent-euler   this tree's Python over an older libf5h.so given with --parent-lib (its f5h_sample)
  euler          this build, Euler through f5h_sample_ode
  midpoint, rk4  this build, 2 and 4 backbone evaluations per step
Every variant is timed at --steps and at half of it, so the per-evaluation cost (the slope) separates from the
per-call fixed cost (prologue + final kernel: the intercept), whose growth with the table rows is reported beside
the host-side prologue milliseconds (Engine.last_call_host_ms). The spread is that of parent-euler's own repeats.

    python tools/ode_method_timing.py --parent-lib /path/to/parent/libf5h.so --out profiles/ode_methods_c2.txt
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "f5-tts_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


def child(args):
    import torch

    from f5_tts_amd import configs, synthetic
    from f5_tts_amd.model import CFM, DiT

    dev = torch.device("cuda", 0)
    arch = configs.get_arch("F5TTS_v1_Base")
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    m = CFM(transformer=net, num_channels=100, compute="bf16", odeint_kwargs=dict(method=args.method)).to(dev)
    inp = synthetic.make_case(B=1, ref_frames=938, total_frames=1876, n_text=300)
    cond, text = inp["cond"].to(dev), inp["text"].to(dev)
    eng = m.transformer.get_engine("bf16", dev)
    res = {"method": args.method, "lib": os.environ.get("F5H_LIB", "")}
    for steps in (args.steps, args.steps // 2):
        def call():
            return m.sample(cond=cond, text=text, duration=inp["duration"], lens=inp["lens"], steps=steps,
                            cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0, keep_trajectory=False)[0]

        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        ms, host = [], []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
            host.append(eng.last_call_host_ms()["prologue"])
        assert torch.isfinite(out).all()
        res[str(steps)] = {"ms": ms, "host_prologue_ms": statistics.median(host)}
    print("ODE_TIMING " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default="", help="libf5h.so of the commit to compare with (variant parent-euler)")
    ap.add_argument("--parent-rev", default="", help="its commit hash, for the record")
    ap.add_argument("--rev", default="", help="this build's commit hash, for the record")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--method", default="euler", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.calls < 10:
        ap.error("--calls must be at least 10")
    variants = ([("parent-euler", "euler", args.parent_lib)] if args.parent_lib else []) + \
        [(mth, mth, "") for mth in ("euler", "midpoint", "rk4")]
    runs = {v[0]: [] for v in variants}
    for rnd in range(args.rounds):
        for name, method, lib in variants:
            env = dict(os.environ)
            env.pop("F5H_LIB", None)
            if lib:
                env["F5H_LIB"] = os.path.abspath(lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--method", method, "--calls", str(args.calls),
                   "--warmup", str(args.warmup), "--steps", str(args.steps)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("ODE_TIMING ")), None)
            if p.returncode != 0 or line is None:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{name}: child failed with status {p.returncode}; stopping")
            runs[name].append(json.loads(line[len("ODE_TIMING "):]))
            print(f"round {rnd} {name}: median {statistics.median(runs[name][-1][str(args.steps)]['ms']):.3f} ms",
                  flush=True)

    hi, lo = str(args.steps), str(args.steps // 2)
    lines = [f"ODE solver timing at C2 (F5TTS_v1_Base, 938+938 frames, bf16, CFG 2, steps {hi}); HIP events around "
             f"CFM.sample, {args.warmup} warm-up + {args.calls} timed calls per process, {args.rounds} interleaved rounds",
             f"this build: {args.rev or '?'}   parent: {args.parent_rev or '?'}", ""]
    table = {}
    for name, method, _ in variants:
        med_hi = [statistics.median(r[hi]["ms"]) for r in runs[name]]
        med_lo = [statistics.median(r[lo]["ms"]) for r in runs[name]]
        ev_hi, ev_lo = args.steps * STAGES[method], (args.steps // 2) * STAGES[method]
        t_hi, t_lo = statistics.median(med_hi), statistics.median(med_lo)
        slope = (t_hi - t_lo) / (ev_hi - ev_lo)
        table[name] = dict(ms=t_hi, rounds=med_hi, evals=ev_hi, per_eval=t_hi / ev_hi, slope=slope,
                           fixed=t_hi - slope * ev_hi,
                           host_prologue=statistics.median(r[hi]["host_prologue_ms"] for r in runs[name]),
                           call_spread=max((max(r[hi]["ms"]) - min(r[hi]["ms"])) for r in runs[name]))
    lines.append(f"{'variant':13s} {'ms/call':>9s} {'evals':>5s} {'ms/eval':>8s} {'slope ms/eval':>13s} "
                 f"{'fixed ms':>8s} {'host prologue ms':>16s}  per-round medians")
    for name, t in table.items():
        lines.append(f"{name:13s} {t['ms']:9.3f} {t['evals']:5d} {t['per_eval']:8.4f} {t['slope']:13.4f} "
                     f"{t['fixed']:8.3f} {t['host_prologue']:16.3f}  " + " ".join(f"{x:.3f}" for x in t["rounds"]))
    base = table.get("parent-euler") or table["euler"]
    spread = max(base["rounds"]) - min(base["rounds"])
    lines += ["", f"spread of {'parent-euler' if 'parent-euler' in table else 'euler'} across its rounds: "
              f"{spread:.3f} ms per call = {spread / base['evals']:.4f} ms per evaluation "
              f"(largest max-min of the timed calls inside one process: {base['call_spread']:.3f} ms)"]
    for name, t in table.items():
        if t is base:
            continue
        lines.append(f"{name}: slope {t['slope'] - base['slope']:+.4f} ms/eval vs base, call/evals "
                     f"{t['per_eval'] - base['per_eval']:+.4f} ms/eval, fixed cost {t['fixed'] - base['fixed']:+.3f} ms, "
                     f"host prologue {t['host_prologue'] - base['host_prologue']:+.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
            f.write("\nraw: " + json.dumps(runs) + "\n")


if __name__ == "__main__":
    main()
