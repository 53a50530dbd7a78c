"""What a C2 call spends at its launch boundaries, per kernel class (DESIGN.md §3 'Launch boundaries').

A dispatch's kernel-trace duration (rocprofv3 --kernel-trace, End - Start) covers more than its workgroups: it ends
when the end-of-kernel release has written back what the launch left dirty in the XCD L2s. The in-kernel span of the
same launch (first workgroup start to last wave end, the kernels' own s_memrealtime stamps, as bench.py's probe
pre-pass reads them) does not. Their difference is what the launch spends outside its workgroups.

    # 1. kernel trace of warm + marked calls (a run of its own: no counters in the same pass)
    rocprofv3 --kernel-trace --output-format csv -d D -o run -- python tools/boundary_cost.py run [POLICY]
    # 2. in-kernel spans, one class probed at a time
    python tools/boundary_cost.py probe SPANS.json [POLICY]
    # 3. the table
    python tools/boundary_cost.py report D/run_kernel_trace.csv SPANS.json [LABEL] > profiles/..._boundary_c2.txt
   (SPANS.json "-": the trace columns only, e.g. for the per-class arms of a store-policy A/B)

POLICY: the engine's store policy (Engine.set_store_policy: -1 auto, 0 plain, 1 write-through, 0x100 | class mask);
ignored with a library that has none (an older build through F5H_LIB, whose source hash then comes from F5H_SRC_HASH).
"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "f5-tts_amd"), os.path.join(REPO, "tools")]

CLASSES = ("qkv", "attention", "out", "ffn1", "ffn2")
# warm and marked calls of a trace run: the call after the capture still runs 1-2 us per launch slower than the
# later ones, and rocprofv3 of this ROCm build gives up after ~12-16k graph-launched dispatches (2.6k per call)
WARM, CALLS = 2, 2
S, L, D, FF, H, DEPTH, NFE = 2, 1876, 1024, 2048, 16, 22, 16  # the C2 launch shape
# bytes a launch of the class stores (16-bit): q, k, v; O; h + hs (the LayerNorm fold's producer); the FFN1 output
STORED = {"qkv": 3 * S * L * D * 2, "attention": S * L * D * 2, "out": 2 * S * L * D * 2, "ffn1": S * L * FF * 2,
          "ffn2": 2 * S * L * D * 2}


def _model(policy):
    import torch

    import bench
    from f5_tts_amd import _lib, synthetic

    dev = torch.device("cuda", 0)
    case = synthetic.c2_case()
    model, _ = bench.build_model(case["preset"], "bf16", dev)
    B = case["B"]
    refs = case["ref"] if isinstance(case["ref"], list) else [case["ref"]] * B
    tots = case["total"] if isinstance(case["total"], list) else [case["total"]] * B
    inp = synthetic.make_case(B=B, ref_frames=refs, total_frames=tots, n_text=case["nt"])
    kw = dict(cond=inp["cond"].to(dev), text=inp["text"].to(dev), duration=inp["duration"], lens=inp["lens"],
              steps=case["nfe"], cfg_strength=case["cfg"], sway_sampling_coef=case["sway"], seed=0,
              keep_trajectory=False)
    eng = model.transformer.get_engine(model.engine_compute(), dev)
    if policy is not None and hasattr(_lib.lib(), "f5h_set_store_policy"):
        eng.set_store_policy(policy)
    return torch, model, eng, kw


def run(policy):
    torch, model, _, kw = _model(policy)
    for _ in range(WARM):
        model.sample(**kw)
    torch.cuda.synchronize()
    marker = torch.rand(64, device="cuda:0")
    torch.sort(marker)  # start marker, as tools/trace_c2.py
    for _ in range(CALLS):
        model.sample(**kw)
    torch.sort(marker)
    torch.cuda.synchronize()
    print("done", flush=True)


def probe(out, policy):
    torch, model, eng, kw = _model(policy)
    model.sample(**kw)
    spans = {}
    for kc in CLASSES:
        eng.probe(kc)
        model.sample(**kw)  # captures the probed step graph
        model.sample(**kw)
        torch.cuda.synchronize()
        n, ms = eng.probe_read()
        eng.probe(None)
        spans[kc] = {"in_kernel_us": round(ms / n * 1e3, 3), "launches": n}
    json.dump({"policy": policy, "spans": spans}, open(out, "w"), indent=1)
    print(json.dumps(spans))


def report(trace, spans_path, label=""):
    import bench
    from class_profile import _trace_rows
    from pmc_classes import classify

    disp = _trace_rows(trace)
    marks = [i for i, d in enumerate(disp) if "sort" in d[1].lower()]
    if len(marks) >= 2:  # the marked calls only
        disp = disp[marks[0] + 1:marks[-1]]
    cls = classify(disp)
    acc = {c: [] for c in CLASSES}
    for i, (_, _, us) in enumerate(disp):
        if cls.get(i) in acc:
            acc[cls[i]].append(us)
    sp = json.load(open(spans_path)) if spans_path != "-" else {"policy": label, "spans": {}}
    stamp = {"head": os.environ.get("F5H_HEAD", "unknown"),
             "src_hash": os.environ.get("F5H_SRC_HASH") or bench.src_hash()}
    print(f"# launch boundary cost at C2 (S={S} x L={L}, depth {DEPTH}, NFE {NFE}, bf16) {label}")
    print(f"# head {stamp['head']} src_hash {stamp['src_hash']} store policy {sp.get('policy')}")
    print("# trace: rocprofv3 --kernel-trace mean dispatch duration over the marked calls; in-kernel: s_memrealtime "
          "stamps, first workgroup start to last wave end; outside = trace - in-kernel; per call: the class's trace mean in each "
          "marked call (the first runs slower in every run; compare like with like); B/6TB/s: the stored bytes at the write-back rate of MI355X_MICROARCH.md's "
          "'boundary' row")
    print(f"{'class':10s} {'n':>6s} {'trace us':>9s} {'median':>8s} {'in-kernel us':>13s} {'outside us':>11s} "
          f"{'per call us':>13s} {'stored MB':>10s} {'B/6TB/s us':>11s}")
    tot_t = tot_o = 0.0
    for c in CLASSES:
        if not acc[c]:
            continue
        t, ik = statistics.mean(acc[c]), sp["spans"].get(c, {}).get("in_kernel_us", float("nan"))
        tot_t += t
        tot_o += t - ik
        per = len(acc[c]) // CALLS  # the class's dispatches of one call, in dispatch order
        calls = [statistics.mean(acc[c][k * per:(k + 1) * per]) for k in range(CALLS)] if per else [t]
        print(f"{c:10s} {len(acc[c]):6d} {t:9.2f} {statistics.median(acc[c]):8.2f} {ik:13.2f} {t - ik:11.2f} "
              f"{'/'.join(f'{x:.2f}' for x in calls):>13s} {STORED[c] / 1e6:10.1f} {STORED[c] / 6e12 * 1e6:11.2f}")
    n = DEPTH * NFE
    print(f"per layer: trace {tot_t:.2f} us, outside {tot_o:.2f} us; per call (x {n} layer passes): trace "
          f"{tot_t * n / 1e3:.2f} ms, outside {tot_o * n / 1e3:.2f} ms")


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "run":
        run(int(sys.argv[2], 0) if len(sys.argv) > 2 else None)
    elif cmd == "probe":
        probe(sys.argv[2], int(sys.argv[3], 0) if len(sys.argv) > 3 else None)
    else:
        report(*sys.argv[2:5])
