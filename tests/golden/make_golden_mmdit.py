"""Generate the MMDiT golden vectors in tests/golden/ by running the REFERENCE implementation.

Run in the build container only (needs the reference source tree, read-only):
    python tests/golden/make_golden_mmdit.py [--only NAME]

The reference's own `f5_tts.model.MMDiT` inside its `CFM`, on the CPU, with the third-party shims, the fp32 noise
recipe and the helpers of make_golden.py. Weights are the hash-PRNG weights of f5_tts_amd.synthetic, inputs come from
synthetic.make_case (seed 7 noise); the cases are the tables of tests/mmdit_reference.py. Only outputs (plus input
checksums) are stored, as float32 .npz, and the names / shapes of the reference state dict as JSON.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))                   # repository root (oracle)
sys.dont_write_bytecode = True

from make_golden import checksum, fp32_noise, install_shims  # noqa: E402

from f5_tts_amd import synthetic  # noqa: E402

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def build_ref(arch, load=True):
    from torch import nn

    from f5_tts.model import CFM, MMDiT

    kw = {k: arch[k] for k in ("dim", "depth", "heads", "dim_head", "ff_mult", "text_mask_padding", "qk_norm",
                                "attn_mask_enabled", "text_num_embeds", "mel_dim")}
    net = MMDiT(**kw)
    ident = nn.Identity()
    ident.n_mel_channels = 100
    model = CFM(transformer=net, mel_spec_module=ident, num_channels=100)
    if load:
        sd = {"transformer." + k: v for k, v in synthetic.make_weights_torch(arch).items()}
        missing, unexpected = model.load_state_dict(sd, strict=False)
        bad = [m for m in missing if not (m.endswith("inv_freq") or m.endswith("freqs_cis"))]
        assert not bad and not unexpected, (bad, unexpected)
    return model.eval()


def run_sample(arch, spec, nfe, sway, cfg, dtype, seed):
    model = build_ref(arch).to(dtype)
    inp = synthetic.make_case(**spec)
    with fp32_noise(), torch.no_grad():
        out, traj = model.sample(cond=inp["cond"], text=inp["text"], duration=inp["duration"], lens=inp["lens"],
                                 steps=nfe, cfg_strength=cfg, sway_sampling_coef=sway, seed=seed)
    return dict(out=out.float().numpy(), traj_1=traj[1].float().numpy(), checksum=checksum(inp))


def run_forward(arch, fi, opts, fwd_t):
    model = build_ref(arch)
    with torch.no_grad():
        out = model.transformer(x=fi["x"], cond=fi["cond"], text=fi["text"], time=torch.tensor(opts.get("t", fwd_t)),
                                mask=fi["mask"], cfg_infer=opts.get("cfg_infer", True),
                                drop_audio_cond=opts.get("drop_audio", False), drop_text=opts.get("drop_text", False),
                                cache=True)
        model.transformer.clear_cache()
    return dict(out=out.float().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    install_shims()
    torch.set_num_threads(8)
    import golden_cases as gc
    import mmdit_reference as mr

    jobs = {}
    for name, (tag, spec, nfe, sway, cfg, dt) in mr.SAMPLE_CASES.items():
        jobs[name] = (lambda *a: (lambda: run_sample(*a)))(mr.arch_of(tag), spec, nfe, sway, cfg, DTYPES[dt], gc.SEED)
    for name, (tag, spec, opts) in mr.FORWARD_CASES.items():
        jobs[name] = (lambda *a: (lambda: run_forward(*a)))(mr.arch_of(tag), mr.forward_inputs(spec), opts, gc.FWD_T)
    for name, fn in jobs.items():
        if args.only and args.only not in name:
            continue
        t0 = time.time()
        res = fn()
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **{k: np.asarray(v) for k, v in res.items()})
        print(f"{name}: {time.time() - t0:.1f}s  out{tuple(res['out'].shape)} absmax {np.abs(res['out']).max():.3f}",
              flush=True)
    if not args.only:
        # names and shapes of the reference's state dict (transformer.* without the prefix; the rotary buffer, which
        # the plugins register on their own, left out), in its order, with and without qk_norm
        sd = {}
        for tag in ("tiny", "tiny_qkn"):
            model = build_ref(mr.arch_of(tag), load=False)
            sd[tag] = [[k, list(v.shape)] for k, v in model.transformer.state_dict().items()
                       if not k.endswith("inv_freq")]
        with open(os.path.join(HERE, "mmdit_state_dict.json"), "w") as f:
            json.dump(sd, f, indent=1)
        print("mmdit_state_dict.json:", {k: len(v) for k, v in sd.items()})


if __name__ == "__main__":
    main()
