"""Reference for the fixed-grid ODE solver tests: torchdiffeq's euler / midpoint / rk4 (the 3/8 rule) steps
written out in torch, and CFM.sample with them, composed from the CPU oracle's pieces (oracle/ref_cpu.py, whose
own cfm_sample is Euler only). tests/test_ode_methods.py checks the stepper on y' = -y."""

from __future__ import annotations

import functools

import torch

from f5_tts_amd import synthetic
from f5_tts_amd.model.utils import ode_eval_times
from oracle import ref_cpu


def integrate(f, y0, t, method):
    """Grid-point trajectory [len(t), ...] of y' = f(t, y) from y0, one fixed step per grid interval. The stage
    times are formed in t's dtype (a 16-bit grid rounds them, as torchdiffeq would); the state keeps y0's."""
    stages = {"euler": 1, "midpoint": 2, "rk4": 4}[method]
    te = ode_eval_times(t, method).reshape(-1, stages).to(y0.dtype)
    t = t.to(y0.dtype)
    y, traj = y0, [y0]
    for k in range(t.numel() - 1):
        dt = t[k + 1] - t[k]
        k1 = f(te[k, 0], y)
        if method == "euler":
            y = y + dt * k1
        elif method == "midpoint":
            y = y + dt * f(te[k, 1], y + k1 * (0.5 * dt))
        else:
            c = 1 / 3
            k2 = f(te[k, 1], y + dt * k1 * c)
            k3 = f(te[k, 2], y + dt * (k2 - k1 * c))
            k4 = f(te[k, 3], y + dt * (k1 - k2 + k3))
            y = y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        traj.append(y)
    return torch.stack(traj)


@torch.no_grad()
def cfm_sample(W, arch, inp, y0, steps, cfg_strength, sway, method, t=None):
    """fp32 CFM.sample (cfm.py:160-223) with the solver `method`: (out, traj [steps+1, B, N, mel], preamble).
    t: the grid, when it is not the fp32 EPSS / sway grid (a 16-bit model's grid, in its dtype)."""
    text = inp["text"]
    pre = ref_cpu.prepare(arch, inp["cond"].float(), text, inp["duration"], inp["lens"])
    fwd = ref_cpu.dit_forward if arch["backbone"] == "DiT" else ref_cpu.unett_forward
    cache = {}

    def fn(t, x):
        if cfg_strength < 1e-5:
            return fwd(W, arch, x, pre["step_cond"], text, t, pre["mask"], cache, packed=False)
        pc, pu = torch.chunk(fwd(W, arch, x, pre["step_cond"], text, t, pre["mask"], cache), 2, 0)
        return pc + (pc - pu) * cfg_strength

    traj = integrate(fn, y0.float(), ref_cpu.epss_sway_grid(steps, sway) if t is None else t, method)
    return torch.where(pre["cond_mask"], pre["cond"], traj[-1]), traj, pre


def noise_for(inp, seed):
    dur = torch.maximum(torch.maximum((inp["text"] != -1).sum(-1), inp["lens"]) + 1, inp["duration"])
    return synthetic.reference_noise(dur, seed)


@functools.lru_cache(maxsize=None)
def case(arch_tag, spec_items, steps, cfg_strength, sway, method, seed=7):
    """One oracle run per (case, method), shared by the tests that compare with it: dict of arch, inputs, y0 and
    the fp32 out / traj. spec_items: tuple(sorted(spec.items())) with lists as tuples (hashable)."""
    import golden_cases as gc

    arch = gc.arch_of(arch_tag)
    spec = {k: (list(v) if isinstance(v, tuple) else v) for k, v in spec_items}
    inp = synthetic.make_case(**spec)
    y0 = noise_for(inp, seed)
    W = synthetic.make_weights_torch(arch)
    out, traj, pre = cfm_sample(W, arch, inp, y0, steps, cfg_strength, sway, method)
    return dict(arch=arch, inp=inp, y0=y0, out=out, traj=traj, cond=pre["cond"], cond_mask=pre["cond_mask"])


def spec_key(spec):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in spec.items()))
