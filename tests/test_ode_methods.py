"""The fixed-grid midpoint and rk4 solvers, host side (no GPU): model construction through every layer of the
Python surface, the stage times (`ode_eval_times`, and the engine's own derivation through the C ABI), the
tableau the solver kernel is instantiated with, and the scalar behaviour of the stepper that the GPU tests
(tests/test_gpu_ode_methods.py) use as their reference."""

import ctypes

import numpy as np
import pytest
import torch

import golden_cases as gc
import ode_reference as ode
from f5_tts_amd import _lib, checkpoint, synthetic
from f5_tts_amd.model import CFM, DiT
from f5_tts_amd.model.utils import ode_eval_times, time_grid

METHODS = ("euler", "midpoint", "rk4")
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


def _net():
    arch = gc.arch_of("tiny")
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    return DiT(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"]), arch


# ---------------------------------------------------------------- construction
@pytest.mark.parametrize("method", ["midpoint", "rk4"])
def test_cfm_constructs_with_the_fixed_grid_solvers(method):
    net, _ = _net()
    m = CFM(transformer=net, num_channels=100, odeint_kwargs=dict(method=method))
    assert m.ode_method == method
    assert m.odeint_kwargs == dict(method=method)


def test_cfm_default_is_euler():
    net, _ = _net()
    assert CFM(transformer=net, num_channels=100).ode_method == "euler"


@pytest.mark.parametrize("kwargs", [dict(method="dopri5"), dict(method="euler", options=dict(step_size=0.1))])
def test_cfm_refuses_what_would_not_be_the_fixed_grid(kwargs):
    net, _ = _net()
    with pytest.raises(NotImplementedError) as ei:
        CFM(transformer=net, num_channels=100, odeint_kwargs=kwargs)
    for name in METHODS:
        assert name in str(ei.value)


def test_load_model_builds_a_midpoint_model(tmp_path):
    net, arch = _net()
    W = synthetic.make_weights_torch(arch)
    W["rotary_embed.inv_freq"] = net.state_dict()["rotary_embed.inv_freq"].clone()
    ckpt = tmp_path / "raw.pt"
    torch.save({"model_state_dict": {f"transformer.{k}": v for k, v in W.items()}}, str(ckpt))
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("".join(f"tok{i}\n" for i in range(arch["text_num_embeds"])), encoding="utf-8")
    cfg = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    m = checkpoint.load_model(DiT, cfg, str(ckpt), vocab_file=str(vocab), ode_method="midpoint", use_ema=False,
                              device="cpu")
    assert m.ode_method == "midpoint"


# ---------------------------------------------------------------- stage times
def _grids(dtype):
    return [time_grid(4, -1.0, True, device="cpu", dtype=dtype),  # EPSS + sway(-1), steps 4
            time_grid(5, None, False, device="cpu", dtype=dtype)]  # linspace


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_ode_eval_times_are_the_closed_forms_in_the_grid_dtype(dtype):
    for t in _grids(dtype):
        steps = t.numel() - 1
        assert torch.equal(ode_eval_times(t, "euler"), t[:-1])
        mid = ode_eval_times(t, "midpoint").reshape(steps, 2)
        rk = ode_eval_times(t, "rk4").reshape(steps, 4)
        assert mid.dtype == dtype and rk.dtype == dtype
        for k in range(steps):  # the same computation on 0-dim tensors of that dtype, as torchdiffeq steps
            t0, t1 = t[k], t[k + 1]
            dt = t1 - t0
            assert torch.equal(mid[k], torch.stack([t0, t0 + 0.5 * dt]))
            assert torch.equal(rk[k], torch.stack([t0, t0 + dt * (1 / 3), t0 + dt * (2 / 3), t1]))
            assert rk[k, 3].item() == t[k + 1].item()  # the grid value itself, not t0 + dt


def test_ode_eval_times_refuses_other_methods():
    with pytest.raises(NotImplementedError):
        ode_eval_times(torch.linspace(0, 1, 3), "dopri5")


@pytest.mark.parametrize("compute,dtype", [("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16),
                                           ("bf16", torch.float32), ("fp16", torch.float32)])
@pytest.mark.parametrize("method", METHODS)
def test_engine_derives_the_same_stage_times(method, compute, dtype):
    """f5h_sample_ode takes the step grid and derives the stage times itself (host code, reached here through
    f5h_debug_ode_eval_times): bit for bit `ode_eval_times` in the dtype the grid was built in -- the engine's
    16-bit operand dtype for a model in its own precision, fp32 for fp32 parameters under a compute override."""
    L = _lib.lib()
    grids = _grids(dtype) + [time_grid(32, -1.0, True, device="cpu", dtype=dtype),
                             torch.rand(40, dtype=torch.float32, generator=torch.Generator().manual_seed(3))
                             .sort().values.to(dtype)]
    for t in grids:
        steps = t.numel() - 1
        tg = np.ascontiguousarray(t.float().numpy())
        out = np.zeros(steps * STAGES[method], dtype=np.float32)
        fp = ctypes.POINTER(ctypes.c_float)
        _lib.check(L.f5h_debug_ode_eval_times(_lib.ODE_METHOD[method], _lib.COMPUTE[compute], tg.ctypes.data_as(fp),
                                              steps, out.ctypes.data_as(fp)))
        want = ode_eval_times(t, method).float().numpy()
        assert np.array_equal(out, want), (method, compute, steps)


# ---------------------------------------------------------------- tableau
def _tableau(method):
    stages = ctypes.c_int32()
    c, a, b = (ctypes.c_float * 4)(), (ctypes.c_float * 16)(), (ctypes.c_float * 4)()
    _lib.check(_lib.lib().f5h_debug_ode_tableau(_lib.ODE_METHOD[method], ctypes.byref(stages), c, a, b))
    return stages.value, np.array(c[:]), np.array(a[:]).reshape(4, 4), np.array(b[:])


@pytest.mark.parametrize("method", METHODS)
def test_kernel_tableau(method):
    stages, c, a, b = _tableau(method)
    assert stages == STAGES[method]
    f32 = np.float32
    third, two_thirds = f32(1 / 3), f32(2 / 3)
    want = {
        "euler": ([0], [[0]], [1]),
        "midpoint": ([0, 0.5], [[0, 0], [0.5, 0]], [0, 1]),
        "rk4": ([0, third, two_thirds, 1],
                [[0, 0, 0, 0], [third, 0, 0, 0], [-third, 1, 0, 0], [1, -1, 1, 0]],
                [0.125, 0.375, 0.375, 0.125]),
    }[method]
    wc, wa, wb = np.zeros(4, f32), np.zeros((4, 4), f32), np.zeros(4, f32)
    wc[:stages], wa[:stages, :stages], wb[:stages] = want
    assert np.array_equal(c, wc) and np.array_equal(a, wa) and np.array_equal(b, wb)
    assert b.sum() == 1.0
    assert np.all(np.triu(a) == 0)  # explicit
    # consistency: each stage's row sum is its time (to one fp32 rounding: 2/3 and 1 - 1/3 round apart)
    assert np.abs(a.astype(np.float64).sum(1) - c).max() <= 2.0 ** -24


def test_tableau_refuses_unknown_method():
    assert _lib.lib().f5h_debug_ode_tableau(3, None, None, None, None) != 0


# ---------------------------------------------------------------- the reference stepper's own check
@pytest.mark.parametrize("method", METHODS)
def test_reference_stepper_on_linear_decay(method):
    """y' = -y on 8 linspace steps: every step multiplies y by the method's amplification factor (euler 1 - dt,
    midpoint 1 - dt + dt^2/2, rk4 the 4-term Taylor factor), which pins the stepper the GPU tests compare with."""
    t = torch.linspace(0, 1, 9, dtype=torch.float64)
    y0 = torch.tensor([1.0, -2.5, 0.3], dtype=torch.float64)
    seen = []

    def f(tt, y):
        seen.append(float(tt))
        return -y

    traj = ode.integrate(f, y0, t, method)
    assert traj.shape == (9, 3) and torch.equal(traj[0], y0)
    dt = 1 / 8
    amp = {"euler": 1 - dt, "midpoint": 1 - dt + dt ** 2 / 2,
           "rk4": 1 - dt + dt ** 2 / 2 - dt ** 3 / 6 + dt ** 4 / 24}[method]
    for k in range(8):
        assert torch.allclose(traj[k + 1], traj[k] * amp, rtol=1e-14, atol=0)
    assert np.allclose(seen, ode_eval_times(t, method).numpy(), rtol=0, atol=1e-15)


def test_oracle_solvers_differ_enough_to_be_told_apart():
    """The GPU tests' bounds (1e-3 max-rel in fp32, 5e-2 rel-L2 in 16 bit) discriminate: at their masked-batch case
    (tiny DiT, B = 3, 3 steps, CFG 2, sway -1) the oracle outputs of any two solvers are >= 0.15 rel-L2 apart."""
    outs = {m: ode.case("tiny", ode.spec_key(gc.B3), 3, 2.0, -1.0, m, gc.SEED)["out"].numpy() for m in METHODS}
    for a, b in (("euler", "midpoint"), ("euler", "rk4"), ("midpoint", "rk4")):
        assert gc.rel_err(outs[a], outs[b]) >= 0.15, (a, b)
