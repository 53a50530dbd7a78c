"""The on-device midpoint and rk4 solvers of the CFM sampler (f5h_sample_ode, cfg_rk_kernel) against the CPU
oracle composed with the same solver (tests/ode_reference.py), plus what the evaluation-indexed step graph
must keep: Euler through the new entry bit for bit, graph == eager, replay counts, per-method graph keys, the
512-evaluation limit, and the LayerNorm fold and phase chain beside a multi-stage solver.

Bounds: fp32 mode max|diff| / max|ref| < 1e-3 (the project's fp32 contract); 16-bit modes rel-L2 <= 5e-2 against
the method's own fp32 oracle (the bound test_edge_sample_matches_reference uses). At these shapes the three
solvers' oracle outputs are 0.06-0.16 rel-L2 apart, so either bound tells a wrong solver from a right one."""

import ctypes

import numpy as np
import pytest
import torch

import golden_cases as gc
import ode_reference as ode
from f5_tts_amd import _lib, synthetic
from f5_tts_amd.model import CFM, DiT, UNetT
from f5_tts_amd.model.utils import time_grid

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3
BF16_TOL = 5e-2
DEV = "cuda:0"
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
SOLVERS = ["midpoint", "rk4"]

B2_200 = dict(B=2, ref_frames=[60, 80], total_frames=[200, 200], n_text=[20, 30], vocab=64)
# name -> (arch tag, input spec, steps, cfg): the path each one covers is in the parity test's docstring
CASES = {
    "dit_b3": ("tiny", gc.B3, 3, 2.0),
    "unett_b1": ("utiny", gc.B1, 2, 2.0),
    "dit_nocfg_b3": ("tiny", gc.B3, 3, 0.0),
    "dit_short": ("tiny", gc.SHORT, 3, 2.0),
    "dit_b2_200": ("tiny", B2_200, 1, 2.0),
    "unett_b3": ("utiny", gc.B3, 3, 2.0),
    "dit_b1": ("tiny", gc.B1, 3, 2.0),
}
SWAY = -1.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ref(name, method):
    tag, spec, steps, cfg = CASES[name]
    return ode.case(tag, ode.spec_key(spec), steps, cfg, SWAY, method, gc.SEED)


def _model(arch, compute, method):
    cls = DiT if arch["backbone"] == "DiT" else UNetT
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = cls(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    return CFM(transformer=net, num_channels=100, compute=compute, odeint_kwargs=dict(method=method)).to(DEV)


def _sample(m, ref, steps, cfg, keep_trajectory=True):
    inp = ref["inp"]
    out, traj = m.sample(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=inp["duration"].to(DEV),
                         lens=inp["lens"].to(DEV), steps=steps, cfg_strength=cfg, sway_sampling_coef=SWAY,
                         y0=ref["y0"].to(DEV), keep_trajectory=keep_trajectory)
    torch.cuda.synchronize()
    return out, traj


def _engine_args(ref, steps):
    """Engine.sample's tensors for a case, from the oracle's host preamble (cfm.py:111-158)."""
    inp = ref["inp"]
    t = time_grid(steps, SWAY, True, device="cpu", dtype=torch.float32).numpy()
    return dict(cond=ref["cond"].to(DEV), cond_mask=ref["cond_mask"][..., 0].to(DEV), text=inp["text"].to(DEV),
                duration=torch.maximum(torch.maximum((inp["text"] != -1).sum(-1), inp["lens"]) + 1,
                                       inp["duration"]).to(DEV),
                y0=ref["y0"].to(DEV), t_grid=t, use_batch_mask=ref["cond"].shape[0] > 1)


# ---------------------------------------------------------------- 1. fp32 parity
@pytest.mark.parametrize("method", SOLVERS)
@pytest.mark.parametrize("name", ["dit_b3", "unett_b1", "dit_nocfg_b3", "dit_short", "dit_b2_200"])
def test_fp32_parity_with_the_oracle(name, method):
    """dit_b3: a masked batch. unett_b1: prediction rows offset by the time token. dit_nocfg_b3: cfg 0, S = B.
    dit_short: 5 frames, fewer elements than one workgroup's threads. dit_b2_200: B N mel = 40,000 > 128 x 256, so
    the grid-stride loop runs; one step, so the call's first evaluation is also a step's first stage."""
    _need_gpu()
    tag, spec, steps, cfg = CASES[name]
    ref = _ref(name, method)
    out, traj = _sample(_model(ref["arch"], "fp32", method), ref, steps, cfg)
    out, traj = out.float().cpu(), traj.float().cpu()
    errs = {k: gc.max_rel(a.numpy(), b.numpy())
            for k, a, b in (("out", out, ref["out"]), ("traj[1]", traj[1], ref["traj"][1]),
                            ("traj[-1]", traj[-1], ref["traj"][-1]))}
    print(f"{name} {method}: max-rel {errs}")
    assert traj.shape[0] == steps + 1 and traj.shape == ref["traj"].shape
    assert torch.equal(traj[0], ref["y0"])
    for i, L in enumerate(ref["inp"]["lens"].tolist()):
        assert torch.equal(out[i, :L], ref["inp"]["cond"][i, :L])
    for k, e in errs.items():
        assert e < FP32_TOL, (k, e)


# ---------------------------------------------------------------- 2. Euler through the new entry
def test_euler_through_sample_ode_is_bitwise_f5h_sample():
    _need_gpu()
    tag, spec, steps, cfg = CASES["dit_b3"]
    ref = _ref("dit_b3", "euler")
    m = _model(ref["arch"], "fp32", "euler")
    eng = m.transformer.get_engine("fp32", m.device)
    kw = _engine_args(ref, steps)
    out, traj = eng.sample(cfg_strength=cfg, method="euler", **kw)
    B, N, mel = kw["cond"].shape
    nt = kw["text"].shape[1]
    L = _lib.lib()
    assert L.f5h_workspace_size_ode(eng._h, B, N, nt, steps, 1, _lib.F5H_EULER) == \
        L.f5h_workspace_size(eng._h, B, N, nt, steps, 1)
    ws = torch.empty(L.f5h_workspace_size(eng._h, B, N, nt, steps, 1), dtype=torch.uint8, device=DEV)
    cond, cmask = kw["cond"].float().contiguous(), kw["cond_mask"].to(torch.uint8).contiguous()
    text, dur = kw["text"].to(torch.int64).contiguous(), kw["duration"].to(torch.int32).contiguous()
    y0 = kw["y0"].float().contiguous()
    tg = np.ascontiguousarray(kw["t_grid"], dtype=np.float32)
    out2 = torch.empty_like(out)
    traj2 = torch.empty_like(traj)
    a = _lib.SampleArgs()
    a.B, a.N, a.nt, a.nfe = B, N, nt, steps
    a.cond, a.cond_mask, a.text, a.duration, a.y0 = (cond.data_ptr(), cmask.data_ptr(), text.data_ptr(),
                                                     dur.data_ptr(), y0.data_ptr())
    a.t_grid = tg.ctypes.data
    a.cfg_strength = cfg
    a.use_batch_mask = 1
    a.out, a.trajectory = out2.data_ptr(), traj2.data_ptr()
    with torch.cuda.device(DEV):
        _lib.check(L.f5h_sample(eng._h, _lib.stream_handle(torch.device(DEV)), ctypes.byref(a), ws.data_ptr(),
                                ws.numel()), "f5h_sample")
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(traj, traj2)
    assert gc.max_rel(out.cpu().numpy(), ref["out"].numpy()) < FP32_TOL


# ---------------------------------------------------------------- 3. graph, replay, keying
@pytest.mark.parametrize("method", SOLVERS)
@pytest.mark.parametrize("name", ["dit_b3", "unett_b3"])
def test_evaluation_graph_bitwise_equals_eager_and_replays(name, method):
    """One captured evaluation (backbone + cfg_rk) replayed steps x stages times equals the eager launches bit for
    bit; the third call of a shape captures nothing, replays steps x stages evaluations and the prologue graph,
    and equals the first."""
    _need_gpu()
    tag, spec, steps, cfg = CASES[name]
    ref = _ref(name, method)
    m = _model(ref["arch"], "bf16", method)
    eng = m.transformer.get_engine("bf16", m.device)

    def run():
        out, traj = _sample(m, ref, steps, cfg)
        return out.clone(), traj.clone(), eng.graph_stats()

    eng.set_graph_mode(False)
    o_e, t_e, _ = run()
    eng.set_graph_mode(True)
    s0 = eng.graph_stats()
    o1, t1, s1 = run()
    o2, t2, s2 = run()
    o3, t3, s3 = run()
    for o, t in ((o1, t1), (o2, t2), (o3, t3)):
        assert torch.equal(o, o_e) and torch.equal(t, t_e)
    assert s1["captures"] == s0["captures"] + 1  # the evaluation graph
    assert s2["captures"] == s1["captures"] + 1  # the shape repeats: its prologue graph
    assert s3["captures"] == s2["captures"], "third call on the same shape must replay"
    assert s3["replays"] - s2["replays"] == steps * STAGES[method] + 1
    assert gc.rel_err(o_e.float().cpu().numpy(), ref["out"].numpy()) <= BF16_TOL


@pytest.mark.parametrize("name", ["dit_b3", "unett_b3"])
def test_methods_on_one_workspace_never_share_a_graph(name):
    _need_gpu()
    tag, spec, steps, cfg = CASES[name]
    ref = _ref(name, "euler")
    m = _model(ref["arch"], "bf16", "euler")
    eng = m.transformer.get_engine("bf16", m.device)
    kw = _engine_args(ref, steps)
    B, N, _ = kw["cond"].shape
    need = max(eng.workspace_bytes(B, N, kw["text"].shape[1], steps, True, mth) for mth in STAGES)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    caps, outs = [eng.graph_stats()["captures"]], []
    for mth in ("midpoint", "rk4", "euler", "midpoint"):
        out, traj = eng.sample(cfg_strength=cfg, method=mth, workspace=ws, **kw)
        torch.cuda.synchronize()
        outs.append((out.clone(), traj.clone()))
        caps.append(eng.graph_stats()["captures"])
    assert [b - a for a, b in zip(caps, caps[1:])] == [1, 1, 1, 1]  # three step graphs, then midpoint's prologue
    assert torch.equal(outs[0][0], outs[3][0]) and torch.equal(outs[0][1], outs[3][1])
    for i, mth in enumerate(("midpoint", "rk4", "euler")):
        assert gc.rel_err(outs[i][0].cpu().numpy(), _ref(name, mth)["out"].numpy()) <= BF16_TOL, mth


# ---------------------------------------------------------------- 4. 16-bit modes
@pytest.mark.parametrize("method", SOLVERS)
@pytest.mark.parametrize("compute", ["bf16", "fp16"])
def test_16bit_modes_stay_within_the_bound_of_their_own_oracle(compute, method):
    _need_gpu()
    tag, spec, steps, cfg = CASES["dit_b3"]
    ref = _ref("dit_b3", method)
    out, _ = _sample(_model(ref["arch"], compute, method), ref, steps, cfg, keep_trajectory=False)
    err = gc.rel_err(out.float().cpu().numpy(), ref["out"].numpy())
    print(f"dit_b3 {method} {compute}: rel-L2 {err:.3e}")
    assert err <= BF16_TOL, err


def test_16bit_parameters_round_the_stage_times_in_their_dtype():
    """A bf16 model builds its grid in bf16 (cfm.py:211-216), as the reference does, and the engine then rounds the
    stage times to bf16 as torchdiffeq would. The reference here is the fp32 oracle on that bf16 grid and its
    bf16-formed stage times (against the fp32 grid's oracle the grid's own rounding, 2^-9 in t under a 1000 t
    sinusoidal embedding of random weights, is the larger part of the difference: 5.2e-2 measured), so what is left
    is the engine's 16-bit arithmetic and the 16-bit bound applies."""
    _need_gpu()
    tag, spec, steps, cfg = CASES["dit_b3"]
    base = _ref("dit_b3", "midpoint")
    t16 = time_grid(steps, SWAY, True, device="cpu", dtype=torch.bfloat16)
    want, _, _ = ode.cfm_sample(synthetic.make_weights_torch(base["arch"]), base["arch"], base["inp"], base["y0"],
                                steps, cfg, SWAY, "midpoint", t=t16)
    m = _model(base["arch"], "auto", "midpoint").to(torch.bfloat16)
    assert m.engine_compute() == "bf16"
    out, _ = _sample(m, base, steps, cfg, keep_trajectory=False)
    assert out.dtype == torch.bfloat16
    err = gc.rel_err(out.float().cpu().numpy(), want.numpy())
    print(f"dit_b3 midpoint, bf16 parameters and grid: rel-L2 {err:.3e} (fp32-grid oracle: "
          f"{gc.rel_err(out.float().cpu().numpy(), base['out'].numpy()):.3e})")
    assert err <= BF16_TOL, err


# ---------------------------------------------------------------- 5. evaluation-count limit
def test_rk4_evaluation_limit():
    """The per-call time tables hold 512 rows: rk4 runs 128 steps (512 evaluations) and refuses 129."""
    _need_gpu()
    tag, spec, _, cfg = CASES["dit_short"]
    ref = _ref("dit_short", "rk4")
    m = _model(ref["arch"], "bf16", "rk4")
    with pytest.raises(RuntimeError, match=r"129 steps x 4 stages = 516 backbone evaluations exceed the 512 rows"):
        _sample(m, ref, 129, cfg)
    out, traj = _sample(m, ref, 128, cfg)
    assert traj.shape[0] == 129
    assert torch.isfinite(out).all() and torch.isfinite(traj).all()


# ---------------------------------------------------------------- 6. LayerNorm fold and phase chain
def test_midpoint_with_ln_fold():
    """B = 1 DiT with dim a multiple of 64, the fold's path: its per-evaluation u / v rows come from the
    evaluation-indexed AdaLN table, and midpoint stays in the 16-bit bound with the fold on and off."""
    _need_gpu()
    tag, spec, steps, cfg = CASES["dit_b1"]
    ref = _ref("dit_b1", "midpoint")
    m = _model(ref["arch"], "bf16", "midpoint")
    eng = m.transformer.get_engine("bf16", m.device)
    assert eng.ln_fold_stats()[0], "the tiny DiT must be able to fold"
    try:
        for fold in (True, False):
            eng.set_ln_fold(fold)
            n0 = eng.ln_fold_stats()[1]
            out, _ = _sample(m, ref, steps, cfg, keep_trajectory=False)
            assert (eng.ln_fold_stats()[1] > n0) == fold
            err = gc.rel_err(out.float().cpu().numpy(), ref["out"].numpy())
            print(f"dit_b1 midpoint bf16, LayerNorm fold {fold}: rel-L2 {err:.3e}")
            assert err <= BF16_TOL, (fold, err)
    finally:
        eng.set_ln_fold(True)


def test_midpoint_is_bitwise_independent_of_the_phase_chain():
    """The chain runs at dim 1024 only: a 3-layer Base DiT, B = 1, 149 frames (a ragged row count), fold off. The
    chained evaluation graph, captured once and replayed by a second call, gives the separate launches' bits."""
    _need_gpu()
    from f5_tts_amd import configs

    arch = configs.get_arch("F5TTS_v1_Base", depth=3)
    m = _model(arch, "bf16", "midpoint")
    eng = m.transformer.get_engine("bf16", m.device)
    inp = synthetic.make_case(B=1, ref_frames=[37], total_frames=[149], n_text=[20], vocab=arch["text_num_embeds"])
    ref = dict(inp=inp, y0=ode.noise_for(inp, 3))
    steps, cfg = 2, 2.0
    try:
        eng.set_ln_fold(False)
        eng.set_chain(False)
        plain = [t.clone() for t in _sample(m, ref, steps, cfg)]
        assert eng.chain_stats()[0] == 0
        eng.set_chain(True)
        for rep in range(2):  # the capturing call, then a replaying one
            n0 = eng.chain_stats()[0]
            out, traj = _sample(m, ref, steps, cfg)
            n1, fault, _ = eng.chain_stats()
            assert fault == 0
            assert n1 - n0 == (arch["depth"] if rep == 0 else 0)  # one chained evaluation graph for the call
            assert torch.equal(out, plain[0]) and torch.equal(traj, plain[1]), rep
        assert torch.isfinite(plain[0]).all()
    finally:
        eng.set_chain(False)
        eng.set_ln_fold(True)
