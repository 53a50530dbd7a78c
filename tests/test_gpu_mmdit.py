"""MMDiT on the GPU: the two kernel changes it needs at the op level (the QKV epilogue's destination panel length and
the attention's split output), then the backbone end to end against the fixtures the reference produced
(tests/golden/make_golden_mmdit.py) and the CPU restatement (tests/mmdit_reference.py).

fp32 contract: max-rel < 1e-3 against the reference's fp32 output. 16-bit modes: the rule of tests/test_gpu_envelope.py
(rel-L2 over the generated frames at most 1.5 x the reference's own error in that dtype, and the measured value + 25 %)."""

import numpy as np
import pytest
import torch

import dit_options_reference as D
import golden_cases as gc
import mmdit_reference as mr
import ode_reference
import op_cases as C
import op_reference as R
from f5_tts_amd import configs, synthetic
from f5_tts_amd.engine import gemm_force_config, op_attention, op_attention_split, op_gemm_epi, store_policy_force
from f5_tts_amd.model import CFM, MMDiT
from test_gpu_contract import _plugin_euler
from test_gpu_parity import GEMM_CONFIGS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
FP32_TOL = 1e-3
MARGIN = 1.5
# The engine's own rel-L2 error over the generated frames against the reference's fp32 output, as measured on MI355X
# (the kernels are deterministic); each case must stay within its value + 25 %. Reference's own error
# in the dtype (e_ref) beside it.
MEASURED = {
    ("mmdit_tiny_sample_b3", "bf16"): 0.00688902,   # e_ref 0.07869
    ("mmdit_tiny_sample_b3", "fp16"): 0.000860614,  # e_ref 0.01454
    ("mmdit_wide_sample_b2", "bf16"): 0.00787749,   # e_ref 0.05303
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------- 1. QKV scatter into joint panels
QKV_K, QKV_S = 128, 2
QKV_SHAPES = [(70, 23), (150, 30)]   # (N, nt): ragged in every row tile; more than one 64 / 128-row tile per stream


def _qkv_stream(compute, H, L, bias_on, norm, key):
    g = C._gen(23, H, L, bias_on, norm, key)
    M, N = QKV_S * L, 3 * H * 64
    A = torch.randn(M, QKV_K, generator=g)
    W = torch.randn(N, QKV_K, generator=g) / QKV_K ** 0.5
    bias = torch.randn(N, generator=g) if bias_on else None
    c = dict(A=A, W=W, bias=bias, A_read=R.rnd(A, compute), W_read=R.rnd(W, compute), H=H, rope_heads=H,
             q_scale=C.Q_SCALE, L=L, u_out=R.U_OUT[compute])
    if norm:
        c["wq"] = 1.0 + 0.3 * torch.randn(64, generator=g)
        c["wk"] = 1.0 + 0.3 * torch.randn(64, generator=g)
    return c


def _qkv_launch(c, compute, **kw):
    norm = dict(q_norm_w=c["wq"], k_norm_w=c["wk"], qk_norm_eps=D.QK_EPS) if "wq" in c else {}
    return op_gemm_epi("qkv", c["A"].to(DEV), c["W"].to(DEV), bias=c["bias"], compute=compute, seq_len=c["L"],
                       heads=c["H"], rope_heads=c["rope_heads"], q_scale=c["q_scale"], **norm, **kw)


def _qkv_joint(ca, ct, compute, N, nt):
    """The audio launch then the text launch into one NaN-filled joint buffer, and each stream's own launch with
    qkv_dst_len = 0; checks ownership after the first launch. Returns ((q, k, v) joint, audio alone, text alone)."""
    H, Lj = ca["H"], N + nt
    bufs = tuple(torch.full((QKV_S, H, Lj, 64), float("nan"), dtype=torch.float32, device=DEV) for _ in range(3))
    _qkv_launch(ca, compute, qkv_dst_len=Lj, qkv_bufs=bufs, qkv_row0=0)
    for t in bufs:  # the audio launch owns rows [0, N) of every panel and touches nothing else
        assert not torch.isnan(t[:, :, :N]).any() and torch.isnan(t[:, :, N:]).all()
    after_audio = tuple(t.clone() for t in bufs)
    _qkv_launch(ct, compute, qkv_dst_len=Lj, qkv_bufs=bufs, qkv_row0=N)
    for t, t0 in zip(bufs, after_audio):
        assert not torch.isnan(t).any()
        assert _bits_equal(t[:, :, :N], t0[:, :, :N]), "the text launch changed audio rows"
    alone_a = _qkv_launch(ca, compute)
    alone_t = _qkv_launch(ct, compute)
    return tuple(t.cpu() for t in bufs), tuple(t.cpu() for t in alone_a), tuple(t.cpu() for t in alone_t)


@pytest.mark.parametrize("compute", C.COMPUTES)
# N = 384: the strip epilogue of the 128-column tiles; 576: the general one; 768: whole 256-column tiles, so the forced
# 256x256 configurations (11, 12, 13) run their own strip / register-only epilogues
@pytest.mark.parametrize("H", [2, 3, 4])
@pytest.mark.parametrize("bias_on,norm", [(True, False), (False, False), (True, True), (False, True)])
def test_qkv_scatter_into_joint_panels(compute, H, bias_on, norm):
    _need_gpu()
    cfgs = GEMM_CONFIGS if compute != "fp32" else [-1]
    pols = (0, 1) if compute != "fp32" else (-1,)
    for N, nt in QKV_SHAPES:
        ca = _qkv_stream(compute, H, N, bias_on, norm, 0)
        ct = _qkv_stream(compute, H, nt, bias_on, norm, 1)
        first = None
        try:
            for cfg in cfgs:
                gemm_force_config(cfg)
                for pol in pols:
                    store_policy_force(pol)
                    joint, alone_a, alone_t = _qkv_joint(ca, ct, compute, N, nt)
                    for j, a, t in zip(joint, alone_a[:3], alone_t[:3]):
                        assert _bits_equal(j[:, :, :N], a), f"audio rows differ from the qkv_dst_len = 0 launch {cfg, pol}"
                        assert _bits_equal(j[:, :, N:], t), f"text rows differ from the qkv_dst_len = 0 launch {cfg, pol}"
                    if first is None:
                        first = (alone_a, alone_t)
                    for o, o0 in zip(alone_a[:3] + alone_t[:3], first[0][:3] + first[1][:3]):
                        assert _bits_equal(o, o0), f"(config, store policy) {cfg, pol} differs from configuration 0"
        finally:
            gemm_force_config(-1)
            store_policy_force(-1)
        # today's reference check on today's path (each stream's launch with qkv_dst_len = 0)
        for c, (q, k, v, rope), nm in ((ca, first[0], "audio"), (ct, first[1], "text")):
            if norm:
                r64, r32 = D.qkn_ref(c, rope, F64), D.qkn_ref(c, rope, F32)
            else:
                r64, r32 = (R.gemm_epi("qkv", c["A_read"], c["W_read"], c["bias"], seq_len=c["L"], heads=H, rope_heads=H,
                                       q_scale=c["q_scale"], rope=rope, dtype=dt) for dt in (F64, F32))
            for n1, o, a, b in zip("qkv", (q, k, v), r64, r32):
                R.assert_close(o, a, b, c["u_out"], f"qkv_joint/{compute}/{nm}-{n1}-H{H}-N{N}-nt{nt}-b{int(bias_on)}-n{int(norm)}")


def test_qkv_dst_len_refusals():
    _need_gpu()
    c = _qkv_stream("bf16", 2, 70, True, False, 0)
    with pytest.raises(RuntimeError, match="qkv_dst_len"):  # a fold consumer with destination panels: refused
        op_gemm_epi("qkv", c["A"].to(DEV), c["W"].to(DEV), compute="bf16", seq_len=70, heads=2, qkv_dst_len=70,
                    qkv_bufs=tuple(torch.zeros(2, 2, 70, 64, device=DEV) for _ in range(3)), ln_nparts=2,
                    ln_part_in=torch.zeros(140, 2, 2, device=DEV), ln_u=torch.zeros(384, device=DEV),
                    ln_v=torch.zeros(384, device=DEV))


# ---------------------------------------------------------------- 2. attention with a split output
ATTN_SHAPES = [(93, 70), (96, 64), (300, 262)]  # (L, split): inside a wave's 32 rows, on a wave boundary, in block 1


@pytest.mark.parametrize("compute", C.COMPUTES)
@pytest.mark.parametrize("L,split", ATTN_SHAPES)
def test_attention_split_output(compute, L, split):
    _need_gpu()
    S, H = 2, 2
    g = C._gen(29, L, split)
    q, k, v = (torch.randn(S, H, L, 64, generator=g).to(DEV) for _ in range(3))
    try:
        for pol in ((0, 1) if compute != "fp32" else (-1,)):
            store_policy_force(pol)
            for pre in (False, True):  # the engine's form (prescaled q) has the write-through variant
                whole = op_attention(q, k, v, compute=compute, q_prescaled=pre)
                o, o2, ws = op_attention_split(q, k, v, split, compute=compute, q_prescaled=pre, poison=True,
                                               return_ws=True)
                assert not torch.isnan(o).any() and not torch.isnan(o2).any()
                assert _bits_equal(o, whole[:, :split]) and _bits_equal(o2, whole[:, split:]), (pol, pre)
                # nothing written past either buffer: the poisoned bytes behind the 16-bit o | o2 stay 0xFF (in the
                # fp32 mode the kernel writes the callers' buffers, whose sizes are exact, and the workspace not at all)
                tail = ws[q.numel() * 8:] if compute != "fp32" else ws
                assert bool((tail == 0xFF).all())
    finally:
        store_policy_force(-1)


# ---------------------------------------------------------------- end to end
def _model(arch, compute, W=None, method="euler"):
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = MMDiT(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    missing, unexpected = net.load_state_dict(synthetic.make_weights_torch(arch) if W is None else W, strict=False)
    assert not unexpected and all(k.endswith("inv_freq") for k in missing), (missing, unexpected)
    return CFM(transformer=net, num_channels=100, compute=compute, odeint_kwargs=dict(method=method)).to(DEV)


def _sample(m, name, spec=None):
    tag, spec0, nfe, sway, cfg, _ = mr.SAMPLE_CASES[name]
    inp, y0 = mr.sample_inputs(spec or spec0)
    out, _ = m.sample(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=inp["duration"].to(DEV),
                      lens=inp["lens"].to(DEV), steps=nfe, cfg_strength=cfg, sway_sampling_coef=sway, y0=y0.to(DEV),
                      keep_trajectory=False)
    torch.cuda.synchronize()
    return out.float().cpu()


def _forward(net, name):
    tag, spec, opts = mr.FORWARD_CASES[name]
    fi = mr.forward_inputs(spec)
    mask = None if fi["mask"] is None else fi["mask"].to(DEV)
    t = torch.tensor(opts.get("t", gc.FWD_T), device=DEV)
    out = net(fi["x"].to(DEV), fi["cond"].to(DEV), fi["text"].to(DEV), t, mask=mask,
              cfg_infer=opts.get("cfg_infer", True), drop_audio_cond=opts.get("drop_audio", False),
              drop_text=opts.get("drop_text", False))
    torch.cuda.synchronize()
    return out.float().cpu().numpy()


# 3. fp32 against every fp32 fixture (the wide case and the 1030-token forward included)
@pytest.mark.parametrize("name", mr.FP32_SAMPLES)
def test_fp32_sample_matches_reference(name):
    _need_gpu()
    m = _model(mr.arch_of(mr.SAMPLE_CASES[name][0]), "fp32")
    out = _sample(m, name).numpy()
    err = gc.max_rel(out, gc.load(name)["out"])
    print(f"{name} [fp32]: max-rel {err:.3e}")
    assert np.isfinite(out).all() and err < FP32_TOL


@pytest.mark.parametrize("name", list(mr.FORWARD_CASES))
def test_fp32_forward_matches_reference(name):
    """Packed, single-branch, drop-flag and per-sample-time forwards through the plugin (7.), and the position clamp."""
    _need_gpu()
    m = _model(mr.arch_of(mr.FORWARD_CASES[name][0]), "fp32")
    err = gc.max_rel(_forward(m.transformer, name), gc.load(name)["out"])
    print(f"{name} [fp32]: max-rel {err:.3e}")
    assert err < FP32_TOL


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["mmdit_tiny_sample_b1", "mmdit_tiny_sample_b3", "mmdit_tiny_qknorm_sample_b3",
                                  "mmdit_tiny_nocfg_b3"])
def test_tile_configurations_agree_bitwise(name, compute):
    _need_gpu()
    m = _model(mr.arch_of(mr.SAMPLE_CASES[name][0]), compute)
    outs = []
    try:
        for cfg in GEMM_CONFIGS:
            gemm_force_config(cfg)
            outs.append(_sample(m, name))
    finally:
        gemm_force_config(-1)
    for cfg, o in zip(GEMM_CONFIGS, outs):
        assert torch.equal(o, outs[0]), f"tile configuration {cfg} differs from {GEMM_CONFIGS[0]}"
    if compute == "fp32":
        assert gc.max_rel(outs[0].numpy(), gc.load(name)["out"]) < FP32_TOL


# 4. 16-bit envelopes
def _gen_frames(x, lens, dur):
    return np.concatenate([x[i, int(lens[i]):int(dur[i])] for i in range(x.shape[0])], axis=0)


ENVELOPES = [("mmdit_tiny_sample_b3", "mmdit_tiny_sample_b3_bf16", "bf16"),
             ("mmdit_tiny_sample_b3", "mmdit_tiny_sample_b3_fp16", "fp16"),
             ("mmdit_wide_sample_b2", "mmdit_wide_sample_b2_bf16", "bf16")]


@pytest.mark.parametrize("case,lo,compute", ENVELOPES, ids=[f"{c}-{m}" for c, _, m in ENVELOPES])
def test_within_reference_envelope(case, lo, compute):
    _need_gpu()
    f32, lof = gc.load(case), gc.load(lo)
    m = _model(mr.arch_of(mr.SAMPLE_CASES[case][0]), compute)
    out = _sample(m, case).numpy()
    assert np.isfinite(out).all()
    inp, _ = mr.sample_inputs(mr.SAMPLE_CASES[case][1])
    dur = torch.maximum(torch.maximum((inp["text"] != -1).sum(-1), inp["lens"]) + 1, inp["duration"])
    ref32 = _gen_frames(f32["out"], inp["lens"], dur)
    e_ours = gc.rel_err(_gen_frames(out, inp["lens"], dur), ref32)
    e_ref = gc.rel_err(_gen_frames(lof["out"], inp["lens"], dur), ref32)
    print(f"envelope {case} [{compute}]: e_ours={e_ours:.5f} e_ref={e_ref:.5f} ratio={e_ours / e_ref:.3f}")
    assert e_ours <= MARGIN * e_ref, (e_ours, e_ref)
    measured = MEASURED.get((case, compute))
    assert measured is not None, f"record the measured e_ours={e_ours:.6g} of {case} [{compute}] in MEASURED"
    assert e_ours <= 1.25 * measured, (e_ours, measured)


# 5. qk_norm: the four gains reach the output
def test_qk_norm_gains_matter():
    _need_gpu()
    name = "mmdit_tiny_qknorm_sample_b3"
    arch = mr.arch_of("tiny_qkn")
    W = synthetic.make_weights_torch(arch)
    with_gains = _sample(_model(arch, "fp32", W), name).numpy()
    assert gc.max_rel(with_gains, gc.load(name)["out"]) < FP32_TOL
    plain = mr.arch_of("tiny")
    no_gains = _sample(_model(plain, "fp32", {k: v for k, v in W.items() if "_norm.weight" not in k}), name).numpy()
    diff = gc.max_rel(no_gains, with_gains)
    print(f"qk_norm on / off: max-rel {diff:.3e}")
    assert diff > 3 * FP32_TOL


# 6. graph replays equal eager launches
def test_graph_equals_eager():
    _need_gpu()
    name = "mmdit_tiny_sample_b3"
    nfe = mr.SAMPLE_CASES[name][2]
    m = _model(mr.arch_of("tiny"), "bf16")
    eng = m.transformer.get_engine("bf16", m.device)
    eng.set_graph_mode(False)
    eager = _sample(m, name)
    eng.set_graph_mode(True)
    stats = [eng.graph_stats()]
    outs = []
    for _ in range(3):
        outs.append(_sample(m, name))
        stats.append(eng.graph_stats())
    for o in outs:
        assert torch.equal(o, eager)
    s0, s1, s2, s3 = stats
    assert s1["captures"] == s0["captures"] + 1 and s2["captures"] == s1["captures"] + 1  # step graph, then prologue
    assert s3["captures"] == s2["captures"], "the third call of a shape captures nothing"
    assert s3["replays"] - s2["replays"] == nfe + 1
    # another text length: the joint sequence changes, so the step is captured anew, and is still right
    spec = dict(gc.B3, n_text=[25, 37, 12])
    other = _sample(m, name, spec)
    s4 = eng.graph_stats()
    assert s4["captures"] > s3["captures"]
    eng.set_graph_mode(False)
    assert torch.equal(other, _sample(m, name, spec))
    tag, _, nfe, sway, cfg, _ = mr.SAMPLE_CASES[name]
    inp, y0 = mr.sample_inputs(spec)
    ref = mr.cfm_sample(synthetic.make_weights_torch(mr.arch_of(tag)), mr.arch_of(tag), inp["cond"], inp["text"],
                        inp["duration"], lens=inp["lens"], steps=nfe, cfg_strength=cfg, sway_sampling_coef=sway, y0=y0)
    fp32 = _sample(_model(mr.arch_of(tag), "fp32"), name, spec)
    assert gc.max_rel(fp32.numpy(), ref.numpy()) < FP32_TOL


# 7. the plugin contract: the reference-style loop over forward(cfg_infer=True, cache=True) is sample, bit for bit
@pytest.mark.parametrize("name", ["mmdit_tiny_sample_b3", "mmdit_tiny_nocfg_b3"])
def test_plugin_loop_reproduces_sample(name):
    _need_gpu()
    tag, spec, nfe, sway, cfg, _ = mr.SAMPLE_CASES[name]
    m = _model(mr.arch_of(tag), "fp32")
    inp, y0 = mr.sample_inputs(spec)
    out, _ = _plugin_euler(m.transformer, inp, inp["duration"], nfe, cfg, sway, y0)
    torch.cuda.synchronize()
    assert torch.equal(out.float().cpu(), _sample(m, name))
    assert gc.max_rel(out.cpu().numpy(), gc.load(name)["out"]) < FP32_TOL


def test_cached_single_branch_forwards_honour_the_drop_flags():
    """One session (cache=True: one kept workspace, the backbone step replayed as a graph) serving the conditional
    branch and then the dropped branches, as a loop that calls the backbone once per CFG branch does. MMDiT's captured
    step reads the text stream's start, so a graph captured for one branch must not serve the other."""
    _need_gpu()
    m = _model(mr.arch_of("tiny"), "fp32")
    net = m.transformer
    fi = mr.forward_inputs(gc.B3)
    x, cond, text, mask = (fi[k].to(DEV) for k in ("x", "cond", "text", "mask"))
    t = torch.tensor(gc.FWD_T, device=DEV)
    calls = [("mmdit_tiny_fwd_b3_single", {}), ("mmdit_tiny_fwd_b3_droptext", dict(drop_text=True)),
             ("mmdit_tiny_fwd_b3_dropaudio", dict(drop_audio_cond=True)), ("mmdit_tiny_fwd_b3_single", {}),
             ("mmdit_tiny_fwd_b3_droptext", dict(drop_text=True))]
    fresh = {}
    for name, kw in calls:  # without the cache: every call computes its own text embedding, nothing is replayed
        fresh[name] = net(x, cond, text, t, mask=mask, cfg_infer=False, **kw).float().cpu()
    net.clear_cache()
    for name, kw in calls:
        out = net(x, cond, text, t, mask=mask, cfg_infer=False, cache=True, **kw).float().cpu()
        err = gc.max_rel(out.numpy(), gc.load(name)["out"])
        print(f"cached {name}: max-rel {err:.3e}")
        assert err < FP32_TOL, name
        assert torch.equal(out, fresh[name]), name
    net.clear_cache()
    # the same on an engine handle: text_cache 1 then 2 with drop_text flipped between the calls
    eng = net.get_engine("fp32", torch.device(DEV))
    B, N = x.shape[:2]
    ws = eng.forward_workspace(B, N, text.shape[1], cfg_infer=False)
    ones = torch.ones(B, N, dtype=torch.uint8, device=DEV)
    dur = mask.sum(1)
    for tc, drop, name in ((1, True, "mmdit_tiny_fwd_b3_droptext"), (2, False, "mmdit_tiny_fwd_b3_single"),
                           (2, True, "mmdit_tiny_fwd_b3_droptext")):
        out = eng.forward(x, cond, ones, text, dur, gc.FWD_T, True, cfg_infer=False, drop_text=drop, text_cache=tc,
                          workspace=ws).float().cpu()
        assert torch.equal(out, fresh[name]), (tc, drop)


# 8. the other solvers: midpoint through MMDiT against the composition with the restatement as f
def test_midpoint_matches_the_restatement():
    _need_gpu()
    name = "mmdit_tiny_sample_b1"
    tag, spec, nfe, sway, cfg, _ = mr.SAMPLE_CASES[name]
    arch = mr.arch_of(tag)
    W = synthetic.make_weights_torch(arch)
    inp, y0 = mr.sample_inputs(spec)
    pre = mr.ref_cpu.prepare(arch, inp["cond"].float(), inp["text"], inp["duration"], inp["lens"])
    with torch.no_grad():
        traj = ode_reference.integrate(mr.flow(W, arch, pre, inp["text"], cfg), y0.float(),
                                       mr.ref_cpu.epss_sway_grid(nfe, sway), "midpoint")
    ref = torch.where(pre["cond_mask"], pre["cond"], traj[-1])
    out = _sample(_model(arch, "fp32", W, method="midpoint"), name)
    err = gc.max_rel(out.numpy(), ref.numpy())
    print(f"midpoint {name}: max-rel {err:.3e}")
    assert err < FP32_TOL
    assert gc.max_rel(out.numpy(), gc.load(name)["out"]) > FP32_TOL  # and it is not the Euler result


# 9. switches that have no effect on MMDiT
def test_no_effect_switches():
    _need_gpu()
    name = "mmdit_tiny_sample_b3"
    m = _model(mr.arch_of("tiny"), "bf16")
    eng = m.transformer.get_engine("bf16", m.device)
    base = _sample(m, name)
    eng.set_chain(True)
    eng.set_ln_fold(True)
    assert torch.equal(_sample(m, name), base)
    assert eng.chain_stats()[0] == 0 and eng.ln_fold_stats()[1] == 0
    eng.set_pad_skip(True)
    assert torch.equal(_sample(m, name), base)
    eng.set_pad_skip(False)
    assert torch.equal(_sample(m, name), base)
    eng.set_cfg_streams(2)
    assert torch.equal(_sample(m, name), base)
    assert eng.chain_stats()[:2] == (0, 0) and eng.ln_fold_stats()[1] == 0


# 10. error paths
def test_attn_mask_enabled_refused_with_a_batch_and_inert_without():
    _need_gpu()
    masked = configs.get_arch("MMDiT_tiny", text_num_embeds=64, attn_mask_enabled=True)
    m = _model(masked, "fp32")
    with pytest.raises(NotImplementedError, match="attn_mask_enabled"):
        _sample(m, "mmdit_tiny_sample_b3")
    eng = m.transformer.get_engine("fp32", m.device)
    inp, y0 = mr.sample_inputs(gc.B3)
    N = y0.shape[1]
    with pytest.raises(NotImplementedError):  # the engine handle refuses the call as well
        eng.sample(torch.zeros(3, N, 100, device=DEV), torch.zeros(3, N, dtype=torch.bool, device=DEV),
                   inp["text"].to(DEV), torch.full((3,), N, device=DEV), y0.to(DEV), [0.0, 0.5, 1.0], 2.0, True)
    one = _sample(m, "mmdit_tiny_sample_b1")
    assert torch.equal(one, _sample(_model(mr.arch_of("tiny"), "fp32"), "mmdit_tiny_sample_b1"))


def test_library_refuses_attn_mask_with_a_batch_mask(monkeypatch):
    """f5h_sample / f5h_forward themselves (the Python check switched off): F5H_EINVAL, the reason in the message."""
    _need_gpu()
    from f5_tts_amd import engine as E

    masked = configs.get_arch("MMDiT_tiny", text_num_embeds=64, attn_mask_enabled=True)
    m = _model(masked, "fp32")
    eng = m.transformer.get_engine("fp32", m.device)
    monkeypatch.setattr(E, "_refuse_mmdit_masked", lambda arch, use_batch_mask: None)
    fi = mr.forward_inputs(gc.B3)
    x, cond, text, mask = (fi[k].to(DEV) for k in ("x", "cond", "text", "mask"))
    ones = torch.ones(x.shape[:2], dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r"f5h_forward failed \(status -1\).*not a prefix"):
        eng.forward(x, cond, ones, text, mask.sum(1), 0.3, True)
    with pytest.raises(RuntimeError, match=r"f5h_sample\w* failed \(status -1\).*not a prefix"):
        eng.sample(cond, ones, text, mask.sum(1), x, [0.0, 0.5, 1.0], 2.0, True)
    assert torch.isfinite(eng.forward(x, cond, ones, text, mask.sum(1), 0.3, False)).all()  # no batch mask: accepted


def test_missing_weight_is_named():
    _need_gpu()
    from f5_tts_amd.engine import Engine

    arch = mr.arch_of("tiny")
    W = synthetic.make_weights_torch(arch)
    del W["transformer_blocks.1.attn.to_q_c.weight"]
    with pytest.raises(RuntimeError, match=r"transformer_blocks\.1\.attn\.to_q_c\.weight"):
        Engine(arch, W, compute="fp32", device=DEV)
