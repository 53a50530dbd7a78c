"""qk_norm="rms_norm", long_skip_connection and text_embedding_average_upsampling on the device: the QKV epilogue
with the norm and the upsampling kernel at the op level (tests/dit_options_reference.py, the op tolerance of
tests/op_reference.py), and CFM.sample / the plugin forward end to end against the CPU oracle composed with the
options. Bounds: fp32 max|diff| / max|ref| < 1e-3; 16-bit rel-L2 <= 5e-2 against the option's own fp32 reference
(the bound test_edge_sample_matches_reference and the ODE tests use); the 16-bit qk_norm cases scale to_q / to_k by
dit_options_reference.QK_SCALE (tests/test_dit_options.py shows why)."""

import pytest
import torch

import dit_options_reference as D
import golden_cases as gc
import op_cases as C
import op_reference as R
from f5_tts_amd import _lib, configs, synthetic
from f5_tts_amd.engine import gemm_force_config, op_gemm_epi, op_text_upsample, store_policy_force
from f5_tts_amd.model import CFM, DiT, UNetT
from test_gpu_parity import GEMM_CONFIGS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
FP32_TOL, BF16_TOL = 1e-3, 5e-2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------- 1. the QKV epilogue with the norm
def _qkn_run(c, compute, norm=True, **fold):
    A, W = c["A"].to(DEV), c["W"].to(DEV)
    kw = dict(q_norm_w=c["wq"], k_norm_w=c["wk"], qk_norm_eps=D.QK_EPS) if norm else {}
    return lambda: tuple(t.cpu() for t in op_gemm_epi("qkv", A, W, bias=c["bias"], compute=compute, seq_len=c["L"],
                                                      heads=c["H"], rope_heads=c["rope_heads"], q_scale=c["q_scale"],
                                                      **kw, **fold))


def _every_config_and_policy(run, compute):
    """run() under every tile configuration and, in the 16-bit modes, both store policies: configuration 0's outputs,
    after asserting all others give the same bits (12 and 13 have no kernel with the norm: they run as 11 or 1)."""
    cfgs = GEMM_CONFIGS if compute != "fp32" else [-1]
    outs = {}
    try:
        for cfg in cfgs:
            gemm_force_config(cfg)
            for pol in ((0, 1) if compute != "fp32" else (-1,)):
                store_policy_force(pol)
                outs[(cfg, pol)] = run()
    finally:
        gemm_force_config(-1)
        store_policy_force(-1)
    first = outs[(cfgs[0], 0 if compute != "fp32" else -1)]
    for key, o in outs.items():
        for i, (t, t0) in enumerate(zip(o, first)):
            assert _bits_equal(t, t0), f"output {i} under (config, store policy) {key} differs from configuration 0"
    return first


@pytest.mark.parametrize("compute", C.COMPUTES)
@pytest.mark.parametrize("H,rope_heads,bias_on", D.QKN_CASES)
def test_qkv_epilogue_with_qk_norm(compute, H, rope_heads, bias_on):
    _need_gpu()
    c = D.qkn_case(compute, H, rope_heads, bias_on)
    what = f"qkv_norm/{compute}/H{H}-rope{rope_heads}-bias{int(bias_on)}"
    q, k, v, rope = _every_config_and_policy(_qkn_run(c, compute), compute)
    r64, r32 = D.qkn_ref(c, rope, F64), D.qkn_ref(c, rope, F32)
    for nm, o, a, b in zip("qkv", (q, k, v), r64, r32):
        R.assert_close(o, a, b, c["u_out"], f"{what}/{nm}")
    assert torch.isfinite(q).all() and torch.isfinite(k).all() and torch.isfinite(v).all()
    if not bias_on:
        assert (q[0, :, D.ROW_ZERO] == 0).all() and (k[0, :, D.ROW_ZERO] == 0).all(), what + ": the all-zero row"
    # v is the v of the same call without the norm; null gains are the unchanged code path
    q0, k0, v0, _ = _qkn_run(c, compute, norm=False)()
    assert _bits_equal(v, v0), what + ": v differs from the call without the norm"
    assert not _bits_equal(q, q0) and not _bits_equal(k, k0)
    p64, p32 = C.qkv_ref(c, rope, F64), C.qkv_ref(c, rope, F32)
    for nm, o, a, b in zip("qkv", (q0, k0, v0), p64, p32):
        R.assert_close(o, a, b, c["u_out"], f"{what}/no-norm-{nm}")


@pytest.mark.parametrize("compute", ["bf16", "fp16"])
def test_null_gains_are_the_parent_s_code_path(compute):
    """Without gains the launch is the kernel the parent launches: its q, k, v are bitwise those of a call whose args
    never mention the norm, under every configuration."""
    _need_gpu()
    c = D.qkn_case(compute, 2, 2, True)
    a = _every_config_and_policy(_qkn_run(c, compute, norm=False), compute)
    A, W = c["A"].to(DEV), c["W"].to(DEV)
    b = op_gemm_epi("qkv", A, W, bias=c["bias"], compute=compute, seq_len=c["L"], heads=c["H"],
                    rope_heads=c["rope_heads"], q_scale=c["q_scale"], q_norm_w=None, k_norm_w=None)
    for t, t0 in zip(b, a):
        assert _bits_equal(t.cpu(), t0)


@pytest.mark.parametrize("compute", ["bf16", "fp16"])
def test_qk_norm_with_the_layernorm_fold_consumer(compute):
    _need_gpu()
    c = D.qkn_fold_case(compute)
    fold = dict(ln_part_in=c["parts"], ln_u=c["u"], ln_v=c["v"], ln_rms=c["rms"], ln_eps=c["eps"])
    q, k, v, rope = _every_config_and_policy(_qkn_run(c, compute, **fold), compute)
    r64, r32 = D.qkn_fold_ref(c, rope, F64), D.qkn_fold_ref(c, rope, F32)
    for nm, o, a, b in zip("qkv", (q, k, v), r64, r32):
        R.assert_close(o, a, b, c["u_out"], f"qkv_norm_fold/{compute}/{nm}")
    v0 = _qkn_run(c, compute, norm=False, **fold)()[2]
    assert _bits_equal(v, v0)


# ---------------------------------------------------------------- 2. the upsampling kernel
@pytest.mark.parametrize("lens", [D.UP_LENS, (39, 22, 7), None])
def test_text_upsample_is_bitwise_the_restatement(lens):
    """(40, 23, 7): a hole among sequence 0's tokens, T = audio_len, no valid token. (39, 22, 7): audio_len no multiple
    of T. None: every sequence takes N frames (the single-utterance path). The output starts as NaN."""
    _need_gpu()
    c = D.upsample_case()
    lt = None if lens is None else torch.tensor(lens, dtype=torch.long)
    out = op_text_upsample(c["te"].to(DEV), c["text"].to(DEV), None if lt is None else lt.to(DEV)).cpu()
    want = D.upsample_ref(c, lt if lt is not None else torch.full((D.UP_S,), D.UP_N, dtype=torch.long))
    assert not torch.isnan(out).any(), "a row was left unwritten"
    assert _bits_equal(out, want)


# ---------------------------------------------------------------- 3 / 4. end to end
def _model(arch, W, compute):
    cls = DiT if arch["backbone"] == "DiT" else UNetT
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = cls(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    missing, unexpected = net.load_state_dict(W, strict=False)
    assert not unexpected and all(k.endswith("inv_freq") for k in missing), (missing, unexpected)
    return CFM(transformer=net, num_channels=100, compute=compute).to(DEV)


def _sample(m, ref, steps=D.STEPS):
    inp = ref["inp"]
    out, _ = m.sample(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=inp["duration"].to(DEV),
                      lens=inp["lens"].to(DEV), steps=steps, cfg_strength=D.CFG, sway_sampling_coef=D.SWAY,
                      y0=ref["y0"].to(DEV), keep_trajectory=False)
    torch.cuda.synchronize()
    return out.float().cpu()


ALL3 = dict(qk_norm="rms_norm", long_skip_connection=True, text_embedding_average_upsampling=True)
# name -> (arch tag, inputs, options, an interior -1 in the text)
E2E = {
    "qk_norm_b3": ("tiny", gc.B3, dict(qk_norm="rms_norm"), False),
    "qk_norm_b1": ("tiny", gc.B1, dict(qk_norm="rms_norm"), False),
    "long_skip_b3": ("tiny", gc.B3, dict(long_skip_connection=True), False),
    "long_skip_b1": ("tiny", gc.B1, dict(long_skip_connection=True), False),
    "upsample_b3": ("tiny", gc.B3, dict(text_embedding_average_upsampling=True), False),
    "upsample_b1": ("tiny", gc.B1, dict(text_embedding_average_upsampling=True), False),
    "all_b3": ("tiny", gc.B3, ALL3, False),
    "unett_qk_norm_b1": ("utiny", gc.B1, dict(qk_norm="rms_norm"), False),
    "qk_norm_pe1_b3": ("tiny", gc.B3, dict(qk_norm="rms_norm", pe_attn_head=1), False),
    "upsample_hole_b3": ("tiny", gc.B3, dict(text_embedding_average_upsampling=True), True),
}


def _plain_options(options):
    return {k: v for k, v in options.items() if k == "pe_attn_head"}


@pytest.mark.parametrize("name", list(E2E))
def test_fp32_sample_matches_the_reference_and_differs_from_options_off(name):
    _need_gpu()
    tag, spec, options, hole = E2E[name]
    ref = D.case(tag, spec, options, hole=hole)
    out = _sample(_model(ref["arch"], ref["W"], "fp32"), ref)
    err = gc.max_rel(out.numpy(), ref["out"].numpy())
    # the same weights (the extra parameters dropped) through an engine without the options
    off_arch = D.arch_with(tag, **_plain_options(options))
    W_off = {k: v for k, v in ref["W"].items() if k in configs.param_shapes(off_arch)}
    off = _sample(_model(off_arch, W_off, "fp32"), ref)
    moved = gc.max_rel(out.numpy(), off.numpy())
    print(f"{name} fp32: max-rel {err:.3e}; moved from the options-off engine by {moved:.3e}")
    assert err < FP32_TOL, err
    assert moved > 3 * FP32_TOL, "the options-off engine gives the same output"


@pytest.mark.parametrize("compute", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["qk_norm_b3", "long_skip_b3", "upsample_b3", "all_b3", "unett_qk_norm_b1"])
def test_16bit_sample_stays_within_the_bound_of_the_option_s_reference(name, compute):
    _need_gpu()
    tag, spec, options, hole = E2E[name]
    ref = D.case(tag, spec, options, qk_scale=D.QK_SCALE if options.get("qk_norm") else 1.0, hole=hole)
    out = _sample(_model(ref["arch"], ref["W"], compute), ref)
    err = gc.rel_err(out.numpy(), ref["out"].numpy())
    print(f"{name} {compute}: rel-L2 {err:.3e}")
    assert err <= BF16_TOL, err


# ---------------------------------------------------------------- 5. graph == eager
def test_graph_equals_eager_with_all_three_options():
    _need_gpu()
    tag, spec, options, hole = E2E["all_b3"]
    ref = D.case(tag, spec, options, qk_scale=D.QK_SCALE)
    m = _model(ref["arch"], ref["W"], "bf16")
    eng = m.transformer.get_engine("bf16", m.device)
    eng.set_graph_mode(False)
    eager = _sample(m, ref)
    eng.set_graph_mode(True)
    s0 = eng.graph_stats()
    o1 = _sample(m, ref)
    s1 = eng.graph_stats()
    o2 = _sample(m, ref)
    s2 = eng.graph_stats()
    o3 = _sample(m, ref)
    s3 = eng.graph_stats()
    for o in (o1, o2, o3):
        assert torch.equal(o, eager)
    assert s1["captures"] == s0["captures"] + 1 and s2["captures"] == s1["captures"] + 1  # step graph, then prologue
    assert s3["captures"] == s2["captures"], "the third call of a shape captures nothing"
    assert s3["replays"] - s2["replays"] == D.STEPS + 1
    assert gc.rel_err(eager.numpy(), ref["out"].numpy()) <= BF16_TOL


# ---------------------------------------------------------------- 6. workspace sizes of option-free archs
# f5h_workspace_size(B, N, nt = 30, nfe, use_cfg = 1) as the build before the options existed returned it on the
# device (the parent commit's library, the same archs and synthetic weights): (arch tag, compute, B, N, nfe) -> bytes
PARENT_WORKSPACE = {
    ("tiny", "bf16", 1, 150, 4): 2017792,
    ("tiny", "fp32", 1, 150, 4): 2837248,
    ("tiny", "bf16", 3, 150, 6): 5775872,
    ("tiny", "fp32", 3, 150, 6): 8332544,
    ("tiny_v0", "bf16", 3, 150, 5): 5755904,
    ("tiny_v0", "fp32", 3, 150, 5): 8322304,
    ("utiny", "bf16", 3, 150, 4): 6233856,
    ("utiny", "fp32", 3, 150, 4): 10275328,
    ("c1", "bf16", 1, 564, 4): 38878208,
    ("c1", "fp32", 1, 564, 4): 56954624,
}


@pytest.mark.parametrize("tag", sorted({k[0] for k in PARENT_WORKSPACE}))
def test_workspace_bytes_unchanged_for_option_free_archs(tag):
    _need_gpu()
    arch = gc.arch_of(tag)
    W = synthetic.make_weights_torch(arch)
    for (t, compute, B, N, nfe), want in PARENT_WORKSPACE.items():
        if t != tag:
            continue
        m = _model(arch, W, compute)
        eng = m.transformer.get_engine(compute, m.device)
        assert eng.workspace_bytes(B, N, 30, nfe) == want, (compute, B, N, nfe)
        assert int(_lib.lib().f5h_workspace_size(eng._h, B, N, 30, nfe, 1)) == want


def test_workspace_grows_only_with_the_options():
    _need_gpu()
    plain = D.arch_with("tiny")
    sizes = {}
    for name, opt in (("plain", {}), ("qk", dict(qk_norm="rms_norm")), ("skip", dict(long_skip_connection=True)),
                      ("up", dict(text_embedding_average_upsampling=True))):
        arch = D.arch_with("tiny", **opt)
        m = _model(arch, D.weights_for(arch), "bf16")
        sizes[name] = m.transformer.get_engine("bf16", m.device).workspace_bytes(3, 150, 30, 4)
    d, td = plain["dim"], plain["text_dim"]
    r256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    assert sizes["qk"] == sizes["plain"]
    assert sizes["skip"] - sizes["plain"] == r256(6 * 150 * d * 2)      # [S, L, d] in the 16-bit residual dtype
    assert sizes["up"] - sizes["plain"] == r256(2 * 3 * 150 * td * 4)   # both branches' text embedding, fp32


# ---------------------------------------------------------------- 7. Base width: chain and fold
@pytest.mark.parametrize("option", ["qk_norm", "long_skip_connection"])
def test_base_width_chain_gated_and_fold_within_bound(option):
    """dim 1024, where the phase chain and the LayerNorm fold live. Engines with qk_norm or the long skip never run
    the chain: set_chain(True) changes neither the bits nor chain_stats. The fold stays on for the
    layers, and both fold settings stay within the 16-bit bound of the reference."""
    _need_gpu()
    opt = dict(qk_norm="rms_norm") if option == "qk_norm" else dict(long_skip_connection=True)
    arch = configs.get_arch("F5TTS_v1_Base", depth=2, **opt)
    W = synthetic.make_weights_torch(arch)
    inp = synthetic.make_case(B=1, ref_frames=[37], total_frames=[149], n_text=[20], vocab=arch["text_num_embeds"])
    y0 = D.noise_for(inp, 3)
    steps = 2
    want = D.cfm_sample(W, arch, inp, y0, steps, D.CFG, D.SWAY)
    ref = dict(inp=inp, y0=y0)
    m = _model(arch, W, "bf16")
    eng = m.transformer.get_engine("bf16", m.device)
    assert eng.ln_fold_stats()[0]
    outs = {}
    try:
        for fold in (True, False):
            eng.set_ln_fold(fold)
            n0 = eng.ln_fold_stats()[1]
            for chain in (False, True):
                eng.set_chain(chain)
                outs[(fold, chain)] = _sample(m, ref, steps)
                launches, fault, _ = eng.chain_stats()
                assert launches == 0 and fault == 0, "the chain must stay off for this engine"
            # (counted where a step is enqueued: the fold setting's one capture; the chain switch changes no graph key)
            assert (eng.ln_fold_stats()[1] > n0) == fold
            assert torch.equal(outs[(fold, True)], outs[(fold, False)])
            err = gc.rel_err(outs[(fold, False)].numpy(), want.numpy())
            print(f"Base depth 2, {option}, bf16, LayerNorm fold {fold}: rel-L2 {err:.3e}")
            assert err <= BF16_TOL, (fold, err)
    finally:
        eng.set_chain(False)
        eng.set_ln_fold(True)


# ---------------------------------------------------------------- 8. plugin contract
def test_plugin_single_branch_forward_with_upsampling():
    """DiT.forward(cfg_infer=False, drop_text=True): the unconditional branch alone, whose upsampling still goes by
    the mask of the undropped text."""
    _need_gpu()
    ref = D.case("tiny", gc.B3, dict(text_embedding_average_upsampling=True), hole=True)
    arch, W, inp = ref["arch"], ref["W"], ref["inp"]
    from oracle import ref_cpu

    pre = ref_cpu.prepare(arch, inp["cond"].float(), inp["text"], inp["duration"], inp["lens"])
    x = ref["y0"].float()
    t = torch.tensor(0.3)
    want = D.dit_forward(W, arch, x, pre["step_cond"], inp["text"], t, pre["mask"], {}, packed=False, drop_text=True)
    both = D.dit_forward(W, arch, x, pre["step_cond"], inp["text"], t, pre["mask"], {}, packed=False, drop_text=False)
    net = _model(arch, W, "fp32").transformer
    got = net.forward(x.to(DEV), pre["step_cond"].to(DEV), inp["text"].to(DEV), t.to(DEV), mask=pre["mask"].to(DEV),
                      cfg_infer=False, drop_text=True, compute="fp32").float().cpu()
    err = gc.max_rel(got.numpy(), want.numpy())
    print(f"plugin forward, drop_text, upsampling: max-rel {err:.3e}")
    assert err < FP32_TOL
    assert gc.max_rel(want.numpy(), both.numpy()) > 3 * FP32_TOL


# ---------------------------------------------------------------- 9. error paths
def test_missing_gain_names_the_tensor():
    _need_gpu()
    arch = D.arch_with("tiny", qk_norm="rms_norm")
    W = D.weights_for(arch)
    del W["transformer_blocks.1.attn.k_norm.weight"]
    from f5_tts_amd.engine import Engine

    with pytest.raises(RuntimeError, match=r"status -1.*transformer_blocks\.1\.attn\.k_norm\.weight"):
        Engine(arch, W, compute="bf16", device=DEV)
    arch = D.arch_with("tiny", long_skip_connection=True)
    W = D.weights_for(arch)
    del W["long_skip_connection.weight"]
    with pytest.raises(RuntimeError, match=r"long_skip_connection\.weight"):
        Engine(arch, W, compute="bf16", device=DEV)
