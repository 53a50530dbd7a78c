"""The launch head of gemm_kernel and attn16_kernel on the device (DESIGN.md §3 'Launch head'): the kernels issue
their first operand DMA from the arguments' hot line, a host-made multiply-shift division and a handful of address
computations, before the rest of their setup. A wrong tile origin, extent or lane offset there reads the wrong rows,
so every case runs with NaN bits around the operand panels (the op hooks' workspace fill) and is held to the fp64
reference of tests/op_reference.py under the bound of tests/test_gpu_ops.py (|out - R64| <= u_out |R64| + 8 max|R32 -
R64|, and for 16-bit attention the P-rounding term derived in test_attention_q_len), and bit for bit across tile
configurations 0 / 1 / 5 and both store policies; attention also bit for bit against the forced SAFE rerun
(f5h_attn_force_safe), which meets the same bound.

Shapes: M 1 / 63 / 65 (tiles whose rows mostly lie past M), 130 and 193 (two to four row tiles, one past the 192-row
tile), N 128 / 384 (one and three column tiles: the division by the column-tile count), K 64 / 128 (fewer K steps
than ring stages), 192 and 1024.
"""

import pytest
import torch

import op_cases as C
import op_reference as R
from f5_tts_amd import configs, synthetic
from f5_tts_amd.engine import (attn_force_safe, gemm_force_config, op_attention, op_attention_ragged,
                               op_attention_ranges, op_gemm_epi, op_linear, store_policy_force)
from f5_tts_amd.model import CFM, DiT
from test_gpu_isolate_ops import _ranges_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
MODES16 = ("bf16", "fp16")
CONFIGS = (0, 1, 5)
EDGE_M, EDGE_N, EDGE_K = (1, 63, 65, 130, 193), (128, 384), (64, 128, 192, 1024)
POISON = 0xFF  # workspace fill: NaN bits in every 16-bit and fp32 slot around the operand panels


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _flat(res):
    return [t for t in (res if isinstance(res, tuple) else (res,)) if t is not None]


def _every_config_and_policy(run, what, configs=CONFIGS):
    """run() under every tile configuration and both store policies; all results bitwise equal. Returns the first."""
    outs = []
    try:
        for cfg in configs:
            gemm_force_config(cfg)
            for mode in (0, 1):
                store_policy_force(mode)
                outs.append((cfg, mode, [t.cpu() for t in _flat(run())]))
    finally:
        gemm_force_config(-1)
        store_policy_force(-1)
    for cfg, mode, o in outs[1:]:
        for i, (a, b) in enumerate(zip(o, outs[0][2])):
            assert _bits_equal(a, b), f"{what}: output {i} differs under cfg {cfg} / store policy {mode}"
    return outs[0][2]


# ---------------------------------------------------------------- GEMM edges
@pytest.mark.parametrize("compute", MODES16)
@pytest.mark.parametrize("M", EDGE_M)
def test_gemm_edges(compute, M):
    """EPI_GELU_TANH (operand out, the strip epilogue with a write-through variant) through op_gemm_epi and the plain
    linear (fp32 out) through op_linear, at every (N, K) of the edge shapes."""
    _need_gpu()
    for N in EDGE_N:
        for K in EDGE_K:
            g = torch.Generator(device="cpu").manual_seed(1000 * M + 10 * N + K)
            A = R.rnd(torch.randn(M, K, generator=g), compute)
            W = R.rnd(torch.randn(N, K, generator=g) / K ** 0.5, compute)
            bias = torch.randn(N, generator=g)
            Ad, Wd, bd = A.to(DEV), W.to(DEV), bias.to(DEV)
            what = f"launch_head/{compute}/gelu_tanh-{M}x{N}x{K}"
            out = _every_config_and_policy(
                lambda: op_gemm_epi("gelu_tanh", Ad, Wd, bias=bd, compute=compute, ws_fill=POISON), what)[0]
            R.assert_close(out, R.gemm_epi("gelu_tanh", A, W, bias, dtype=F64),
                           R.gemm_epi("gelu_tanh", A, W, bias, dtype=F32), R.U_OUT[compute], what)
            what = f"launch_head/{compute}/linear-{M}x{N}x{K}"
            lin = _every_config_and_policy(lambda: op_linear(Ad, Wd, bd, compute=compute), what)[0]
            R.assert_close(lin, R.gemm_epi("store", A, W, bias, dtype=F64), R.gemm_epi("store", A, W, bias, dtype=F32),
                           0.0, what)


# ---------------------------------------------------------------- epilogue fields that moved in the struct
def _case_kw(c):
    return dict(bias=c["bias"], C=c.get("C"), A2=None if c.get("A2") is None else c["A2"].to(DEV),
                k_split=c.get("k_split", 0), resid=c.get("resid"), gate=c.get("gate"), rowkeep=c.get("keep"),
                live_len=c.get("live_len"), live_seq=c.get("live_seq", 0), add=c.get("add"),
                dual_rows=c.get("dual_rows", 0))


@pytest.mark.parametrize("compute", MODES16)
@pytest.mark.parametrize("name", ["resid16_keep", "resid16_gate_r", "resid_plain", "resid_gate_keep_r", "store_a2_lo",
                                  "store16_a2_hi", "inproj", "inproj_dual"])
def test_epilogue_fields(compute, name):
    """gate / resid / rowkeep present and absent, A2 with k_split low and high (the skip GEMM; the columns the kernel
    must not read are NaN), add / ld_add / dual_rows: the cases of tests/op_cases.py at M = 130 (two 64-row tiles and
    a ragged one) and M = 77 with ragged N."""
    _need_gpu()
    for M, N, K in [s for s in C.gemm_shapes_of(name) if s[0] in (77, 130)]:
        c = C.gemm_case(compute, name, M, N, K)
        A, W = c["A"].to(DEV), c["W"].to(DEV)
        what = f"launch_head/{compute}/{name}-{M}x{N}x{K}"
        out = _every_config_and_policy(
            lambda: op_gemm_epi(c["epi"], A, W, compute=compute, ws_fill=POISON, **_case_kw(c)), what)[0]
        R.assert_close(out, C.gemm_ref(c, F64), C.gemm_ref(c, F32), c["u_out"], what)


@pytest.mark.parametrize("compute", MODES16)
def test_qkv_fields(compute):
    """EPI_QKV at M = 140 (two sequences of 70 rows): rope_heads < heads, q scaled, and qkv_dst_len (panels of 100 rows,
    the launch filling rows [10, 80): the other rows stay NaN)."""
    _need_gpu()
    H, rh, qs, K = 4, 1, C.Q_SCALE, 512
    c = C.qkv_case(compute, H, rh, qs, K)
    A, W = c["A"].to(DEV), c["W"].to(DEV)
    kw = dict(bias=c["bias"], compute=compute, seq_len=C.QKV_L, heads=H, rope_heads=rh, q_scale=qs, ws_fill=POISON)
    q, k, v, rope = _every_config_and_policy(lambda: op_gemm_epi("qkv", A, W, **kw), f"launch_head/{compute}/qkv")
    r64, r32 = C.qkv_ref(c, rope, F64), C.qkv_ref(c, rope, F32)
    for nm, o, a, b in zip("qkv", (q, k, v), r64, r32):
        R.assert_close(o, a, b, c["u_out"], f"launch_head/{compute}/qkv-{nm}")
    q2, k2, v2, _ = _every_config_and_policy(lambda: op_gemm_epi("qkv", A, W, qkv_dst_len=100, qkv_row0=10, **kw),
                                             f"launch_head/{compute}/qkv_dst_len")
    for o2, o in ((q2, q), (k2, k), (v2, v)):
        assert _bits_equal(o2[:, :, 10:80], o)
        assert torch.isnan(o2[:, :, :10]).all() and torch.isnan(o2[:, :, 80:]).all(), "rows outside the launch's"


@pytest.mark.parametrize("compute", MODES16)
@pytest.mark.parametrize("form", ["ln", "rms"])
def test_fold_forms_at_m70(compute, form):
    """The fold producer and both fold consumers at M = 70 (hs / hs_scale / ln_part, ln_part_in / ln_u / ln_v /
    ln_nparts / ln_rms / ln_eps): the cases and references of tests/test_gpu_fold_ops.py."""
    _need_gpu()
    variant = C.FOLD_PROD_VARIANTS[form][0]
    c = C.fold_prod_case(compute, form, variant, 70, 1024, 64)
    A, W = c["A"].to(DEV), c["W"].to(DEV)
    what = f"launch_head/{compute}/{form}/producer"
    Cf, *_ = _every_config_and_policy(
        lambda: op_gemm_epi("resid16", A, W, bias=c["bias"], C=c["C"], resid=c.get("resid"), gate=c["gate"],
                            rowkeep=c.get("keep"), compute=compute, ln_producer=True, hs_scale=c.get("hs_scale"),
                            ln_rms=c["rms"], poison=True, ws_fill=POISON), what)
    R.assert_close(Cf, C.gemm_ref(c, F64), C.gemm_ref(c, F32), c["u_out"], what)
    cc = C.fold_cons_case(compute, form, 70, 1024, 256)
    Ac, Wc = cc["A"].to(DEV), cc["W"].to(DEV)
    ckw = dict(bias=cc["bias"], compute=compute, ln_part_in=cc["parts"], ln_u=cc["u"], ln_v=cc["v"], ln_rms=cc["rms"],
               ln_eps=cc["eps"], ws_fill=POISON)
    what = f"launch_head/{compute}/{form}/consumer-gelu"
    out = _every_config_and_policy(lambda: op_gemm_epi("gelu_tanh", Ac, Wc, **ckw), what)[0]
    R.assert_close(out, C.fold_gelu_ref(cc, F64), C.fold_gelu_ref(cc, F32), cc["u_out"], what)
    spec = (70, 1024, 1, C.Q_SCALE)
    cq = C.fold_cons_case(compute, form, 140, 1024, 3 * C.FOLD_QKV_H * 64)
    Aq, Wq = cq["A"].to(DEV), cq["W"].to(DEV)
    qkw = dict(bias=cq["bias"], compute=compute, ln_part_in=cq["parts"], ln_u=cq["u"], ln_v=cq["v"], ln_rms=cq["rms"],
               ln_eps=cq["eps"], seq_len=70, heads=C.FOLD_QKV_H, rope_heads=1, q_scale=C.Q_SCALE, ws_fill=POISON)
    what = f"launch_head/{compute}/{form}/consumer-qkv"
    q, k, v, rope = _every_config_and_policy(lambda: op_gemm_epi("qkv", Aq, Wq, **qkw), what)
    r64, r32 = C.fold_qkv_ref(cq, spec, rope, F64), C.fold_qkv_ref(cq, spec, rope, F32)
    for nm, o, a, b in zip("qkv", (q, k, v), r64, r32):
        R.assert_close(o, a, b, cq["u_out"], f"{what}-{nm}")


# ---------------------------------------------------------------- pad-row skip
@pytest.mark.parametrize("compute", MODES16)
def test_pad_row_skip_leaves_no_dma_behind(compute):
    """EPI_RESID16 with live_len = [70, 0] over two 130-row sequences: the second sequence's row tiles leave before
    any DMA is issued (a wave that ended with LDS-DMA in flight would write into LDS the next workgroup owns). Eight
    launches back to back on one stream, each followed by a plain GEMM that uses the whole LDS ring of every CU: every
    output is bitwise the first launch's and within the bound of the reference."""
    _need_gpu()
    M, N, K, L = 260, 128, 256, 130
    g = torch.Generator(device="cpu").manual_seed(260)
    A = R.rnd(torch.randn(M, K, generator=g), compute)
    W = R.rnd(torch.randn(N, K, generator=g) / K ** 0.5, compute)
    bias, gate = torch.randn(N, generator=g), torch.randn(N, generator=g)
    C0 = R.rnd(torch.randn(M, N, generator=g), compute)
    ll = torch.tensor([70, 0], dtype=torch.int32)
    keep = (torch.arange(L)[None, :] < ll[:, None]).reshape(-1)
    Ad, Wd = A.to(DEV), W.to(DEV)
    Mb, Nb, Kb = 4096, 2048, 256  # 64 x 16 = 1024 tiles of 64 x 128: several per CU, every stage of the ring in use
    Ab = torch.randn(Mb, Kb, generator=g).to(DEV)
    Wb = (torch.randn(Nb, Kb, generator=g) / Kb ** 0.5).to(DEV)
    for cfg in CONFIGS:
        outs, bigs = [], []
        try:
            gemm_force_config(cfg)
            for _ in range(8):
                outs.append(op_gemm_epi("resid16", Ad, Wd, bias=bias, C=C0, gate=gate, rowkeep=keep, live_len=ll,
                                        live_seq=L, compute=compute, ws_fill=POISON))
                bigs.append(op_linear(Ab, Wb, None, compute=compute))
        finally:
            gemm_force_config(-1)
        torch.cuda.synchronize()
        for o, b in zip(outs[1:], bigs[1:]):
            assert _bits_equal(o.cpu(), outs[0].cpu()) and _bits_equal(b.cpu(), bigs[0].cpu()), (compute, cfg)
        ref = lambda dt: R.gemm_epi("resid16", A, W, bias, C=C0, gate=gate, keep=keep, dtype=dt)  # noqa: E731
        R.assert_close(outs[0].cpu(), ref(F64), ref(F32), R.U_OUT[compute], f"launch_head/{compute}/pad-skip-cfg{cfg}")
        assert torch.isfinite(bigs[0]).all()


# ---------------------------------------------------------------- attention
def _attn_inputs(compute, S, H, L, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    Q, K, V = (torch.randn(S, H, L, 64, generator=g) for _ in range(3))
    return R.rnd(Q * C.Q_SCALE, compute), R.rnd(K, compute), R.rnd(V, compute)


def _attn_policies_and_safe(run, what):
    """run() under both store policies, and under the forced SAFE rerun: (default result, SAFE result); the policies
    and the rerun agree bit for bit."""
    res = []
    try:
        for safe in (False, True):
            attn_force_safe(safe)
            outs = []
            for mode in (0, 1):
                store_policy_force(mode)
                outs.append(run().cpu())
            assert _bits_equal(outs[0], outs[1]), f"{what}: store policies differ (safe={safe})"
            res.append(outs[0])
        # (N(0,1) scores never run 8 log2 units above their row's first-tile max: the rerun re-bases nothing)
        assert _bits_equal(res[0], res[1]), f"{what}: the forced SAFE rerun differs"
    finally:
        attn_force_safe(False)
        store_policy_force(-1)
    return res


def _attn_check(O, Os, rows, Q, K, V, valid, compute, what):
    """rows: boolean [S, L] of the query rows the reference covers; O and the SAFE rerun's Os meet the bound there."""
    u = R.U_OUT[compute]
    r64, pv2, p2 = _ranges_ref(Q, K, V, valid, F64)
    r32 = _ranges_ref(Q, K, V, valid, F32)[0]
    extra = 6 * u / 3 ** 0.5 * (pv2 + p2 * r64.abs())
    for nm, o in (("", O), ("/safe", Os)):
        R.assert_close(o[rows], r64[rows], r32[rows], u, what + nm, extra=extra[rows])


@pytest.mark.parametrize("compute", MODES16)
@pytest.mark.parametrize("L", [1, 64, 65, 257])
def test_attention_forms(compute, L):
    """S * H = 3 (one sequence of three heads would hide a wrong bh / H; S = 3, H = 1 and S = 1, H = 3 both run), L
    1 / 64 / 65 / 257 (one key, a full tile, one key past it, a second query block of one row): plain, kv_len + q_len
    with a dead query block where L allows one, two key ranges, and ragged output."""
    _need_gpu()
    for S, H in ((3, 1), (1, 3)):
        Q, K, V = _attn_inputs(compute, S, H, L, 31 * L + S)
        Qd, Kd, Vd = Q.to(DEV), K.to(DEV), V.to(DEV)
        what = f"launch_head/{compute}/attn-L{L}-S{S}H{H}"
        pos = torch.arange(L)[None, :]
        allv = torch.ones(S, L, dtype=torch.bool)
        # plain
        O, Os = _attn_policies_and_safe(
            lambda: op_attention(Qd, Kd, Vd, compute=compute, q_prescaled=True, poison=True), what + "/plain")
        _attn_check(O, Os, allv, Q, K, V, allv, compute, what + "/plain")
        # kv_len / q_len: the last sequence keeps one row (L > 256: its second query block is dead and stays NaN)
        lens = torch.tensor([L] * (S - 1) + [max(1, L // 4)], dtype=torch.int32)
        live = pos < lens[:, None]
        O, Os = _attn_policies_and_safe(
            lambda: op_attention(Qd, Kd, Vd, lens, compute=compute, q_prescaled=True, poison=True, q_len=lens),
            what + "/q_len")
        _attn_check(O, Os, live, Q, K, V, live, compute, what + "/q_len")
        if L > 256:
            assert torch.isnan(O[-1, 256:]).all(), what + ": a dead query block was written"
        # two key ranges
        if L >= 64:
            st2 = L // 2 + 1
            kv1 = [min(L // 3, st2)] * S
            kv2 = [max(1, (L - st2) // 2)] * S
            valid = (pos < torch.tensor(kv1)[:, None]) | ((pos >= st2) & (pos < st2 + torch.tensor(kv2)[:, None]))
            O, Os = _attn_policies_and_safe(
                lambda: op_attention_ranges(Qd, Kd, Vd, kv1, st2, kv2, compute=compute, q_prescaled=True),
                what + "/ranges")
            _attn_check(O, Os, allv, Q, K, V, valid, compute, what + "/ranges")
        # ragged output: packed rows, every sequence at its own length
        seg = [0]
        for s in range(S):
            seg.append(seg[-1] + int(lens[s]))
        O, Os = _attn_policies_and_safe(
            lambda: op_attention_ragged(Qd, Kd, Vd, seg, compute=compute, q_prescaled=True), what + "/ragged")
        u = R.U_OUT[compute]
        r64, pv2, p2 = _ranges_ref(Q, K, V, live, F64)
        r32 = _ranges_ref(Q, K, V, live, F32)[0]
        extra = 6 * u / 3 ** 0.5 * (pv2 + p2 * r64.abs())
        pack = lambda t: torch.cat([t[s, :int(lens[s])] for s in range(S)])  # noqa: E731
        for nm, o in (("", O), ("/safe", Os)):
            assert o.shape == (seg[-1], H * 64)
            R.assert_close(o, pack(r64), pack(r32), u, what + "/ragged" + nm, extra=pack(extra))


# ---------------------------------------------------------------- probe
@pytest.mark.parametrize("compute", ["bf16"])
def test_probed_launches_keep_the_result(compute):
    """A tiny DiT: with each of the five hot classes probed in turn (the head's probed branch, its dependent load of
    the step tick) the sample is bitwise the unprobed one, and probe_read reports launches of the class."""
    _need_gpu()
    arch = configs.get_arch("DiT_tiny", text_num_embeds=64)
    inp = synthetic.make_case(B=1, ref_frames=60, total_frames=150, n_text=30, vocab=64)
    dur = torch.tensor([150])
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    m = CFM(transformer=net, num_channels=100, compute=compute).to(DEV)
    eng = m.transformer.get_engine(compute, m.device)
    skw = dict(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=dur.to(DEV), lens=inp["lens"].to(DEV),
               y0=synthetic.reference_noise(dur, 3).to(DEV), steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0,
               keep_trajectory=False)
    base = m.sample(**skw)[0].clone()
    assert torch.isfinite(base).all()
    try:
        for kclass in ("qkv", "attention", "out", "ffn1", "ffn2"):
            eng.probe(kclass)
            out = m.sample(**skw)[0].clone()
            torch.cuda.synchronize()
            n, ms = eng.probe_read()
            print(f"[launch-head] probe {kclass}: {n} launches, {ms:.4f} ms")
            assert torch.equal(out, base), f"probing {kclass} changed the result"
            assert n > 0 and ms > 0.0, (kclass, n, ms)
    finally:
        eng.probe(None)
    assert torch.equal(m.sample(**skw)[0], base)
