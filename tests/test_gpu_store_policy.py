"""The store policy of the hot-path launches (DESIGN.md §3 'Launch boundaries') changes no value: the write-through
variants of the 64x128 / 128x128 / 192x128 GEMM kernels (EPI_QKV, EPI_RESID16, EPI_GELU_TANH, plain and in the
LayerNorm-fold forms) and of the 16-bit attention kernel give the bits of the plain-store kernels, NaN payloads
included, and write nothing the plain kernels do not write.

Op level: every buffer a launch may write starts as 0xFF bytes (NaN in fp32 and in both 16-bit types). What changed
between the two kernels is the range-checked store, so the checks are on what must stay untouched: rows past M of the
strip epilogue's ragged last tile (they would land behind the output in the workspace, whose bytes past the last buffer
must stay 0xFF), the guard rows of hs and of the strip statistics, and the O rows of dead attention waves.
Whole path: the third of three sample calls (a capture and two replays) is bitwise equal across policies, and a policy
change after a capture is seen in the engine's launch counters (the step graph is keyed by the policy)."""

import pytest
import torch

from f5_tts_amd import _lib, configs, synthetic
from f5_tts_amd.engine import attn_force_safe, gemm_force_config, op_attention, op_gemm_epi, store_policy_force
from f5_tts_amd.model import CFM, DiT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("bf16", "fp16")
G = _lib.OP_GUARD_ROWS
Q_SCALE = 0.125 * 1.4426950408889634
# one full 64-row tile plus a ragged one (two 64x128 tiles, one ragged 128- or 192-row tile); 200: a full 192-row
# tile plus a ragged one, and four 64-row tiles
ROWS = (70, 200)
K = 128  # two 64-column stages


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _al(n):
    return (n + 255) // 256 * 256


def _tail_untouched(ws, sizes, what):
    """sizes: the byte sizes of the workspace buffers in the order f5h_op_gemm_epi / f5h_op_attention take them (each
    starts on a multiple of 256). Every byte past the last buffer still holds the 0xFF fill."""
    end = sum(_al(s) for s in sizes[:-1]) + sizes[-1]
    assert end < ws.numel()
    assert bool((ws[end:] == 0xFF).all()), what + ": bytes behind the last output buffer were written"


def _inputs(M, N, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    A[3, 5] = float("nan")  # a NaN row: payloads must agree too
    W = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    return g, A.to(DEV), W.to(DEV), bias.to(DEV)


def _both_policies(run):
    """run() under plain and under write-through stores: (plain, write-through) results."""
    outs = []
    try:
        for mode in (0, 1):
            store_policy_force(mode)
            outs.append(run())
    finally:
        store_policy_force(-1)
    return outs


def _flat(res):
    return [t for t in (res if isinstance(res, tuple) else (res,)) if t is not None]


def _compare(plain, wt, what):
    for i, (a, b) in enumerate(zip(_flat(plain), _flat(wt))):
        assert _bits_equal(a.cpu(), b.cpu()), f"{what}: output {i} differs between plain and write-through stores"


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("cfg", [0, 1, 5])
def test_gemm_epilogues_bitwise_under_both_policies(compute, cfg):
    _need_gpu()
    try:
        gemm_force_config(cfg)
        for M in ROWS:
            what = f"{compute}/cfg{cfg}/M{M}"
            N = 128
            g, A, W, bias = _inputs(M, N, 100 * cfg + M)
            gate = torch.randn(N, generator=g).to(DEV)
            C0 = torch.randn(M, N, generator=g).to(DEV)
            base = [_al(N * K * 2), M * K * 2]  # W (rows padded to 128), A

            # EPI_RESID16 in place, EPI_GELU_TANH: the output is the workspace's last buffer
            for epi, kw in (("resid16", dict(C=C0, gate=gate)), ("gelu_tanh", {})):
                p, w = _both_policies(lambda: op_gemm_epi(epi, A, W, bias=bias, compute=compute, ws_fill=0xFF,
                                                          return_ws=True, **kw))
                _compare(p[0], w[0], f"{what}/{epi}")
                assert torch.isnan(p[0][3]).all() and torch.isfinite(p[0][4:]).all(), what
                for ws in (p[1], w[1]):
                    _tail_untouched(ws, base + [M * N * 2], f"{what}/{epi}")

            # the fold producer: C, hs, strip statistics; guard rows past M stay NaN under both policies
            sc = (0.3 * torch.randn(N, generator=g)).to(DEV)
            p, w = _both_policies(lambda: op_gemm_epi("resid16", A, W, bias=bias, C=C0, gate=gate, compute=compute,
                                                      ln_producer=True, hs_scale=sc, poison=True, ws_fill=0xFF,
                                                      return_ws=True))
            _compare(p[0], w[0], what + "/producer")
            for (Cf, hs, parts), ws in (p, w):
                assert hs.shape == (M + G, N) and parts.shape == (M + G, N // 64, 2)
                assert torch.isnan(hs[M:]).all() and torch.isnan(parts[M:]).all(), what + ": guard rows were written"
                live = torch.arange(M) != 3
                assert torch.isfinite(hs[:M][live]).all() and torch.isfinite(parts[:M][live]).all(), what
                _tail_untouched(ws, base + [M * N * 2, (M + G) * N * 2], what + "/producer")

            # the fold consumers (their statistics come from the producer above; K / 64 = 2 strips)
            gA = torch.randn(M, K, generator=g).to(DEV)
            parts_in = torch.stack((0.1 * torch.randn(M, 2, generator=g), 1.0 + torch.rand(M, 2, generator=g)), -1).to(DEV)
            parts_in[5] = float("nan")
            u, v = torch.randn(N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
            ckw = dict(ln_part_in=parts_in, ln_u=u, ln_v=v, ln_eps=1e-6)
            p, w = _both_policies(lambda: op_gemm_epi("gelu_tanh", gA, W, bias=bias, compute=compute, ws_fill=0xFF,
                                                      return_ws=True, **ckw))
            _compare(p[0], w[0], what + "/consumer-gelu")
            for ws in (p[1], w[1]):
                _tail_untouched(ws, base + [M * N * 2], what + "/consumer-gelu")

            # EPI_QKV, N = 384 (H = 2), two sequences, RoPE on the first head, q scaled: plain and fold consumer
            H, Nq, L = 2, 384, M // 2
            g, A, Wq, bq = _inputs(M, Nq, 100 * cfg + M + 1)
            uq, vq = torch.randn(Nq, generator=g).to(DEV), torch.randn(Nq, generator=g).to(DEV)
            qkw = dict(bias=bq, compute=compute, seq_len=L, heads=H, rope_heads=1, q_scale=Q_SCALE, ws_fill=0xFF,
                       return_ws=True)
            sizes = [_al(Nq * K * 2), M * K * 2, L * 256] + [M * H * 64 * 2] * 3
            for nm, kw in (("qkv", {}), ("consumer-qkv", dict(ln_part_in=parts_in, ln_u=uq, ln_v=vq, ln_eps=1e-6))):
                p, w = _both_policies(lambda: op_gemm_epi("qkv", A, Wq, **qkw, **kw))
                _compare(p[0], w[0], f"{what}/{nm}")
                assert not torch.isnan(p[0][0][:, :, 6:]).any(), what  # every live row written (rows 3 / 5: NaN inputs)
                for ws in (p[1], w[1]):
                    _tail_untouched(ws, sizes, f"{what}/{nm}")
    finally:
        gemm_force_config(-1)


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("N", [70, 300])
def test_attention_bitwise_under_both_policies(compute, N):
    """N = 70: one query block with six dead-row waves and a ragged key tile; N = 300: two query blocks, the second with
    44 live rows. O starts as NaN (the poisoned workspace), so a row the write-through form failed to store, or a
    foreign key row it read, shows; with q_len the rows of dead waves stay NaN under both policies."""
    _need_gpu()
    S, H = 2, 2
    g = torch.Generator(device="cpu").manual_seed(N)
    Q, Kk, V = (torch.randn(S, H, N, 64, generator=g).to(DEV) for _ in range(3))
    Q = Q * Q_SCALE  # the engine's form: q carries scale * log2(e)
    n = Q.numel()
    cases = {"full": {}, "q_len": dict(q_len=torch.tensor([N, 40]), kv_len=torch.tensor([N, 40]))}
    for nm, kw in cases.items():
        for safe in (False, True):
            try:
                attn_force_safe(safe)
                p, w = _both_policies(lambda: op_attention(Q, Kk, V, compute=compute, q_prescaled=True, poison=True,
                                                           return_ws=True, **kw))
            finally:
                attn_force_safe(False)
            what = f"attention/{compute}/N{N}/{nm}/safe{int(safe)}"
            _compare(p[0], w[0], what)
            for O, ws in (p, w):
                if nm == "full":
                    assert torch.isfinite(O).all(), what
                else:
                    assert torch.isfinite(O[0]).all() and torch.isfinite(O[1, :40]).all(), what
                    assert torch.isnan(O[1, 64:]).all(), what + ": a dead wave's rows were written"
                _tail_untouched(ws, [n * 8], what)


def _tiny():
    arch = configs.get_arch("DiT_tiny", text_num_embeds=64)
    inp = synthetic.make_case(B=1, ref_frames=60, total_frames=150, n_text=30, vocab=64)
    return arch, inp, torch.tensor([150])


def _base2():
    arch = configs.get_arch("F5TTS_v1_Base", depth=2)
    inp = synthetic.make_case(B=1, ref_frames=[120], total_frames=[333], n_text=[40])
    return arch, inp, torch.tensor([333])


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("case", [_tiny, _base2], ids=["DiT_tiny", "F5TTS_v1_Base-depth2"])
def test_sample_bitwise_under_both_policies(compute, case):
    """Fold on, three sample calls per policy (a capture and two graph replays): the third is bitwise equal across
    policies. The engine's counters of hot launches enqueued with write-through / plain stores move only on eager
    launches and captures, so they also show that a policy change after a capture is not served by the old graph."""
    _need_gpu()
    arch, inp, dur = case()
    kw = {k: v for k, v in arch.items() if k not in ("backbone", "text_num_embeds", "mel_dim")}
    net = DiT(**kw, text_num_embeds=arch["text_num_embeds"], mel_dim=arch["mel_dim"])
    net.load_state_dict(synthetic.make_weights_torch(arch), strict=False)
    m = CFM(transformer=net, num_channels=100, compute=compute).to(DEV)
    eng = m.transformer.get_engine(compute, m.device)
    y0 = synthetic.reference_noise(dur, 3)
    skw = dict(cond=inp["cond"].to(DEV), text=inp["text"].to(DEV), duration=dur.to(DEV), lens=inp["lens"].to(DEV),
               y0=y0.to(DEV), steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, keep_trajectory=False)
    hot = 5 * arch["depth"]  # hot launches of one backbone pass
    third = {}
    try:
        eng.set_ln_fold(True)
        for mode in (1, 0, -1):
            eng.set_store_policy(mode)
            wt0, pl0 = eng.store_policy_stats()
            cap0 = eng.graph_stats()["captures"]
            for _ in range(3):
                out = m.sample(**skw)[0]
            third[mode] = out.clone()
            wt1, pl1 = eng.store_policy_stats()
            assert eng.graph_stats()["captures"] > cap0, f"policy {mode}: the earlier policy's step graph was replayed"
            # -1: a single utterance of this size is one wave of workgroups in every hot launch
            if mode == 0:
                assert pl1 - pl0 >= hot and wt1 == wt0, (mode, wt1 - wt0, pl1 - pl0)
            else:
                assert wt1 - wt0 >= hot and pl1 == pl0, (mode, wt1 - wt0, pl1 - pl0)
    finally:
        eng.set_store_policy(-1)
    assert torch.isfinite(third[0]).all()
    assert torch.equal(third[1], third[0]), "write-through stores changed the result"
    assert torch.equal(third[-1], third[0]), "the automatic policy changed the result"
