"""Reference for the MMDiT backbone: the case table of the fixtures tests/golden/make_golden_mmdit.py produced with the
reference's own model, and a CPU restatement of that model from the oracle's pieces (oracle/ref_cpu.py, which has no
MMDiT), written from the model definition (mmdit.py:32-262; modules.py:371-441 Attention with context_dim, 563-705
JointAttnProcessor, 763-846 MMDiTBlock, 333-347 AdaLayerNorm_Final), not from the kernels. Shared by
tests/test_mmdit.py (CPU) and tests/test_gpu_mmdit.py.

`variant` names one deliberate deviation from the model (the "wrong variant" checks of tests/test_mmdit.py): a
restatement that cannot tell these apart from the model would not pin the engine either."""

from __future__ import annotations

import torch
import torch.nn.functional as F

import golden_cases as gc
from f5_tts_amd import configs, synthetic
from oracle import ref_cpu

QK_EPS = 1e-6      # RMSNorm(dim_head, eps=1e-6), modules.py:406-407, 419-420
MAX_POS = 1024     # TextEmbedding.precompute_max_pos, mmdit.py:39
VARIANTS = ("separate_softmax", "text_rope_continues", "last_block_swapped", "no_c_mask", "mask_after_drop",
            "no_pos_clamp")

# ---------------------------------------------------------------- cases
LONGTEXT = dict(B=1, ref_frames=15, total_frames=40, n_text=1030, vocab=64)
WIDE_B2 = dict(B=2, ref_frames=[100, 60], total_frames=[300, 220], n_text=[50, 40])


def arch_of(tag):
    if tag == "tiny":
        return configs.get_arch("MMDiT_tiny", text_num_embeds=64)
    if tag == "tiny_qkn":
        return configs.get_arch("MMDiT_tiny", text_num_embeds=64, qk_norm="rms_norm")
    if tag == "wide":
        return configs.get_arch(dict(backbone="MMDiT", dim=1024, heads=16, depth=2, ff_mult=2))
    raise KeyError(tag)


# name -> (arch tag, input spec, nfe, sway, cfg, reference dtype)
SAMPLE_CASES = {
    "mmdit_tiny_sample_b1": ("tiny", gc.B1, 4, -1.0, 2.0, "fp32"),
    "mmdit_tiny_sample_b3": ("tiny", gc.B3, 4, -1.0, 2.0, "fp32"),
    "mmdit_tiny_qknorm_sample_b3": ("tiny_qkn", gc.B3, 4, -1.0, 2.0, "fp32"),
    "mmdit_tiny_nocfg_b3": ("tiny", gc.B3, 4, -1.0, 0.0, "fp32"),
    "mmdit_tiny_sample_b3_bf16": ("tiny", gc.B3, 4, -1.0, 2.0, "bf16"),
    "mmdit_tiny_sample_b3_fp16": ("tiny", gc.B3, 4, -1.0, 2.0, "fp16"),
    "mmdit_wide_sample_b2": ("wide", WIDE_B2, 2, -1.0, 2.0, "fp32"),
    "mmdit_wide_sample_b2_bf16": ("wide", WIDE_B2, 2, -1.0, 2.0, "bf16"),
}
# name -> (arch tag, input spec, options as golden_cases.FORWARD_CASES)
FORWARD_CASES = {
    "mmdit_tiny_fwd_b3": ("tiny", gc.B3, {}),
    "mmdit_tiny_fwd_b3_single": ("tiny", gc.B3, {"cfg_infer": False}),
    "mmdit_tiny_fwd_b3_dropaudio": ("tiny", gc.B3, {"cfg_infer": False, "drop_audio": True}),
    "mmdit_tiny_fwd_b3_droptext": ("tiny", gc.B3, {"cfg_infer": False, "drop_text": True}),
    "mmdit_tiny_fwd_b3_tvec": ("tiny", gc.B3, {"t": [0.1, 0.7, 0.1]}),
    "mmdit_tiny_fwd_b1_longtext": ("tiny", LONGTEXT, {}),
    # 377 positions past the clamp: with 1030 tokens only 7 are, and a missing clamp moves the output by 1.2e-3, too
    # little for the wrong-variant check of tests/test_mmdit.py (4.8e-2 here)
    "mmdit_tiny_fwd_b1_longtext1400": ("tiny", dict(LONGTEXT, n_text=1400), {}),
}
FP32_SAMPLES = [n for n, c in SAMPLE_CASES.items() if c[5] == "fp32"]


def forward_inputs(spec, seed=gc.SEED):
    """x, step_cond, text, mask of a forward case, as make_golden.run_forward forms them."""
    inp = synthetic.make_case(**spec)
    B = inp["cond"].shape[0]
    dur = inp["duration"]
    N = int(dur.max())
    cond = F.pad(inp["cond"], (0, 0, 0, N - inp["cond"].shape[1]))
    cmask = (torch.arange(N)[None] < inp["lens"][:, None])[..., None]
    step_cond = torch.where(cmask, cond, torch.zeros_like(cond))
    x = synthetic.reference_noise(dur, seed)
    mask = (torch.arange(N)[None] < dur[:, None]) if B > 1 else None
    return dict(x=x, cond=step_cond, text=inp["text"], mask=mask, duration=dur, lens=inp["lens"])


# ---------------------------------------------------------------- the model
def text_embed(W, arch, text, drop_text, variant=None):
    """TextEmbedding.forward (mmdit.py:42-63): Embedding(text + 1) of the model width + freqs_cis[min(j, 1023)], the
    filler rows (mask taken BEFORE drop_text) zeroed; not padded to the audio length, no ConvNeXt blocks."""
    text = text + 1
    if variant == "mask_after_drop" and drop_text:
        text = torch.zeros_like(text)
    fill = text == 0
    if drop_text:
        text = torch.zeros_like(text)
    e = W["text_embed.text_embed.weight"][text]
    nt = text.shape[1]
    pos = torch.arange(nt)
    if variant == "no_pos_clamp":
        fc = ref_cpu.freqs_cis_table(arch["dim"], max(nt, MAX_POS))[pos]
    else:
        fc = ref_cpu.freqs_cis_table(arch["dim"], MAX_POS)[pos.clamp(max=MAX_POS - 1)]
    e = e + fc
    if arch["text_mask_padding"]:
        e = e.masked_fill(fill[..., None], 0.0)
    return e


def audio_embed(W, x, cond, drop_audio):
    """AudioEmbedding.forward (mmdit.py:75-81): Linear(cat(x, cond)) then conv_pos_embed(h) + h (no mask)."""
    if drop_audio:
        cond = torch.zeros_like(cond)
    h = F.linear(torch.cat((x, cond), -1), W["audio_embed.linear.weight"], W["audio_embed.linear.bias"])
    y = h.transpose(1, 2)
    for j in (0, 2):
        y = F.mish(F.conv1d(y, W[f"audio_embed.conv_pos_embed.conv1d.{j}.weight"],
                            W[f"audio_embed.conv_pos_embed.conv1d.{j}.bias"], padding=15, groups=16))
    return y.transpose(1, 2) + h


def joint_attention(W, p, arch, x, c, mask, c_mask, last, variant=None):
    """JointAttnProcessor (modules.py:581-705): both streams projected by their own weights, qk_norm per stream, RoPE
    from position 0 on each stream, one softmax over [audio; text], split at row N, to_out / to_out_c, pad rows zeroed."""
    S, N, _ = x.shape
    nt = c.shape[1]
    H, Dh = arch["heads"], arch["dim_head"]

    def proj(t, n, sfx):
        return F.linear(t, W[p + n + sfx + ".weight"], W[p + n + sfx + ".bias"]).view(S, -1, H, Dh).transpose(1, 2)

    q, k, v = (proj(x, n, "") for n in ("to_q", "to_k", "to_v"))
    cq, ck, cv = (proj(c, n, "_c") for n in ("to_q", "to_k", "to_v"))
    if arch.get("qk_norm") == "rms_norm":
        q = F.rms_norm(q, (Dh,), W[p + "q_norm.weight"], QK_EPS)
        k = F.rms_norm(k, (Dh,), W[p + "k_norm.weight"], QK_EPS)
        cq = F.rms_norm(cq, (Dh,), W[p + "c_q_norm.weight"], QK_EPS)
        ck = F.rms_norm(ck, (Dh,), W[p + "c_k_norm.weight"], QK_EPS)
    cos, sin = ref_cpu.rope_cos_sin(N + nt, Dh)
    q, k = ref_cpu.apply_rope(q, cos[:N], sin[:N]), ref_cpu.apply_rope(k, cos[:N], sin[:N])
    t0 = N if variant == "text_rope_continues" else 0
    cq = ref_cpu.apply_rope(cq, cos[t0:t0 + nt], sin[t0:t0 + nt])
    ck = ref_cpu.apply_rope(ck, cos[t0:t0 + nt], sin[t0:t0 + nt])
    am = None
    if arch["attn_mask_enabled"] and mask is not None:
        am = torch.cat((mask, c_mask), 1)[:, None, None, :].expand(S, H, N + nt, N + nt)
    if variant == "separate_softmax":
        o = torch.cat((F.scaled_dot_product_attention(q, k, v), F.scaled_dot_product_attention(cq, ck, cv)), 2)
    else:
        o = F.scaled_dot_product_attention(torch.cat((q, cq), 2), torch.cat((k, ck), 2), torch.cat((v, cv), 2),
                                           attn_mask=am)
    o = o.transpose(1, 2).reshape(S, N + nt, H * Dh)
    ox = F.linear(o[:, :N], W[p + "to_out.0.weight"], W[p + "to_out.0.bias"])
    oc = None
    if not last:
        oc = F.linear(o[:, N:], W[p + "to_out_c.weight"], W[p + "to_out_c.bias"])
        if variant != "no_c_mask":
            oc = oc.masked_fill(~c_mask[..., None], 0.0)
    if mask is not None:
        ox = ox.masked_fill(~mask[..., None], 0.0)
    return ox, oc


def ffn(W, p, x):
    h = F.gelu(F.linear(x, W[p + "0.0.weight"], W[p + "0.0.bias"]), approximate="tanh")
    return F.linear(h, W[p + "2.weight"], W[p + "2.bias"])


def block(W, i, arch, x, c, t_emb, mask, c_mask, variant=None):
    """MMDiTBlock.forward (modules.py:816-846); the last block is context_pre_only: AdaLayerNorm_Final on c, chunk
    order (scale, shift), and c ends there."""
    p = f"transformer_blocks.{i}."
    last = i == arch["depth"] - 1
    st = F.silu(t_emb)
    ec = F.linear(st, W[p + "attn_norm_c.linear.weight"], W[p + "attn_norm_c.linear.bias"])
    ex = F.linear(st, W[p + "attn_norm_x.linear.weight"], W[p + "attn_norm_x.linear.bias"])
    if last:
        sc, sh = torch.chunk(ec, 2, dim=1)
        if variant == "last_block_swapped":
            sc, sh = sh, sc
        nc = ref_cpu.ln(c) * (1 + sc[:, None]) + sh[:, None]
    else:
        csh1, csc1, cg1, csh2, csc2, cg2 = torch.chunk(ec, 6, dim=1)
        nc = ref_cpu.ln(c) * (1 + csc1[:, None]) + csh1[:, None]
    sh1, sc1, g1, sh2, sc2, g2 = torch.chunk(ex, 6, dim=1)
    nx = ref_cpu.ln(x) * (1 + sc1[:, None]) + sh1[:, None]
    ox, oc = joint_attention(W, p + "attn.", arch, nx, nc, mask, c_mask, last, variant)
    if last:
        c = None
    else:
        c = c + cg1[:, None] * oc
        c = c + cg2[:, None] * ffn(W, p + "ff_c.ff.", ref_cpu.ln(c) * (1 + csc2[:, None]) + csh2[:, None])
    x = x + g1[:, None] * ox
    x = x + g2[:, None] * ffn(W, p + "ff_x.ff.", ref_cpu.ln(x) * (1 + sc2[:, None]) + sh2[:, None])
    return c, x


def mmdit_forward(W, arch, x, cond, text, t, mask, text_cache, packed=True, drop_audio=False, drop_text=False,
                  variant=None):
    """MMDiT.forward (mmdit.py:214-262): packed cond/uncond (cfg_infer) -> [2b,n,mel], or one branch with the drop
    flags -> [b,n,mel]. text_cache: the dict that plays the text_cond / text_uncond cache of one sample() call."""
    b = x.shape[0]
    t = t.reshape(-1).expand(b) if t.numel() == 1 else t
    te = ref_cpu.time_embed(W, t)
    c_mask = (text + 1) != 0
    if "cond" not in text_cache:
        text_cache["cond"] = text_embed(W, arch, text, False, variant)
        text_cache["uncond"] = text_embed(W, arch, text, True, variant)
    if packed:
        h = torch.cat((audio_embed(W, x, cond, False), audio_embed(W, x, cond, True)), 0)
        c = torch.cat((text_cache["cond"], text_cache["uncond"]), 0)
        te = torch.cat((te, te), 0)
        mask = None if mask is None else torch.cat((mask, mask), 0)
        c_mask = torch.cat((c_mask, c_mask), 0)
    else:
        h = audio_embed(W, x, cond, drop_audio)
        c = text_cache["uncond" if drop_text else "cond"]
    for i in range(arch["depth"]):
        c, h = block(W, i, arch, h, c, te, mask, c_mask, variant)
    e = F.linear(F.silu(te), W["norm_out.linear.weight"], W["norm_out.linear.bias"])
    sc, sh = torch.chunk(e, 2, dim=1)  # scale first (modules.py:343)
    h = ref_cpu.ln(h) * (1 + sc[:, None]) + sh[:, None]
    return F.linear(h, W["proj_out.weight"], W["proj_out.bias"])


def flow(W, arch, pre, text, cfg_strength, variant=None):
    """The CFG-combined flow fn(t, x) of one sample() call (cfm.py:160-191), with its text cache."""
    cache = {}

    def fn(t, x):
        if cfg_strength < 1e-5:
            return mmdit_forward(W, arch, x, pre["step_cond"], text, t, pre["mask"], cache, packed=False,
                                 variant=variant)
        p = mmdit_forward(W, arch, x, pre["step_cond"], text, t, pre["mask"], cache, variant=variant)
        pc, pu = torch.chunk(p, 2, 0)
        return pc + (pc - pu) * cfg_strength

    return fn


@torch.no_grad()
def cfm_sample(W, arch, cond, text, duration, *, lens=None, steps=32, cfg_strength=1.0, sway_sampling_coef=None,
               y0=None, variant=None):
    """ref_cpu.cfm_sample with the MMDiT backbone (Euler on the EPSS / sway grid)."""
    pre = ref_cpu.prepare(arch, cond.float(), text, duration, lens)
    fn = flow(W, arch, pre, text, cfg_strength, variant)
    t = ref_cpu.epss_sway_grid(steps, sway_sampling_coef)
    y = y0.float()
    for k in range(steps):
        y = y + (t[k + 1] - t[k]) * fn(t[k], y)
    return torch.where(pre["cond_mask"], pre["cond"], y)


def sample_inputs(spec, seed=gc.SEED):
    """Inputs of a sample case and the y0 the reference drew (fp32 noise of the rule's durations)."""
    inp = synthetic.make_case(**spec)
    dur = torch.maximum(torch.maximum((inp["text"] != -1).sum(-1), inp["lens"]) + 1, inp["duration"])
    return inp, synthetic.reference_noise(dur, seed)


def run_sample_case(name, variant=None, W=None):
    tag, spec, nfe, sway, cfg, _ = SAMPLE_CASES[name]
    arch = arch_of(tag)
    W = synthetic.make_weights_torch(arch) if W is None else W
    inp, y0 = sample_inputs(spec)
    return cfm_sample(W, arch, inp["cond"], inp["text"], inp["duration"], lens=inp["lens"], steps=nfe,
                      cfg_strength=cfg, sway_sampling_coef=sway, y0=y0, variant=variant)


@torch.no_grad()
def run_forward_case(name, variant=None):
    tag, spec, opts = FORWARD_CASES[name]
    arch = arch_of(tag)
    W = synthetic.make_weights_torch(arch)
    fi = forward_inputs(spec)
    t = torch.tensor(opts.get("t", gc.FWD_T))
    return mmdit_forward(W, arch, fi["x"], fi["cond"], fi["text"], t, fi["mask"], {},
                         packed=opts.get("cfg_infer", True), drop_audio=opts.get("drop_audio", False),
                         drop_text=opts.get("drop_text", False), variant=variant)
