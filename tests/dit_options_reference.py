"""Reference for the DiT / UNetT options qk_norm="rms_norm", long_skip_connection and
text_embedding_average_upsampling: the CPU oracle's pieces (oracle/ref_cpu.py, which has none of the three) composed
with the options as the reference model applies them (modules.py:286-305, 402-407, 493-496; dit.py:41-84, 131-137,
228, 354-365), plus the op-level references and seeded inputs of the QKV epilogue with the norm and of the
upsampling kernel, shared by tests/test_dit_options.py (CPU) and tests/test_gpu_dit_options.py.

Every function here is written from the model definition, not from the kernels."""

from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

import op_cases as C
import op_reference as R
from f5_tts_amd import synthetic
from oracle import ref_cpu

QK_EPS = 1e-6  # RMSNorm(dim_head, eps=1e-6), modules.py:406-407


# ---------------------------------------------------------------- model pieces with the options
def attention(W, p, arch, x, mask, rope):
    """ref_cpu.attention with F.rms_norm of q and k over the head channels ahead of apply_rope (modules.py:493-509):
    every head, also those pe_attn_head leaves unrotated; v untouched."""
    S, N, _ = x.shape
    H, Dh = arch["heads"], arch["dim_head"]
    q = F.linear(x, W[p + "to_q.weight"], W[p + "to_q.bias"]).view(S, N, H, Dh).transpose(1, 2)
    k = F.linear(x, W[p + "to_k.weight"], W[p + "to_k.bias"]).view(S, N, H, Dh).transpose(1, 2)
    v = F.linear(x, W[p + "to_v.weight"], W[p + "to_v.bias"]).view(S, N, H, Dh).transpose(1, 2)
    if arch.get("qk_norm") == "rms_norm":
        q = F.rms_norm(q, (Dh,), W[p + "q_norm.weight"], QK_EPS)
        k = F.rms_norm(k, (Dh,), W[p + "k_norm.weight"], QK_EPS)
    elif arch.get("qk_norm") is not None:
        raise ValueError(f"Unimplemented qk_norm: {arch['qk_norm']}")
    cos, sin = rope
    pn = arch["pe_attn_head"]
    if pn is None:
        q, k = ref_cpu.apply_rope(q, cos, sin), ref_cpu.apply_rope(k, cos, sin)
    else:
        q = torch.cat((ref_cpu.apply_rope(q[:, :pn], cos, sin), q[:, pn:]), 1)
        k = torch.cat((ref_cpu.apply_rope(k[:, :pn], cos, sin), k[:, pn:]), 1)
    am = None
    if arch["attn_mask_enabled"] and mask is not None:
        am = mask[:, None, None, :].expand(S, H, N, N)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=am)
    o = o.transpose(1, 2).reshape(S, N, H * Dh)
    o = F.linear(o, W[p + "to_out.0.weight"], W[p + "to_out.0.bias"])
    if mask is not None:
        o = o.masked_fill(~mask[..., None], 0.0)
    return o


def dit_block(W, i, arch, x, t_emb, mask, rope):
    p = f"transformer_blocks.{i}."
    e = F.linear(F.silu(t_emb), W[p + "attn_norm.linear.weight"], W[p + "attn_norm.linear.bias"])
    sh1, sc1, g1, sh2, sc2, g2 = torch.chunk(e, 6, dim=1)
    a = ref_cpu.ln(x) * (1 + sc1[:, None]) + sh1[:, None]
    x = x + g1[:, None] * attention(W, p + "attn.", arch, a, mask, rope)
    f = ref_cpu.ln(x) * (1 + sc2[:, None]) + sh2[:, None]
    return x + g2[:, None] * ref_cpu.ffn(W, p + "ff.", f)


def average_upsample_text_by_mask(text, text_mask, target_lens):
    """TextEmbedding.average_upsample_text_by_mask (dit.py:55-84) restated: per sequence the T valid rows (text_mask,
    not necessarily a prefix) are spread over the first audio_len frames, the first T - rem repeated base times and
    the last rem repeated base + 1 times (base, rem = divmod(audio_len, T)); every other frame is zero."""
    out = torch.zeros_like(text)
    for i in range(text.shape[0]):
        T, audio_len = int(text_mask[i].sum()), int(target_lens[i])
        if T == 0 or audio_len <= 0:
            continue
        valid = text[i, torch.where(text_mask[i])[0]]
        base, rem = divmod(audio_len, T)
        reps = torch.tensor([base + (1 if j >= T - rem else 0) for j in range(T)])
        idx = torch.repeat_interleave(torch.arange(T), reps)[:audio_len]
        out[i, :audio_len] = valid[idx]
    return out


def text_fill_mask(text, seq_len):
    """The filler mask of TextEmbedding.forward (dit.py:87-104): after the +1 shift, the cut / pad to the frame count
    and the per-sample valid range; taken before drop_text."""
    text = text + 1
    per_sample = torch.is_tensor(seq_len)
    n = int(seq_len.max()) if per_sample else int(seq_len)
    text = F.pad(text[:, :n], (0, max(n - text.shape[1], 0)), value=0)
    if per_sample:
        text = text.masked_fill(~(torch.arange(n)[None, :] < seq_len[:, None]), 0)
    return text == 0


def text_embed_dit(W, arch, text, seq_len, drop_text):
    e = ref_cpu.text_embed_dit(W, arch, text, seq_len, drop_text)
    if arch.get("text_embedding_average_upsampling"):
        assert arch["text_mask_padding"], "text_embedding_average_upsampling requires text_mask_padding to be True"
        n = e.shape[1]
        target = seq_len if torch.is_tensor(seq_len) else torch.full((e.shape[0],), int(seq_len), dtype=torch.long)
        e = average_upsample_text_by_mask(e, ~text_fill_mask(text, seq_len)[:, :n], target)
    return e


def dit_forward(W, arch, x, cond, text, t, mask, text_cache, packed=True, drop_audio=False, drop_text=False):
    """ref_cpu.dit_forward with the three options (dit.py:319-370)."""
    b, n = x.shape[:2]
    t = t.reshape(-1).expand(b) if t.numel() == 1 else t
    te = ref_cpu.time_embed(W, t)
    if "cond" not in text_cache:
        seq = n if mask is None else mask.sum(1)
        text_cache["cond"] = text_embed_dit(W, arch, text, seq, False)
        text_cache["uncond"] = text_embed_dit(W, arch, text, seq, True)
    if packed:
        xc = ref_cpu.input_embed(W, x, cond, text_cache["cond"], False, mask)
        xu = ref_cpu.input_embed(W, x, cond, text_cache["uncond"], True, mask)
        h = torch.cat((xc, xu), 0)
        te = torch.cat((te, te), 0)
        m2 = None if mask is None else torch.cat((mask, mask), 0)
    else:
        h = ref_cpu.input_embed(W, x, cond, text_cache["uncond" if drop_text else "cond"], drop_audio, mask)
        m2 = mask
    rope = ref_cpu.rope_cos_sin(n, arch["dim_head"])
    kept = h
    for i in range(arch["depth"]):
        h = dit_block(W, i, arch, h, te, m2, rope)
    if arch.get("long_skip_connection"):
        h = F.linear(torch.cat((h, kept), -1), W["long_skip_connection.weight"])
    e = F.linear(F.silu(te), W["norm_out.linear.weight"], W["norm_out.linear.bias"])
    sc, sh = torch.chunk(e, 2, dim=1)
    h = ref_cpu.ln(h) * (1 + sc[:, None]) + sh[:, None]
    return F.linear(h, W["proj_out.weight"], W["proj_out.bias"])


def unett_forward(W, arch, x, cond, text, t, mask, text_cache, packed=True, drop_audio=False, drop_text=False):
    """ref_cpu.unett_forward with qk_norm in its attention (unett.py:244-307)."""
    b, n = x.shape[:2]
    t = t.reshape(-1).expand(b) if t.numel() == 1 else t
    te = ref_cpu.time_embed(W, t)
    if "cond" not in text_cache:
        text_cache["cond"] = ref_cpu.text_embed_unett(W, arch, text, n, False)
        text_cache["uncond"] = ref_cpu.text_embed_unett(W, arch, text, n, True)
    if packed:
        xc = ref_cpu.input_embed(W, x, cond, text_cache["cond"], False, None)
        xu = ref_cpu.input_embed(W, x, cond, text_cache["uncond"], True, None)
        h = torch.cat((xc, xu), 0)
        te = torch.cat((te, te), 0)
        m2 = None if mask is None else torch.cat((mask, mask), 0)
    else:
        h = ref_cpu.input_embed(W, x, cond, text_cache["uncond" if drop_text else "cond"], drop_audio, None)
        m2 = mask
    h = torch.cat((te[:, None], h), 1)
    if m2 is not None:
        m2 = F.pad(m2, (1, 0), value=True)
    rope = ref_cpu.rope_cos_sin(n + 1, arch["dim_head"])
    depth = arch["depth"]
    skips = []
    for i in range(depth):
        p = f"layers.{i}."
        if i < depth // 2:
            skips.append(h)
        else:
            h = F.linear(torch.cat((h, skips.pop()), -1), W[p + "0.weight"])
        h = attention(W, p + "2.", arch, ref_cpu.rms_norm(h, W[p + "1.g"]), m2, rope) + h
        h = ref_cpu.ffn(W, p + "4.", ref_cpu.rms_norm(h, W[p + "3.g"])) + h
    h = ref_cpu.rms_norm(h, W["norm_out.g"])[:, 1:]
    return F.linear(h, W["proj_out.weight"], W["proj_out.bias"])


@torch.no_grad()
def cfm_sample(W, arch, inp, y0, steps, cfg_strength, sway):
    """fp32 CFM.sample (Euler, cfm.py:160-223) over the forwards above: the output [B, N, mel]."""
    text = inp["text"]
    pre = ref_cpu.prepare(arch, inp["cond"].float(), text, inp["duration"], inp["lens"])
    fwd = dit_forward if arch["backbone"] == "DiT" else unett_forward
    cache = {}
    t = ref_cpu.epss_sway_grid(steps, sway)
    y = y0.float()
    for k in range(steps):
        if cfg_strength < 1e-5:
            v = fwd(W, arch, y, pre["step_cond"], text, t[k], pre["mask"], cache, packed=False)
        else:
            pc, pu = torch.chunk(fwd(W, arch, y, pre["step_cond"], text, t[k], pre["mask"], cache), 2, 0)
            v = pc + (pc - pu) * cfg_strength
        y = y + (t[k + 1] - t[k]) * v
    return torch.where(pre["cond_mask"], pre["cond"], y)


# ---------------------------------------------------------------- end-to-end cases
SWAY, CFG, STEPS, SEED = -1.0, 2.0, 3, 7
QK_SCALE = 4.0  # the 16-bit qk_norm cases multiply to_q / to_k weights and biases by this (see the separation test)
BASE = {"tiny": ("DiT_tiny", dict(text_num_embeds=64)), "utiny": ("UNetT_tiny", dict(text_num_embeds=64))}


def arch_with(tag, **options):
    from f5_tts_amd import configs

    name, kw = BASE[tag]
    return configs.get_arch(name, **kw, **options)


def weights_for(arch, qk_scale=1.0):
    W = synthetic.make_weights_torch(arch)
    if qk_scale != 1.0:
        for k in W:
            if ".to_q." in k or ".to_k." in k:
                W[k] = W[k] * qk_scale
    return W


def noise_for(inp, seed=SEED):
    dur = torch.maximum(torch.maximum((inp["text"] != -1).sum(-1), inp["lens"]) + 1, inp["duration"])
    return synthetic.reference_noise(dur, seed)


def _hashable(d):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in d.items()))


@functools.lru_cache(maxsize=None)
def _case(tag, spec_items, opt_items, qk_scale, hole):
    spec = {k: (list(v) if isinstance(v, tuple) else v) for k, v in spec_items}
    arch = arch_with(tag, **dict(opt_items))
    inp = synthetic.make_case(**spec)
    if hole:  # one interior padding token: the valid tokens are no prefix
        inp = dict(inp, text=inp["text"].clone())
        inp["text"][0, 3] = -1
    y0 = noise_for(inp)
    W = weights_for(arch, qk_scale)
    return dict(arch=arch, inp=inp, y0=y0, W=W, out=cfm_sample(W, arch, inp, y0, STEPS, CFG, SWAY))


def case(tag, spec, options, qk_scale=1.0, hole=False):
    """One oracle run per (arch, inputs, options), shared by the tests that compare with it: arch, inputs, y0, the
    weights and the fp32 output."""
    return _case(tag, _hashable(spec), _hashable(options), float(qk_scale), bool(hole))


# ---------------------------------------------------------------- QKV epilogue with the norm (op level)
WRONG_QKN = ("gain_after_rope", "rms_over_all_heads", "norm_on_v", "wk_for_q", "eps_1e-5")
QKN_K = 128
# (heads, rope_heads, bias): H = 2 -> q | k | v are one 128-column tile each (whole-column tiles, the strip epilogue);
# H = 3 -> N = 576 is no multiple of 128 (the general epilogue). rope_heads H and 1; q_scale on throughout.
QKN_CASES = [(H, rh, bias) for H in (2, 3) for rh in (H, 1) for bias in (True, False)]
ROW_ZERO, ROW_SMALL, ROW_LARGE = 3, 4, 5


@functools.lru_cache(maxsize=None)
def qkn_case(compute, H, rope_heads, bias_on):
    """S = 2 sequences of L = 70 rows (strips straddle the sequence seam, the last row tile is ragged), K = 128. Row 3:
    all-zero activations (with no bias q = k = 0); row 4: activations of 1e-3 (mean(q^2) ~ the 1e-6 epsilon); row 5:
    activations of 1e2."""
    M, N = C.QKV_S * C.QKV_L, 3 * H * 64
    g = C._gen(11, H, rope_heads, bias_on)
    A = torch.randn(M, QKN_K, generator=g)
    A[ROW_ZERO] = 0.0
    A[ROW_SMALL] *= 1e-3
    A[ROW_LARGE] *= 1e2
    W = torch.randn(N, QKN_K, generator=g) / QKN_K ** 0.5
    bias = torch.randn(N, generator=g) if bias_on else None
    wq = 1.0 + 0.3 * torch.randn(64, generator=g)
    wk = 1.0 + 0.3 * torch.randn(64, generator=g)
    return dict(A=A, W=W, bias=bias, A_read=R.rnd(A, compute), W_read=R.rnd(W, compute), H=H, rope_heads=rope_heads,
                q_scale=C.Q_SCALE, wq=wq, wk=wk, L=C.QKV_L, u_out=R.U_OUT[compute])


def qk_norm_pre(pre, heads, wq, wk, eps=QK_EPS, dtype=torch.float64, variant=None, gain=True):
    """The pre-activation [M, 3 heads 64] (bias included) with q and k normalised per (row, head):
    x rsqrt(mean_64(x^2) + eps) w. gain=False leaves the gain out (the gain_after_rope variant applies it later)."""
    M = pre.shape[0]
    x = pre.to(dtype).reshape(M, 3, heads, 64)
    if variant == "eps_1e-5":
        eps = 1e-5
    ms = x.square().mean(dim=(-2, -1) if variant == "rms_over_all_heads" else -1, keepdim=True)
    n = x * torch.rsqrt(ms + eps)
    if gain:
        wq, wk = wq.to(dtype), wk.to(dtype)
        n = n * torch.stack((wk if variant == "wk_for_q" else wq, wk, wk))[:, None, :]
    last = 3 if variant == "norm_on_v" else 2
    return torch.cat((n[:, :last], x[:, last:]), dim=1).reshape(M, -1)


def qkv_norm_from_pre(pre, c, rope, dtype, variant=None):
    """(q, k, v) [S,H,L,64] from the pre-activation: the norm, then op_reference.gemm_epi's RoPE / q scale / scatter."""
    after = variant == "gain_after_rope"
    x = qk_norm_pre(pre, c["H"], c["wq"], c["wk"], dtype=dtype, variant=variant, gain=not after)
    q, k, v = R.gemm_epi("qkv", None, None, pre=x, seq_len=c["L"], heads=c["H"], rope_heads=c["rope_heads"],
                         q_scale=c["q_scale"], rope=rope, dtype=dtype)
    if after:
        q, k = q * c["wq"].to(dtype), k * c["wk"].to(dtype)
    return q, k, v


def qkn_ref(c, rope, dtype, variant=None):
    pre = R.gemm_epi("store", c["A_read"], c["W_read"], c["bias"], dtype=dtype)
    return qkv_norm_from_pre(pre, c, rope, dtype, variant)


QKN_FOLD = (70, 768, 1, C.Q_SCALE)  # (seq_len, d, rope_heads, q_scale) of op_cases.FOLD_QKV_CASES, heads = FOLD_QKV_H


@functools.lru_cache(maxsize=None)
def qkn_fold_case(compute):
    """The LayerNorm-fold consumer inputs of op_cases (hs, strip partials, u, v) with the norm's gains added."""
    L, d, rh, qs = QKN_FOLD
    c = dict(C.fold_cons_case(compute, "ln", 2 * L, d, 3 * C.FOLD_QKV_H * 64))
    g = C._gen(12, d)
    c.update(H=C.FOLD_QKV_H, rope_heads=rh, q_scale=qs, L=L, wq=1.0 + 0.3 * torch.randn(64, generator=g),
             wk=1.0 + 0.3 * torch.randn(64, generator=g))
    return c


def qkn_fold_ref(c, rope, dtype, variant=None):
    """op_reference.fold_consumer (x = rstd (hs W^T - mean u) + v + bias) followed by the norm, RoPE and the q scale."""
    pre = R.fold_consumer("store", c["A"], c["W"], c["bias"], c["parts"], c["u"], c["v"], c["eps"], dtype=dtype)
    return qkv_norm_from_pre(pre, c, rope, dtype, variant)


# ---------------------------------------------------------------- upsampling kernel (op level)
UP_S, UP_N, UP_TD, UP_NT = 3, 40, 64, 30
UP_LENS = (40, 23, 7)     # target lengths: the full frame count, T = audio_len, and a short sequence with no token
UP_VALID = (5, 23, 0)     # valid tokens: 40 = 8 x 5 but with a hole (below); 23 / 23 -> base 1, rem 0; none


@functools.lru_cache(maxsize=None)
def upsample_case():
    """Sequence 0: 6 token slots of which slot 2 is padding (5 valid, not a prefix), 40 frames: base 8, rem 0 — and,
    with target 39 in the second call of the test, base 7, rem 4. Sequence 1: 23 tokens over 23 frames (T =
    audio_len) with more tokens past frame 23 that the valid range cuts. Sequence 2: no valid token."""
    g = C._gen(13)
    text = torch.full((UP_S, UP_NT), -1, dtype=torch.int64)
    text[0, :6] = torch.randint(0, 60, (6,), generator=g)
    text[0, 2] = -1
    text[1, :UP_NT] = torch.randint(0, 60, (UP_NT,), generator=g)
    te = torch.randn(UP_S, UP_N, UP_TD, generator=g)
    return dict(text=text, te=te, lens=torch.tensor(UP_LENS, dtype=torch.long))


def upsample_ref(c, lens=None):
    """lens [S]: each sequence's frame count (default: the case's own)."""
    lens = c["lens"] if lens is None else lens
    mask = ~text_fill_mask(c["text"], lens)
    mask = F.pad(mask, (0, UP_N - mask.shape[1]), value=False)
    return average_upsample_text_by_mask(c["te"], mask, lens)
