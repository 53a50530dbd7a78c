"""MMDiT backbone plugin (engine-backed): joint text-audio attention.

Same constructor signature and state-dict names as the reference MMDiT
(`src/f5_tts/model/backbones/mmdit.py:87-133`): a text stream of the model's width
(`text_embed`, positions clamped at 1023), an audio stream (`audio_embed`: Linear over
cat(x, cond) + conv position embedding) and MM-DiT blocks that project both streams with
their own weights, rotate them independently, attend them as one sequence and split them
again; the last block only pre-normalises the text stream. The forward pass is the HIP engine.

`attn_mask_enabled=True` together with a plain batch mask (B > 1) raises NotImplementedError: the
joint sequence's valid keys are not a prefix. With B = 1 or no mask the flag has
no effect in the reference either and is accepted; an isolated call (`isolate=True`) masks the audio
range [0, dur) and the text range [N, N + text length) itself and is served.
"""

from __future__ import annotations

from .base import EngineBackbone


class MMDiT(EngineBackbone):
    backbone_name = "MMDiT"

    def __init__(self, *, dim, depth=8, heads=8, dim_head=64, dropout=0.1, ff_mult=4, mel_dim=100,
                 text_num_embeds=256, text_mask_padding=True, qk_norm=None, checkpoint_activations=False,
                 attn_backend="torch", attn_mask_enabled=False):
        super().__init__()
        del dropout, attn_backend, checkpoint_activations  # no effect on inference arithmetic
        self._setup(dict(
            backbone="MMDiT", dim=dim, depth=depth, heads=heads, dim_head=dim_head, ff_mult=ff_mult, mel_dim=mel_dim,
            text_num_embeds=text_num_embeds, text_mask_padding=text_mask_padding, qk_norm=qk_norm,
            attn_mask_enabled=attn_mask_enabled,
        ))

    def forward(self, x, cond, text, time, mask=None, drop_audio_cond=False, drop_text=False, cfg_infer=False,
                cache=False, compute: str | None = None, isolate: bool = False):
        if self.arch.get("attn_mask_enabled") and mask is not None and not (isolate and x.shape[0] > 1):
            from ...engine import _refuse_mmdit_masked

            _refuse_mmdit_masked(self.arch, True)  # before any device work (engine creation included)
        return super().forward(x, cond, text, time, mask=mask, drop_audio_cond=drop_audio_cond, drop_text=drop_text,
                               cfg_infer=cfg_infer, cache=cache, compute=compute, isolate=isolate)
