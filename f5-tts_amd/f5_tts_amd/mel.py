"""Vocos log-mel front end on the HIP engine (reference `model/modules.py:80-151`).

`MelSpec` keeps the reference module's constructor and call surface (wav [B, L] or [B, 1, L] ->
log-mel [B, n_mels, 1 + L // hop]) and runs `f5h_mel_forward` (include/f5h.h): reflect-padded
frames, DFT and HTK filterbank as fp32 MFMA GEMMs, magnitude and clamp/log kernels. CFM.sample
calls it on raw-audio conditioning (cfm.py:106-108). There is no PyTorch fallback; the CPU
restatement used to check it lives in oracle/mel_cpu.py. `forward_ragged` takes waves of unequal length
(`f5h_mel_forward_ragged`) and returns the zero-padded, frame-major batch of their log-mels that `CFM.sample` takes.
"""

from __future__ import annotations

import ctypes
import threading

import torch
from torch import nn

from . import _lib


class MelSpec(nn.Module):
    def __init__(self, n_fft=1024, hop_length=256, win_length=1024, n_mel_channels=100, target_sample_rate=24_000,
                 mel_spec_type="vocos"):
        super().__init__()
        if mel_spec_type != "vocos":
            raise NotImplementedError("only the vocos mel front end is provided (bigvgan's vocoder is not shipped)")
        if win_length != n_fft:
            raise NotImplementedError("win_length must equal n_fft (the vocos front end)")
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.n_mel_channels, self.target_sample_rate = n_mel_channels, target_sample_rate
        self._h = {}
        self._lock = threading.Lock()

    def _engine(self, device: torch.device):
        h = self._h.get(device.index)
        if h is None:
            a = _lib.MelArch(self.n_fft, self.hop_length, self.n_mel_channels, self.target_sample_rate)
            h = ctypes.c_void_p()
            with torch.cuda.device(device):
                _lib.check(_lib.lib().f5h_mel_create(ctypes.byref(a), device.index, ctypes.byref(h)), "f5h_mel_create")
            self._h[device.index] = h
        return h

    def forward(self, wav: torch.Tensor) -> torch.Tensor:
        if wav.ndim == 3:
            wav = wav.squeeze(1)
        assert wav.ndim == 2
        if wav.device.type != "cuda":
            raise RuntimeError("MelSpec runs on the HIP engine: move the waveform to a GPU device")
        dev = torch.device("cuda", wav.device.index if wav.device.index is not None else torch.cuda.current_device())
        B, L = wav.shape
        wav = wav.to(torch.float32).contiguous()
        T = 1 + L // self.hop_length
        out = torch.empty(B, self.n_mel_channels, T, dtype=torch.float32, device=dev)
        with self._lock:
            h = self._engine(dev)
            L_ = _lib.lib()
            ws = torch.empty(max(int(L_.f5h_mel_workspace_size(h, B, L)), 256), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(L_.f5h_mel_forward(h, _lib.stream_handle(dev), B, L, wav.data_ptr(), out.data_ptr(),
                                              ws.data_ptr(), ws.numel()), "f5h_mel_forward")
        return out

    def forward_ragged(self, wavs, lens=None, length=None):
        """Waves of unequal length in one pass (`f5h_mel_forward_ragged`): `wavs` is a list of 1-D or [1, L_i]
        device tensors, or a padded [B, Lmax] tensor with host `lens` (ints, a list or a CPU tensor; a device
        tensor raises ValueError). Returns (cond [B, T, n_mels], frames): wave i gives frames[i] = 1 + L_i // hop
        frames, reflected at its own end, followed by exact zeros up to T = `length` (default: the longest).
        `cond` is the frame-major batch `CFM.sample` takes and equals the zero-padded per-wave log-mels bit for
        bit; samples beyond `lens[i]` of a padded input are never read."""
        if torch.is_tensor(wavs):
            if wavs.ndim == 3:
                wavs = wavs.squeeze(1)
            if wavs.ndim != 2:
                raise ValueError(f"a padded wave batch must be [B, Lmax], got {tuple(wavs.shape)}")
            B, Lmax = wavs.shape
            if B < 1:
                raise ValueError("forward_ragged needs at least one wave")
            lens = _lib.host_ints(Lmax if lens is None else lens, B, "lens")
        else:
            wavs = [w.squeeze(0) if w.ndim == 2 and w.shape[0] == 1 else w for w in wavs]
            if not wavs or any(w.ndim != 1 for w in wavs):
                raise ValueError("wavs must be a non-empty list of 1-D (or [1, L]) tensors")
            B = len(wavs)
            if lens is not None and _lib.host_ints(lens, B, "lens") != [w.shape[0] for w in wavs]:
                raise ValueError("lens differ from the lengths of the listed waves")
            lens = [w.shape[0] for w in wavs]
            Lmax = max(lens)
        for i, n in enumerate(lens):
            if n <= self.n_fft // 2:
                raise ValueError(f"wave {i}: {n} samples, reflect padding needs more than n_fft/2 = {self.n_fft // 2}")
            if n > Lmax:
                raise ValueError(f"wave {i}: length {n} exceeds the {Lmax} samples of the batch")
        frames = [1 + n // self.hop_length for n in lens]
        T = max(frames) if length is None else int(length)
        if T < max(frames):
            raise ValueError(f"length {T} is shorter than the longest wave's {max(frames)} frames")
        if sum(frames) > 1 << 24 or B * T > 1 << 24:
            raise ValueError("at most 2^24 frames per call")
        if not torch.is_tensor(wavs):
            wavs = torch.nn.utils.rnn.pad_sequence([w.to(torch.float32) for w in wavs], batch_first=True)
        if wavs.device.type != "cuda":
            raise RuntimeError("MelSpec runs on the HIP engine: move the waveforms to a GPU device")
        if not _lib.has_ragged():
            raise RuntimeError("this libf5h.so has no ragged batch entry points (f5h_mel_forward_ragged)")
        dev = torch.device("cuda", wavs.device.index if wavs.device.index is not None else torch.cuda.current_device())
        wavs = wavs.to(torch.float32)
        if wavs.stride(1) != 1:
            wavs = wavs.contiguous()
        cond = torch.empty(B, T, self.n_mel_channels, dtype=torch.float32, device=dev)
        with self._lock:
            h = self._engine(dev)
            L_ = _lib.lib()
            need = int(L_.f5h_mel_ragged_workspace_size(h, B, sum(frames)))
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(L_.f5h_mel_forward_ragged(h, _lib.stream_handle(dev), B, wavs.data_ptr(), wavs.stride(0),
                                                     (ctypes.c_int32 * B)(*lens), T, cond.data_ptr(), ws.data_ptr(),
                                                     ws.numel()), "f5h_mel_forward_ragged")
        return cond, frames

    def __del__(self):
        for h in getattr(self, "_h", {}).values():
            try:
                _lib.lib().f5h_mel_destroy(h)
            except Exception:
                pass
