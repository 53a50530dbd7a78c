"""Python handle on the HIP engine (libf5h.so). Plumbing only: device memory and the
current stream come from PyTorch; every FLOP runs in the engine's kernels."""

from __future__ import annotations

import ctypes
import threading

import numpy as np
import torch

from . import _lib


_VIEW_DT = {torch.float32: _lib.F5H_DT_F32, torch.bfloat16: _lib.F5H_DT_BF16, torch.float16: _lib.F5H_DT_F16}


def _arch_struct(arch: dict, compute: str) -> _lib.Arch:
    if arch["backbone"] == "MMDiT":
        return _mmdit_arch_struct(arch, compute)
    a = _lib.Arch()
    a.backbone = _lib.F5H_DIT if arch["backbone"] == "DiT" else _lib.F5H_UNETT
    a.dim = arch["dim"]
    a.depth = arch["depth"]
    a.heads = arch["heads"]
    a.dim_head = arch.get("dim_head", 64)
    a.ff_dim = int(arch["dim"] * arch["ff_mult"])
    a.text_dim = arch["text_dim"] if arch.get("text_dim") is not None else arch["mel_dim"]
    a.text_num_embeds = arch["text_num_embeds"]
    a.mel_dim = arch["mel_dim"]
    a.conv_layers = arch.get("conv_layers", 0)
    a.text_mask_padding = int(bool(arch.get("text_mask_padding", True)))
    a.pe_attn_head = int(arch.get("pe_attn_head") or 0)
    a.attn_mask_enabled = int(bool(arch.get("attn_mask_enabled", False)))
    a.compute = _lib.COMPUTE[compute]
    qk_norm = arch.get("qk_norm")
    if qk_norm not in (None, "rms_norm"):
        raise ValueError(f"Unimplemented qk_norm: {qk_norm}")  # as modules.py:408-409
    dit = arch["backbone"] == "DiT"
    a.qk_norm = 1 if qk_norm else 0
    a.long_skip_connection = int(bool(dit and arch.get("long_skip_connection")))
    a.text_average_upsampling = int(bool(dit and arch.get("text_embedding_average_upsampling")))
    if a.text_average_upsampling:
        assert a.text_mask_padding, "text_embedding_average_upsampling requires text_mask_padding to be True"
    if (a.qk_norm or a.long_skip_connection or a.text_average_upsampling) and not _lib.has_dit_options():
        raise RuntimeError("the loaded libf5h.so has no f5h_op_text_upsample (an older build): it would ignore qk_norm, "
                           "long_skip_connection and text_embedding_average_upsampling")
    return a


def _mmdit_arch_struct(arch: dict, compute: str) -> _lib.Arch:
    """MMDiT (mmdit.py:88-133): the text embedding has the model width, no ConvNeXt text blocks, RoPE on every head, no
    DiT options. A dict that says otherwise is refused here, before any device work (the library checks the same)."""
    d = arch["dim"]
    for key, want in (("text_dim", d), ("conv_layers", 0), ("pe_attn_head", None), ("long_skip_connection", False),
                      ("text_embedding_average_upsampling", False)):
        have = arch.get(key, want)
        if (have or None) != (want or None):
            raise ValueError(f"MMDiT: {key} must be {want!r}, got {have!r}")
    if arch["depth"] < 1:
        raise ValueError(f"MMDiT: depth must be >= 1, got {arch['depth']}")
    qk_norm = arch.get("qk_norm")
    if qk_norm not in (None, "rms_norm"):
        raise ValueError(f"Unimplemented qk_norm: {qk_norm}")  # as modules.py:408-409
    if not _lib.has_mmdit():
        raise RuntimeError("the loaded libf5h.so has no f5h_op_attention_split (an older build): it cannot run MMDiT")
    a = _lib.Arch()
    a.backbone = _lib.F5H_MMDIT
    a.dim, a.depth, a.heads, a.dim_head = d, arch["depth"], arch["heads"], arch.get("dim_head", 64)
    a.ff_dim = int(d * arch["ff_mult"])
    a.text_dim = d
    a.text_num_embeds, a.mel_dim = arch["text_num_embeds"], arch["mel_dim"]
    a.text_mask_padding = int(bool(arch.get("text_mask_padding", True)))
    a.attn_mask_enabled = int(bool(arch.get("attn_mask_enabled", False)))
    a.compute = _lib.COMPUTE[compute]
    a.qk_norm = 1 if qk_norm else 0
    return a


def _is_isolated(use_batch_mask) -> bool:
    return use_batch_mask is not True and use_batch_mask == 2


def _refuse_mmdit_masked(arch: dict, use_batch_mask) -> None:
    """MMDiT with attn_mask_enabled and a plain batch mask (B > 1): the joint sequence's valid keys are [0, dur) and
    [N, N + text length), not a prefix, and the reference's masked mode is not wired to the two-range attention.
    Refused before any device work (f5h_sample / f5h_forward return F5H_EINVAL for the same call). An isolated call
    (use_batch_mask == 2) masks both ranges itself, whatever the flag says, and is served."""
    if arch["backbone"] == "MMDiT" and arch.get("attn_mask_enabled") and use_batch_mask \
            and not _is_isolated(use_batch_mask):
        raise NotImplementedError(
            "MMDiT with attn_mask_enabled=True and a batch mask is not supported: the valid keys of the joint "
            "text-audio sequence are not a prefix and the attention kernel masks a suffix only (DESIGN.md §8); "
            "run single utterances, isolated batches (isolate=True), or the model without attn_mask_enabled")


def _mask_mode(arch: dict, use_batch_mask) -> int:
    """f5h_sample_args.use_batch_mask of a call: 0 none, 1 the batch mask, 2 the batch mask plus isolation (every
    utterance computed as if it were sampled alone). An older library (F5H_LIB) without f5h_op_attention_ranges has no
    isolation: refused before any device work."""
    mode = 2 if _is_isolated(use_batch_mask) else int(bool(use_batch_mask))
    if mode == 2 and not _lib.has_isolate():
        raise NotImplementedError("the loaded libf5h.so has no f5h_op_attention_ranges (an older build): it cannot "
                                  "run isolated batches (isolate=True / use_batch_mask=2)")
    return mode


def _refuse_ragged(arch: dict) -> None:
    """Ragged sampling (f5h_sample_ragged) serves the DiT backbone without text average upsampling. Everything else is
    refused before any device work: NotImplementedError for a model the path does not serve, RuntimeError for an older
    library (F5H_LIB) without the entry point."""
    if arch["backbone"] != "DiT":
        raise NotImplementedError(
            f"ragged sampling serves the DiT backbone only, not {arch['backbone']}: UNetT carries a time-token row per "
            "sequence and MMDiT a joint text-audio sequence, neither of which is packed (DESIGN.md §8); use "
            "isolate=True")
    if arch.get("text_embedding_average_upsampling"):
        raise NotImplementedError("ragged sampling does not serve text_embedding_average_upsampling; use isolate=True")
    if not _lib.has_ragged_sampler():
        raise RuntimeError("the loaded libf5h.so has no f5h_sample_ragged (an older build): it cannot sample ragged "
                           "batches (ragged=True)")


def _refuse_mx8(arch: dict) -> None:
    """compute="mxfp8" serves the DiT backbone with dim, heads * 64 and ff_dim multiples of 128 (the MX8 GEMM's K-step).
    Everything else is refused before any device work: NotImplementedError for a model the mode does not serve,
    RuntimeError for an older library (F5H_LIB) without the mode."""
    if arch["backbone"] != "DiT":
        raise NotImplementedError(f"compute='mxfp8' serves the DiT backbone only, not {arch['backbone']}")
    d, inner, ff = arch["dim"], arch["heads"] * arch.get("dim_head", 64), int(arch["dim"] * arch["ff_mult"])
    for name, val in (("dim", d), ("heads * dim_head", inner), ("ff_dim", ff)):
        if val % 128:
            raise NotImplementedError(f"compute='mxfp8' needs {name} to be a multiple of 128, got {val}: the MX8 GEMM "
                                      "takes K in steps of 128")
    if not _lib.has_mx8():
        raise RuntimeError("the loaded libf5h.so has no f5h_set_mx8_classes (an older build): it has no "
                           "compute='mxfp8'")


def _seg_array(seg_off):
    vals = [int(v) for v in seg_off]
    return (ctypes.c_int32 * len(vals))(*vals), vals


def _ode_method(method: str) -> int:
    if method not in _lib.ODE_METHOD:
        raise NotImplementedError(f"ode method {method!r}: the engine has 'euler', 'midpoint' and 'rk4'")
    if method != "euler" and not _lib.has_ode():
        raise RuntimeError(f"the loaded libf5h.so has no f5h_sample_ode (an older build): ode method {method!r} needs it")
    return _lib.ODE_METHOD[method]


class Engine:
    """One packed model on one device. Immutable after construction, so one instance may
    serve concurrent `sample` calls from several host threads (each call allocates its own
    workspace from the torch caching allocator)."""

    def __init__(self, arch: dict, weights: dict, compute: str = "bf16", device=None):
        if compute == "mxfp8":
            _refuse_mx8(arch)
        L = _lib.lib()
        self.arch = dict(arch)
        self.compute = compute
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        # typed views of the parameters in their own dtype and placement (utils_infer.py:190-232 leaves
        # them fp16/bf16/fp32 on the device): the engine packs from them on the device, no host copy
        keep, views = [], []
        for k, v in weights.items():
            k = k[len("transformer."):] if k.startswith("transformer.") else k
            t = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
            if t.dtype not in _VIEW_DT:
                t = t.to(torch.float32)
            if t.is_cuda and t.device != self.device:
                t = t.to(self.device)
            t = t.contiguous()
            keep.append(t)
            views.append((k.encode(), t))
        arr = (_lib.TensorView * len(views))()
        for i, (name, t) in enumerate(views):
            arr[i].name = name
            arr[i].data = t.data_ptr()
            arr[i].dtype = _VIEW_DT[t.dtype]
            arr[i].on_device = int(t.is_cuda)
            arr[i].numel = t.numel()
        a = _arch_struct(self.arch, compute)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            # device views are read on the engine's internal stream: the producers must be done
            if any(t.is_cuda for t in keep):
                torch.cuda.current_stream(self.device).synchronize()
            _lib.check(L.f5h_engine_create_views(ctypes.byref(a), arr, len(views), self.device.index,
                                                 ctypes.byref(h)), "f5h_engine_create_views")
        del keep
        self._h = h
        self._lock = threading.Lock()
        # per-(stream, size) workspaces kept across calls: the engine's NFE-step hipGraph is keyed
        # by the workspace address, so a stable workspace makes every call after the first a replay.
        # A call holds its workspace's lock while it enqueues, so calls sharing a stream serialise
        # in stream order and calls on different streams never share a workspace.
        self._ws_cache: dict = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.lib().f5h_engine_destroy(h)
            except Exception:
                pass
            self._h = None

    # ------------------------------------------------------------------ workspace
    def workspace_bytes(self, B, N, nt, nfe, use_cfg=True, method="euler") -> int:
        """Bytes for a call of `nfe` grid steps with the solver `method` ("euler", "midpoint", "rk4")."""
        m = _ode_method(method)
        if not _lib.has_ode():
            return int(_lib.lib().f5h_workspace_size(self._h, B, N, nt, nfe, int(use_cfg)))
        return int(_lib.lib().f5h_workspace_size_ode(self._h, B, N, nt, nfe, int(use_cfg), m))

    def _workspace(self, nbytes):
        return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)

    def _cached_workspace(self, nbytes, stream):
        with self._lock:
            ent = self._ws_cache.get((stream, nbytes))
            if ent is None:
                if len(self._ws_cache) >= 4:
                    self._ws_cache.pop(next(iter(self._ws_cache)))
                ent = (self._workspace(nbytes), threading.Lock())
                self._ws_cache[(stream, nbytes)] = ent
            return ent

    def set_graph_mode(self, on: bool):
        """True: the NFE loop replays one captured hipGraph step (default); False: eager launches."""
        _lib.check(_lib.lib().f5h_set_graph_mode(self._h, int(bool(on))), "set_graph_mode")

    def set_cfg_streams(self, n: int):
        """2: the captured step runs the two CFG branches as parallel launch chains; 1: one chain;
        0: automatic (the default; currently one chain, the faster form at C2, C3 and C5)."""
        _lib.check(_lib.lib().f5h_set_cfg_streams(self._h, int(n)), "set_cfg_streams")

    def set_pad_skip(self, on: bool):
        """Skip the batch path's dead pad-row work (attention query blocks and out-proj row tiles of
        padding only; default on). Results are bitwise identical either way."""
        _lib.check(_lib.lib().f5h_set_pad_skip(self._h, int(bool(on))), "set_pad_skip")

    def set_chain(self, on: bool):
        """Run each DiT layer's row-local seams (out-proj .. next QKV) as one phase-chain launch (16-bit DiT
        path without row masks; f5h_set_chain; default on). Results are bitwise identical either way."""
        _lib.check(_lib.lib().f5h_set_chain(self._h, int(bool(on))), "set_chain")

    def set_ln_fold(self, on: bool):
        """Run the AdaLN LayerNorms between the residual GEMMs and their consumers inside those GEMMs (16-bit DiT
        path without row masks; f5h_set_ln_fold; default on). Not bitwise the separate launches."""
        _lib.check(_lib.lib().f5h_set_ln_fold(self._h, int(bool(on))), "set_ln_fold")

    def ln_fold_stats(self):
        """(the engine can fold, backbone passes enqueued with the fold)."""
        sup, n = ctypes.c_int32(), ctypes.c_int64()
        _lib.check(_lib.lib().f5h_ln_fold_stats(self._h, ctypes.byref(sup), ctypes.byref(n)), "ln_fold_stats")
        return bool(sup.value), int(n.value)

    # class bits of set_store_policy's per-class form (0x100 | mask)
    STORE_CLASS_BITS = {"qkv": 1, "attn": 2, "out": 4, "ffn1": 8, "ffn2": 16}

    def set_store_policy(self, mode: int):
        """Store policy of the layer's hot launches (f5h_set_store_policy; DESIGN.md §3 'Launch boundaries'): -1 = auto
        (write-through stores when the launch is a single wave of workgroups, i.e. single-utterance calls), 0 = plain
        stores, 1 = write-through wherever a kernel variant exists, 0x100 | mask = write-through for the classes in
        mask (STORE_CLASS_BITS; A/B runs). Results are bitwise identical under every policy."""
        _lib.check(_lib.lib().f5h_set_store_policy(self._h, int(mode)), "set_store_policy")

    def store_policy_stats(self):
        """(hot launches this engine enqueued with write-through stores, with plain stores); eager launches and
        graph captures count, replays do not."""
        wt, plain = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.lib().f5h_store_policy_stats(self._h, ctypes.byref(wt), ctypes.byref(plain)), "store_policy_stats")
        return int(wt.value), int(plain.value)

    def set_mx8_classes(self, classes):
        """compute="mxfp8" engines: the per-layer GEMM classes that run on MXFP8 operands (f5h_set_mx8_classes): a mask
        of _lib.MX8_CLASS_BITS, or an iterable of their names. A class left out runs the bf16 mode's launch; none at
        all is the bf16 mode bit for bit. Default: all four."""
        if not isinstance(classes, int):
            classes = sum(_lib.MX8_CLASS_BITS[c] for c in set(classes))
        if not _lib.has_mx8():
            raise RuntimeError("the loaded libf5h.so has no f5h_set_mx8_classes (an older build)")
        _lib.check(_lib.lib().f5h_set_mx8_classes(self._h, int(classes)), "set_mx8_classes")

    def mx8_stats(self):
        """(the MX8 class mask, MX8 GEMM launches the device has run for this engine, graph replays included).
        Synchronous; call after the engine's work has completed (f5h_mx8_stats)."""
        if not _lib.has_mx8():
            raise RuntimeError("the loaded libf5h.so has no f5h_mx8_stats (an older build)")
        m, n = ctypes.c_int32(), ctypes.c_int64()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().f5h_mx8_stats(self._h, ctypes.byref(m), ctypes.byref(n)), "mx8_stats")
        return int(m.value), int(n.value)

    def chain_stats(self):
        """(phase-chain launches this engine enqueued, 1 if one of its chain waits gave up and the engine has not
        reported it yet, chained calls of this process that the per-device concurrency rule sent to the separate
        launches). Synchronous; call after the engine's work has completed (f5h_chain_stats)."""
        n, f, r = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
        _lib.check(_lib.lib().f5h_chain_stats(self._h, ctypes.byref(n), ctypes.byref(f), ctypes.byref(r)),
                   "chain_stats")
        return int(n.value), int(f.value), int(r.value)

    HOST_PHASES = ("total", "prologue", "cache_lock", "reap", "capture", "instantiate", "launch", "final")

    def last_call_host_ms(self):
        """Host milliseconds of this engine's newest sample call by phase (f5h_last_call_host_ms)."""
        buf = (ctypes.c_double * 8)()
        _lib.check(_lib.lib().f5h_last_call_host_ms(self._h, buf, 8), "last_call_host_ms")
        return {k: round(buf[i], 4) for i, k in enumerate(self.HOST_PHASES)}

    def graph_stats(self):
        cap, rep, n = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        _lib.check(_lib.lib().f5h_graph_stats(self._h, ctypes.byref(cap), ctypes.byref(rep), ctypes.byref(n)),
                   "graph_stats")
        return {"captures": cap.value, "replays": rep.value, "cached": n.value}

    # ------------------------------------------------------------------ calls
    def sample(self, cond, cond_mask, text, duration, y0, t_grid, cfg_strength, use_batch_mask,
               out=None, keep_trajectory=True, workspace=None, method="euler"):
        """Run the CFM ODE loop. Tensors on this engine's device:
        cond f32 [B,N,mel], cond_mask bool/u8 [B,N], text int64 [B,nt], duration int [B],
        y0 f32 [B,N,mel]; t_grid: host sequence of nfe+1 floats, the step grid. method: the fixed-grid
        solver, "euler", "midpoint" or "rk4" (1, 2, 4 backbone evaluations per step; f5h_sample_ode);
        the trajectory holds the nfe+1 grid points for every method. use_batch_mask: False / True, or 2 for the
        batch mask plus isolation (rows below duration[b] do not depend on the rest of the batch; f5h.h)."""
        _refuse_mmdit_masked(self.arch, use_batch_mask)
        mode = _mask_mode(self.arch, use_batch_mask)
        B, N, mel = cond.shape
        nt = text.shape[1]
        tg = np.ascontiguousarray(np.asarray(t_grid, dtype=np.float32))
        nfe = tg.shape[0] - 1
        cond = cond.to(self.device, torch.float32).contiguous()
        cmask = cond_mask.to(self.device, torch.uint8).contiguous()
        text = text.to(self.device, torch.int64).contiguous()
        dur = duration.to(self.device, torch.int32).contiguous()
        y0 = y0.to(self.device, torch.float32).contiguous()
        if out is None:
            out = torch.empty(B, N, mel, dtype=torch.float32, device=self.device)
        traj = (torch.empty(nfe + 1, B, N, mel, dtype=torch.float32, device=self.device)
                if keep_trajectory else None)
        use_cfg = cfg_strength >= 1e-5
        m = _ode_method(method)
        need = self.workspace_bytes(B, N, nt, nfe, use_cfg, method)
        stream = _lib.stream_handle(self.device)
        if workspace is not None and workspace.numel() >= need:
            ws, wlock = workspace, threading.Lock()
        else:
            ws, wlock = self._cached_workspace(need, stream)
        a = _lib.SampleArgs()
        a.B, a.N, a.nt, a.nfe = B, N, nt, nfe
        a.cond, a.cond_mask, a.text, a.duration, a.y0 = (cond.data_ptr(), cmask.data_ptr(), text.data_ptr(),
                                                         dur.data_ptr(), y0.data_ptr())
        a.t_grid = tg.ctypes.data
        a.cfg_strength = float(cfg_strength)
        a.use_batch_mask = mode
        a.out = out.data_ptr()
        a.trajectory = traj.data_ptr() if traj is not None else None
        with torch.cuda.device(self.device), wlock:
            if _lib.has_ode():
                _lib.check(_lib.lib().f5h_sample_ode(self._h, stream, ctypes.byref(a), m, ws.data_ptr(), ws.numel()),
                           "f5h_sample_ode")
            else:  # an older build through F5H_LIB (one-box A/Bs): its Euler entry
                _lib.check(_lib.lib().f5h_sample(self._h, stream, ctypes.byref(a), ws.data_ptr(), ws.numel()),
                           "f5h_sample")
        return out, traj

    def workspace_bytes_ragged(self, durations, nt, nfe, use_cfg=True, method="euler", lmax=None) -> int:
        """Bytes for a ragged call over utterances of `durations` frames (f5h_workspace_size_ragged)."""
        _refuse_ragged(self.arch)
        dur = [int(d) for d in durations]
        return int(_lib.lib().f5h_workspace_size_ragged(self._h, len(dur), sum(dur), int(lmax or max(dur)), nt, nfe,
                                                        int(use_cfg), _ode_method(method)))

    def sample_ragged(self, cond, cond_mask, text, durations, y0, t_grid, cfg_strength, keep_trajectory=True,
                      workspace=None, method="euler", lmax=None):
        """The CFM ODE loop over B utterances as packed rows, no pad frames (f5h_sample_ragged; DiT). durations: HOST
        ints [B], R = their sum; cond f32 [R,mel], cond_mask bool/u8 [R], y0 f32 [R,mel]: utterance b owns the rows
        from sum(durations[:b]); text int64 [B,nt]. Returns (out [R,mel], trajectory [nfe+1,R,mel] or None). Every
        utterance's rows equal its own B = 1 call bit for bit. lmax (default max(durations)): the geometry of the
        per-utterance launches; calls with equal (B, R, lmax) replay one step graph whatever the lengths."""
        _refuse_ragged(self.arch)
        dur = _lib.host_ints(durations, len(durations), "durations")
        B, R = len(dur), sum(dur)
        lmax = int(lmax or max(dur))
        mel = cond.shape[-1]
        if tuple(cond.shape) != (R, mel) or tuple(y0.shape) != (R, mel) or cond_mask.numel() != R or text.shape[0] != B:
            raise ValueError(f"ragged sample: packed tensors must hold R = {R} rows and text {B} rows")
        nt = text.shape[1]
        tg = np.ascontiguousarray(np.asarray(t_grid, dtype=np.float32))
        nfe = tg.shape[0] - 1
        cond = cond.to(self.device, torch.float32).contiguous()
        cmask = cond_mask.to(self.device, torch.uint8).contiguous()
        text = text.to(self.device, torch.int64).contiguous()
        y0 = y0.to(self.device, torch.float32).contiguous()
        out = torch.empty(R, mel, dtype=torch.float32, device=self.device)
        traj = torch.empty(nfe + 1, R, mel, dtype=torch.float32, device=self.device) if keep_trajectory else None
        use_cfg = cfg_strength >= 1e-5
        m = _ode_method(method)
        need = self.workspace_bytes_ragged(dur, nt, nfe, use_cfg, method, lmax)
        if need == 0:  # the shape is outside the path: the call below names the reason
            need = 256
        stream = _lib.stream_handle(self.device)
        if workspace is not None and workspace.numel() >= need:
            ws, wlock = workspace, threading.Lock()
        else:
            ws, wlock = self._cached_workspace(need, stream)
        darr = (ctypes.c_int32 * B)(*dur)
        a = _lib.RaggedArgs()
        a.B, a.Lmax, a.nt, a.nfe, a.R = B, lmax, nt, nfe, R
        a.cond, a.cond_mask, a.text, a.y0 = cond.data_ptr(), cmask.data_ptr(), text.data_ptr(), y0.data_ptr()
        a.duration = ctypes.cast(darr, ctypes.c_void_p).value
        a.t_grid = tg.ctypes.data
        a.cfg_strength = float(cfg_strength)
        a.out = out.data_ptr()
        a.trajectory = traj.data_ptr() if traj is not None else None
        with torch.cuda.device(self.device), wlock:
            _lib.check(_lib.lib().f5h_sample_ragged(self._h, stream, ctypes.byref(a), m, ws.data_ptr(), ws.numel()),
                       "f5h_sample_ragged")
        return out, traj

    def forward_workspace(self, B, N, nt, cfg_infer=True):
        """A workspace for `forward`; one kept across calls carries the text cache (text_cache=1/2)."""
        return self._workspace(self.workspace_bytes(B, N, nt, 1, cfg_infer))

    def forward(self, x, cond, cond_mask, text, duration, t, use_batch_mask, cfg_infer=True,
                drop_audio_cond=False, drop_text=False, text_cache=0, workspace=None):
        """One backbone forward at time t (DiT.forward / UNetT.forward, dit.py:319-370).
        cfg_infer: packed cond/uncond -> pred [2B,N,mel]; else one branch -> [B,N,mel] honouring
        drop_audio_cond / drop_text. t: a python float, or a one-element device tensor (read on the
        stream, no host sync). text_cache: 0 = compute the text embedding for this call, 1 = compute
        and keep it in `workspace`, 2 = reuse the one kept there (dit.py:294-317). use_batch_mask: as `sample`."""
        _refuse_mmdit_masked(self.arch, use_batch_mask)
        mode = _mask_mode(self.arch, use_batch_mask)
        B, N, mel = x.shape
        nt = text.shape[1]
        x = x.to(self.device, torch.float32).contiguous()
        cond = cond.to(self.device, torch.float32).contiguous()
        cmask = cond_mask.to(self.device, torch.uint8).contiguous()
        text = text.to(self.device, torch.int64).contiguous()
        dur = duration.to(self.device, torch.int32).contiguous()
        S = 2 * B if cfg_infer else B
        pred = torch.empty(S, N, mel, dtype=torch.float32, device=self.device)
        need = self.workspace_bytes(B, N, nt, 1, cfg_infer)
        if text_cache and (workspace is None or workspace.numel() < need):
            raise ValueError("text_cache needs a kept workspace of workspace_bytes(B, N, nt, 1, cfg_infer) bytes")
        ws = workspace if workspace is not None and workspace.numel() >= need else self._workspace(need)
        t_dev = None
        if torch.is_tensor(t):
            t_dev = t.reshape(-1)[:1].to(self.device, torch.float32).contiguous()
        a = _lib.ForwardArgs()
        a.B, a.N, a.nt = B, N, nt
        a.x, a.cond, a.cond_mask, a.text, a.duration = (x.data_ptr(), cond.data_ptr(), cmask.data_ptr(),
                                                        text.data_ptr(), dur.data_ptr())
        a.t = 0.0 if t_dev is not None else float(t)
        a.t_dev = t_dev.data_ptr() if t_dev is not None else None
        a.text_cache = int(text_cache)
        a.use_batch_mask = mode
        a.pred = pred.data_ptr()
        a.cfg_infer = int(bool(cfg_infer))
        a.drop_audio_cond = int(bool(drop_audio_cond))
        a.drop_text = int(bool(drop_text))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().f5h_forward(self._h, _lib.stream_handle(self.device), ctypes.byref(a),
                                              ws.data_ptr(), ws.numel()), "f5h_forward")
        return pred

    # ------------------------------------------------------------------ kernel probe
    def probe(self, kclass: str | None):
        L = _lib.lib()
        if kclass is None:
            _lib.check(L.f5h_probe_enable(self._h, 0, 0), "probe")
        else:
            _lib.check(L.f5h_probe_enable(self._h, _lib.KCLASS[kclass], 1), "probe")

    def probe_timeline(self, max_wg: int = 8192):
        """Per-workgroup [entry, loop entered, loop done, exit] stamps (microseconds from the earliest
        entry) of the probed class's first launch in the first probed step, as a [n_wg, 4] array."""
        buf = (ctypes.c_uint64 * (4 * max_wg))()
        n, khz = ctypes.c_int32(), ctypes.c_double()
        _lib.check(_lib.lib().f5h_probe_timeline(self._h, buf, max_wg, ctypes.byref(n), ctypes.byref(khz)),
                   "probe_timeline")
        a = np.frombuffer(buf, dtype=np.uint64, count=4 * n.value).reshape(n.value, 4).astype(np.float64)
        if n.value == 0 or khz.value <= 0:
            return a
        t0 = a[:, 0][a[:, 0] > 0].min()
        return np.where(a > 0, (a - t0) * 1e3 / khz.value, np.nan)

    def probe_read(self):
        n = ctypes.c_int64()
        ms = ctypes.c_double()
        _lib.check(_lib.lib().f5h_probe_read(self._h, ctypes.byref(n), ctypes.byref(ms)), "probe_read")
        return n.value, ms.value


# ---------------------------------------------------------------- op-level helpers (tests)
def op_linear(A, W, bias=None, compute="bf16"):
    M, K = A.shape
    N = W.shape[0]
    C = torch.empty(M, N, dtype=torch.float32, device=A.device)
    ws = torch.empty(((N + 127) // 128 * 128) * K * 4 + 512 + M * K * 4, dtype=torch.uint8, device=A.device)
    _lib.check(_lib.lib().f5h_op_linear(_lib.stream_handle(A.device), _lib.COMPUTE[compute], M, N, K,
                                        A.contiguous().data_ptr(), W.contiguous().data_ptr(), _lib.ptr(bias),
                                        C.data_ptr(), ws.data_ptr(), ws.numel()), "f5h_op_linear")
    return C


def op_attention(Q, K, V, kv_len=None, compute="bf16", q_prescaled=False, poison=False, q_len=None, return_ws=False):
    """O[S,N,H*64] = softmax(Q K^T/8) V; q_prescaled: Q already carries (1/8)*log2(e). poison: fill the
    workspace (16-bit q | k | v | o, back to back) with NaN bits first, so a kernel that reads key rows past N
    (the next (sequence, head)'s rows, or past V into O) turns its output NaN. q_len [S]: live query rows per
    sequence (the batch path's pad skip); with poison, O is NaN as well before the call, so rows the kernel
    leaves unwritten come back NaN in every compute mode. return_ws: (O, the workspace bytes) — past the 16-bit o
    (8 bytes per element of Q in all) nothing is ever written, so a poisoned workspace keeps its 0xFF there."""
    S, H, N, D = Q.shape
    assert D == 64
    O = torch.empty(S, N, H * 64, dtype=torch.float32, device=Q.device)
    ws = torch.empty(Q.numel() * 8 + 1024, dtype=torch.uint8, device=Q.device)
    if poison:
        ws.fill_(0xFF)
    kv = None if kv_len is None else kv_len.to(Q.device, torch.int32).contiguous()
    if q_len is None:
        _lib.check(_lib.lib().f5h_op_attention(_lib.stream_handle(Q.device), _lib.COMPUTE[compute], S, H, N,
                                               Q.contiguous().data_ptr(), K.contiguous().data_ptr(),
                                               V.contiguous().data_ptr(), _lib.ptr(kv), int(bool(q_prescaled)),
                                               O.data_ptr(), ws.data_ptr(), ws.numel()), "f5h_op_attention")
        return (O, ws) if return_ws else O
    if poison:
        O.fill_(float("nan"))
    ql = q_len.to(Q.device, torch.int32).contiguous()
    _lib.check(_lib.lib().f5h_op_attention_qlen(_lib.stream_handle(Q.device), _lib.COMPUTE[compute], S, H, N,
                                                Q.contiguous().data_ptr(), K.contiguous().data_ptr(),
                                                V.contiguous().data_ptr(), _lib.ptr(kv), ql.data_ptr(),
                                                int(bool(q_prescaled)), O.data_ptr(), ws.data_ptr(), ws.numel()),
               "f5h_op_attention_qlen")
    return (O, ws) if return_ws else O


def op_attention_split(Q, K, V, o_split, kv_len=None, q_len=None, compute="bf16", q_prescaled=False, poison=False,
                       return_ws=False):
    """op_attention with the output split at row `o_split` (f5h_op_attention_split; MMDiT joint attention): returns
    (O [S, o_split, H*64], O2 [S, N - o_split, H*64]). Both start as NaN; poison fills the workspace (16-bit q | k | v
    | o | o2, back to back, 8 bytes per element of Q in all) with NaN bits first, so unwritten rows come back NaN in
    every mode and the bytes past o2 show a write past either buffer. return_ws appends the workspace."""
    if not _lib.has_mmdit():
        raise RuntimeError("the loaded libf5h.so has no f5h_op_attention_split (an older build)")
    S, H, N, D = Q.shape
    assert D == 64 and 0 < o_split < N
    O = torch.full((S, o_split, H * 64), float("nan"), dtype=torch.float32, device=Q.device)
    O2 = torch.full((S, N - o_split, H * 64), float("nan"), dtype=torch.float32, device=Q.device)
    ws = torch.empty(Q.numel() * 8 + 1024, dtype=torch.uint8, device=Q.device)
    if poison:
        ws.fill_(0xFF)
    kv = None if kv_len is None else kv_len.to(Q.device, torch.int32).contiguous()
    ql = None if q_len is None else q_len.to(Q.device, torch.int32).contiguous()
    _lib.check(_lib.lib().f5h_op_attention_split(_lib.stream_handle(Q.device), _lib.COMPUTE[compute], S, H, N,
                                                 Q.contiguous().data_ptr(), K.contiguous().data_ptr(),
                                                 V.contiguous().data_ptr(), _lib.ptr(kv), _lib.ptr(ql),
                                                 int(bool(q_prescaled)), int(o_split), O.data_ptr(), O2.data_ptr(),
                                                 ws.data_ptr(), ws.numel()), "f5h_op_attention_split")
    return (O, O2, ws) if return_ws else (O, O2)


def op_attention_ranges(Q, K, V, kv_len=None, kv_start2=0, kv_len2=None, q_len=None, compute="bf16",
                        q_prescaled=False):
    """op_attention over two key ranges per sequence (f5h_op_attention_ranges): the valid keys of sequence s are
    [0, kv_len[s]) and [kv_start2, kv_start2 + kv_len2[s]). kv_len2 None: f5h_op_attention_qlen's kernels."""
    if not _lib.has_isolate():
        raise RuntimeError("the loaded libf5h.so has no f5h_op_attention_ranges (an older build)")
    S, H, N, D = Q.shape
    assert D == 64
    O = torch.zeros(S, N, H * 64, dtype=torch.float32, device=Q.device)
    ws = torch.zeros(Q.numel() * 8 + 1024, dtype=torch.uint8, device=Q.device)
    i32 = lambda t: None if t is None else torch.as_tensor(t).to(Q.device, torch.int32).contiguous()  # noqa: E731
    kv, kv2, ql = i32(kv_len), i32(kv_len2), i32(q_len)
    _lib.check(_lib.lib().f5h_op_attention_ranges(_lib.stream_handle(Q.device), _lib.COMPUTE[compute], S, H, N,
                                                  Q.contiguous().data_ptr(), K.contiguous().data_ptr(),
                                                  V.contiguous().data_ptr(), _lib.ptr(kv), int(kv_start2),
                                                  _lib.ptr(kv2), _lib.ptr(ql), int(bool(q_prescaled)), O.data_ptr(),
                                                  ws.data_ptr(), ws.numel()), "f5h_op_attention_ranges")
    return O


def op_attention_ragged(Q, K, V, seg_off, compute="bf16", q_prescaled=False):
    """Attention over S sequences of unequal length with packed output rows (f5h_op_attention_ragged): Q, K, V padded
    panels [S,H,Lmax,64] (rows past a sequence's length are never read), seg_off [S+1] host ints from 0 to R. Returns
    O [R, H*64] (NaN where the kernel wrote nothing)."""
    if not _lib.has_ragged_sampler():
        raise RuntimeError("the loaded libf5h.so has no f5h_op_attention_ragged (an older build)")
    S, H, Lmax, D = Q.shape
    assert D == 64
    arr, off = _seg_array(seg_off)
    R = off[-1]
    O = torch.full((R, H * 64), float("nan"), dtype=torch.float32, device=Q.device)
    ws = torch.empty(Q.numel() * 6 + O.numel() * 2 + R * 8 + S * 8 + 4096, dtype=torch.uint8, device=Q.device)
    _lib.check(_lib.lib().f5h_op_attention_ragged(_lib.stream_handle(Q.device), _lib.COMPUTE[compute], S, H, Lmax, R,
                                                  arr, Q.contiguous().data_ptr(), K.contiguous().data_ptr(),
                                                  V.contiguous().data_ptr(), int(bool(q_prescaled)), O.data_ptr(),
                                                  ws.data_ptr(), ws.numel()), "f5h_op_attention_ragged")
    return O


def op_conv_pos_ragged(x, w, bias, seg_off, mode=0, resid=None, x_as_f32=True, compute="bf16"):
    """One ConvPositionEmbedding layer over packed rows (f5h_op_conv_pos_ragged): x, resid [R,d], seg_off [S+1] host
    ints; taps outside a row's own segment read zero. Returns y [R,d] (NaN where the kernel wrote nothing)."""
    if not _lib.has_ragged_sampler():
        raise RuntimeError("the loaded libf5h.so has no f5h_op_conv_pos_ragged (an older build)")
    R, d = x.shape
    dev = x.device
    x, w, bias, resid = _f32(x), _f32(w, dev), _f32(bias, dev), _f32(resid, dev)
    arr, off = _seg_array(seg_off)
    S, lmax = len(off) - 1, max(b - a for a, b in zip(off, off[1:]))
    y = torch.full((R, d), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty(16 * 31 * 64 * 64 * 4 + x.numel() * 4 + S * 4 + 4096, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().f5h_op_conv_pos_ragged(_lib.stream_handle(dev), _lib.COMPUTE[compute], S, lmax, R, d, arr,
                                                 x.data_ptr(), w.data_ptr(), bias.data_ptr(), int(mode),
                                                 _lib.ptr(resid), int(bool(x_as_f32)), y.data_ptr(), ws.data_ptr(),
                                                 ws.numel()), "f5h_op_conv_pos_ragged")
    return y


def op_grn_ragged(x, gamma, beta, seg_off, compute="bf16"):
    """GRN over packed rows (f5h_op_grn_ragged): x [R,C], seg_off [S+1] host ints; every sequence is normed over its
    own rows. Returns out [R,C]."""
    if not _lib.has_ragged_sampler():
        raise RuntimeError("the loaded libf5h.so has no f5h_op_grn_ragged (an older build)")
    R, C = x.shape
    dev = x.device
    x, gamma, beta = (_f32(t, dev) for t in (x, gamma, beta))
    arr, off = _seg_array(seg_off)
    S, lmax = len(off) - 1, max(b - a for a, b in zip(off, off[1:]))
    out = torch.full((R, C), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty(((lmax + 63) // 64 + 1) * S * C * 4 + x.numel() * 2 + S * 4 + 4096, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().f5h_op_grn_ragged(_lib.stream_handle(dev), _lib.COMPUTE[compute], S, lmax, R, C, arr,
                                            x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                            ws.data_ptr(), ws.numel()), "f5h_op_grn_ragged")
    return out


def _f32(t, dev=None):
    return None if t is None else t.to(device=dev or t.device, dtype=torch.float32).contiguous()


def _u8(t, dev):
    return None if t is None else t.to(device=dev, dtype=torch.uint8).contiguous()


def op_conv_pos(x, w, bias, rowkeep=None, mode=0, resid=None, x_as_f32=True, y=None, y_row_off=0, compute="bf16"):
    """One ConvPositionEmbedding layer (f5h_op_conv_pos): x [S,L,d], w [d, d/16, 31], bias [d], rowkeep [S,L] or
    None. mode 0 returns y [S,L,d]; modes 1 / 2 write rows y_row_off.. of each sequence of `y` [S, rows, d] in
    place (a fresh [S, L + y_row_off, d] of NaN when None) and return it."""
    S, L, d = x.shape
    dev = x.device
    x, w, bias, resid = _f32(x), _f32(w, dev), _f32(bias, dev), _f32(resid, dev)
    if y is None:
        y = torch.full((S, L + (y_row_off if mode else 0), d), float("nan"), dtype=torch.float32, device=dev)
    assert y.is_contiguous() and y.dtype == torch.float32
    keep = _u8(rowkeep, dev)
    ws = torch.empty(16 * 31 * 64 * 64 * 4 + x.numel() * 2 + y.numel() * 2 + 1024, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().f5h_op_conv_pos(_lib.stream_handle(dev), _lib.COMPUTE[compute], S, L, d, x.data_ptr(),
                                          w.data_ptr(), bias.data_ptr(), _lib.ptr(keep), int(mode),
                                          _lib.ptr(resid), int(bool(x_as_f32)), y.shape[1], int(y_row_off),
                                          y.data_ptr(), ws.data_ptr(), ws.numel()), "f5h_op_conv_pos")
    return y


def op_norm(kind, h, p0, p1=None, h16=False, compute="bf16"):
    """kind "ln": LayerNorm(h) * (1 + p1) + p0 (p0 shift, p1 scale); kind "rms": RMSNorm with gain p0. h [M,d]."""
    M, d = h.shape
    dev = h.device
    h, p0, p1 = _f32(h), _f32(p0, dev), _f32(p1, dev)
    out = torch.empty(M, d, dtype=torch.float32, device=dev)
    ws = torch.empty(h.numel() * 4 + 1024, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().f5h_op_norm(_lib.stream_handle(dev), _lib.COMPUTE[compute], {"ln": 0, "rms": 1}[kind],
                                      int(bool(h16)), M, d, h.data_ptr(), p0.data_ptr(), _lib.ptr(p1),
                                      out.data_ptr(), ws.data_ptr(), ws.numel()), "f5h_op_norm")
    return out


def op_dwconv_ln(x, dw_w, dw_b, ln_w, ln_b, compute="bf16", seq_len=None):
    """LayerNorm(dwconv7(x) + dw_b) * ln_w + ln_b; x [S,L,C], dw_w [C,7]. seq_len [S] (f5h_op_dwconv_ln_len):
    sequence s ends at row seq_len[s], taps past it are zero."""
    S, L, C = x.shape
    dev = x.device
    x, dw_w, dw_b, ln_w, ln_b = (_f32(t, dev) for t in (x, dw_w, dw_b, ln_w, ln_b))
    out = torch.empty(S, L, C, dtype=torch.float32, device=dev)
    ws = torch.empty(x.numel() * 2 + 1024, dtype=torch.uint8, device=dev)
    if seq_len is not None:
        if not _lib.has_isolate():
            raise RuntimeError("the loaded libf5h.so has no f5h_op_dwconv_ln_len (an older build)")
        ln = torch.as_tensor(seq_len).to(dev, torch.int32).contiguous()
        assert ln.numel() == S
        _lib.check(_lib.lib().f5h_op_dwconv_ln_len(_lib.stream_handle(dev), _lib.COMPUTE[compute], S, L, C,
                                                   x.data_ptr(), dw_w.data_ptr(), dw_b.data_ptr(), ln_w.data_ptr(),
                                                   ln_b.data_ptr(), ln.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                   ws.numel()), "f5h_op_dwconv_ln_len")
        return out
    _lib.check(_lib.lib().f5h_op_dwconv_ln(_lib.stream_handle(dev), _lib.COMPUTE[compute], S, L, C, x.data_ptr(),
                                           dw_w.data_ptr(), dw_b.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(),
                                           out.data_ptr(), ws.data_ptr(), ws.numel()), "f5h_op_dwconv_ln")
    return out


def op_grn(x, gamma, beta, compute="bf16", seq_len=None):
    """GRN over time: gamma * (x * Nx) + beta + x; x [S,L,C]. seq_len [S] (f5h_op_grn_len): the norm of sequence s
    runs over its rows below seq_len[s] only."""
    S, L, C = x.shape
    dev = x.device
    x, gamma, beta = (_f32(t, dev) for t in (x, gamma, beta))
    out = torch.empty(S, L, C, dtype=torch.float32, device=dev)
    ws = torch.empty(((L + 63) // 64 + 1) * S * C * 4 + x.numel() * 2 + 1024, dtype=torch.uint8, device=dev)
    if seq_len is not None:
        if not _lib.has_isolate():
            raise RuntimeError("the loaded libf5h.so has no f5h_op_grn_len (an older build)")
        ln = torch.as_tensor(seq_len).to(dev, torch.int32).contiguous()
        assert ln.numel() == S
        _lib.check(_lib.lib().f5h_op_grn_len(_lib.stream_handle(dev), _lib.COMPUTE[compute], S, L, C, x.data_ptr(),
                                             gamma.data_ptr(), beta.data_ptr(), ln.data_ptr(), out.data_ptr(),
                                             ws.data_ptr(), ws.numel()), "f5h_op_grn_len")
        return out
    _lib.check(_lib.lib().f5h_op_grn(_lib.stream_handle(dev), _lib.COMPUTE[compute], S, L, C, x.data_ptr(),
                                     gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel()),
               "f5h_op_grn")
    return out


EPI = {"store": 0, "silu": 1, "gelu_tanh": 2, "gelu_erf": 3, "resid": 4, "resid_fill": 5, "inproj": 6, "qkv": 7,
       "gelu_erf_op": 8, "resid16": 9, "store16": 10}


def op_gemm_epi(epi, A, W, bias=None, C=None, compute="bf16", A2=None, k_split=0, resid=None, gate=None, rowkeep=None,
                live_len=None, live_seq=0, add=None, dual_rows=0, seq_len=0, heads=0, rope_heads=0, q_scale=0.0,
                hs_scale=None, ln_producer=False, ln_part_in=None, ln_u=None, ln_v=None, ln_rms=False, ln_eps=0.0,
                ln_nparts=None, poison=False, ws_fill=None, return_ws=False, q_norm_w=None, k_norm_w=None,
                qk_norm_eps=1e-6, qkv_dst_len=0, qkv_bufs=None, qkv_row0=0, seg_off=None, _mx8=None):
    """A GEMM with epilogue `epi` (a key of EPI; f5h_op_gemm_epi). The in/out epilogues update a copy of C and
    return it; "inproj" returns C [M + dual_rows, N]; "qkv" returns (q, k, v [S,H,L,64], rope [L,32,2]).

    LayerNorm / RMSNorm fold forms (f5h_op_gemm_args in include/f5h.h). ln_producer ("resid16"): returns (C, hs,
    parts) with parts [M + OP_GUARD_ROWS, N / 64, 2] the strips' (mean, M2) and hs [M + OP_GUARD_ROWS, N] =
    round(C (1 + hs_scale)) (None with ln_rms, which writes none); the guard rows past M start as NaN, the live rows
    too with poison. ln_part_in [M, K / 64, 2] ("gelu_tanh" / "qkv"): the consumer, with ln_u, ln_v [N] (LayerNorm
    form) or ln_rms, and the variance epsilon ln_eps. ln_nparts overrides the strip count (validation tests).
    ws_fill: byte the workspace is filled with before the call; return_ws: the workspace is appended to the result
    (its buffers are taken in f5h_op_gemm_epi's order, each from a multiple of 256 bytes; the bytes past the last one
    are never written). q_norm_w, k_norm_w [64] ("qkv"): qk_norm = "rms_norm" with epsilon qk_norm_eps, the RMSNorm
    of every q / k head after the bias and ahead of RoPE; both None: no norm. qkv_dst_len ("qkv"; 0: none): the
    destination panels hold qkv_dst_len rows, q / k / v are [S,H,qkv_dst_len,64] — qkv_bufs (q, k, v), updated in place,
    or fresh NaN buffers — and the launch writes rows [qkv_row0, qkv_row0 + seq_len) of every panel (the pointers it
    gets are advanced by qkv_row0 * 64 elements) and leaves the other rows alone. seg_off ("qkv"; host ints [S+1] from
    0 to M): the rows are S packed sequences of unequal length; row seg_off[s] + n is rotated by rope[n] and stored at
    row n of panel (s, head) of q / k / v [S,H,qkv_dst_len,64] (seq_len is then the rope table's rows, qkv_dst_len)."""
    M, K = A.shape
    N = W.shape[0]
    dev = A.device
    A, A2, W, bias, resid, gate, add = (_f32(t, dev) for t in (A, A2, W, bias, resid, gate, add))
    keep = _u8(rowkeep, dev)
    ll = None if live_len is None else live_len.to(dev, torch.int32).contiguous()
    a = _lib.OpGemmArgs()
    a.compute, a.epi, a.M, a.N, a.K, a.k_split = _lib.COMPUTE[compute], EPI[epi], M, N, K, int(k_split)
    a.A, a.A2, a.W, a.bias = A.data_ptr(), _lib.ptr(A2), W.data_ptr(), _lib.ptr(bias)
    a.resid, a.gate, a.rowkeep, a.live_len, a.live_seq = _lib.ptr(resid), _lib.ptr(gate), _lib.ptr(keep), \
        _lib.ptr(ll), int(live_seq)
    a.add, a.ld_add, a.dual_rows = _lib.ptr(add), (0 if add is None else add.shape[1]), int(dual_rows)
    ws_bytes = ((N + 127) // 128 * 128) * K * 4 + 3 * M * K * 4 + 3 * (M + int(dual_rows)) * N * 4 + 4096
    hs_scale, ln_part_in, ln_u, ln_v = (_f32(t, dev) for t in (hs_scale, ln_part_in, ln_u, ln_v))
    hs = parts = None
    if ln_producer:
        G = _lib.OP_GUARD_ROWS
        a.ln_nparts = N // 64 if ln_nparts is None else int(ln_nparts)
        parts = torch.empty(M + G, max(a.ln_nparts, 1), 2, dtype=torch.float32, device=dev)
        a.ln_part_out = parts.data_ptr()
        if hs_scale is not None:
            hs = torch.empty(M + G, N, dtype=torch.float32, device=dev)
            a.hs_scale, a.hs_out = hs_scale.data_ptr(), hs.data_ptr()
            ws_bytes += (M + G) * N * 2 + 256
    elif ln_part_in is not None:
        a.ln_nparts = K // 64 if ln_nparts is None else int(ln_nparts)
        a.ln_part_in, a.ln_u, a.ln_v = ln_part_in.data_ptr(), _lib.ptr(ln_u), _lib.ptr(ln_v)
    a.ln_rms, a.ln_eps, a.poison = int(bool(ln_rms)), float(ln_eps), int(bool(poison))
    out = None
    if epi == "qkv":
        seg_arr = None
        if seg_off is not None:
            if not _lib.has_ragged_sampler():
                raise RuntimeError("the loaded libf5h.so has no ragged QKV rows (an older build)")
            seg_arr, segs = _seg_array(seg_off)
            seq_len = int(qkv_dst_len)
        S = M // seq_len if seq_len > 0 else 0
        rope = torch.empty(max(seq_len, 0), 32, 2, dtype=torch.float32, device=dev)
        a.seq_len, a.heads, a.rope_heads, a.q_scale = int(seq_len), int(heads), int(rope_heads), float(q_scale)
        if seg_arr is not None:
            S = len(segs) - 1
            q, k, v = qkv_bufs if qkv_bufs is not None else (
                torch.full((S, heads, qkv_dst_len, 64), float("nan"), dtype=torch.float32, device=dev)
                for _ in range(3))
            a.qkv_dst_len = int(qkv_dst_len)
            a.seg_off, a.n_seq = ctypes.cast(seg_arr, ctypes.c_void_p).value, S
            a.q, a.k, a.v, a.rope_out = q.data_ptr(), k.data_ptr(), v.data_ptr(), rope.data_ptr()
            ws_bytes += 3 * S * heads * qkv_dst_len * 64 * 4 + M * 8 + S * 4 + 2048
        elif qkv_dst_len:
            if not _lib.has_mmdit():
                raise RuntimeError("the loaded libf5h.so has no qkv_dst_len (an older build)")
            assert 0 <= qkv_row0 and qkv_row0 + seq_len <= qkv_dst_len, "the launch's rows lie inside the panels"
            q, k, v = qkv_bufs if qkv_bufs is not None else (
                torch.full((S, heads, qkv_dst_len, 64), float("nan"), dtype=torch.float32, device=dev)
                for _ in range(3))
            for t in (q, k, v):
                assert t.shape == (S, heads, qkv_dst_len, 64) and t.is_contiguous() and t.dtype == torch.float32
            a.qkv_dst_len = int(qkv_dst_len)
            off = int(qkv_row0) * 64 * 4
            a.q, a.k, a.v, a.rope_out = q.data_ptr() + off, k.data_ptr() + off, v.data_ptr() + off, rope.data_ptr()
            ws_bytes += 3 * S * heads * qkv_dst_len * 64 * 4
        else:
            q, k, v = (torch.full((S, heads, seq_len, 64), float("nan"), dtype=torch.float32, device=dev)
                       for _ in range(3))
            a.q, a.k, a.v, a.rope_out = q.data_ptr(), k.data_ptr(), v.data_ptr(), rope.data_ptr()
        if q_norm_w is not None or k_norm_w is not None:
            if not _lib.has_dit_options():
                raise RuntimeError("the loaded libf5h.so has no qk_norm (an older build)")
            q_norm_w, k_norm_w = _f32(q_norm_w, dev), _f32(k_norm_w, dev)
            a.q_norm_w, a.k_norm_w, a.qk_norm_eps = _lib.ptr(q_norm_w), _lib.ptr(k_norm_w), float(qk_norm_eps)
        ws_bytes += max(seq_len, 0) * 256 + 1024
        out = (q, k, v, rope)
    else:
        if C is None:
            C = torch.full((M + int(dual_rows), N), float("nan"), dtype=torch.float32, device=dev)
        else:
            C = _f32(C, dev).clone()
        a.C = C.data_ptr()
        out = C
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if ws_fill is not None:
        ws.fill_(int(ws_fill))
    if _mx8 is not None:  # op_gemm_mx8: the same arguments through the MX8 hook, which also returns the operands
        _lib.check(_lib.lib().f5h_op_gemm_mx8(_lib.stream_handle(dev), ctypes.byref(a), *(t.data_ptr() for t in _mx8),
                                              ws.data_ptr(), ws.numel()), "f5h_op_gemm_mx8")
        return out
    _lib.check(_lib.lib().f5h_op_gemm_epi(_lib.stream_handle(dev), ctypes.byref(a), ws.data_ptr(), ws.numel()),
               "f5h_op_gemm_epi")
    res = (out, hs, parts) if ln_producer else out
    return (res, ws) if return_ws else res


def _need_mx8():
    if not _lib.has_mx8():
        raise RuntimeError("the loaded libf5h.so has no MXFP8 op hooks (an older build)")


def op_quant_mx8(x):
    """quant_rows_mx8 alone (f5h_op_quant_mx8): x [M, K] fp32, rounded to bf16 and quantised on the device. Returns
    (q [M, K], s [M, K / 32]) uint8: e4m3fn element bytes and E8M0 scale bytes."""
    _need_mx8()
    M, K = x.shape
    x = _f32(x)
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    s = torch.empty(M, K // 32, dtype=torch.uint8, device=x.device)
    ws = torch.empty(M * K * 2 + 512, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().f5h_op_quant_mx8(_lib.stream_handle(x.device), M, K, x.data_ptr(), q.data_ptr(), s.data_ptr(),
                                           ws.data_ptr(), ws.numel()), "f5h_op_quant_mx8")
    return q, s


def op_ln_modulate_mx8(h, shift, scale, h16=True):
    """ln_modulate writing MX8 (f5h_op_ln_modulate_mx8): LayerNorm(h) (1 + scale) + shift, rounded to bf16, quantised.
    h16: the kernel reads the bf16-rounded h (the 16-bit residual stream). Returns (q [M, d], s [M, d / 32]) uint8."""
    _need_mx8()
    M, d = h.shape
    dev = h.device
    h, shift, scale = _f32(h, dev), _f32(shift, dev), _f32(scale, dev)
    q = torch.empty(M, d, dtype=torch.uint8, device=dev)
    s = torch.empty(M, d // 32, dtype=torch.uint8, device=dev)
    ws = torch.empty(M * d * 2 + 512, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().f5h_op_ln_modulate_mx8(_lib.stream_handle(dev), int(bool(h16)), M, d, h.data_ptr(),
                                                 shift.data_ptr(), scale.data_ptr(), q.data_ptr(), s.data_ptr(),
                                                 ws.data_ptr(), ws.numel()), "f5h_op_ln_modulate_mx8")
    return q, s


def op_gemm_mx8(epi, A, W, **kw):
    """The MX8 GEMM with epilogue "qkv", "resid16" or "gelu_tanh" (f5h_op_gemm_mx8): op_gemm_epi's arguments and
    result, A and W rounded to bf16 and quantised on the device. Returns (result, (a8, as, w8, ws)): the quantised
    operands the product ran on, uint8 [M, K], [M, K / 32], [N, K], [N, K / 32]."""
    _need_mx8()
    (M, K), N, dev = A.shape, W.shape[0], A.device
    ops = (torch.empty(M, K, dtype=torch.uint8, device=dev), torch.empty(M, K // 32, dtype=torch.uint8, device=dev),
           torch.empty(N, K, dtype=torch.uint8, device=dev), torch.empty(N, K // 32, dtype=torch.uint8, device=dev))
    return op_gemm_epi(epi, A, W, compute="bf16", _mx8=ops, **kw), ops


def mx8_quant_block_host(v32):
    """One block of 32 fp32 values through the library's quantisation rule on the host (f5h_debug_mx8_quant_block): the
    code the device kernels run. Returns (32 element bytes, the scale byte)."""
    _need_mx8()
    v = (ctypes.c_float * 32)(*[float(x) for x in v32])
    q, s = (ctypes.c_uint8 * 32)(), ctypes.c_uint8()
    _lib.check(_lib.lib().f5h_debug_mx8_quant_block(v, q, ctypes.byref(s)), "f5h_debug_mx8_quant_block")
    return list(q), int(s.value)


def op_text_upsample(te, text, seq_len=None, out=None):
    """average_upsample_text_by_mask alone (f5h_op_text_upsample): te [B,N,td] fp32, text [B,nt] int64 (-1 = padding),
    seq_len [B] or None (= N). Returns `out` (a fresh [B,N,td] of NaN when None) with every row written."""
    B, N, td = te.shape
    dev = te.device
    te = _f32(te)
    text = text.to(dev, torch.int64).contiguous()
    sl = None if seq_len is None else seq_len.to(dev, torch.int32).contiguous()
    if out is None:
        out = torch.full((B, N, td), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().f5h_op_text_upsample(_lib.stream_handle(dev), B, text.shape[1], N, td, text.data_ptr(),
                                               _lib.ptr(sl), te.data_ptr(), out.data_ptr()), "f5h_op_text_upsample")
    return out


def op_lnfold_uv(table, W1, Wqkv, nfe, out_off, compute="bf16"):
    """lnfold_uv alone (f5h_op_lnfold_uv): table [rows >= nfe, stride] fp32 with the AdaLN modulation rows of
    `depth` layers in its first 6 d depth columns; W1 [depth, F, d], Wqkv [depth, 3d, d]. Returns a copy of the
    table with the u / v blocks of steps < nfe written from column out_off on."""
    depth, F, d = W1.shape
    dev = table.device
    table = _f32(table).clone()
    W1, Wqkv = _f32(W1, dev), _f32(Wqkv, dev)
    ws = torch.empty((W1.numel() + Wqkv.numel()) * 2 + 16 * depth + 2048, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().f5h_op_lnfold_uv(_lib.stream_handle(dev), _lib.COMPUTE[compute], int(nfe), depth, d, F,
                                           table.data_ptr(), table.shape[1], int(out_off), W1.data_ptr(),
                                           Wqkv.data_ptr(), ws.data_ptr(), ws.numel()), "f5h_op_lnfold_uv")
    return table


def op_scale_cols(W, g, compute="bf16"):
    """scale_cols alone (f5h_op_scale_cols): round(round(W) g[None, :]) as fp32; W [rows, K], g [K]."""
    rows, K = W.shape
    dev = W.device
    W, g = _f32(W), _f32(g, dev)
    out = torch.empty(rows, K, dtype=torch.float32, device=dev)
    ws = torch.empty(W.numel() * 4 + 1024, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().f5h_op_scale_cols(_lib.stream_handle(dev), _lib.COMPUTE[compute], rows, K, W.data_ptr(),
                                            g.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel()),
               "f5h_op_scale_cols")
    return out


# ---------------------------------------------------------------- op-level helpers: audio glue, prologue, ODE step
# One launcher call each on the caller's tensors (f5h_op_* of csrc/engine_ops_glue.cpp): no staging, so a buffer in the
# operand dtype comes back as a torch.bfloat16 / torch.float16 tensor. Every output is a view of a buffer that starts
# as NaN (integers: OP_FILL) and ends in OP_GUARD more such elements: an element the kernel leaves alone comes back as
# that fill, and op_guard_intact(out) tells whether it wrote past the end.
OP_TORCH_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "mxfp8": torch.bfloat16}
OP_GUARD, OP_FILL = 256, 0x5A


def _guarded(shape, dev, dtype=torch.float32):
    n = 1
    for s in shape:
        n *= int(s)
    fill = float("nan") if dtype.is_floating_point else OP_FILL
    return torch.full((n + OP_GUARD,), fill, dtype=dtype, device=dev)[:n].view(*shape)


def op_guard_intact(out) -> bool:
    """True when the OP_GUARD elements behind an op_* output still hold their fill."""
    tail = out._base[out.numel():]
    return bool((torch.isnan(tail) if tail.dtype.is_floating_point else tail == OP_FILL).all())


def _glue(name, *args):
    if not _lib.has_glue_ops():
        raise RuntimeError(f"the loaded libf5h.so has no {name} (an older build)")
    _lib.check(getattr(_lib.lib(), name)(*args), name)


def _dp(t):
    """Device pointer of a view, also when it has no elements (the guard behind it is still there)."""
    return t.data_ptr() or t._base.data_ptr()


def _i32(vals, dev):
    return torch.tensor([int(v) for v in vals], dtype=torch.int32).to(dev)


def _offsets(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + int(n))
    return off


def op_mel_frames(wav, n_fft, hop):
    """wav [B, L] -> frames [B, T, n_fft], T = 1 + L // hop (mel_frames: centred, reflect-padded windows)."""
    B, L = wav.shape
    wav = _f32(wav)
    out = _guarded((B, 1 + L // hop, n_fft), wav.device)
    _glue("f5h_op_mel_frames", _lib.stream_handle(wav.device), B, L, int(n_fft), int(hop), wav.data_ptr(), _dp(out))
    return out


def op_mel_frames_ragged(wav, lens, n_fft, hop):
    """wav [B, wav_st] with wave s in its first lens[s] samples (host ints) -> packed frames [sum T_s, n_fft]."""
    B, wav_st = wav.shape
    wav = _f32(wav)
    lens = [int(n) for n in lens]
    assert len(lens) == B and all(n_fft // 2 < n <= wav_st for n in lens), "every wave needs n_fft/2 < len <= stride"
    off = _offsets(1 + n // hop for n in lens)
    out = _guarded((off[-1], n_fft), wav.device)
    off_d, len_d = _i32(off, wav.device), _i32(lens, wav.device)  # (held until the launch is enqueued)
    _glue("f5h_op_mel_frames_ragged", _lib.stream_handle(wav.device), B, off[-1], int(n_fft), int(hop),
          wav.data_ptr(), wav_st, off_d.data_ptr(), len_d.data_ptr(), _dp(out))
    return out


def op_mel_mag(spec, bins, ld_mag):
    """spec [rows, ld_spec] interleaved (re, im) -> mag [rows, ld_mag] (mel_mag)."""
    rows, ld_spec = spec.shape
    spec = _f32(spec)
    out = _guarded((rows, ld_mag), spec.device)
    _glue("f5h_op_mel_mag", _lib.stream_handle(spec.device), rows, int(bins), ld_spec, int(ld_mag), spec.data_ptr(),
          _dp(out))
    return out


def op_mel_log(mel, B, T):
    """mel [B * T, n_mels] -> log(max(mel, 1e-5)) as [B, n_mels, T] (mel_log)."""
    mel = _f32(mel)
    assert mel.shape[0] == B * T
    out = _guarded((B, mel.shape[1], T), mel.device)
    _glue("f5h_op_mel_log", _lib.stream_handle(mel.device), int(B), int(T), mel.shape[1], mel.data_ptr(), _dp(out))
    return out


def op_mel_log_ragged(mel, frames, T_out):
    """mel [sum frames, n_mels] packed, frames: host ints T_s -> [B, T_out, n_mels], zeros past T_s (mel_log_ragged)."""
    mel = _f32(mel)
    off = _offsets(frames)
    assert off[-1] == mel.shape[0] and all(1 <= t <= T_out for t in frames)
    out = _guarded((len(frames), T_out, mel.shape[1]), mel.device)
    off_d = _i32(off, mel.device)
    _glue("f5h_op_mel_log_ragged", _lib.stream_handle(mel.device), len(frames), int(T_out), mel.shape[1],
          mel.data_ptr(), off_d.data_ptr(), _dp(out))
    return out


def op_vocos_im2col(mel, Kp, compute="fp32"):
    """mel [B, C, T] -> the embed conv's im2col [B * T, Kp] in the operand dtype (vocos_im2col)."""
    B, C, T = mel.shape
    mel = _f32(mel)
    out = _guarded((B * T, Kp), mel.device, OP_TORCH_DTYPE[compute])
    _glue("f5h_op_vocos_imcol", _lib.stream_handle(mel.device), _lib.COMPUTE[compute], B, T, C, int(Kp),
          mel.data_ptr(), _dp(out))
    return out


def op_vocos_im2col_ragged(src, layout, starts, lens, Kp, compute="fp32"):
    """src: "BNC" [B, N, C] or "BCT" [B, C, T]; utterance s = frames [starts[s], starts[s] + lens[s]) of row s (host
    ints) -> packed im2col rows [sum lens, Kp] (vocos_im2col_ragged), read in place through element strides."""
    src = _f32(src)
    B = src.shape[0]
    if layout == "BNC":
        n_frames, C = src.shape[1], src.shape[2]
        strides = (n_frames * C, C, 1)
    else:
        assert layout == "BCT"
        C, n_frames = src.shape[1], src.shape[2]
        strides = (C * n_frames, 1, n_frames)
    assert len(starts) == len(lens) == B
    assert all(s >= 0 and n >= 1 and s + n <= n_frames for s, n in zip(starts, lens))
    off = _offsets(lens)
    out = _guarded((off[-1], Kp), src.device, OP_TORCH_DTYPE[compute])
    off_d, start_d = _i32(off, src.device), _i32(starts, src.device)  # (held until the launch is enqueued)
    _glue("f5h_op_vocos_imcol_ragged", _lib.stream_handle(src.device), _lib.COMPUTE[compute], B, off[-1], C, int(Kp),
          src.data_ptr(), *strides, off_d.data_ptr(), start_d.data_ptr(), _dp(out))
    return out


def op_vocos_spec(x, bins):
    """x [rows, ld] of (log-magnitude, phase) pairs -> (re, im) pairs, pad columns zero (vocos_spec; on a copy)."""
    rows, ld = x.shape
    out = _guarded((rows, ld), x.device)
    out.copy_(x)
    _glue("f5h_op_vocos_spec", _lib.stream_handle(x.device), rows, int(bins), ld, _dp(out))
    return out


def op_vocos_ola(frames, win, B, T, hop):
    """frames [B * T, n_fft] windowed, win [n_fft] -> y [B, (T - 1) * hop] (vocos_ola)."""
    frames, win = _f32(frames), _f32(win, frames.device)
    n_fft = frames.shape[1]
    assert frames.shape[0] == B * T and win.numel() == n_fft
    out = _guarded((B, (T - 1) * hop), frames.device)
    _glue("f5h_op_vocos_ola", _lib.stream_handle(frames.device), int(B), int(T), n_fft, int(hop), frames.data_ptr(),
          win.data_ptr(), _dp(out))
    return out


def op_vocos_ola_ragged(frames, win, lens, hop):
    """frames [sum lens, n_fft] packed -> y [(sum lens - B) * hop] packed (vocos_ola_ragged)."""
    frames, win = _f32(frames), _f32(win, frames.device)
    n_fft = frames.shape[1]
    off = _offsets(lens)
    assert off[-1] == frames.shape[0] and all(n >= 1 for n in lens) and win.numel() == n_fft
    out = _guarded(((off[-1] - len(lens)) * hop,), frames.device)
    off_d = _i32(off, frames.device)
    _glue("f5h_op_vocos_ola_ragged", _lib.stream_handle(frames.device), len(lens), off[-1], n_fft, int(hop),
          frames.data_ptr(), win.data_ptr(), off_d.data_ptr(), _dp(out))
    return out


def op_time_sinus(t, dev=False, device="cuda:0"):
    """t: n time values -> [n, 256] sinusoidal embedding. dev=False: time_sinus (host values as kernel arguments);
    dev=True: time_sinus_dev (the values read from device memory)."""
    vals = [float(v) for v in (t.reshape(-1).tolist() if torch.is_tensor(t) else t)]
    n = len(vals)
    out = _guarded((n, 256), device)
    if dev:
        tg = torch.tensor(vals + [0.0], dtype=torch.float32).to(device)  # (one spare value: never a null pointer)
        _glue("f5h_op_time_sinus", _lib.stream_handle(device), 1, n, tg.data_ptr(), _dp(out))
    else:
        arr = (ctypes.c_float * (n + 1))(*vals)
        _glue("f5h_op_time_sinus", _lib.stream_handle(device), 0, n, ctypes.addressof(arr), _dp(out))
    return out


def op_rope_table(L, device="cuda:0"):
    """[L, 32, 2] (cos, sin) rotary table (rope_table)."""
    out = _guarded((L, 32, 2), device)
    _glue("f5h_op_rope_table", _lib.stream_handle(device), int(L), _dp(out))
    return out


def op_text_embed(text, table, N, seq_len=None, freqs=None, freq_rows=0, mask_padding=False, seg_lens=None):
    """text_embed alone: text [B, nt] int64 (-1 = filler), table [V, td], freqs [rows, td] or None. Returns (out_c,
    out_u [B, N, td], keep [2, B, N] bytes). seg_lens (host ints): the ragged form, N is ignored and the outputs are
    packed rows [sum seg_lens, td], keep [2, R]."""
    dev = text.device
    B, nt = text.shape
    text = text.to(torch.int64).contiguous()
    table, freqs = _f32(table, dev), _f32(freqs, dev)
    V, td = table.shape
    assert int(text.min()) >= -1 and int(text.max()) + 1 < V, "token ids must index the table"
    sl = off = None
    if seg_lens is not None:
        assert seq_len is None and len(seg_lens) == B and all(n >= 1 for n in seg_lens)
        offs = _offsets(seg_lens)
        N, rows, longest = offs[-1], offs[-1], max(seg_lens)
        off = _i32(offs, dev)
    else:
        rows, longest = B * N, N
        if seq_len is not None:
            sl = _i32(seq_len, dev)
            assert sl.numel() == B
    if freqs is not None:
        assert freqs.shape[1] == td and freqs.shape[0] >= (freq_rows if freq_rows else longest)
    shape = (rows, td) if seg_lens is not None else (B, N, td)
    out_c, out_u = _guarded(shape, dev), _guarded(shape, dev)
    keep = _guarded((2, rows) if seg_lens is not None else (2, B, N), dev, torch.uint8)
    _glue("f5h_op_text_embed", _lib.stream_handle(dev), B, nt, int(N), td, text.data_ptr(), _lib.ptr(sl),
          table.data_ptr(), _lib.ptr(freqs), int(freq_rows), int(bool(mask_padding)), _dp(out_c), _dp(out_u),
          _dp(keep), _lib.ptr(off))
    return out_c, out_u, keep


def op_build_ct(cond, cond_mask, text_c, text_u, S, drop_audio=False, drop_text=False, compute="fp32"):
    """build_ct alone: cond [B, N, 100], cond_mask [B, N], text_c / text_u [B, N, td] -> [S * N, 128 + roundup(td,
    64)] in the operand dtype."""
    B, N, mel = cond.shape
    assert mel == 100
    dev = cond.device
    cond, text_c, text_u = _f32(cond), _f32(text_c, dev), _f32(text_u, dev)
    td = text_c.shape[2]
    assert text_c.shape == text_u.shape == (B, N, td)
    cm = _u8(cond_mask, dev)
    out = _guarded((S * N, 128 + (td + 63) // 64 * 64), dev, OP_TORCH_DTYPE[compute])
    _glue("f5h_op_build_ct", _lib.stream_handle(dev), _lib.COMPUTE[compute], B, N, td, int(S), int(bool(drop_audio)),
          int(bool(drop_text)), cond.data_ptr(), cm.data_ptr(), text_c.data_ptr(), text_u.data_ptr(), _dp(out))
    return out


def op_pack_y(y, compute="fp32"):
    """y [rows, mel] fp32 -> [rows, 128] in the operand dtype, pad columns zero (pack_y)."""
    rows, mel = y.shape
    y = _f32(y)
    out = _guarded((rows, 128), y.device, OP_TORCH_DTYPE[compute])
    _glue("f5h_op_pack_y", _lib.stream_handle(y.device), _lib.COMPUTE[compute], rows, mel, y.data_ptr(), _dp(out))
    return out


MASK_KIND = {"build_rowkeep": 0, "build_kvlen": 1, "build_textkeep": 2, "build_textlen": 3}


def op_masks(kind, src, S, L=0, off=0):
    """The mask builders. build_rowkeep / build_kvlen: src = dur [B] int32 -> keep [S, L] bytes / kv_len [S] int32;
    build_textkeep / build_textlen: src = text [B, nt] int64 -> keep [S, nt] bytes / len [S] int32."""
    dev = src.device
    k = MASK_KIND[kind]
    if k < 2:
        src = src.to(torch.int32).contiguous()
        B = src.numel()
    else:
        src = src.to(torch.int64).contiguous()
        B, L = src.shape
    out = _guarded((S, L), dev, torch.uint8) if k in (0, 2) else _guarded((S,), dev, torch.int32)
    _glue("f5h_op_masks", _lib.stream_handle(dev), k, B, int(S), int(L), int(off), src.data_ptr(), _dp(out))
    return out


def _fault_word(fault, dev):
    return None if fault is None else torch.tensor([int(fault)], dtype=torch.int32).to(dev)


def op_final_where_out(cond, cond_mask, y, fault=None):
    """where(cond_mask, cond, y) over [B, N, mel]; fault: None (no fault word), 0 or 1 (NaN output)."""
    B, N, mel = y.shape
    dev = y.device
    cond, y, cm, fw = _f32(cond, dev), _f32(y), _u8(cond_mask, dev), _fault_word(fault, dev)
    out = _guarded((B, N, mel), dev)
    _glue("f5h_op_final_where_out", _lib.stream_handle(dev), B, N, mel, cond.data_ptr(), cm.data_ptr(), y.data_ptr(),
          _dp(out), _lib.ptr(fw))
    return out


def op_copy_pred(p, row_off, mel, fault=None):
    """p [S, L, p_ld] -> rows [row_off, L) and columns [0, mel) of every sequence, [S, L - row_off, mel]."""
    S, L, p_ld = p.shape
    p, fw = _f32(p), _fault_word(fault, p.device)
    out = _guarded((S, L - row_off, mel), p.device)
    _glue("f5h_op_copy_pred", _lib.stream_handle(p.device), S, L, int(row_off), int(mel), p_ld, p.data_ptr(), _dp(out),
          _lib.ptr(fw))
    return out


def _op_step(name, method, y, p, p_row_off, use_cfg, cfg, compute, ypad, kbuf, dt, traj, k, grid, n_count, table,
             next_n, trajp, arrive, tick):
    """Shared body of op_cfg_euler / op_cfg_rk: builds the side buffers, launches once, returns them all."""
    B, N, mel = y.shape
    dev = y.device
    total = B * N * mel
    y, p = _f32(y).clone(), _f32(p)
    a = _lib.OpStepArgs()
    a.compute, a.method, a.B, a.N, a.mel, a.use_cfg = _lib.COMPUTE[compute], method, B, N, mel, int(bool(use_cfg))
    a.cfg = float(cfg)
    a.y, a.p = y.data_ptr(), p.data_ptr()
    a.p_seq_stride, a.p_ld, a.p_row_off = p.shape[1] * p.shape[2], p.shape[2], int(p_row_off)
    assert p.shape[0] >= (2 * B if use_cfg else B) and p.shape[1] >= p_row_off + N and p.shape[2] >= mel
    res = {"y": y}
    if ypad is not None:
        res["ypad"] = _guarded((B * N, 128), dev, OP_TORCH_DTYPE[ypad])
        assert ypad == compute, "the launch writes ypad in its compute mode's operand dtype"
        a.ypad = _dp(res["ypad"])
    if kbuf is not None:
        res["kbuf"] = _f32(kbuf).clone()
        assert res["kbuf"].numel() == 3 * total
        a.kbuf = res["kbuf"].data_ptr()
    if k is None:  # host form (Euler)
        a.dt = float(dt)
        if traj:
            res["traj"] = _guarded((B, N, mel), dev)
            a.traj = _dp(res["traj"])
    else:
        steps = len(grid) - 1
        a.nfe = int(n_count)
        res["grid"] = torch.tensor([float(v) for v in grid], dtype=torch.float32).to(dev)
        res["kstep"] = torch.tensor([int(k), OP_FILL], dtype=torch.int32).to(dev)
        a.kstep, a.tgrid = res["kstep"].data_ptr(), res["grid"].data_ptr()
        if trajp is not None:  # False: a slot holding a null base; True: a [steps + 1] trajectory of NaN
            if trajp:
                res["traj"] = _guarded((steps + 1, B, N, mel), dev)
            res["trajp"] = torch.tensor([_dp(res["traj"]) if trajp else 0], dtype=torch.int64).to(dev)
            a.trajp = res["trajp"].data_ptr()
        if table is not None:
            table = _f32(table, dev)
            assert table.shape[0] >= n_count
            nn = table.shape[1] if next_n is None else int(next_n)
            res["next_dst"] = _guarded((nn,), dev)
            a.next_src, a.next_stride, a.next_n, a.next_dst = table.data_ptr(), table.shape[1], nn, _dp(res["next_dst"])
        if arrive:
            res["arrive"] = torch.tensor([0, OP_FILL], dtype=torch.int32).to(dev)
            a.arrive = res["arrive"].data_ptr()
            if tick is not None:
                res["tick"] = torch.tensor([int(tick), OP_FILL], dtype=torch.int32).to(dev)
                a.tick = res["tick"].data_ptr()
    _glue(name, _lib.stream_handle(dev), ctypes.byref(a))
    return res


def op_cfg_euler(y, p, p_row_off=0, use_cfg=True, cfg=2.0, compute="fp32", ypad=None, dt=None, traj=False, k=None,
                 tgrid=None, table=None, next_n=None, trajp=True, arrive=True, tick=0):
    """One cfg_euler launch on a copy of y [B, N, mel] with predictions p [S, rows, p_ld] (sequence B + b is the
    unconditional branch). ypad: None, or the compute mode whose operand copy [B N, 128] to refresh. Host form: dt,
    traj (a trajectory slot). Device-indexed form (k given): tgrid (host values, nfe + 1), table [nfe, stride] (its
    row k + 1 goes to next_dst [next_n]), trajp (None: no slot pointer, False: a null base, True: a [nfe + 1, B, N,
    mel] trajectory), arrive (the step-index bump), tick (None: no tick word). Returns a dict of every buffer the
    launch may write: y, ypad, traj, next_dst, kstep, arrive, tick (int words come with one fill word behind)."""
    n = None if k is None else len(tgrid) - 1
    return _op_step("f5h_op_cfg_euler", _lib.F5H_EULER, y, p, p_row_off, use_cfg, cfg, compute, ypad, None, dt, traj,
                    k, tgrid, n, table, next_n, trajp if k is not None else None, arrive, tick)


def op_cfg_rk(method, y, p, e, sgrid, kbuf=None, p_row_off=0, use_cfg=True, cfg=2.0, compute="fp32", table=None,
              next_n=None, trajp=True, arrive=True, tick=0):
    """One cfg_rk launch (method "midpoint" / "rk4") for evaluation e of the steps of sgrid (host values), on copies
    of y and kbuf [3, B N mel] (rk4). Returns the dict of op_cfg_euler plus kbuf; kstep is the evaluation counter."""
    m = _lib.ODE_METHOD[method]
    stages = {1: 2, 2: 4}[m]
    return _op_step("f5h_op_cfg_rk", m, y, p, p_row_off, use_cfg, cfg, compute, compute, kbuf, None, False, e, sgrid,
                    stages * (len(sgrid) - 1), table, next_n, trajp, arrive, tick)


def attn_force_safe(on: bool):
    """Test hook: every later 16-bit attention launch reruns its key loop in the lazy-running-max form."""
    _lib.check(_lib.lib().f5h_attn_force_safe(int(bool(on))), "attn_force_safe")


def gemm_force_config(cfg: int = -1):
    """Pin the 16-bit GEMM tile configuration (0, 1, 5, 11, 12, 13) for this process; -1 = automatic."""
    _lib.check(_lib.lib().f5h_gemm_force_config(int(cfg)), "gemm_force_config")


def store_policy_force(mode: int = -1):
    """Test / A/B hook: every later GEMM and attention launch of this process (the op entry points included) stores
    plain (0) or write-through wherever a variant exists (1); -1 = as the caller (the engine's policy) chose."""
    _lib.check(_lib.lib().f5h_store_policy_force(int(mode)), "store_policy_force")


def chain_debug_spin_limit(limit: int = -1):
    """Test hook: polls before a phase-chain wait gives up (0: at the first poll that finds its rows not yet
    produced); -1 restores the default (~0.3 s). Applies to launches and graph captures made afterwards."""
    _lib.check(_lib.lib().f5h_chain_debug_spin_limit(int(limit)), "chain_debug_spin_limit")
