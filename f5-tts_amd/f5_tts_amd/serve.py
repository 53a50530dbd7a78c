"""In-process request batcher: concurrent `submit()` calls become bucketed ragged batches.

`BatchingSynthesizer` is the layer above `infer.infer_batch` for a process that receives requests from several
threads. A request's wave is bit for bit the wave of its own single run (`infer_batch` of that one item with
`isolate=True` and the LayerNorm fold off), whatever else is queued: every sampler call is an isolated batch
(`CFM.sample(ragged=True)` for DiT models, `isolate=True` for UNetT and MMDiT, the latter to the rounding `isolate`
documents), and a call never carries one utterance alone, because the one-utterance call is the plain call, which
folds the AdaLN LayerNorms on a 16-bit DiT and is then not bitwise the batch's launches. The engine's fold switch is
shared state of the model object and is left alone; instead every call carries at least one filler utterance.

Policy (one dispatcher thread, one completion thread, one non-default stream; DESIGN.md §3 'Request batcher'):
requests are grouped by `(nfe_step, cfg_strength, sway_sampling_coef)`, groups are served oldest head first, FIFO
within a group, at most `max_batch` requests and `max_rows` frames per call (a larger request goes alone). A call
starts when a group is full, when the oldest request has waited `max_wait_ms`, or when fewer than `max_inflight`
batches are in flight (an idle device never waits); never more than `2 * max_inflight` batches are enqueued at once,
so that an overloaded process queues requests, not device buffers.

Capacities: each call's `(B, R, Lmax, nt)` is rounded up by `capacity()` and the gap is filled with filler
utterances (zero-frame prompt, no text, zero noise; outputs dropped), so that different traffic replays one captured
step graph instead of capturing one per call.
"""

from __future__ import annotations

import collections
import contextlib
import threading
import time
from concurrent.futures import Future

import torch

from . import infer
from .model.utils import list_str_to_idx, list_str_to_tensor

B_STEP = 4  # utterances per call round up to a multiple of this
NT_STEP = 16  # text width
LMAX_STEP = 64  # the geometry of the per-utterance launches (one key tile)
MAX_DURATION = 65536  # CFM.sample's max_duration default


def _up(v: int, step: int) -> int:
    return -(-int(v) // step) * step


def capacity(B: int, R: int, Lmax: int, nt: int, row_bucket: int = 256):
    """The shape `(B_cap, R_cap, Lmax_cap, nt_cap)` a sampler call of `B` utterances over `R` frames, the longest
    `Lmax` frames, `nt` text ids wide, is rounded up to. `B` and `R` count the whole call: a call of n requests over r
    frames goes at `capacity(n + 1, r + 1, ...)`, the one filler of one frame every call carries at least.

    * `B_cap`: the next multiple of 4; `nt_cap`: of 16;
    * `Lmax_cap`: the next multiple of 64, and at least `row_bucket` rounded up to one (a filler is at most
      `Lmax_cap` frames long, and one filler must be able to take a whole bucket of rows);
    * `R_cap`: the next multiple of `row_bucket` at or above `R + (B_cap - B)`: every filler has at least one frame.

    Idempotent (`capacity(*capacity(x), rb) == capacity(x, rb)`), never below its arguments, and non-decreasing in
    `R`, `Lmax` and `nt`; `B_cap`, `Lmax_cap` and `nt_cap` are non-decreasing in `B` too. `R_cap` is not: the rows
    reserved for the fillers, `B_cap - B`, shrink to zero as `B` reaches a multiple of 4, so `capacity(5, 254, ..)`
    needs 512 rows at `row_bucket = 256` where `capacity(8, 254, ..)` needs 256. Filler rows of a call,
    `R_cap - r`, stay at or below `row_bucket + B_cap - n`."""
    B, R, Lmax, nt, rb = int(B), int(R), int(Lmax), int(nt), int(row_bucket)
    if min(B, R, Lmax, rb) < 1 or nt < 0 or R < B:
        raise ValueError(f"capacity: B, R, Lmax and row_bucket are at least 1, nt at least 0 and R at least B, got "
                         f"{(B, R, Lmax, nt, rb)}")
    B_cap = _up(B, B_STEP)
    return (B_cap, _up(R + B_cap - B, rb), max(_up(Lmax, LMAX_STEP), _up(rb, LMAX_STEP)), _up(max(nt, 1), NT_STEP))


def filler_lengths(n: int, rows: int) -> "list[int]":
    """`rows` frames over `n` fillers as evenly as they go (the first `rows % n` one frame longer)."""
    return [rows // n + (1 if i < rows % n else 0) for i in range(n)]


class _Request:
    __slots__ = ("seq", "t", "key", "audio", "rms", "ids", "ref", "total", "dur", "seed", "future")


class _Done:
    """The completion marker of a device without streams (CPU fakes): nothing to wait for."""

    def synchronize(self):
        pass


class BatchingSynthesizer:
    """Thread-safe request batcher over one `model_obj` / `vocoder` pair on one device (one synthesizer per process
    and device). `submit()` returns a `concurrent.futures.Future` of `(wave, 24000)`, `wave` a 1-D float32 numpy
    array as `infer.infer_batch` returns it. See the module docstring for the policy and the invariance it keeps.
    `clock` (seconds, monotonic) times the `max_wait_ms` rule; tests inject their own."""

    def __init__(self, model_obj, vocoder, *, max_batch=32, max_rows=None, max_wait_ms=5.0, max_inflight=2,
                 row_bucket=256, target_rms=0.1, device=None, clock=time.monotonic):
        if max_batch < 1 or max_inflight < 1 or row_bucket < 1 or (max_rows is not None and max_rows < 1):
            raise ValueError("max_batch, max_inflight, row_bucket and max_rows are at least 1")
        self.model_obj, self.vocoder = model_obj, vocoder
        self.max_batch, self.max_rows, self.max_wait = int(max_batch), max_rows, float(max_wait_ms) * 1e-3
        self.max_inflight, self.row_bucket, self.target_rms = int(max_inflight), int(row_bucket), target_rms
        self.device = torch.device(device or getattr(model_obj, "device", None) or infer._default_device())
        self._cuda = self.device.type == "cuda"
        self._clock = clock
        self._route = self._pick_route(model_obj)
        self._mel = int(getattr(model_obj, "num_channels", None) or infer.n_mel_channels)
        self._stream = torch.cuda.Stream(self.device) if self._cuda else None
        self._cv = threading.Condition()
        self._groups: "collections.OrderedDict[tuple, collections.deque]" = collections.OrderedDict()
        self._voices: dict = {}
        self._seq = 0
        self._flush_until = 0  # requests up to this sequence number are due at once (hold() exit, close())
        self._held = 0
        self._inflight = 0
        self._closing = False
        self._done: "collections.deque" = collections.deque()  # (event, batch requests, host buffer, offsets)
        self._stats = dict(requests=0, calls=0, failed_calls=0, rows_live=0, rows_filler=0)
        self._calls: "collections.deque" = collections.deque(maxlen=256)
        self._dispatcher = threading.Thread(target=self._dispatch_loop, name="f5-serve-dispatch", daemon=True)
        self._completer = threading.Thread(target=self._complete_loop, name="f5-serve-complete", daemon=True)
        self._dispatcher.start()
        self._completer.start()

    # ------------------------------------------------------------------ the public surface
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close(wait=True)

    def register_voice(self, name, ref_audio, ref_text):
        """The prompt intake once: the prepared wave stays on the device, `submit(voice=name, gen_text=...)` reuses
        it. Registering a name again replaces the voice for later submits."""
        audio, rms, ref_text, ref = infer.prepare_prompt(ref_audio, ref_text, self.target_rms)
        audio = audio.contiguous()
        if self._cuda:
            audio = audio.to(self.device)
            torch.cuda.current_stream(self.device).synchronize()  # set-up call: the wave is resident before any use
        with self._cv:
            self._voices[name] = (audio, rms, ref_text, ref)

    def submit(self, ref_audio=None, ref_text=None, gen_text=None, *, voice=None, nfe_step=32, cfg_strength=2.0,
               sway_sampling_coef=-1.0, speed=1.0, seed=None, fix_duration=None) -> Future:
        """Queue one request; the intake (`infer.prepare_prompt` / `prepare_item`, the tokens, the duration rule)
        runs here, in the caller's thread, and whatever `infer_batch` refuses is raised here as the same ValueError:
        a bad request never enters the queue."""
        if gen_text is None:
            raise ValueError("submit needs gen_text")
        if voice is not None:
            if ref_audio is not None or ref_text is not None:
                raise ValueError("submit takes a registered voice or ref_audio / ref_text, not both")
            with self._cv:
                if voice not in self._voices:
                    raise ValueError(f"voice {voice!r} is not registered")
                prompt = self._voices[voice]
        else:
            if ref_audio is None or ref_text is None:
                raise ValueError("submit needs ref_audio and ref_text, or a registered voice")
            prompt = infer.prepare_prompt(ref_audio, ref_text, self.target_rms)
        item = infer.prepare_item(prompt, gen_text, speed, "request", fix_duration)
        vmap = getattr(self.model_obj, "vocab_char_map", None)
        ids = (list_str_to_idx([item["text"]], vmap) if vmap is not None else list_str_to_tensor([item["text"]]))[0]
        r = _Request()
        r.audio, r.rms, r.ref, r.total = item["audio"].contiguous(), item["rms"], item["ref"], item["total"]
        if self._cuda and r.audio.device.type == "cpu":
            r.audio = r.audio.pin_memory()  # the dispatcher's upload is then a non-blocking copy
        r.ids = ids.to(torch.long)
        # the duration rule of CFM.sample (cfm.py:135-139): the frames this request's own call would have
        r.dur = min(max(max(int(r.ids.numel()), r.ref) + 1, r.total), MAX_DURATION)
        r.seed = None if seed is None else int(seed)
        r.key = (int(nfe_step), float(cfg_strength), None if sway_sampling_coef is None else float(sway_sampling_coef))
        r.future = Future()
        with self._cv:
            if self._closing:
                raise RuntimeError("the synthesizer is closed")
            self._seq += 1
            r.seq, r.t = self._seq, self._clock()
            self._groups.setdefault(r.key, collections.deque()).append(r)
            self._stats["requests"] += 1
            self._cv.notify_all()
        return r.future

    @contextlib.contextmanager
    def hold(self):
        """While open, the dispatcher starts no new call; on exit, batches are formed from everything queued, at
        once and in the documented order, so the composition of the batches is deterministic."""
        with self._cv:
            self._held += 1
        try:
            yield self
        finally:
            with self._cv:
                self._held -= 1
                self._flush_until = self._seq
                self._cv.notify_all()

    def close(self, wait=True):
        """`wait=True`: serve everything queued, then stop. `wait=False`: cancel the queued futures (batches already
        enqueued on the device still resolve). Idempotent."""
        with self._cv:
            self._closing = True
            if not wait:
                for q in self._groups.values():
                    for r in q:
                        r.future.cancel()
                self._groups.clear()
            self._flush_until = self._seq
            self._cv.notify_all()
        self._dispatcher.join()
        self._completer.join()

    def stats(self):
        """Counters since construction: requests, sampler calls (failed ones apart), live and filler rows, the newest
        calls as `dict(live=(B, R, Lmax, nt), cap=(B_cap, R_cap, Lmax_cap, nt_cap), key=..., fillers=[frames],
        host_ms=the engine's host phases of the call)`, what is queued and in flight, and the engine's step-graph capture count (None for a model without an engine)."""
        with self._cv:
            s = dict(self._stats)
            s["calls_detail"] = list(self._calls)
            s["queued"] = sum(len(q) for q in self._groups.values())
            s["inflight"] = self._inflight
        s["filler_share"] = s["rows_filler"] / s["rows_live"] if s["rows_live"] else 0.0
        s["graph_captures"] = self._graph_captures()
        return s

    # ------------------------------------------------------------------ internals
    @staticmethod
    def _pick_route(model_obj) -> str:
        """"ragged" for models `CFM.sample(ragged=True)` serves (DiT), "isolate" for the others."""
        arch = getattr(getattr(model_obj, "transformer", None), "arch", None)
        if arch is None:
            return getattr(model_obj, "serve_route", "ragged")
        from .engine import _refuse_ragged

        try:
            _refuse_ragged(arch)
        except NotImplementedError:
            return "isolate"
        return "ragged"

    def _engine(self):
        net = getattr(self.model_obj, "transformer", None)
        if net is None or not hasattr(net, "get_engine"):
            return None
        return net.get_engine(self.model_obj.engine_compute(), self.model_obj.device)

    def _graph_captures(self):
        eng = self._engine()
        return None if eng is None else eng.graph_stats()["captures"]

    def _host_ms(self):
        """The engine's host milliseconds by phase of the sampler call just made (capture and instantiate among
        them); host counters, nothing waits for the device."""
        eng = self._engine()
        return None if eng is None else eng.last_call_host_ms()

    def _new_event(self):
        if not self._cuda:
            return _Done()
        ev = torch.cuda.Event()
        ev.record(self._stream)
        return ev

    def _take(self, q):
        """The head of a group's queue that one call takes: FIFO, at most max_batch requests and max_rows frames; the
        first always goes (a request above max_rows goes alone). Returns (count, the group is full)."""
        n = rows = 0
        for r in q:
            if n and (n >= self.max_batch or (self.max_rows is not None and rows + r.dur > self.max_rows)):
                break
            n, rows = n + 1, rows + r.dur
        return n, n >= self.max_batch or n < len(q) or (self.max_rows is not None and rows >= self.max_rows)

    def _next_batch(self):
        """Under the lock: the batch to start now, or (None, seconds until the oldest request is due / None)."""
        if (self._held and not self._closing) or not self._groups:
            return None, None
        if self._inflight >= 2 * self.max_inflight:
            return None, None  # a completion wakes the dispatcher
        key = min(self._groups, key=lambda k: self._groups[k][0].seq)  # the group with the oldest head
        q = self._groups[key]
        age = self._clock() - q[0].t
        due = (self._inflight < self.max_inflight or age >= self.max_wait or q[0].seq <= self._flush_until
               or self._closing or any(self._take(g)[1] for g in self._groups.values()))
        if not due:
            return None, max(self.max_wait - age, 1e-4)
        n, _ = self._take(q)
        batch = [q.popleft() for _ in range(n)]
        if not q:
            del self._groups[key]
        return batch, None

    def _dispatch_loop(self):
        while True:
            with self._cv:
                while True:
                    batch, wait = self._next_batch()
                    if batch is not None:
                        self._inflight += 1
                        break
                    if self._closing and not self._groups:
                        self._done.append(None)
                        self._cv.notify_all()
                        return
                    self._cv.wait(wait)
            batch = [r for r in batch if r.future.set_running_or_notify_cancel()]
            entry = None
            if batch:
                try:
                    entry = self._run(batch)
                except BaseException as e:  # this batch's futures only; the synthesizer goes on serving
                    for r in batch:
                        r.future.set_exception(e)
                    with self._cv:
                        self._stats["failed_calls"] += 1
            with self._cv:
                if entry is None:
                    self._inflight -= 1
                else:
                    self._done.append(entry)
                self._cv.notify_all()

    def _complete_loop(self):
        while True:
            with self._cv:
                while not self._done:
                    self._cv.wait()
                entry = self._done.popleft()
            if entry is None:
                return
            event, batch, host, offs = entry
            try:
                event.synchronize()
                waves = [host[a:b].numpy().copy() for a, b in offs]
            except BaseException as e:
                for r in batch:
                    r.future.set_exception(e)
            else:
                for r, w in zip(batch, waves):
                    r.future.set_result((w, infer.target_sample_rate))
            with self._cv:
                self._inflight -= 1
                self._cv.notify_all()

    def _noise(self, r, dtype):
        """Request r's noise: what `torch.manual_seed(seed); torch.randn(dur, mel, device=..., dtype=...)` draws, from
        a generator of the request's own, so other threads' use of the global generator does not enter."""
        g = torch.Generator(device=self.device)
        if r.seed is None:
            g.seed()
        else:
            g.manual_seed(r.seed)
        return torch.randn(r.dur, self._mel, generator=g, device=self.device, dtype=dtype)

    def _run(self, batch):
        """Enqueue one batch on the synthesizer's stream; nothing here waits for the device."""
        ctx = torch.cuda.stream(self._stream) if self._cuda else contextlib.nullcontext()
        with ctx, torch.inference_mode():
            return self._enqueue(batch)

    def _enqueue(self, batch):
        m, n = self.model_obj, len(batch)
        nfe, cfg, sway = batch[0].key
        dur = [r.dur for r in batch]
        live = (n, sum(dur), max(dur), max(int(r.ids.numel()) for r in batch))
        ragged = self._route == "ragged"
        if ragged:
            cap = capacity(n + 1, live[1] + 1, live[2], live[3], self.row_bucket)
            fill = filler_lengths(cap[0] - n, cap[1] - live[1])
        else:  # a padded batch: its shape is (B, N, nt); one filler of Lmax_cap frames sets N, the others one frame
            cap = capacity(n + 1, live[1] + 1, live[2], live[3], 1)
            fill = [cap[2]] + [1] * (cap[0] - n - 1)
            cap = (cap[0], cap[0] * cap[2], cap[2], cap[3])
        B_cap, R_cap, L_cap, nt_cap = cap
        assert all(1 <= f <= L_cap for f in fill) and len(fill) >= 1
        pdtype = next(m.parameters()).dtype if hasattr(m, "parameters") else torch.float32

        wavs = [r.audio.to(self.device, non_blocking=True) for r in batch]
        ref = [r.ref for r in batch]
        cond_live, frames = m.mel_spec.forward_ragged(wavs)
        assert frames == ref
        cond = cond_live.new_zeros(B_cap, cond_live.shape[1], cond_live.shape[2])
        cond[:n] = cond_live
        text = torch.full((B_cap, nt_cap), -1, dtype=torch.long)
        for i, r in enumerate(batch):
            text[i, : r.ids.numel()] = r.ids
        N = max(dur + fill)
        y0 = torch.zeros(B_cap, N, self._mel, device=self.device, dtype=pdtype)
        for i, r in enumerate(batch):
            y0[i, : r.dur] = self._noise(r, pdtype)
        total = [r.total for r in batch] + fill
        kw = dict(ragged=True, ragged_lmax=L_cap) if ragged else dict(isolate=True)
        generated, _ = m.sample(cond=cond, text=text, duration=torch.tensor(total, dtype=torch.long),
                                lens=torch.tensor(ref + [0] * len(fill), dtype=torch.long), steps=nfe,
                                cfg_strength=cfg, sway_sampling_coef=sway, y0=y0, keep_trajectory=False, **kw)
        del _
        host_ms = self._host_ms()
        # the live utterances only: the fillers' frames are dropped here
        wavs = self.vocoder.decode_ragged(generated[:n], ref, [r.total - r.ref for r in batch])
        out = []
        for r, wav in zip(batch, wavs):
            if r.rms < self.target_rms:
                wav = wav * r.rms / self.target_rms
            out.append(wav)
        offs, a = [], 0
        for w in out:
            offs.append((a, a + int(w.shape[0])))
            a += int(w.shape[0])
        packed = torch.cat(out) if len(out) > 1 else out[0]
        if self._cuda:
            host = torch.empty(a, dtype=torch.float32, pin_memory=True)
            host.copy_(packed, non_blocking=True)
        else:
            host = packed.to(torch.float32).contiguous()
        event = self._new_event()
        with self._cv:
            self._stats["calls"] += 1
            self._stats["rows_live"] += live[1]
            self._stats["rows_filler"] += R_cap - live[1]
            self._calls.append(dict(live=live, cap=cap, key=batch[0].key, fillers=fill, host_ms=host_ms))
        return event, batch, host, offs
