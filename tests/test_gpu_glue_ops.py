"""Op-level parity of the audio glue (csrc/melspec.hip, csrc/vocos.hip), prologue and ODE step kernels
(csrc/elementwise.hip): each kernel alone, through its production launcher (f5h_op_* of csrc/engine_ops_glue.cpp), on
the inputs where it can go wrong (tests/op_cases.py lists the branch or edge every shape is there for). Every output
buffer starts as NaN (integers: a fill value) with guard elements behind it, so an element the kernel leaves unwritten
and a write past the contract both show.

Two kinds of comparison.

Bitwise (torch.equal; NaN-aware only where NaN is the expected value) against a float32 torch restatement
(tests/op_reference.py): the gathers mel_frames, vocos_im2col, text_embed, build_ct, pack_y, the mask builders,
final_where_out, copy_pred, and the uncontracted fp32 arithmetic of cfg_euler / cfg_rk (state, trajectory, kbuf and the
16-bit ypad). tests/test_op_refs.py ties each restatement to an independent definition (F.conv1d, torch.stft, the
oracle's TextEmbedding, tests/ode_reference.py).

Against float64 with the measured bound of tests/test_gpu_ops.py,
    |out - R64| <= u_out |R64| + 8 max|R32 - R64|       (all outputs here are fp32: u_out = 0)
with R32 the reference's formula in float32 torch on the CPU: mel_mag, mel_log, vocos_spec, vocos_ola, time_sinus.
Where the reference is NaN or +-inf the kernel must give the same special value (R.assert_close_special).
rope_table uses the bound test_gemm_qkv applies to it, 4 L 2^-24 + 1e-6. tests/test_op_refs.py shows that the wrong
variants of every reference miss these bounds on the same inputs.

Worst measured ratio on the MI355X per op (the bound is 8):

    op                ratio
    mel_mag           1.21
    mel_log           3.64      (ragged form included)
    vocos_spec        1.60
    vocos_ola         1.00      (ragged form included)
    time_sinus        1.11
    rope_table        0.33 of its own bound at L = 8192
"""

import pytest
import torch

import op_cases as C
import op_reference as R
from f5_tts_amd.engine import (OP_FILL, op_build_ct, op_cfg_euler, op_cfg_rk, op_copy_pred, op_final_where_out,
                               op_guard_intact, op_masks, op_mel_frames, op_mel_frames_ragged, op_mel_log,
                               op_mel_log_ragged, op_mel_mag, op_pack_y, op_rope_table, op_text_embed, op_time_sinus,
                               op_vocos_im2col, op_vocos_im2col_ragged, op_vocos_ola, op_vocos_ola_ragged,
                               op_vocos_spec)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(t):
    return None if t is None else t.to(DEV)


def _host(out):
    """The output on the host, after checking that the guard elements behind it were left alone."""
    assert op_guard_intact(out), "the kernel wrote past the end of its output"
    return out.cpu()


def _same_bits(a, b):
    """torch.equal with NaN == NaN (for outputs where NaN is the expected value of some elements)."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ================================================================ bitwise against a torch restatement
@pytest.mark.parametrize("n_fft,hop,L", C.MEL_FRAMES_CASES)
def test_mel_frames(n_fft, hop, L):
    """Centred, reflect-padded framing at B = 3: the shortest legal wave (one frame reflects at both ends), hop
    multiples, interior frames, and the product's n_fft 1024 / hop 256."""
    _need_gpu()
    wav = C.mel_frames_case(n_fft, hop, L)
    out = _host(op_mel_frames(_dev(wav), n_fft, hop))
    assert torch.equal(out, R.mel_frames(wav, n_fft, hop))


def test_mel_frames_refuses_half_window_wave():
    """L = n_fft / 2 has no reflection (torch refuses it too): F5H_EINVAL, nothing launched."""
    _need_gpu()
    with pytest.raises(RuntimeError, match="L > n_fft / 2"):
        op_mel_frames(torch.zeros(3, 32, device=DEV), 64, 16)


def test_mel_frames_ragged():
    """Waves of lengths (33, 1000, 64, 257) in one launch, row stride 1024, NaN past every wave's length: the frames
    are finite (each wave reflects at its own end, nothing reads the padding or the neighbour) and equal the plain
    launch on each wave alone."""
    _need_gpu()
    m = C.MEL_RAGGED
    wav = C.mel_frames_ragged_case()
    out = _host(op_mel_frames_ragged(_dev(wav), m["lens"], m["n_fft"], m["hop"]))
    assert torch.isfinite(out).all()
    o = 0
    for s, n in enumerate(m["lens"]):
        alone = _host(op_mel_frames(_dev(wav[s:s + 1, :n].contiguous()), m["n_fft"], m["hop"]))[0]
        assert torch.equal(alone, R.mel_frames(wav[s:s + 1, :n], m["n_fft"], m["hop"])[0])
        assert torch.equal(out[o:o + alone.shape[0]], alone), f"wave {s}"
        o += alone.shape[0]
    assert o == out.shape[0]


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_vocos_im2col(compute):
    """The embed conv's im2col at T below, at and above the 7-tap window, B = 2; pad columns 700..703 zero."""
    _need_gpu()
    m = C.IM2COL
    for T in m["Ts"]:
        mel = C.im2col_case(T)
        out = _host(op_vocos_im2col(_dev(mel), m["Kp"], compute))
        assert out.dtype == R.OP_DTYPE[compute] and (out[:, 700:] == 0).all()
        assert torch.equal(out, R.im2col7(mel, m["Kp"], compute)), f"T = {T}"


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("layout", ["BNC", "BCT"])
def test_vocos_im2col_ragged(compute, layout):
    """Utterances of lengths (1, 2, 9, 4) gathered in place from the sampler's [B][N][C] output (start > 0) and from
    vocos' [B][C][T], every source frame outside an utterance NaN: the packed rows are finite (taps stop at the
    utterance's own ends) and equal the plain im2col of each utterance alone."""
    _need_gpu()
    m, Kp = C.IM2COL_RAGGED, C.IM2COL["Kp"]
    src, utts = C.im2col_ragged_case(layout)
    out = _host(op_vocos_im2col_ragged(_dev(src), layout, m["starts"], m["lens"], Kp, compute))
    assert torch.isfinite(out.float()).all()
    want = torch.cat([R.im2col7(u, Kp, compute) for u in utts])
    assert torch.equal(out, want)
    for s, u in enumerate(utts):  # and the plain kernel on the utterance alone
        o = sum(m["lens"][:s])
        assert torch.equal(_host(op_vocos_im2col(_dev(u), Kp, compute)), out[o:o + m["lens"][s]])


def test_text_embed():
    """text_embed against TextEmbedding.forward's restatement, both CFG branches and both halves of keep: N cutting,
    matching and padding the text; td with a ragged last lane group; seq_len null and per sample; no freqs, a full
    table, and the 4-row table whose last row serves positions 4..8; mask_padding; fillers inside and at the end."""
    _need_gpu()
    text = _dev(C.TEXT)
    for case in C.TEXT_CASES:
        a = C.text_embed_args(*case)
        ec, eu, keep = op_text_embed(text, _dev(a["table"]), a["N"], seq_len=a["seq_len"], freqs=_dev(a["freqs"]),
                                     freq_rows=a["freq_rows"], mask_padding=a["mask_padding"])
        rc, ru, rk = R.text_embed(C.TEXT, **a)
        assert torch.equal(_host(ec), rc) and torch.equal(_host(eu), ru), case
        assert torch.equal(_host(keep), rk), case


@pytest.mark.parametrize("td", [100, 512])
def test_text_embed_ragged(td):
    """The seg_off form: packed rows of utterances of lengths (7, 3) equal the plain call on each utterance alone
    (N = its length), with and without the masked filler rows."""
    _need_gpu()
    table, freqs = C.text_table(td)
    for fr, mp in ((None, False), (freqs, False), (freqs, True)):
        ec, eu, keep = op_text_embed(_dev(C.TEXT), _dev(table), 0, freqs=_dev(fr), mask_padding=mp,
                                     seg_lens=C.TEXT_SEG_LENS)
        ec, eu, keep = _host(ec), _host(eu), _host(keep)
        o = 0
        for b, n in enumerate(C.TEXT_SEG_LENS):
            ac, au, ak = op_text_embed(_dev(C.TEXT[b:b + 1]), _dev(table), n, freqs=_dev(fr), mask_padding=mp)
            rc, ru, rk = R.text_embed(C.TEXT[b:b + 1], table, n, freqs=fr, mask_padding=mp)
            assert torch.equal(_host(ac), rc) and torch.equal(_host(au), ru) and torch.equal(_host(ak), rk)
            assert torch.equal(ec[o:o + n], rc[0]) and torch.equal(eu[o:o + n], ru[0])
            assert torch.equal(keep[:, o:o + n], rk[:, 0])
            o += n


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_build_ct(compute):
    """The input projection's operand in the three operand dtypes: both branches, and the single-branch forward
    under the four drop-flag combinations; pad columns zero up to 128 and up to the text block's rounded width."""
    _need_gpu()
    for td in C.CT_TDS:
        c = C.ct_case(td)
        for S, da, dt in C.CT_CASES:
            out = _host(op_build_ct(_dev(c["cond"]), _dev(c["cond_mask"]), _dev(c["text_c"]), _dev(c["text_u"]), S,
                                    drop_audio=da, drop_text=dt, compute=compute))
            want = R.build_ct(c["cond"], c["cond_mask"], c["text_c"], c["text_u"], S, da, dt, compute)
            assert out.dtype == want.dtype and torch.equal(out, want), (td, S, da, dt)
            assert (out[:, 100:128] == 0).all() and (out[:, 128 + td:] == 0).all()


@pytest.mark.parametrize("compute", C.COMPUTES)
def test_pack_y(compute):
    _need_gpu()
    for mel in C.PACK_Y["mels"]:
        y = torch.randn(C.PACK_Y["rows"], mel, generator=torch.Generator().manual_seed(mel))
        out = _host(op_pack_y(_dev(y), compute))
        assert torch.equal(out, R.pack_y(y, compute)) and (out[:, mel:] == 0).all()


def test_mask_builders():
    """Exact integers: rowkeep and kvlen with off 0 and 1 over S = 2 B sequences, textkeep, and textlen at nt below,
    at and above the wave's 64 lanes with all-filler, interior-filler and last-position-valid rows."""
    _need_gpu()
    dur = torch.tensor(C.MASK_DUR, dtype=torch.int32)
    S = 2 * dur.numel()
    for off in (0, 1):
        L = C.MASK_L + off
        assert torch.equal(_host(op_masks("build_rowkeep", _dev(dur), S, L, off)),
                           R.masks("build_rowkeep", dur, S, L, off))
        assert torch.equal(_host(op_masks("build_kvlen", _dev(dur), S, off=off)), R.masks("build_kvlen", dur, S, 0, off))
    for nt in C.TEXTLEN_NTS:
        text = C.textlen_case(nt)
        assert torch.equal(_host(op_masks("build_textkeep", _dev(text), S)), R.masks("build_textkeep", text, S))
        got = _host(op_masks("build_textlen", _dev(text), S))
        assert torch.equal(got, R.masks("build_textlen", text, S)), (nt, got)


def test_final_where_out_and_copy_pred():
    """where(cond_mask, cond, y) without a fault word, with it clear, and with it set (all NaN); copy_pred's row
    offset 0 and 1 out of rows of 128 with NaN in the columns past mel."""
    _need_gpu()
    c = C.where_case()
    for fault in (None, 0, 1):
        out = _host(op_final_where_out(_dev(c["cond"]), _dev(c["cond_mask"]), _dev(c["y"]), fault))
        want = R.final_where_out(c["cond"], c["cond_mask"], c["y"], fault)
        assert _same_bits(out, want) and bool(torch.isnan(out).all()) == bool(fault)
    p = C.copy_pred_case()
    for row_off in (0, 1):
        for fault in (None, 0, 1):
            out = _host(op_copy_pred(_dev(p), row_off, 100, fault))
            assert _same_bits(out, R.copy_pred(p, row_off, 100, fault)) and bool(torch.isnan(out).any()) == bool(fault)


# ---------------------------------------------------------------- CFG + ODE updates
STEP_PARAMS = [(shape, lay) for shape in C.STEP_SHAPES for lay in C.STEP_P_LAYOUTS]


def _check_ypad(ypad, yn, compute, mel):
    """The refreshed operand copy: columns < mel are round-to-nearest-even of the new state, bit for bit; the pad
    columns are not the update's to write (they keep the NaN they started with)."""
    ypad = _host(ypad)
    assert ypad.dtype == R.OP_DTYPE[compute]
    assert torch.equal(ypad[:, :mel], R.ypad_of(yn, compute))
    assert torch.isnan(ypad[:, mel:].float()).all()


@pytest.mark.parametrize("shape,layout", STEP_PARAMS)
@pytest.mark.parametrize("use_cfg", [False, True])
def test_cfg_euler_host_form(shape, layout, use_cfg):
    """y += dt (pc + (pc - pu) cfg) with dt and the trajectory slot from the host, in one block and with the
    grid-stride loop wrapping, from both prediction layouts; ypad absent and in each operand dtype."""
    _need_gpu()
    B, N, mel = shape
    row_off, p_ld = layout
    c = C.step_case(B, N, mel, row_off, p_ld)
    dt = 0.15625 + 2.0 ** -20
    want = R.euler_update(c["y"], R.cfg_slope(c["p"], B, N, mel, row_off, use_cfg, C.STEP_CFG), dt)
    for compute, ypad in (("fp32", None), ("fp32", "fp32"), ("bf16", "bf16"), ("fp16", "fp16")):
        for traj in (False, True):
            r = op_cfg_euler(_dev(c["y"]), _dev(c["p"]), p_row_off=row_off, use_cfg=use_cfg, cfg=C.STEP_CFG,
                             compute=compute, ypad=ypad, dt=dt, traj=traj)
            assert torch.equal(r["y"].cpu(), want)
            if traj:
                assert torch.equal(_host(r["traj"]), want)
            if ypad:
                _check_ypad(r["ypad"], want, compute, mel)
            assert set(r) == {"y"} | ({"traj"} if traj else set()) | ({"ypad"} if ypad else set())


def _check_bookkeeping(r, k, n_count, table, traj_slot, yn, untouched_traj=True):
    """The folded step bookkeeping of one device-indexed launch at counter value k of n_count."""
    assert r["kstep"].tolist() == [k + 1, OP_FILL], "the counter is bumped exactly once"
    assert r["arrive"].tolist() == [0, OP_FILL], "the arrival counter is back at 0"
    assert r["tick"].tolist() == [8, OP_FILL], "the tick is bumped once"
    nd = _host(r["next_dst"])
    if k + 1 < n_count:
        assert torch.equal(nd, table[k + 1, :nd.numel()]), "the next table row"
    else:
        assert torch.isnan(nd).all(), "no row is copied at the last step"
    traj = _host(r["traj"])
    for slot in range(traj.shape[0]):
        if slot == traj_slot:
            assert torch.equal(traj[slot], yn), "the trajectory slot k + 1"
        else:
            assert torch.isnan(traj[slot]).all(), f"trajectory slot {slot} was written"


@pytest.mark.parametrize("shape,layout", STEP_PARAMS)
def test_cfg_euler_device_form(shape, layout):
    """The device-indexed form at k = 0, a middle step and k = nfe - 1: dt from the device grid, the trajectory slot
    k + 1 and no other, the next table row except at the last step, the counters; and the forms without a
    trajectory pointer, with a null trajectory base, and without the bump."""
    _need_gpu()
    B, N, mel = shape
    row_off, p_ld = layout
    c = C.step_case(B, N, mel, row_off, p_ld)
    nfe = len(C.STEP_GRID) - 1
    table = C.step_table(nfe)
    v = R.cfg_slope(c["p"], B, N, mel, row_off, True, C.STEP_CFG)
    for k in (0, 2, nfe - 1):
        want = R.euler_update(c["y"], v, R.grid_dt(C.STEP_GRID, k))
        r = op_cfg_euler(_dev(c["y"]), _dev(c["p"]), p_row_off=row_off, cfg=C.STEP_CFG, compute="bf16", ypad="bf16",
                         k=k, tgrid=C.STEP_GRID, table=table, next_n=16, tick=7)
        assert torch.equal(r["y"].cpu(), want)
        _check_ypad(r["ypad"], want, "bf16", mel)
        _check_bookkeeping(r, k, nfe, table, k + 1, want)
    want = R.euler_update(c["y"], v, R.grid_dt(C.STEP_GRID, 1))
    for trajp in (None, False):  # no slot pointer; a slot pointer holding a null base
        r = op_cfg_euler(_dev(c["y"]), _dev(c["p"]), p_row_off=row_off, cfg=C.STEP_CFG, k=1, tgrid=C.STEP_GRID,
                         trajp=trajp, tick=None)
        assert torch.equal(r["y"].cpu(), want) and r["kstep"].tolist() == [2, OP_FILL]
        assert r["arrive"].tolist() == [0, OP_FILL] and "traj" not in r
    r = op_cfg_euler(_dev(c["y"]), _dev(c["p"]), p_row_off=row_off, cfg=C.STEP_CFG, k=1, tgrid=C.STEP_GRID,
                     arrive=False)
    assert torch.equal(r["y"].cpu(), want) and r["kstep"].tolist() == [1, OP_FILL], "no bump without arrive"
    assert torch.equal(_host(r["traj"])[2], want)


@pytest.mark.parametrize("shape,layout", STEP_PARAMS)
@pytest.mark.parametrize("compute", C.COMPUTES)
def test_cfg_rk_midpoint(shape, layout, compute):
    """Both midpoint stages at the first, a middle and the last step: stage 0 writes the stage point to ypad only
    (y, the trajectory untouched), stage 1 updates y, ypad and slot k + 1; the counter counts evaluations."""
    _need_gpu()
    B, N, mel = shape
    row_off, p_ld = layout
    steps = len(C.STEP_GRID) - 1
    neval = 2 * steps
    table = C.step_table(neval)
    c = C.step_case(B, N, mel, row_off, p_ld)
    v = R.cfg_slope(c["p"], B, N, mel, row_off, True, C.STEP_CFG)
    for k in (0, 1, steps - 1):
        dt = R.grid_dt(C.STEP_GRID, k)
        for s in (0, 1):
            e = 2 * k + s
            yn, _ = R.rk_stage("midpoint", s, c["y"], v, dt)
            r = op_cfg_rk("midpoint", _dev(c["y"]), _dev(c["p"]), e, C.STEP_GRID, p_row_off=row_off, cfg=C.STEP_CFG,
                          compute=compute, table=table, next_n=16, tick=7)
            assert torch.equal(r["y"].cpu(), yn if s == 1 else c["y"])
            _check_ypad(r["ypad"], yn, compute, mel)
            _check_bookkeeping(r, e, neval, table, k + 1 if s == 1 else -1, yn)


@pytest.mark.parametrize("shape,layout", STEP_PARAMS)
@pytest.mark.parametrize("use_cfg", [False, True])
def test_cfg_rk4_two_steps(shape, layout, use_cfg):
    """All four rk4 stages of two consecutive steps (the last two of the grid) on one kbuf, each launch fed the
    previous launch's y and kbuf and a fresh prediction: the kept slopes, the stage points, y1 and the trajectory
    agree bit for bit, slopes of the first step do not leak into the second, and the last evaluation copies no row."""
    _need_gpu()
    B, N, mel = shape
    row_off, p_ld = layout
    steps = len(C.STEP_GRID) - 1
    neval = 4 * steps
    table = C.step_table(neval)
    y = C.step_case(B, N, mel, row_off, p_ld)["y"]
    kbuf = torch.full((3, B * N * mel), float("nan"))  # no stage reads a slope before the step has written it
    for k in (steps - 2, steps - 1):
        dt = R.grid_dt(C.STEP_GRID, k)
        for s in range(4):
            e = 4 * k + s
            p = C.step_case(B, N, mel, row_off, p_ld, seed=1 + e)["p"]
            v = R.cfg_slope(p, B, N, mel, row_off, use_cfg, C.STEP_CFG)
            yn, kwant = R.rk_stage("rk4", s, y, v, dt, kbuf.reshape(3, B, N, mel))
            r = op_cfg_rk("rk4", _dev(y), _dev(p), e, C.STEP_GRID, kbuf=_dev(kbuf), p_row_off=row_off,
                          use_cfg=use_cfg, cfg=C.STEP_CFG, compute="fp16", table=table, next_n=16, tick=7)
            assert torch.equal(r["y"].cpu(), yn if s == 3 else y), (k, s)
            assert _same_bits(r["kbuf"].cpu(), kwant.reshape(3, -1)), (k, s)
            _check_ypad(r["ypad"], yn, "fp16", mel)
            _check_bookkeeping(r, e, neval, table, k + 1 if s == 3 else -1, yn)
            y, kbuf = r["y"].cpu(), r["kbuf"].cpu()
        assert torch.isfinite(y).all()


# ================================================================ against float64 with the measured bound
def test_mel_mag():
    """|X_k| over magnitudes from 1e-6 to 1e3 with exact zeros; the spec columns past 2 bins hold NaN and are never
    read, the mag columns past bins come back zero."""
    _need_gpu()
    c = C.mel_mag_case()
    out = _host(op_mel_mag(_dev(c["spec"]), c["bins"], c["ld_mag"]))
    assert (out[:, c["bins"]:] == 0).all() and (out[:, ::37][:, :14] == 0).all()
    R.assert_close(out, C.mel_mag_ref(c, F64), C.mel_mag_ref(c, F32), 0.0, "mel_mag/fp32")


@pytest.mark.parametrize("T", C.MEL_LOG_T)
def test_mel_log(T):
    """log(max(mel, 1e-5)) into the channel-first [B, n_mels, T] layout, around the clamp's edge; +inf stays +inf
    and NaN stays NaN (a NaN bin must not come out as log(1e-5), silence)."""
    _need_gpu()
    B = C.MEL_LOG_B
    c = C.mel_log_case(B * T)
    out = _host(op_mel_log(_dev(c["mel"]), B, T))
    assert out.shape == (B, C.MEL_LOG_NMELS, T)
    frames = [T] * B
    assert int(torch.isnan(out).sum()) == B * T, "one NaN bin per frame went in"
    R.assert_close_special(out, C.mel_log_ref(c, frames, None, F64), C.mel_log_ref(c, frames, None, F32), 0.0,
                           f"mel_log/fp32/T{T}")


def test_mel_log_ragged():
    """The frame-major ragged form: T_s = (1, 3) in T_out = 4, rows past T_s exact zeros, NaN and +inf kept."""
    _need_gpu()
    m = C.MEL_LOG_RAGGED
    c = C.mel_log_case(sum(m["frames"]))
    out = _host(op_mel_log_ragged(_dev(c["mel"]), m["frames"], m["T_out"]))
    for s, t in enumerate(m["frames"]):
        assert (out[s, t:] == 0).all() and not torch.signbit(out[s, t:]).any()
    assert int(torch.isnan(out).sum()) == sum(m["frames"])
    R.assert_close_special(out, C.mel_log_ref(c, m["frames"], m["T_out"], F64),
                           C.mel_log_ref(c, m["frames"], m["T_out"], F32), 0.0, "mel_log/fp32/ragged")


def test_vocos_spec():
    """clip(exp(m), 100) (cos p, sin p) across the clip, at m = +-inf, at phases near 0, +-pi, 1e2 and 1e4; a NaN
    log-magnitude and a NaN phase each give a NaN pair (not magnitude 100); the pad pairs come back zero."""
    _need_gpu()
    c = C.spec_case()
    out = _host(op_vocos_spec(_dev(c["x"]), c["bins"]))
    assert (out[:, 2 * c["bins"]:] == 0).all()
    pairs = out.reshape(c["rows"], -1, 2)
    assert torch.isnan(pairs[0, 5]).all() and torch.isnan(pairs[1, 7]).all() and int(torch.isnan(out).sum()) == 4
    R.assert_close_special(out, C.spec_ref(c, F64), C.spec_ref(c, F32), 0.0, "vocos_spec/fp32")


@pytest.mark.parametrize("n_fft,hop", C.OLA_FFT)
def test_vocos_ola(n_fft, hop):
    """Overlap-add over the squared periodic Hann envelope at B = 2 with fewer, as many and more frames than a
    window covers; T = 1 launches nothing and leaves y untouched."""
    _need_gpu()
    for T in C.OLA_TS:
        c = C.ola_case(n_fft, hop, (T,) * C.OLA_B)
        out = _host(op_vocos_ola(_dev(c["frames"]), c["win"], C.OLA_B, T, hop))
        assert out.shape == (C.OLA_B, (T - 1) * hop)
        R.assert_close(out.reshape(-1), C.ola_ref(c, F64), C.ola_ref(c, F32), 0.0, f"vocos_ola/fp32/{n_fft}-T{T}")
    c = C.ola_case(n_fft, hop, (1,) * C.OLA_B)
    out = op_vocos_ola(_dev(c["frames"]), c["win"], C.OLA_B, 1, hop)
    assert out.shape == (C.OLA_B, 0) and op_guard_intact(out)


@pytest.mark.parametrize("n_fft,hop", C.OLA_FFT)
def test_vocos_ola_ragged(n_fft, hop):
    """Lengths (1, 2, 5, 1, 9): utterance s at (off[s] - s) hop, summed over its own frames only; the packed result
    also equals the plain kernel on each utterance alone, bit for bit. One-frame utterances only: nothing launched."""
    _need_gpu()
    lens = C.OLA_RAGGED_LENS
    c = C.ola_case(n_fft, hop, lens)
    out = _host(op_vocos_ola_ragged(_dev(c["frames"]), c["win"], lens, hop))
    assert out.shape == ((sum(lens) - len(lens)) * hop,)
    R.assert_close(out, C.ola_ref(c, F64), C.ola_ref(c, F32), 0.0, f"vocos_ola/fp32/{n_fft}-ragged")
    o = 0
    for s, T in enumerate(lens):
        alone = _host(op_vocos_ola(_dev(c["frames"][o:o + T]), c["win"], 1, T, hop))[0]
        at = (o - s) * hop
        assert torch.equal(out[at:at + (T - 1) * hop], alone), f"utterance {s}"
        o += T
    c1 = C.ola_case(n_fft, hop, (1, 1, 1))
    out = op_vocos_ola_ragged(_dev(c1["frames"]), c1["win"], (1, 1, 1), hop)
    assert out.numel() == 0 and op_guard_intact(out)


@pytest.mark.parametrize("n", sorted(C.TIME_SINUS_T))
def test_time_sinus(n):
    """The sinusoidal time embedding at n = 1, 5 and the launcher's limit 512: the host-argument form and the
    device-grid form agree bit for bit, both meet the bound, and the row after the last stays NaN (the guard)."""
    _need_gpu()
    c = C.time_sinus_case(n)
    host, dev = _host(op_time_sinus(c["t"], dev=False)), _host(op_time_sinus(c["t"], dev=True))
    assert host.shape == (n, 256) and torch.equal(host, dev)
    if n == 5:
        assert (host[0, :128] == 0).all() and (host[0, 128:] == 1).all(), "t = 0: sin 0, cos 1"
    R.assert_close(host, C.time_sinus_ref(c, F64), C.time_sinus_ref(c, F32), 0.0, f"time_sinus/fp32/n{n}")


def test_time_sinus_refuses_bad_counts():
    _need_gpu()
    for n in (0, 513):
        for dev in (False, True):
            with pytest.raises(RuntimeError, match="1 <= n <= 512"):
                op_time_sinus([0.5] * n, dev=dev)


@pytest.mark.parametrize("L", C.ROPE_LS)
def test_rope_table(L):
    """The rotary table against float64 with the bound test_gemm_qkv applies to it: 4 L 2^-24 + 1e-6."""
    _need_gpu()
    out = _host(op_rope_table(L))
    err = float((out.double() - R.rope_table(L)).abs().max())
    bound = 4 * L * 2.0 ** -24 + 1e-6
    print(f"[op-parity] rope_table/L{L}: max err {err:.3e} = {err / bound:.3f} of the bound {bound:.3e}")
    assert err <= bound
