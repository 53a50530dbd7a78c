"""Which modes a call runs in (csrc/engine_modes.cpp step_modes, through the host-only hook f5h_debug_step_modes):
a truth table written down here, and a Python restatement of the conditions as they stood while they were spread
over call_begin, chain_for_call, backbone_part and run_steps, run against the hook over the cross product of the
boolean inputs. No GPU, no engine, no environment."""

import ctypes
import itertools
from types import SimpleNamespace

import pytest

DIT, UNETT, MMDIT = 0, 1, 2
FFN1, ATTN, QKV, FFN2, CONV, OUT, NORM, CHAIN = range(8)  # probe classes (_lib.KCLASS)

IN = ("backbone", "dim", "qk_norm", "long_skip", "bf", "lnf_ok", "rmsf_ok", "chain_slot", "mx8_engine", "chain",
      "lnfold", "pad_skip", "graph_mode", "split_cfg", "mx8_mask", "probe_class", "res32", "skip_ln", "use_cfg",
      "batch_mask", "ragged")
OUT_NAMES = ("mx", "r16", "do_ln", "split", "chain_call", "chain_eligible", "lnfold", "fold_on", "rms_on",
             "out_live_skip", "pad_skip", "probe_class")
BOOLS = ("qk_norm", "long_skip", "lnf_ok", "rmsf_ok", "chain_slot", "mx8_engine", "chain", "lnfold", "pad_skip",
         "graph_mode", "res32", "skip_ln", "use_cfg", "batch_mask", "ragged")


def hook(**kw):
    from f5_tts_amd import _lib

    assert set(kw) == set(IN), set(kw) ^ set(IN)
    a = (ctypes.c_int32 * len(IN))(*[int(kw[n]) for n in IN])
    o = (ctypes.c_int32 * len(OUT_NAMES))()
    assert _lib.lib().f5h_debug_step_modes(a, len(IN), o, len(OUT_NAMES)) == 0
    return dict(zip(OUT_NAMES, o))


def restated(**kw):
    """The conditions of the engine before step_modes existed, place by place."""
    i = SimpleNamespace(**kw)
    dit = i.backbone == DIT
    # call_begin: the MX8 mask of the call; ragged and MX8 calls never ask chain_for_call
    c_mx8 = i.mx8_mask if i.mx8_engine else 0
    # chain_for_call, before chain_admit
    two_parts = i.graph_mode and i.split_cfg == 1 and i.use_cfg
    refused = (not i.chain or not dit or i.bf == 0 or i.res32 or i.dim != 1024 or i.batch_mask or two_parts
               or not i.chain_slot or i.qk_norm or i.long_skip)
    c_chain = False if (i.ragged or c_mx8) else not refused
    c_lnfold = (not i.ragged and not c_mx8 and i.lnfold and not c_chain
                and ((i.lnf_ok and not i.batch_mask) or i.rmsf_ok))
    # backbone_part (backbone_mmdit: r16 = bf != 0 and nothing else)
    mx = c_mx8 if dit else 0
    r16 = i.bf != 0 and (not dit or not i.res32 or mx != 0)
    do_ln = not (i.skip_ln and r16)
    keep = bool(i.batch_mask)
    chain_on = (c_chain and dit and r16 and do_ln and not keep and i.dim == 1024
                and (i.probe_class < 0 or i.probe_class in (ATTN, CONV, CHAIN)))  # (and b.chain, the whole batch)
    fold_on = c_lnfold and dit and r16 and do_ln and not keep and not chain_on and i.lnf_ok  # (and b.lnp)
    rms_on = c_lnfold and i.backbone == UNETT and r16 and i.rmsf_ok  # (and b.lnp)
    live = keep and i.pad_skip and not rms_on and not mx  # (and the out-projection in place)
    # run_steps
    split = i.split_cfg == 1 and not i.ragged
    vals = (mx, r16, do_ln, split, c_chain, chain_on, c_lnfold, fold_on, rms_on, live, i.pad_skip, i.probe_class)
    return {n: int(v) for n, v in zip(OUT_NAMES, vals)}


def case(backbone=DIT, **kw):
    """An engine as f5h_engine_create leaves it (bf16, dim 1024, the defaults of the switches) and a single-utterance
    CFG call, with `kw` laid over it."""
    d = dict(backbone=backbone, dim=1024, qk_norm=0, long_skip=0, bf=1, lnf_ok=int(backbone == DIT),
             rmsf_ok=int(backbone == UNETT), chain_slot=int(backbone == DIT), mx8_engine=0, chain=0,
             lnfold=int(backbone == DIT), pad_skip=1, graph_mode=1, split_cfg=2, mx8_mask=0, probe_class=-1, res32=0,
             skip_ln=0, use_cfg=1, batch_mask=0, ragged=0)
    assert set(kw) <= set(d), kw
    d.update(kw)
    if d["bf"] == 0:  # what creation derives from the compute mode
        d["lnf_ok"] = d["rmsf_ok"] = 0
    return d


MX8 = dict(mx8_engine=1, res32=1)  # (each MX8 row also sets F5H_RES32: the residual stays 16-bit)
ALL_OFF = dict(chain_call=0, chain_eligible=0, lnfold=0, fold_on=0, rms_on=0)
ROWS = [
    ("dit defaults", case(), dict(mx=0, r16=1, do_ln=1, split=0, chain_call=0, chain_eligible=0, lnfold=1, fold_on=1,
                                  rms_on=0, out_live_skip=0, pad_skip=1, probe_class=-1)),
    ("dit chain", case(chain=1), dict(chain_call=1, chain_eligible=1, lnfold=0, fold_on=0, r16=1)),
    ("chain: dim", case(chain=1, dim=512), dict(chain_call=0, chain_eligible=0, fold_on=1)),
    ("chain: batch mask", case(chain=1, batch_mask=1), dict(chain_call=0, chain_eligible=0, fold_on=0)),
    ("chain: two cfg parts", case(chain=1, split_cfg=1), dict(chain_call=0, chain_eligible=0, split=1, fold_on=1)),
    ("chain: cfg parts, eager", case(chain=1, split_cfg=1, graph_mode=0), dict(chain_call=1, chain_eligible=1)),
    ("chain: cfg parts, no cfg", case(chain=1, split_cfg=1, use_cfg=0), dict(chain_call=1, chain_eligible=1)),
    ("chain: qk_norm", case(chain=1, qk_norm=1), dict(chain_call=0, chain_eligible=0, fold_on=1)),
    ("chain: long skip", case(chain=1, long_skip=1), dict(chain_call=0, chain_eligible=0, fold_on=1)),
    ("chain: res32", case(chain=1, res32=1), dict(r16=0, chain_call=0, chain_eligible=0, fold_on=0)),
    ("chain: no fault word", case(chain=1, chain_slot=0), dict(chain_call=0, chain_eligible=0, fold_on=1)),
    # a probed class the chain would absorb: its launches run one by one; the call still counts as chained (gate,
    # graph key, fault word), so the fold stays off as well
    ("chain: probe ffn1", case(chain=1, probe_class=FFN1), dict(chain_call=1, chain_eligible=0, lnfold=0, fold_on=0)),
    ("chain: probe attention", case(chain=1, probe_class=ATTN), dict(chain_call=1, chain_eligible=1)),
    ("chain: probe conv", case(chain=1, probe_class=CONV), dict(chain_call=1, chain_eligible=1)),
    ("chain: probe chain", case(chain=1, probe_class=CHAIN), dict(chain_call=1, chain_eligible=1, probe_class=CHAIN)),
    ("dit batch mask", case(batch_mask=1), dict(lnfold=0, fold_on=0, out_live_skip=1, r16=1)),
    ("dit batch mask, no pad skip", case(batch_mask=1, pad_skip=0), dict(fold_on=0, out_live_skip=0, pad_skip=0)),
    ("dit ragged", case(ragged=1, chain=1, split_cfg=1), dict(**ALL_OFF, split=0, r16=1)),
    ("mx8 all classes", case(mx8_mask=29, chain=1, **MX8), dict(mx=29, r16=1, **ALL_OFF, out_live_skip=0)),
    ("mx8 one class, batch mask", case(mx8_mask=4, batch_mask=1, **MX8), dict(mx=4, r16=1, **ALL_OFF, out_live_skip=0)),
    ("res32", case(res32=1), dict(r16=0, do_ln=1, fold_on=0, chain_eligible=0)),
    ("skip_ln", case(skip_ln=1), dict(r16=1, do_ln=0, fold_on=0, chain_eligible=0)),
    ("skip_ln, chain", case(skip_ln=1, chain=1), dict(do_ln=0, fold_on=0, chain_call=1, chain_eligible=0)),
    ("skip_ln, res32", case(skip_ln=1, res32=1), dict(r16=0, do_ln=1, fold_on=0)),
    ("fp32", case(bf=0, chain=1, batch_mask=0), dict(mx=0, r16=0, do_ln=1, **ALL_OFF)),
    ("fp16", case(bf=2), dict(r16=1, fold_on=1)),
    ("lnfold off", case(lnfold=0), dict(lnfold=0, fold_on=0, chain_eligible=0)),
    ("unett defaults", case(UNETT), dict(mx=0, r16=1, **ALL_OFF)),
    ("unett res32", case(UNETT, res32=1), dict(r16=1)),
    ("unett lnfold", case(UNETT, lnfold=1), dict(lnfold=1, rms_on=1, fold_on=0, mx=0, out_live_skip=0)),
    ("unett lnfold, batch mask", case(UNETT, lnfold=1, batch_mask=1), dict(lnfold=1, rms_on=1, out_live_skip=0, mx=0)),
    ("unett batch mask", case(UNETT, batch_mask=1), dict(rms_on=0, out_live_skip=1)),
    ("unett chain switch", case(UNETT, chain=1, lnfold=1), dict(chain_call=0, chain_eligible=0, rms_on=1, mx=0)),
    ("unett fp32", case(UNETT, bf=0, lnfold=1), dict(r16=0, **ALL_OFF)),
    ("mmdit", case(MMDIT, chain=1, lnfold=1), dict(mx=0, r16=1, **ALL_OFF)),
    ("mmdit batch mask", case(MMDIT, batch_mask=1), dict(mx=0, **ALL_OFF)),
]


@pytest.mark.parametrize("name,inp,want", ROWS, ids=[r[0] for r in ROWS])
def test_truth_table(name, inp, want):
    got = hook(**inp)
    assert {k: got[k] for k in want} == want
    assert restated(**inp) == got


@pytest.mark.parametrize("kw", [dict(), dict(chain=1), dict(batch_mask=1), dict(res32=1)], ids=str)
def test_mx8_engine_with_mask_zero_is_the_bf16_mode(kw):
    assert hook(**case(mx8_engine=1, mx8_mask=0, **kw)) == hook(**case(**kw))


def test_hook_checks_its_array_lengths():
    from f5_tts_amd import _lib

    a = (ctypes.c_int32 * len(IN))()
    o = (ctypes.c_int32 * len(OUT_NAMES))()
    assert _lib.lib().f5h_debug_step_modes(a, len(IN) - 1, o, len(OUT_NAMES)) == -1
    assert _lib.lib().f5h_debug_step_modes(a, len(IN), o, len(OUT_NAMES) + 1) == -1


def reachable(d):
    """Inputs an engine and a call can produce: the capabilities follow the backbone and the compute mode
    (f5h_engine_create), ragged calls are DiT calls without a batch mask (f5h_sample_ragged)."""
    dit, bf = d["backbone"] == DIT, d["bf"] != 0
    if d["lnf_ok"] and not (dit and bf):
        return False
    if d["rmsf_ok"] and not (d["backbone"] == UNETT and bf):
        return False
    if d["mx8_engine"] and not (dit and d["bf"] == 1):
        return False
    if d["chain_slot"] and not dit:
        return False
    if d["ragged"] and (not dit or d["batch_mask"]):
        return False
    return True


# (backbone, dim, bf, split_cfg, mx8_mask, probe_class): every value the conditions tell apart
SETTINGS = [(DIT, 1024, 1, 2, 0, -1), (DIT, 1024, 1, 1, 29, -1), (DIT, 1024, 2, 0, 4, FFN1), (DIT, 512, 1, 2, 0, ATTN),
            (DIT, 1024, 0, 1, 0, -1), (DIT, 1024, 1, 1, 0, CHAIN), (DIT, 1024, 1, 2, 8, NORM),
            (UNETT, 1024, 1, 1, 0, -1), (UNETT, 512, 2, 2, 0, OUT), (UNETT, 1024, 0, 2, 0, -1),
            (MMDIT, 1024, 1, 1, 0, -1), (MMDIT, 512, 0, 2, 0, QKV)]


def test_restatement_agrees_over_the_boolean_cross_product():
    n = 0
    for backbone, dim, bf, split_cfg, mx8_mask, probe_class in SETTINGS:
        for bits in itertools.product((0, 1), repeat=len(BOOLS)):
            d = dict(zip(BOOLS, bits), backbone=backbone, dim=dim, bf=bf, split_cfg=split_cfg, mx8_mask=mx8_mask,
                     probe_class=probe_class)
            if not reachable(d):
                continue
            n += 1
            assert hook(**d) == restated(**d), d
    assert n > 20000
