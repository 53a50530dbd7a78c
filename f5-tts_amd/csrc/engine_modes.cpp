// f5h engine: which modes a call runs in (see engine_internal.h for the map of the engine's files). Host only: no
// device work, and nothing but proc_switches reads the environment.
#include "engine_internal.h"

const ProcSwitches& proc_switches() {
  static const ProcSwitches s = [] {
    const char *r = getenv("F5H_RES32"), *k = getenv("F5H_DIAG_SKIP_LN"), *z = getenv("F5H_CHAIN_ZERO");
    const ProcSwitches p{r && *r == '1', k && *k == '1', z && !strcmp(z, "memset")};
    if (p.skip_ln)
      std::fprintf(stderr, "[f5h] F5H_DIAG_SKIP_LN=1: LayerNorm launches skipped, results are WRONG (timing only)\n");
    return p;
  }();
  return s;
}

// Probe classes (f5h_probe_enable's kclass) whose launches the phase chain does not absorb: the chain may run while one
// of them is probed; the others' launches are timed one by one
static bool probe_beside_chain(int kclass) {
  return kclass < 0 || kclass == KC_ATTN || kclass == KC_CONV || kclass == KC_CHAIN;
}

StepModes step_modes(const ModeIn& in) {
  const bool dit = in.backbone == F5H_DIT, unett = in.backbone == F5H_UNETT;
  const bool bf = in.bf != 0, mask = in.batch_mask != 0, ragged = in.ragged != 0, res32 = in.res32 != 0;
  StepModes m{};
  m.pad_skip = in.pad_skip;
  m.probe_class = in.probe_class;
  // F5H_MXFP8 (DiT only): with any class on MX8 operands the residual stream is 16-bit whatever F5H_RES32 says, and the
  // chain, the fold and the out-projection's live-row skip are off; mask 0 is the bf16 mode, with all of them
  m.mx = (in.mx8_engine && dit) ? in.mx8_mask : 0;
  // residual stream: the operand dtype (as the reference keeps it in the parameter dtype), fp32 in the fp32 parity mode
  m.r16 = bf && (!dit || !res32 || m.mx != 0);
  m.do_ln = !(in.skip_ln && m.r16);
  // auto (split_cfg 2): one packed chain. Ragged: always one chain (the segment tables address the whole packed batch)
  m.split = in.split_cfg == 1 && !ragged;
  // Phase chain: the 16-bit DiT path at dim 1024 without row masks (single-utterance calls, never ragged), and only on
  // the whole packed batch, so not with the CFG branches as two parts. qk_norm / long_skip_connection: the chain's own
  // QKV phase has no norm and its last launch carries the final LayerNorm, which the long skip projection must precede
  const bool two_parts = in.graph_mode && in.split_cfg == 1 && in.use_cfg;
  m.chain_call = in.chain && !ragged && !m.mx && dit && bf && !res32 && in.dim == 1024 && !mask && !two_parts &&
                 in.chain_slot && !in.qk_norm && !in.long_skip;
  m.chain_eligible = m.chain_call && m.r16 && m.do_ln && probe_beside_chain(in.probe_class);
  // Norm folds: never beside the chain, never ragged (each utterance has the bits of its own unfolded call). The DiT
  // LayerNorm fold needs a call without row masks; the UNetT RMSNorm fold serves masked batches too, but then no
  // producer may skip pad-row tiles (their rows' statistics would stay unwritten)
  m.lnfold = !ragged && !m.mx && in.lnfold && !m.chain_call && ((in.lnf_ok && !mask) || in.rmsf_ok);
  m.fold_on = m.lnfold && dit && m.r16 && m.do_ln && !mask && in.lnf_ok;
  m.rms_on = m.lnfold && unett && m.r16 && in.rmsf_ok;
  m.out_live_skip = mask && in.pad_skip && !m.rms_on && !m.mx;
  return m;
}

extern "C" int f5h_debug_step_modes(const int32_t* in, int32_t n_in, int32_t* out, int32_t n_out) {
  if (!in || !out || n_in != (int32_t)(sizeof(ModeIn) / 4) || n_out != (int32_t)(sizeof(StepModes) / 4))
    return fail(F5H_EINVAL, "step_modes: " + std::to_string(sizeof(ModeIn) / 4) + " inputs, " +
                                std::to_string(sizeof(StepModes) / 4) + " outputs");
  ModeIn mi;
  std::memcpy(&mi, in, sizeof(mi));
  const StepModes m = step_modes(mi);
  std::memcpy(out, &m, sizeof(m));
  return 0;
}
