// f5h engine: the error string, switches, statistics and probes (see engine_internal.h for the map of the engine's
// files).
#include "engine_internal.h"
#include "capi_util.h"

thread_local std::string g_err;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int f5h_internal_fail(int code, const std::string& msg) { return fail(code, msg); }

extern "C" {

const char* f5h_last_error(void) { return g_err.c_str(); }
const char* f5h_version(void) { return "f5h 0.1 gfx950"; }

int f5h_probe_enable(f5h_engine* e, int32_t kclass, int32_t enable) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  std::lock_guard<std::mutex> g(e->pm);
  e->probe_class = enable ? kclass : -1;
  if (e->pstamp) {  // tick = 0, start stamps = max, end stamps = 0
    HIPCK(hipSetDevice(e->dev));
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemset(e->pstamp, 0, 64 * sizeof(unsigned long long)));
    HIPCK(hipMemset(e->pslots, 0xff, (size_t)kProbeEnd * sizeof(unsigned long long)));
    HIPCK(hipMemset(e->pslots + kProbeEnd, 0, (size_t)kProbeEnd * sizeof(unsigned long long)));
    HIPCK(hipMemset(e->ptl, 0, (size_t)kTimelineWG * 4 * sizeof(unsigned long long)));
    HIPCK(hipDeviceSynchronize());
  }
  return 0;
}

int f5h_probe_timeline(f5h_engine* e, uint64_t* stamps, int32_t max_wg, int32_t* n_wg, double* tick_khz) {
  if (!e || !stamps || max_wg <= 0) return fail(F5H_EINVAL, "null engine / buffer");
  std::lock_guard<std::mutex> g(e->pm);
  HIPCK(hipSetDevice(e->dev));
  HIPCK(hipDeviceSynchronize());
  const int n = std::min<int>(max_wg, kTimelineWG);
  HIPCK(hipMemcpy(stamps, e->ptl, (size_t)n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  int last = 0;
  for (int i = 0; i < n; ++i)
    if (stamps[4 * i]) last = i + 1;
  if (n_wg) *n_wg = last;
  if (tick_khz) *tick_khz = e->wall_khz;
  return 0;
}

int f5h_probe_read(f5h_engine* e, int64_t* launches, double* total_ms) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  std::lock_guard<std::mutex> g(e->pm);
  double ms = 0.0;
  int64_t n = 0;
  if (e->pstamp && e->wall_khz > 0.0) {
    HIPCK(hipSetDevice(e->dev));
    HIPCK(hipDeviceSynchronize());
    std::vector<unsigned long long> h(2 * (size_t)kProbeEnd);
    HIPCK(hipMemcpy(h.data(), e->pslots, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long ticks = 0;
    for (int64_t i = 0; i < kProbeEnd; i += (int64_t)kProbeLanes * kProbeStride) {  // one (site, tick)
      unsigned long long t0 = ~0ull, t1 = 0;
      for (int l = 0; l < kProbeLanes; ++l) {
        t0 = std::min(t0, h[i + l * kProbeStride]);
        t1 = std::max(t1, h[kProbeEnd + i + l * kProbeStride]);
      }
      if (t1 == 0 || t0 == ~0ull || t1 < t0) continue;  // no finished launch at this site and tick
      ticks += t1 - t0;
      ++n;
    }
    ms = (double)ticks / e->wall_khz;
  }
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  return 0;
}

int f5h_set_graph_mode(f5h_engine* e, int32_t mode) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (mode != 0 && mode != 1) return fail(F5H_EINVAL, "graph mode must be 0 (eager) or 1 (step graph)");
  std::lock_guard<std::mutex> g(e->gm);
  e->graph_mode = mode;
  return 0;
}

int f5h_set_cfg_streams(f5h_engine* e, int32_t n) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (n < 0 || n > 2) return fail(F5H_EINVAL, "cfg streams must be 0 (auto), 1 or 2");
  std::lock_guard<std::mutex> g(e->gm);
  e->split_cfg = n == 0 ? 2 : (n == 2 ? 1 : 0);
  return 0;
}

int f5h_set_pad_skip(f5h_engine* e, int32_t enable) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (enable != 0 && enable != 1) return fail(F5H_EINVAL, "pad skip must be 0 or 1");
  std::lock_guard<std::mutex> g(e->gm);
  e->pad_skip = enable;
  return 0;
}

int f5h_set_ln_fold(f5h_engine* e, int32_t enable) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (enable != 0 && enable != 1) return fail(F5H_EINVAL, "ln fold must be 0 or 1");
  std::lock_guard<std::mutex> g(e->gm);
  e->lnfold = enable;
  return 0;
}

int f5h_ln_fold_stats(f5h_engine* e, int32_t* supported, int64_t* passes) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (supported) *supported = (e->lnf_ok || e->rmsf_ok) ? 1 : 0;
  if (passes) *passes = e->n_lnfold.load(std::memory_order_relaxed);
  return 0;
}

int f5h_set_store_policy(f5h_engine* e, int32_t mode) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (mode != -1 && mode != 0 && mode != 1 && (mode < 0x100 || mode > 0x11F))
    return fail(F5H_EINVAL, "store policy must be -1 (auto), 0 (plain), 1 (write-through) or 0x100 | class mask");
  std::lock_guard<std::mutex> g(e->gm);
  e->store_policy = mode;  // part of the step graph's key: a cached graph of another policy is not replayed
  return 0;
}

int f5h_store_policy_stats(f5h_engine* e, int64_t* write_through, int64_t* plain) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (write_through) *write_through = e->n_store_wt.load(std::memory_order_relaxed);
  if (plain) *plain = e->n_store_plain.load(std::memory_order_relaxed);
  return 0;
}

int f5h_set_mx8_classes(f5h_engine* e, int32_t mask) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (!e->mx8) return fail(F5H_EINVAL, "set_mx8_classes: not an F5H_MXFP8 engine");
  if (mask & ~(1 | 4 | 8 | 16))
    return fail(F5H_EINVAL, "MX8 class mask: bits 1 (QKV), 4 (out-proj), 8 (FFN1) and 16 (FFN2) only");
  std::lock_guard<std::mutex> g(e->gm);
  e->mx8_mask = mask;  // part of the step graph's key: a cached graph of another mask is not replayed
  return 0;
}

int f5h_mx8_stats(f5h_engine* e, int32_t* mask, int64_t* launches) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (mask) *mask = e->mx8 ? e->mx8_mask : 0;
  if (launches) {
    unsigned long long n = 0;
    if (e->mx8_count) {
      HIPCK(hipSetDevice(e->dev));
      HIPCK(hipMemcpy(&n, e->mx8_count, sizeof(n), hipMemcpyDeviceToHost));
    }
    *launches = (int64_t)n;
  }
  return 0;
}

int f5h_store_policy_force(int32_t mode) {
  if (mode < -1 || mode > 1) return fail(F5H_EINVAL, "forced store policy must be -1 (off), 0 (plain) or 1 (write-through)");
  store_policy_force(mode);
  g_kernel_epoch.fetch_add(1);  // captured graphs hold the old kernel choice
  return 0;
}

int f5h_last_call_host_ms(f5h_engine* e, double* ms, int32_t n) {
  if (!e || !ms || n <= 0) return fail(F5H_EINVAL, "null engine / buffer");
  std::lock_guard<std::mutex> g(e->hm);
  for (int i = 0; i < n; ++i) ms[i] = i < kHostPhases ? e->last_host[i] : 0.0;
  return 0;
}

int f5h_graph_stats(f5h_engine* e, int64_t* captures, int64_t* replays, int32_t* cached) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  std::lock_guard<std::mutex> g(e->gm);
  if (captures) *captures = e->n_captures;
  if (replays) *replays = e->n_replays;
  if (cached) *cached = (int32_t)e->graphs.size();
  return 0;
}

int f5h_gemm_force_config(int32_t cfg) {
  if (cfg != -1 && cfg != 0 && cfg != 1 && cfg != 5 && cfg != 11 && cfg != 12 && cfg != 13)
    return fail(F5H_EINVAL, "gemm config must be -1, 0, 1, 5, 11, 12 or 13");
  gemm_force_config(cfg);
  g_kernel_epoch.fetch_add(1);
  return 0;
}

int f5h_attn_force_safe(int32_t on) {
  attention_force_safe(on);
  g_kernel_epoch.fetch_add(1);  // captured graphs hold the old kernel arguments
  return 0;
}

}  // extern "C"
