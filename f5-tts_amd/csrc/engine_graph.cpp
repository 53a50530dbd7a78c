// f5h engine: the hipGraph cache (see engine_internal.h for the map of the engine's files).
#include "engine_internal.h"

static constexpr size_t kGraphCache = 16;  // cached graphs (prologue and step graphs together)

// The step graph touches only workspace buffers (the ODE state, the trajectory base and the step
// index live in the workspace), so it is keyed by the workspace and the launch shape alone.
// Captured step graphs bake in the kernel choice: forcing a GEMM config or an attention variant
// (tuning/tests) moves the epoch so that later calls capture afresh.
std::atomic<uint64_t> g_kernel_epoch{0};

// F5H_HOST_TRACE=1: host time of the graph-cache phases on stderr (diagnostic)
static bool host_trace() {
  static const bool on = [] {
    const char* v = getenv("F5H_HOST_TRACE");
    return v && *v == '1';
  }();
  return on;
}
// Destroy graveyard entries that nothing replays any more: every event recorded after their
// replays has completed and no caller holds them. Non-blocking (hipEventQuery); caller holds e->gm.
static void reap_graphs(f5h_engine* e) {
  auto done = [e](GraphEntry& g) {
    size_t k = 0;
    for (hipEvent_t ev : g.inflight) {
      if (hipEventQuery(ev) == hipSuccess)
        e->ev_pool.push_back(ev);
      else
        g.inflight[k++] = ev;
    }
    (void)hipGetLastError();  // hipErrorNotReady is the expected answer for a pending event
    g.inflight.resize(k);
    return k == 0;
  };
  for (auto& g : e->graphs)
    if (g->inflight.size() > 4) done(*g);  // keep live entries' lists short
  size_t k = 0;
  for (size_t i = 0; i < e->graveyard.size(); ++i) {
    auto& g = e->graveyard[i];
    if (done(*g) && g.use_count() == 1) {
      ++e->n_reaped;
      continue;  // last reference: destroyed when the slot is overwritten or the vector shrinks
    }
    if (k != i) std::swap(e->graveyard[k], e->graveyard[i]);
    ++k;
  }
  e->graveyard.resize(k);
}

// Record, on `st`, an event after the launches just enqueued from `g` (the entry stays in the
// graveyard until it completes).
int note_replays(f5h_engine* e, GraphEntry* g, hipStream_t st) {
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(e->gm);
    if (!e->ev_pool.empty()) {
      ev = e->ev_pool.back();
      e->ev_pool.pop_back();
    }
  }
  if (!ev) HIPCK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPCK(hipEventRecord(ev, st));
  std::lock_guard<std::mutex> lk(e->gm);
  g->inflight.push_back(ev);
  return 0;
}

// The cached graph for `key`, captured from `body` on the private capture stream(s) when absent.
// An evicted entry moves to the graveyard (no device synchronisation, no wait under the mutex).
int graph_get(Ctx& c, const GraphKey& key, bool split, const std::function<int(Ctx&)>& body,
              std::shared_ptr<GraphEntry>& hold, int64_t replays) {
  f5h_engine* e = c.e;
  const double t0 = host_ms();
  std::lock_guard<std::mutex> g(e->gm);
  const double t1 = host_ms();
  const int64_t reaped0 = e->n_reaped;
  reap_graphs(e);
  const double t2 = host_ms();
  if (c.hp) {
    c.hp[HP_LOCK] += t1 - t0;
    c.hp[HP_REAP] += t2 - t1;
  }
  if (host_trace())
    std::fprintf(stderr, "[f5h host] graph_get kind %d: lock %.3f ms, reap %.3f ms (%lld destroyed)\n", key.kind,
                 t1 - t0, t2 - t1, (long long)(e->n_reaped - reaped0));
  for (const auto& x : e->graphs)
    if (x->key == key) hold = x;
  if (!hold) {
    if (!e->cap) HIPCK(hipStreamCreateWithFlags(&e->cap, hipStreamNonBlocking));
    if (split && !e->cap2) {
      HIPCK(hipStreamCreateWithFlags(&e->cap2, hipStreamNonBlocking));
      HIPCK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
      HIPCK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    }
    auto ne = std::make_shared<GraphEntry>();
    ne->key = key;
    Ctx cc = c;
    cc.st = e->cap;
    cc.st2 = split ? e->cap2 : nullptr;
    const double c0 = host_ms();
    hipError_t be = hipStreamBeginCapture(e->cap, hipStreamCaptureModeThreadLocal);
    if (be != hipSuccess) return fail(F5H_EHIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(be));
    const int rc = body(cc);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(e->cap, &graph);
    if (rc || ce != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      if (rc) return rc;
      return fail(F5H_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    }
    const double c1 = host_ms();
    const hipError_t ie = hipGraphInstantiate(&ne->exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (c.hp) {
      c.hp[HP_CAPTURE] += c1 - c0;
      c.hp[HP_INSTANTIATE] += host_ms() - c1;
    }
    if (host_trace())
      std::fprintf(stderr, "[f5h host] capture %.3f ms, instantiate %.3f ms\n", c1 - c0, host_ms() - c1);
    if (ie != hipSuccess) {
      ne->exec = nullptr;
      return fail(F5H_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
    }
    if (e->graphs.size() >= kGraphCache) {  // evict the least recently used graph to the graveyard
      size_t lru = 0;
      for (size_t i = 1; i < e->graphs.size(); ++i)
        if (e->graphs[i]->stamp < e->graphs[lru]->stamp) lru = i;
      e->graveyard.push_back(std::move(e->graphs[lru]));
      e->graphs.erase(e->graphs.begin() + lru);
      ++e->n_evicted;
    }
    e->graphs.push_back(ne);
    e->n_captures++;
    hold = ne;
  }
  hold->stamp = ++e->use_ctr;
  e->n_replays += replays;
  return 0;
}

// Prologue graphs pay off only when a shape repeats: true when the prologue graph for `key` is
// cached or the key was seen before (remembered in a short FIFO); a first sighting is recorded.
bool prologue_repeats(f5h_engine* e, const GraphKey& key) {
  std::lock_guard<std::mutex> g(e->gm);
  for (const auto& x : e->graphs)
    if (x->key == key) return true;
  for (const auto& k : e->pro_seen)
    if (k == key) return true;
  if (e->pro_seen.size() >= 64) e->pro_seen.erase(e->pro_seen.begin());
  e->pro_seen.push_back(key);
  return false;
}
