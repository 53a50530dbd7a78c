// f5h engine: phase-chain admission and fault word (see engine_internal.h for the map of the engine's files).
#include "engine_internal.h"

// Pinned host words the engines' fault copies land in: one slab per process (allocated once; a hipHostFree per engine
// could wait for the device), slots handed out and returned by index.
static std::mutex g_slot_m;
static unsigned* g_slots = nullptr;
static std::vector<int> g_free_slots;
static constexpr int kFaultSlots = 4096;
int fault_slot_take(volatile unsigned** host) {
  std::lock_guard<std::mutex> lk(g_slot_m);
  if (!g_slots) {
    void* p = nullptr;
    if (hipHostMalloc(&p, kFaultSlots * 64, hipHostMallocDefault) != hipSuccess) return -1;
    g_slots = static_cast<unsigned*>(p);
    for (int i = kFaultSlots - 1; i >= 0; --i) g_free_slots.push_back(i);
  }
  if (g_free_slots.empty()) return -1;
  const int i = g_free_slots.back();
  g_free_slots.pop_back();
  *host = g_slots + (size_t)i * 16;  // one 64-B line per slot
  **host = 0u;
  return i;
}
void fault_slot_give(int i) {
  if (i < 0) return;
  std::lock_guard<std::mutex> lk(g_slot_m);
  g_free_slots.push_back(i);
}

// Per-device admission of chained calls. Two phase-chain launches in flight at once starve each
// other: each one's waiting workgroups hold CU slots the other's producers need (C2 72 instead of 49 ms with the two
// CFG branches on their own streams, profiles/r05_ab_c2_prio_split.txt). A call that would chain while a chained
// call from ANOTHER stream is still being enqueued or still runs on the device (its "done" event not complete) takes
// the separate launches instead (bitwise identical results). Calls on one stream are ordered by the stream itself.
// Non-blocking: one hipEventQuery, no wait.
struct ChainGate {
  std::mutex m;
  hipStream_t owner = nullptr;
  bool owned = false;
  int enqueuing = 0;          // chained calls of the owner stream being enqueued
  hipEvent_t done = nullptr;  // recorded on the owner stream after its last chained call
  bool pending = false;
};
static ChainGate g_gate[64];
static std::atomic<int64_t> g_gate_refused{0};

static bool chain_admit(int dev, hipStream_t st) {
  ChainGate& g = g_gate[dev & 63];
  std::lock_guard<std::mutex> lk(g.m);
  if (g.owned && g.owner != st) {
    bool busy = g.enqueuing > 0;
    if (!busy && g.pending) {
      busy = hipEventQuery(g.done) == hipErrorNotReady;
      (void)hipGetLastError();  // hipErrorNotReady is the expected answer for a pending event
      if (!busy) g.pending = false;
    }
    if (busy) {
      g_gate_refused.fetch_add(1, std::memory_order_relaxed);
      return false;
    }
  }
  g.owner = st;
  g.owned = true;
  ++g.enqueuing;
  return true;
}
static void chain_leave(int dev, hipStream_t st) {
  ChainGate& g = g_gate[dev & 63];
  std::lock_guard<std::mutex> lk(g.m);
  --g.enqueuing;
  if (!g.done && hipEventCreateWithFlags(&g.done, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    g.done = nullptr;
    return;
  }
  if (hipEventRecord(g.done, st) == hipSuccess)
    g.pending = true;
  else
    (void)hipGetLastError();
}
ChainTicket::~ChainTicket() {
  if (held) chain_leave(dev, st);
}
// A call whose modes allow the chain (StepModes::chain_call) asks the gate; admitted, it holds the ticket.
bool chain_for_call(f5h_engine* e, const Ctx& c, ChainTicket& t) {
  if (!c.m.chain_call || !chain_admit(e->dev, c.st)) return false;
  t.dev = e->dev;
  t.st = c.st;
  t.held = true;
  return true;
}
// Start of every sample/forward call: a give-up recorded by an earlier chained call of this engine (its copy in the
// pinned word, landed once that call completed) fails this call and switches the chain off for the engine.
int chain_fault_check(f5h_engine* e, hipStream_t st) {
  if (!e->fault_host || *e->fault_host == 0u) return 0;
  *e->fault_host = 0u;
  {
    std::lock_guard<std::mutex> g(e->gm);
    e->chain = 0;
  }
  (void)hipMemsetAsync(e->chain_fault, 0, sizeof(unsigned), st);
  return fail(F5H_EHIP,
              "phase chain: a wait for a producer row group gave up in an earlier call of this engine (its output was "
              "set to NaN); the chain is now off for this engine (f5h_set_chain re-enables it)");
}
// End of a chained call: the fault word's copy to the pinned host word, stream-ordered behind the call
int chain_fault_note(f5h_engine* e, hipStream_t st) {
  if (!e->fault_host) return 0;
  HIPCK(hipMemcpyAsync(const_cast<unsigned*>(e->fault_host), e->chain_fault, sizeof(unsigned), hipMemcpyDeviceToHost,
                       st));
  return 0;
}

extern "C" {

int f5h_set_chain(f5h_engine* e, int32_t enable) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (enable != 0 && enable != 1) return fail(F5H_EINVAL, "chain must be 0 or 1");
  std::lock_guard<std::mutex> g(e->gm);
  e->chain = enable;
  return 0;
}

int f5h_chain_stats(f5h_engine* e, int64_t* launches, int32_t* fault, int64_t* refused) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (launches) *launches = e->n_chain.load(std::memory_order_relaxed);
  if (refused) *refused = g_gate_refused.load(std::memory_order_relaxed);
  if (fault) {
    *fault = 0;
    if (e->chain_fault) {  // the caller has synchronised with the engine's calls (the device word is final)
      unsigned v = 0;
      HIPCK(hipSetDevice(e->dev));
      HIPCK(hipMemcpyAsync(&v, e->chain_fault, sizeof(v), hipMemcpyDeviceToHost, e->mstream));
      HIPCK(hipStreamSynchronize(e->mstream));
      *fault = v ? 1 : 0;
    }
  }
  return 0;
}

int f5h_chain_debug_spin_limit(int64_t limit) {
  chain_set_spin_limit(limit);
  g_kernel_epoch.fetch_add(1);  // captured graphs hold the old kernel arguments
  return 0;
}

}  // extern "C"
