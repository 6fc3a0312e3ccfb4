// dmx — the optimizer object of include/dmx.h (dmx_optim): the static chunk table, the ring of per-step
// row tables and the step's launches (launch.h launch_optim_step).  Included by engine.hip only (uses its
// Error / HIPCHK / REQUIRE).
#pragma once
#include "launch.h"
#include "optim_table.h"

// One staging buffer of the ring: the rows in pinned host memory, their device copy, and an event
// recorded behind the last work that reads either (the upload, then the step's kernels).
struct dmx_optim_slot {
  dmx_optim_tensor* host = nullptr;
  dmx_optim_tensor* dev = nullptr;
  hipEvent_t done = nullptr;
  bool used = false;
};

struct dmx_optim {
  int device = 0;
  std::vector<int64_t> numel;
  int64_t n_chunks = 0;
  dmx_optim_chunk* chunks = nullptr;  // device, written once
  double* partials = nullptr;         // device [n_chunks]
  // A slot is rewritten only when its event has completed.  While the device lags, the ring grows up to
  // RING_MAX slots instead of making the host wait; past that the host waits for the oldest step.
  static constexpr int RING_MAX = 8;
  std::vector<dmx_optim_slot> ring;
  int next = 0;
  int cur = -1;  // the slot dmx_optim_set_step filled and no step has consumed yet
};

namespace dmx {

static void optim_free(dmx_optim* o) {
  for (auto& s : o->ring) {
    if (s.done) (void)hipEventSynchronize(s.done), (void)hipEventDestroy(s.done);
    if (s.host) (void)hipHostFree(s.host);
    if (s.dev) (void)hipFree(s.dev);
  }
  if (o->chunks) (void)hipFree(o->chunks);
  if (o->partials) (void)hipFree(o->partials);
  delete o;
}

static dmx_optim_slot optim_new_slot(size_t n) {
  dmx_optim_slot s;
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(dmx_optim_tensor);
  HIPCHK(hipHostMalloc((void**)&s.host, bytes, hipHostMallocDefault));
  HIPCHK(hipMalloc((void**)&s.dev, bytes));
  HIPCHK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  return s;
}

// The slot the next step's rows go to: the next free one in ring order, a new one while the ring may
// grow, else the next in order once its step has finished.
static int optim_take_slot(dmx_optim* o) {
  const int R = (int)o->ring.size();
  for (int k = 0; k < R; ++k) {
    const int i = (o->next + k) % R;
    dmx_optim_slot& s = o->ring[i];
    if (s.used && hipEventQuery(s.done) != hipSuccess) continue;
    (void)hipGetLastError();  // (hipErrorNotReady of a query is no error)
    return i;
  }
  (void)hipGetLastError();
  if (R < dmx_optim::RING_MAX) {
    o->ring.push_back(optim_new_slot(o->numel.size()));
    return R;
  }
  HIPCHK(hipEventSynchronize(o->ring[o->next].done));
  return o->next;
}

static void optim_set_step(dmx_optim* o, const dmx_optim_tensor* rows, int n, hipStream_t st) {
  REQUIRE(n == (int)o->numel.size(), "row count differs from the optimizer's tensor count");
  REQUIRE(rows != nullptr || n == 0, "null rows");
  for (int i = 0; i < n; ++i) {
    const char* bad = optim_row_error(rows[i], o->numel[i]);
    REQUIRE(bad == nullptr, bad);
  }
  const int i = optim_take_slot(o);
  dmx_optim_slot& s = o->ring[i];
  for (int t = 0; t < n; ++t) s.host[t] = optim_row(rows[t]);
  if (n > 0) HIPCHK(hipMemcpyAsync(s.dev, s.host, (size_t)n * sizeof(dmx_optim_tensor), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(s.done, st));
  s.used = true;
  o->cur = i;
  o->next = (i + 1) % (int)o->ring.size();
}

static void optim_step(dmx_optim* o, float max_norm, float ema_d, float ema_omd, float* norm_out, hipStream_t st) {
  if (o->cur < 0) throw Error(DMX_E_STATE, "dmx_optim_step without rows (dmx_optim_set_step)");
  REQUIRE(!(max_norm > 0.f) || norm_out != nullptr, "clipping needs norm_out");
  REQUIRE(std::isfinite(ema_d) && std::isfinite(ema_omd), "ema coefficients must be finite");
  dmx_optim_slot& s = o->ring[o->cur];
  launch_optim_step(OptimLaunch{o->chunks, o->n_chunks, s.dev, o->partials, max_norm, ema_d, ema_omd, norm_out}, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(s.done, st));  // (re-recorded: now behind the kernels that read s.dev)
  o->cur = -1;
}

}  // namespace dmx
