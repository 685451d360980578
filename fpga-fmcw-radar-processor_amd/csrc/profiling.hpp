// profiling.hpp -- per-kernel timing of a handle (fmcw_set_profiling / fmcw_kernel_times): the event
// pool, the scope of one kernel's launches, and the launch wrapper that attaches the events.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <vector>

#include "internal.hpp"

namespace fmcw {

struct Profiler {
  struct Pending {
    int kid;
    hipEvent_t a, b;
  };
  bool on = false;
  std::vector<Pending> pending;
  std::vector<hipEvent_t> free_events;  // the event pool: created on demand, reused, destroyed with the handle
  double ms[FMCW_K_COUNT] = {};
  uint64_t launches[FMCW_K_COUNT] = {};

  hipEvent_t take_event() {
    hipEvent_t e = nullptr;
    if (free_events.empty()) return hipEventCreate(&e) == hipSuccess ? e : nullptr;
    e = free_events.back();
    free_events.pop_back();
    return e;
  }
  // waits for the pending scopes and adds them to ms / launches
  int collect() {
    for (auto& pe : pending) {
      HIP_TRY(hipEventSynchronize(pe.b));
      float t = 0.f;
      HIP_TRY(hipEventElapsedTime(&t, pe.a, pe.b));
      ms[pe.kid] += t;
      launches[pe.kid] += 1;
      free_events.push_back(pe.a);
      free_events.push_back(pe.b);
    }
    pending.clear();
    return FMCW_OK;
  }
  void destroy_events() {
    for (auto& pe : pending) hipEventDestroy(pe.a), hipEventDestroy(pe.b);
    for (auto e : free_events) hipEventDestroy(e);
  }
};

// The scope's first launch takes the start event and its last launch the stop event through
// hipExtLaunchKernelGGL, so the events carry the dispatches' own begin / end timestamps -- the
// kernels' span, as rocprofv3's kernel trace reports it, without the event marker packets (and
// their dispatch gaps) that hipEventRecord around a launch adds.
struct ProfScope {
  Profiler* p;
  int kid;
  hipEvent_t a = nullptr, b = nullptr;
  bool started = false;
  ProfScope(Profiler* p_, int kid_) : p(p_), kid(kid_) {
    if (p->on) {
      a = p->take_event();
      b = a ? p->take_event() : nullptr;
      if (!b && a) p->free_events.push_back(a), a = nullptr;
    }
  }
  // events for one launch of the scope: start on the first, stop on the one flagged last
  hipEvent_t start() {
    if (started) return nullptr;
    started = true;
    return a;
  }
  hipEvent_t stop(bool last) const { return last ? b : nullptr; }
  ~ProfScope() {
    if (a && b && started) p->pending.push_back({kid, a, b});
    else if (a && b) p->free_events.push_back(a), p->free_events.push_back(b);
  }
};

// hipLaunchKernelGGL with the scope's events (none outside profiling)
template <typename F, typename... Args>
void launch_k(ProfScope& ps, bool last, F fn, dim3 grid, dim3 block, uint32_t smem, hipStream_t s, Args... args) {
  if (ps.a) hipExtLaunchKernelGGL(fn, grid, block, smem, s, ps.start(), ps.stop(last), 0u, args...);
  else hipLaunchKernelGGL(fn, grid, block, smem, s, args...);
}

}  // namespace fmcw
