// dmx — composed-guidance kernels (compose.h) and their launchers.
#include "compose.h"

namespace dmx {

void launch_compose_tail4(const StepTailParams& p, const ComposeParams& q, bool ddim, bool dpm, dim3 grid,
                          hipStream_t st) {
  if (p.p_o != nullptr && p.d_s != nullptr) {  // a v-model's x0-form instances
    if (dpm) compose_tail4_kernel<false, true, PRED_X0><<<grid, 256, 0, st>>>(p, q);
    else if (ddim) compose_tail4_kernel<true, false, PRED_X0><<<grid, 256, 0, st>>>(p, q);
    else compose_tail4_kernel<false, false, PRED_X0><<<grid, 256, 0, st>>>(p, q);
  } else if (p.p_o != nullptr) {  // a v-model's instances
    if (dpm) compose_tail4_kernel<false, true, PRED_V><<<grid, 256, 0, st>>>(p, q);
    else if (ddim) compose_tail4_kernel<true, false, PRED_V><<<grid, 256, 0, st>>>(p, q);
    else compose_tail4_kernel<false, false, PRED_V><<<grid, 256, 0, st>>>(p, q);
  } else if (dpm) compose_tail4_kernel<false, true><<<grid, 256, 0, st>>>(p, q);
  else if (ddim) compose_tail4_kernel<true><<<grid, 256, 0, st>>>(p, q);
  else compose_tail4_kernel<false><<<grid, 256, 0, st>>>(p, q);
}

void launch_compose_eps(const float* e, const float* weight, int K, int n, int64_t chw, float* eps, hipStream_t st) {
  const int64_t blocks = ((int64_t)n * chw + 255) / 256;
  compose_eps_kernel<<<(unsigned)blocks, 256, 0, st>>>(e, weight, K, n, chw, eps);
}

}  // namespace dmx
