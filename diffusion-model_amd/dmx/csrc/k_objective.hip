// dmx — training-objective kernels (objective.h) and their launchers.
#include "objective.h"

#include "launch.h"

namespace dmx {

void launch_train_noise(const dmx_noise_args& a, float* target, hipStream_t st) {
  const int64_t chw = (int64_t)a.C * a.h * a.w, Q = (chw + 3) / 4, total = (int64_t)a.B * Q;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  const void* ptrs[] = {a.z, a.noise, a.z_noisy, target};
  if (objective_aligned16(chw, ptrs, 4)) train_noise_kernel<true><<<blocks, 256, 0, st>>>(a, target, chw, Q, total);
  else train_noise_kernel<false><<<blocks, 256, 0, st>>>(a, target, chw, Q, total);
}

void launch_objective_loss(const dmx_objective_args& a, hipStream_t st) {
  const int64_t chw = (int64_t)a.C * a.h * a.w;
  const void* ptrs[] = {a.eps, a.noise};
  if (objective_aligned16(chw, ptrs, 2)) objective_loss_kernel<true><<<(unsigned)a.B, 256, 0, st>>>(a, chw);
  else objective_loss_kernel<false><<<(unsigned)a.B, 256, 0, st>>>(a, chw);
  objective_finish_kernel<<<1, 256, 0, st>>>(a, chw);
}

void launch_objective_seed(const dmx_objective_args& a, const float* up, float* d_eps, float* d_geom,
                           hipStream_t st) {
  const int64_t chw = (int64_t)a.C * a.h * a.w, Q = (chw + 3) / 4, total = (int64_t)a.B * Q;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  const void* ptrs[] = {a.eps, a.noise, d_eps};
  if (objective_aligned16(chw, ptrs, 3))
    objective_seed_kernel<true><<<blocks, 256, 0, st>>>(a, up, d_eps, d_geom, chw, Q, total);
  else
    objective_seed_kernel<false><<<blocks, 256, 0, st>>>(a, up, d_eps, d_geom, chw, Q, total);
}

}  // namespace dmx
