// dmx — geometry-guidance kernels (geom.h) and their launchers.
#include "geom.h"

namespace dmx {

void launch_geom_seed(const float* geom, const float* vals, const float* mask, int n, int gd, float* loss, float* seed,
                      hipStream_t st) {
  geom_seed_kernel<<<(unsigned)((n + 63) / 64), 64, 0, st>>>(geom, vals, mask, n, gd, loss, seed);
}

void launch_geom_mix(const float* eps, const float* grad, const dmx_geom_guide& gg, const int64_t* pos, int pos_stride,
                     int n, int64_t chw, float* eps_out, int* range_flag, hipStream_t st) {
  const int64_t blocks = ((int64_t)n * chw + 255) / 256;
  geom_mix_kernel<<<(unsigned)blocks, 256, 0, st>>>(eps, grad, gg.scale, gg.sig, gg.S, pos, pos_stride, n, chw, eps_out,
                                                    range_flag);
}

void launch_conv0_dgrad(const float* dr, const float* w, int Ci, int n, int H, int W, float* dx, hipStream_t st) {
  conv0_dgrad_kernel<<<dim3((unsigned)((H * W + 63) / 64), (unsigned)n), 256, 0, st>>>(dr, w, Ci, H, W, dx);
}

}  // namespace dmx
