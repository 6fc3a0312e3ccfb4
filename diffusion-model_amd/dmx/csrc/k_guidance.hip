// dmx — CFG rescale kernels (guidance.h) and their launchers.
#include "guidance.h"

namespace dmx {

void launch_cfg_stats(const CfgHeadParams& p, float* eg, double* part, int nb, hipStream_t st) {
  const dim3 grid(nb, p.B);
  if (p.Co == 4) cfg_stats4_kernel<<<grid, 256, 0, st>>>(p, eg, part);
  else cfg_stats_kernel<<<grid, 256, 0, st>>>(p, eg, part);
}

void launch_cfg_scale(float* eg, const double* part, int nb, int pixb, int Co, int HW, int B, float phi,
                      float* ratio_out, hipStream_t st) {
  cfg_scale_kernel<<<dim3((Co * HW + 1023) / 1024, B), 256, 0, st>>>(eg, part, nb, pixb, Co, HW, phi, ratio_out);
}

void launch_cfg_rescale(const float* eu, const float* ec, float g, float phi, float* eps, float* ratio_out, int n,
                        int64_t total, hipStream_t st) {
  cfg_rescale_kernel<<<n, 256, 0, st>>>(eu, ec, g, phi, eps, ratio_out, total);
}

}  // namespace dmx
