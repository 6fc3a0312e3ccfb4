// dmx — the standalone v-prediction conversion (prediction.h) and its launcher.
#include "prediction.h"

#include "launch.h"

namespace dmx {

void launch_pred_to_eps(const float* out, const float* x, const int64_t* t, int t_stride, const float* p_o,
                        const float* p_x, int T, int n, int64_t chw, float* eps_out, hipStream_t st) {
  const int64_t blocks = ((int64_t)n * chw + 255) / 256;
  pred_to_eps_kernel<<<(unsigned)blocks, 256, 0, st>>>(out, x, t, t_stride, p_o, p_x, T, n, chw, eps_out);
}

void launch_pred_split(const float* out, const float* x, const int64_t* t, int t_stride, const float* p_o,
                       const float* p_x, int T, int n, int64_t chw, float* x0_out, float* eps_out, hipStream_t st) {
  const int64_t blocks = ((int64_t)n * chw + 255) / 256;
  pred_split_kernel<<<(unsigned)blocks, 256, 0, st>>>(out, x, t, t_stride, p_o, p_x, T, n, chw, x0_out, eps_out);
}

}  // namespace dmx
