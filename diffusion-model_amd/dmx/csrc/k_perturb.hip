// dmx — perturbed-attention guidance kernel (perturb.h) and its launcher.
#include "perturb.h"

namespace dmx {

void launch_attn_identity(const float* qkv, float* out, int64_t M, int C, hipStream_t st) {
  const int sh = C == 64 ? 4 : C == 128 ? 5 : 6;  // log2(C / 4); C in {64, 128, 256} (checked by the callers)
  const int64_t total4 = M << sh;
  if (total4 <= 0) return;
  attn_identity_kernel<<<(unsigned)((total4 + 255) / 256), 256, 0, st>>>(qkv, out, total4, sh);
}

}  // namespace dmx
