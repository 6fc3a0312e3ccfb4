// dmx — the optimizer step's kernels (optim.h) and their launcher.
#include "optim.h"

#include "launch.h"

namespace dmx {

void launch_optim_step(const OptimLaunch& o, hipStream_t st) {
  const bool clip = o.max_norm > 0.f && o.norm_out != nullptr;
  if (clip) {
    if (o.n_chunks > 0)
      optim_sqnorm_partials<<<(unsigned)o.n_chunks, 256, 0, st>>>(o.chunks, o.rows, o.partials);
    optim_norm_finish<<<1, 256, 0, st>>>(o.partials, o.n_chunks, o.max_norm, o.norm_out);
  }
  if (o.n_chunks > 0)
    optim_adam_update<<<(unsigned)o.n_chunks, 256, 0, st>>>(o.chunks, o.rows, clip ? o.norm_out : nullptr, o.ema_d,
                                                            o.ema_omd);
}

}  // namespace dmx
