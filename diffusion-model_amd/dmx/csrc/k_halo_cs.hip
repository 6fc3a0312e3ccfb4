// dmx — igemm_halo_cs_kernel instantiations: the chunk-staged halo conv of the low-resolution maps
// (W = 8, 4: 256-pixel tiles of whole samples, stacked halos, BN = 64; igemm_halo.h), EPI_PARTIAL
// (split-K over channel chunks) and EPI_STATS (W = 8 only: 32-row GroupNorm partials need
// H W % 32 == 0).
#include "igemm_halo.h"
#include "launch.h"

namespace dmx {

template <int SA, int X1>
static void cs_shape(int epi, int w, const X3Params& p, dim3 grid, hipStream_t st) {
  if (w == 8) {
    if (epi == EPI_STATS) igemm_halo_cs_kernel<EPI_STATS, SA, X1, 8><<<grid, 1024, 0, st>>>(p);
    else igemm_halo_cs_kernel<EPI_PARTIAL, SA, X1, 8><<<grid, 1024, 0, st>>>(p);
  } else {
    igemm_halo_cs_kernel<EPI_PARTIAL, SA, X1, 4><<<grid, 1024, 0, st>>>(p);
  }
}

void launch_halo_cs(int epi, int w, int sa, int x1, const X3Params& p, dim3 grid, hipStream_t st) {
  if (sa) { if (x1) cs_shape<1, 1>(epi, w, p, grid, st); else cs_shape<1, 0>(epi, w, p, grid, st); }
  else { if (x1) cs_shape<0, 1>(epi, w, p, grid, st); else cs_shape<0, 0>(epi, w, p, grid, st); }
}

}  // namespace dmx
