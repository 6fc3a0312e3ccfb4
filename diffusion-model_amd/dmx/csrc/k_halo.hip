// dmx — igemm_halo_kernel (halo-staged split-precision 3x3 conv, whole image rows at W = 16 / 32)
// instantiations (see launch.h).  16-wave blocks: 4 x 4 waves of 64 x 32 at BN = 128, 8 x 2 waves
// of 32 x 32 at BN = 64.
#include "igemm_halo.h"
#include "launch.h"

namespace dmx {

template <int BN, int SA, int X1, int W>
static void go(int gna, const X3Params& p, dim3 grid, hipStream_t st) {
  constexpr int NWN = BN == 128 ? 4 : 2, NWM = 16 / NWN;
  if constexpr (SA == 0) {
    if (gna == 1) {
      igemm_halo_kernel<BN, EPI_STATS, 0, X1, W, 1, NWN, NWM><<<grid, 1024, 0, st>>>(p);
      return;
    }
    if (gna == 2) {
      igemm_halo_kernel<BN, EPI_STATS, 0, X1, W, 2, NWN, NWM><<<grid, 1024, 0, st>>>(p);
      return;
    }
  }
  igemm_halo_kernel<BN, EPI_STATS, SA, X1, W, 0, NWN, NWM><<<grid, 1024, 0, st>>>(p);
}

template <int SA, int X1>
static void by_shape(int bn, int w, int gna, const X3Params& p, dim3 grid, hipStream_t st) {
  if (w == 32) {
    if (bn == 128) go<128, SA, X1, 32>(gna, p, grid, st); else go<64, SA, X1, 32>(gna, p, grid, st);
  } else {
    if (bn == 128) go<128, SA, X1, 16>(gna, p, grid, st); else go<64, SA, X1, 16>(gna, p, grid, st);
  }
}

void launch_halo(int bn, int w, int sa, int x1, int gna, const X3Params& p, dim3 grid, hipStream_t st) {
  if (sa) { if (x1) by_shape<1, 1>(bn, w, 0, p, grid, st); else by_shape<1, 0>(bn, w, 0, p, grid, st); }
  else { if (x1) by_shape<0, 1>(bn, w, gna, p, grid, st); else by_shape<0, 0>(bn, w, gna, p, grid, st); }
}

}  // namespace dmx
