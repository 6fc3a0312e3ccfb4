// dmx — the small device helpers the step tails share with the CFG-rescale kernels (guidance.h):
// the range-guard flag, the one-rounding barrier and the 16-lane DPP sum.
#pragma once
#include <type_traits>

#include "common.h"

namespace dmx {

// Range guard of the split-precision modes: an operand beyond the f16 range (|v| >= 65520)
// becomes inf in its hi plane, and any inf / NaN reaching a network output makes that output
// non-finite.  Output kernels raise a sticky flag (a plain vector store) that the host reads
// at its checkpoints and answers by recomputing in exact-fp32 MFMA mode.
DMX_DEV void flag_nonfinite(int* flag, float v) {
  if (flag != nullptr && !(fabsf(v) <= 3.402823466e38f)) *flag = 1;
}

// One IEEE rounding per reference op: the product is forced through a register
// (opaque asm barrier) so no multiply-add pair can be contracted into an FMA,
// whatever the -ffp-contract mode of the including code.
DMX_DEV float rnd(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

DMX_DEV float group_sum16(float s) {  // sum over aligned 16-lane rows (DPP), same bits in every lane
  auto dpp = [](float v, auto ctrl) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value,
                                                                 0xF, 0xF, false));
  };
  s += dpp(s, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
  s += dpp(s, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
  s += dpp(s, std::integral_constant<int, 0x141>{});  // row_half_mirror
  s += dpp(s, std::integral_constant<int, 0x140>{});  // row_mirror
  return s;
}

}  // namespace dmx
