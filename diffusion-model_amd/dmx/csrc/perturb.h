// dmx — perturbed-attention guidance: the identity-attention core of a perturbed branch.
// Included by k_perturb.hip only.
#pragma once
#include "common.h"
#include "launch.h"
#include "source.h"

namespace dmx {

// ---------------------------------------------------------------------------
// Perturbed-attention guidance (include/dmx.h dmx_perturb): in a perturbed block the softmax of the
// attention core is replaced by the identity, so a token's attention output is its own value vector,
//   ao[m][c] = qkv[m][2C + c]
// the V third of the in_proj output, bias included.  An exact fp32 copy in every precision mode: the
// consumer (tok_attn_out_kernel, or the out_proj GEMM) rounds its operand as it always does.
// One float4 per thread; rows are 3C and C floats with C in {64, 128, 256}, so both sides stay 16-byte
// aligned.  total4 = M * C / 4 float4 of output, sh = log2(C / 4); the row offsets are 64-bit
// (M * 3C * 4 bytes passes 2^31 at N = 320, L = 1024).  Every element of the range is written.
// The kernel lives in a translation unit of its own (k_perturb.hip; launcher in launch.h): the code
// object of engine.hip gains no kernel.
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void attn_identity_kernel(const float* __restrict__ qkv,
                                                                   float* __restrict__ out, int64_t total4, int sh) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int64_t m = i >> sh;                       // token
  const int64_t c4 = i - (m << sh);                // float4 within the token's C channels
  const int64_t src = ((m * 3 + 2) << sh) + c4;    // float4 index of qkv[m][2C + 4 c4]
  *reinterpret_cast<floatx4*>(out + 4 * i) = ld4(qkv + 4 * src);
}

}  // namespace dmx
