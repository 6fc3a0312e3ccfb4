// dmx — MI355X (gfx950) native CFG latent-diffusion sampler: shared device/host helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DMX_DEV __device__ __forceinline__

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace dmx {

// ---------------------------------------------------------------------------
// Whole-wave (64-lane) sums without the LDS pipe: DPP inside each 16-lane row (quad_perm [1,0,3,2],
// [2,3,0,1], row_half_mirror, row_mirror), then v_permlane32_swap (rows 0+2, 1+3) and
// v_permlane16_swap (the two pairs) — six VALU steps instead of six dependent ds_bpermute round
// trips (__shfl_xor).  Fixed order; every lane gets the same bits.
// ---------------------------------------------------------------------------
template <int CTRL>
DMX_DEV unsigned dpp_u32(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
DMX_DEV float dpp_f32(float v) {
  return __builtin_bit_cast(float, dpp_u32<CTRL>(__builtin_bit_cast(unsigned, v)));
}
template <int CTRL>
DMX_DEV double dpp_f64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned long long lo = dpp_u32<CTRL>((unsigned)u), hi = dpp_u32<CTRL>((unsigned)(u >> 32));
  return __builtin_bit_cast(double, lo | (hi << 32));
}
DMX_DEV float wave_sum_dpp(float s) {
  s += dpp_f32<0xB1>(s);
  s += dpp_f32<0x4E>(s);
  s += dpp_f32<0x141>(s);
  s += dpp_f32<0x140>(s);
  unsigned u = __builtin_bit_cast(unsigned, s);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  s = __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
  u = __builtin_bit_cast(unsigned, s);
  r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}
DMX_DEV double wave_sum_dpp(double s) {
  s += dpp_f64<0xB1>(s);
  s += dpp_f64<0x4E>(s);
  s += dpp_f64<0x141>(s);
  s += dpp_f64<0x140>(s);
  auto swap = [](double v, bool sixteen) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
    const auto a = sixteen ? __builtin_amdgcn_permlane16_swap(lo, lo, false, false)
                           : __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto b = sixteen ? __builtin_amdgcn_permlane16_swap(hi, hi, false, false)
                           : __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    const double x = __builtin_bit_cast(double, (unsigned long long)(unsigned)a[0] | ((unsigned long long)(unsigned)b[0] << 32));
    const double y = __builtin_bit_cast(double, (unsigned long long)(unsigned)a[1] | ((unsigned long long)(unsigned)b[1] << 32));
    return x + y;
  };
  s = swap(s, false);
  return swap(s, true);
}

// ---------------------------------------------------------------------------
// Exact (erf) GELU and SiLU in fp32, matching the reference's nn.GELU() /
// F.gelu default (approximate='none') and nn.SiLU (models/unet_cond.py:21,28,63).
// ---------------------------------------------------------------------------
// GELU = x Phi(x), Phi(x) = erfc(-x / sqrt 2) / 2, with erfc(z) = t exp(-z^2 + P(t)), t = 1 / (1 + z / 2)
// for z = |x| / sqrt 2 >= 0 (the classic erfcc Chebyshev fit, fractional error < 1.2e-7): 17 VALU
// operations instead of erff's two-branch ~35, which the GroupNorm-on-load convs pay per staged
// element.  Absolute error <= 2.1e-7 on [0, 3], <= 8.2e-8 on [-3, 0] and <= 3.9e-7 above — the size of
// the reference's own fp32 rounding of 0.5 x (1 + erf(x / sqrt 2)) (<= 2.5e-7 / 4.7e-8 / 4.5e-7 there),
// and far more accurate than that form in the negative tail, where it cancels.  Every GELU of the
// inference path uses this one function, so fused and unfused paths stay bit-identical.
// The exact-fp32 mode (precision 0: the training forward, the fp32 reference mode) keeps the erf
// form (gelu_exact; kernels shared by both modes select it with a uniform flag): the training
// gradients are pinned to the reference's autograd at 1e-4, which the fit's bias does not meet at
// the bench shape.
DMX_DEV float gelu_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
DMX_DEV float gelu(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.5f, z, 1.0f));
  float p = 0.17087277f;
  p = fmaf(p, t, -0.82215223f);
  p = fmaf(p, t, 1.48851587f);
  p = fmaf(p, t, -1.13520398f);
  p = fmaf(p, t, 0.27886807f);
  p = fmaf(p, t, -0.18628806f);
  p = fmaf(p, t, 0.09678418f);
  p = fmaf(p, t, 0.37409196f);
  p = fmaf(p, t, 1.00002368f);
  p = fmaf(p, t, -1.26551223f);
  const float e = t * __builtin_amdgcn_exp2f(fmaf(-z, z, p) * 1.44269504088896340736f);  // erfc(z)
  const float phi = x >= 0.f ? fmaf(-0.5f, e, 1.0f) : 0.5f * e;
  return x * phi;
}
DMX_DEV float silu(float x) { return x / (1.0f + expf(-x)); }

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// fp32 pair -> packed f16 hi pair (v_cvt_pk_f16_f32, RNE) and packed f16 lo pair
// lo = f16(v - hi): v_fma_mix{lo,hi}_f16 computes v * 1.0 - hi with hi read as f16 and rounds
// the exact result once to f16 — the same value as f16((float)(v - (float)hi)) (v - hi is
// exact in fp32 by Sterbenz), in one VOP3P op per element instead of cvt + sub + cvt.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// 2^e with max|x| 2^e in [2^12, 2^13) from the bits of max|x| (0 / non-finite: e = 0)
DMX_DEV int amax_exp(unsigned bits) {
  const float mx = __uint_as_float(bits);
  if (!(mx > 0.f) || !(mx < 3.0e38f)) return 0;
  return min(100, max(-100, 12 - ilogbf(mx)));
}

DMX_DEV void split2u(float a, float b, unsigned& h, unsigned& l) {
  h = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, half2v));
  unsigned t;
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(t) : "v"(a), "v"(h));
  asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(t) : "v"(b), "v"(h));
  l = t;
}

// fp32 -> f16 hi + f16 lo (split-precision operand; lo = f16(v - hi) is exact to ~2^-22 |v|)
DMX_DEV void split4(floatx4 v, half4& h, half4& l) {
  unsigned h0, h1, l0, l1;
  split2u(v[0], v[1], h0, l0);
  split2u(v[2], v[3], h1, l1);
  h = __builtin_bit_cast(half4, (u32x2){h0, h1});
  l = __builtin_bit_cast(half4, (u32x2){l0, l1});
}

// split4 of v * s.  The product is rounded to fp32 once and hi and lo are both taken from that one value
// (split2u's asm reads it from a register).  Written as plain C — h = (_Float16)(v * s), l = (_Float16)(v * s
// - (float)h) — the compiler contracts the two uses of the product differently: the stored hi from the
// fp32-rounded product (v_mul_f32 + v_cvt_pk_f16_f32), lo as v_fma_mix(v, s, -hi') with hi' = f16 of the
// unrounded product.  Where the product lies within an fp32 rounding of an f16 tie, hi and hi' are different
// neighbours and the pair is off by a whole f16 ulp of hi (2^-11 relative instead of 2^-22): about one
// element in 2^13.
DMX_DEV void split4_scaled(floatx4 v, float s, half4& h, half4& l) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] *= s;
  split4(v, h, l);
}

// Input-source modes of a convolution / token GEMM (how the A operand's
// element (n, iy, ix, c) is produced from HBM).
enum SrcMode : int {
  SRC_PLAIN = 0,    // NHWC tensor src0[n][iy][ix][c]
  SRC_GNACT = 1,    // GELU(GroupNorm(src0)) using per-(n,g) (mean, rstd) stats
  SRC_MAXPOOL = 2,  // max_pool2d(src0, 2): src0 is [n][2H'][2W'][c] (floor mode)
  SRC_UPCAT = 3,    // cat[src0 (skip, C0 ch), pad(bilinear_x2_align(src1))]
  SRC_NCHW = 4,     // NCHW tensor src0[n][c][iy][ix], optionally divided by `scale`
};

// Epilogues of the implicit GEMM.
enum EpiMode : int {
  EPI_STATS = 0,     // store (acc + bias?) and per-row GroupNorm partial sums
  EPI_BIAS = 1,      // acc + bias
  EPI_BIAS_GELU = 2, // GELU(acc + bias)
  EPI_BIAS_RES = 3,  // acc + bias + res
  EPI_PARTIAL = 4,   // split-K: raw accumulator into slab[split] (epilogue in splitk_reduce)
};

struct SrcDesc {
  const float* src0;       // primary tensor
  const float* src1;       // UPCAT: the low-resolution tensor to upsample
  const float2* stats;     // GNACT: (mean, rstd) per (n, g)
  const float* gamma;      // GNACT affine
  const float* beta;
  int C;                   // total channels delivered
  int C0;                  // UPCAT: channels of src0 (skip); src1 has C - C0
  int G;                   // GNACT: groups
  int Hs, Ws;              // MAXPOOL: src0 spatial dims; UPCAT: src1 spatial dims
  int padT, padL;          // UPCAT: F.pad offsets of the upsampled map
  int act;                 // GNACT: 1 => apply GELU after the affine
  float scale;             // NCHW: divide by scale (VAE z / 0.18215), 1 => identity
  int n_mod;               // NCHW / UPCAT skip: sample index taken modulo n_mod (CFG: halves share it)
};

}  // namespace dmx
