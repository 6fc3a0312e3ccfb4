// dmx — the optimizer step's kernels (include/dmx.h dmx_optim): fused multi-tensor Adam / AdamW with
// global-norm clipping and EMA weights.  Included by k_optim.hip only.
#pragma once
#include "common.h"
#include "dmx.h"
#include "source.h"

namespace dmx {

// ---------------------------------------------------------------------------
// One block of 256 threads per chunk (optim_table.h): the chunk names its tensor, the tensor's row holds
// the pointers and coefficients of this step.  Both are block-uniform, so they come through the scalar
// cache.  Memory-bound throughout: 28 B per element (read p, g, m, v; write p, m, v), +8 B with EMA,
// +4 B for the norm pass; about 25 fp32 operations per element, the correctly rounded sqrt and divide
// included, against the ~170 the VALUs could issue per element at the HBM rate.
//
// DMX_OPTIM_CHUNK = 4096 elements = 4 float4 per thread and array: a block moves 112 KiB, the U-Net's
// 23.4 M elements make ~5.8 k blocks (23 per CU, so the last wave of blocks is a few per cent of the
// run), and a tensor's short last chunk (the 191 tensors include 64..512-element biases) wastes at most
// one block's launch, not a share of a larger tile.  At 8 resident waves per SIMD a CU keeps
// 2048 x 4..5 x 16 B = 128..160 KiB of loads in flight, above the ~50 KiB per CU that the HBM rate times
// its latency asks for, so the loop is left rolled.
//
// 128-bit accesses where the row's 16-byte bit is set (chunks start at multiples of 4096 elements, so a
// chunk of an aligned tensor is aligned), for the chunk's multiple-of-4 body; scalar accesses for the
// tail (< 4 elements) and for every element of an unaligned tensor.  All offsets are 64-bit.
// ---------------------------------------------------------------------------

// Block sum in a fixed order (per-thread order is the caller's; whole-wave DPP sum; the four waves in
// index order).  Every thread of the block must call it; thread 0 gets the sum.
DMX_DEV double optim_block_sum(double s) {
  __shared__ double part[4];
  s = wave_sum_dpp(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

// partials[chunk] = sum of squares of the chunk's gradient (0 where the tensor has none), in double: the
// products of fp32 values are exact there, and the sum's rounding stays far below the fp32 result's.
static __global__ __launch_bounds__(256) void optim_sqnorm_partials(const dmx_optim_chunk* __restrict__ chunks,
                                                                    const dmx_optim_tensor* __restrict__ rows,
                                                                    double* __restrict__ partials) {
  const dmx_optim_chunk c = chunks[blockIdx.x];
  const dmx_optim_tensor& r = rows[c.tensor];
  const float* g = r.g;
  double s = 0.0;
  if (g != nullptr) {  // (block-uniform)
    g += c.offset;
    const int body = (r.flags & DMX_OPTIM_ALIGNED) ? (c.len & ~3) : 0;
    for (int i = threadIdx.x * 4; i < body; i += 1024) {
      const floatx4 x = ld4(g + i);
      s += (double)x[0] * x[0];
      s += (double)x[1] * x[1];
      s += (double)x[2] * x[2];
      s += (double)x[3] * x[3];
    }
    for (int i = body + threadIdx.x; i < c.len; i += 256) s += (double)g[i] * g[i];
  }
  s = optim_block_sum(s);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One block: out[0] = norm = sqrt(sum of the n partials), out[1] = coef = min(1, max_norm / (norm + 1e-6))
// in fp32 as torch.nn.utils.clip_grad_norm_ computes it (a NaN norm gives a NaN coef, as there).
static __global__ __launch_bounds__(256) void optim_norm_finish(const double* __restrict__ partials, int64_t n,
                                                                float max_norm, float* __restrict__ out) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += partials[i];
  s = optim_block_sum(s);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    const float c = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = c > 1.0f ? 1.0f : c;
  }
}

struct OptimCoef {
  float coef, step_size, inv_sqrt_bc2, lr_wd, eps, wd, omb1, beta2, omb2, ema_d, ema_omd;
  bool decoupled, ema;
};

DMX_DEV void optim_adam_elem(const OptimCoef& k, float& p, float g, float& m, float& v, float& e) {
  g *= k.coef;
  if (k.decoupled) p = fmaf(-k.lr_wd, p, p);
  else g = fmaf(k.wd, p, g);
  m = fmaf(g - m, k.omb1, m);
  v = fmaf(k.beta2, v, k.omb2 * g * g);
  const float denom = fmaf(sqrtf(v), k.inv_sqrt_bc2, k.eps);
  p -= k.step_size * (m / denom);
  if (k.ema) e = fmaf(k.ema_d, e, k.ema_omd * p);
}

// norm_coef: optim_norm_finish's output, or null without clipping (coef = 1).
static __global__ __launch_bounds__(256) void optim_adam_update(const dmx_optim_chunk* __restrict__ chunks,
                                                                const dmx_optim_tensor* __restrict__ rows,
                                                                const float* __restrict__ norm_coef, float ema_d,
                                                                float ema_omd) {
  const dmx_optim_chunk c = chunks[blockIdx.x];
  const dmx_optim_tensor& r = rows[c.tensor];
  if (r.g == nullptr) return;  // (block-uniform) no gradient this step: the tensor and its state stay
  OptimCoef k;
  k.coef = norm_coef != nullptr ? norm_coef[1] : 1.0f;
  k.step_size = r.step_size;
  k.inv_sqrt_bc2 = r.inv_sqrt_bc2;
  k.lr_wd = r.lr_wd;
  k.eps = r.eps;
  k.wd = r.wd;
  k.omb1 = r.omb1;
  k.beta2 = r.beta2;
  k.omb2 = r.omb2;
  k.ema_d = ema_d;
  k.ema_omd = ema_omd;
  k.decoupled = (r.flags & DMX_OPTIM_DECOUPLED) != 0;
  k.ema = r.ema != nullptr;
  float* __restrict__ p = r.p + c.offset;
  const float* __restrict__ g = r.g + c.offset;
  float* __restrict__ m = r.m + c.offset;
  float* __restrict__ v = r.v + c.offset;
  float* __restrict__ e = k.ema ? r.ema + c.offset : nullptr;
  const int body = (r.flags & DMX_OPTIM_ALIGNED) ? (c.len & ~3) : 0;
  for (int i = threadIdx.x * 4; i < body; i += 1024) {
    floatx4 p4 = ld4(p + i), m4 = ld4(m + i), v4 = ld4(v + i), e4 = {0.f, 0.f, 0.f, 0.f};
    const floatx4 g4 = ld4(g + i);
    if (k.ema) e4 = ld4(e + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float p1 = p4[j], m1 = m4[j], v1 = v4[j], e1 = e4[j];
      optim_adam_elem(k, p1, g4[j], m1, v1, e1);
      p4[j] = p1;
      m4[j] = m1;
      v4[j] = v1;
      e4[j] = e1;
    }
    *reinterpret_cast<floatx4*>(p + i) = p4;
    *reinterpret_cast<floatx4*>(m + i) = m4;
    *reinterpret_cast<floatx4*>(v + i) = v4;
    if (k.ema) *reinterpret_cast<floatx4*>(e + i) = e4;
  }
  for (int i = body + threadIdx.x; i < c.len; i += 256) {
    float p1 = p[i], m1 = m[i], v1 = v[i], e1 = k.ema ? e[i] : 0.f;
    optim_adam_elem(k, p1, g[i], m1, v1, e1);
    p[i] = p1;
    m[i] = m1;
    v[i] = v1;
    if (k.ema) e[i] = e1;
  }
}

}  // namespace dmx
