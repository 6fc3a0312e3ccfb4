// dmx — geometry guidance: the masked-regression loss seed on the GeomHead's output, the mix of its
// input gradient into a prediction, and the data gradient of the network's first conv.  Included by
// k_geom.hip only.
#pragma once
#include "common.h"
#include "dmx.h"
#include "launch.h"
#include "source.h"
#include "tail_math.h"

namespace dmx {

// ---------------------------------------------------------------------------
// Classifier guidance by the GeomHead (include/dmx.h dmx_geom_guide; Dhariwal & Nichol 2021, §4.1):
//   L_n = sum_j m_nj (geom_nj - v_nj)^2 / max(sum_j m_nj, 1e-6)
//   eps' = eps + (s_n sqrt(1 - ab_t)) dL_n/dx
// The kernels live in a translation unit of their own (k_geom.hip; launchers in launch.h): the code
// object of engine.hip gains no kernel.
// ---------------------------------------------------------------------------
// One thread per sample, j in ascending order, one IEEE rounding per operation:
//   d = g - v;  num += (m * (d * d));  den += m;  c = max(den, 1e-6)
//   L = num / c;  seed_j = ((2 * m) * d) / c
// A row whose mask is all zero gives L = 0 and an exactly zero seed (+0: a -0 product is cleared).
static __global__ __launch_bounds__(64) void geom_seed_kernel(const float* geom, const float* vals, const float* mask,
                                                              int n, int gd, float* loss, float* seed) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float *g = geom + (size_t)i * gd, *v = vals + (size_t)i * gd, *m = mask + (size_t)i * gd;
  float num = 0.f, den = 0.f;
  for (int j = 0; j < gd; ++j) {
    const float d = rnd(g[j] - v[j]);
    num = rnd(num + rnd(m[j] * rnd(d * d)));
    den = rnd(den + m[j]);
  }
  const float c = den > 1e-6f ? den : 1e-6f;
  if (loss != nullptr) loss[i] = num / c;
  for (int j = 0; j < gd; ++j) {
    const float d = rnd(g[j] - v[j]);
    const float s = rnd(rnd(2.f * m[j]) * d) / c;
    seed[(size_t)i * gd + j] = m[j] == 0.f ? 0.f : s;
  }
}

// eps' = eps + rnd(rnd(s_n * sig[p - 1]) * g), one element per thread, grid cdiv(n * chw, 256); p is
// the sample's position clamped to [1, S].  Where s_n == 0 or g == 0 the element is copied: eps' has
// eps's bits (a signed zero included, whatever the other operand).  eps_out may alias eps.
static __global__ __launch_bounds__(256) void geom_mix_kernel(const float* eps, const float* grad, const float* scale,
                                                              const float* sig, int S, const int64_t* pos,
                                                              int pos_stride, int n, int64_t chw, float* eps_out,
                                                              int* range_flag) {
  const int64_t total = (int64_t)n * chw, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int s = (int)(i / chw);
  int64_t p = pos[(size_t)s * pos_stride];
  p = p < 1 ? 1 : (p > S ? S : p);
  const float e = eps[i], g = grad[i], sc = scale[s];
  float out = e;
  if (sc != 0.f && g != 0.f) out = e + rnd(rnd(sc * sig[p - 1]) * g);
  flag_nonfinite(range_flag, out);
  eps_out[i] = out;
}

// Data gradient of the first conv (3x3, pad 1, no bias; weight [64][Ci][3][3], Ci <= 4) with respect
// to the network input: dx[n][ci][y][x] = sum_{ky,kx,co} dr[n][y+1-ky][x+1-kx][co] W[co][ci][ky][kx],
// dr NHWC with 64 channels, dx NCHW.  16 lanes per pixel, each holding 4 of the 64 channels (one
// float4 load per tap); a lane accumulates its four channels over the nine taps in tap order with
// FMAs, the 16 partial sums meet in the fixed DPP tree of group_sum16, and lane ci of the group
// stores channel ci.  64 pixels per block (four rounds of 16), the weight staged once per block in
// LDS as [tap][ci][co]; grid (cdiv(HW, 64), N).  Exact fp32, no atomics, a sample's result does not
// depend on the batch.
static __global__ __launch_bounds__(256) void conv0_dgrad_kernel(const float* dr, const float* w, int Ci, int H, int W,
                                                                 float* dx) {
  __shared__ float wl[9 * 4 * 64];
  for (int i = threadIdx.x; i < 9 * 4 * 64; i += 256) {
    const int co = i & 63, ci = (i >> 6) & 3, tap = i >> 8;
    wl[i] = ci < Ci ? w[((size_t)co * Ci + ci) * 9 + tap] : 0.f;
  }
  __syncthreads();
  const int sub = threadIdx.x & 15, n = blockIdx.y, HW = H * W;
  const float* base = dr + (size_t)n * HW * 64 + 4 * sub;
  for (int r = 0; r < 4; ++r) {
    const int pix = blockIdx.x * 64 + r * 16 + (threadIdx.x >> 4);
    const bool valid = pix < HW;
    const int y = valid ? pix / W : 0, x = valid ? pix % W : 0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int yy = y + 1 - tap / 3, xx = x + 1 - tap % 3;
      if (valid && yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const floatx4 d = ld4(base + (size_t)(yy * W + xx) * 64);
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const float* wp = wl + (tap * 4 + ci) * 64 + 4 * sub;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[ci] = __builtin_fmaf(wp[j], d[j], acc[ci]);
        }
      }
    }
    float out[4];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) out[ci] = group_sum16(acc[ci]);
    if (valid && sub < Ci) {
      const float v = sub == 0 ? out[0] : sub == 1 ? out[1] : sub == 2 ? out[2] : out[3];
      dx[((size_t)n * Ci + sub) * HW + pix] = v;
    }
  }
}

}  // namespace dmx
