// dmx — CFG rescale: the kernels between the out head and the update of a rescaled CFG step, and the
// standalone form for foreign models.  Included by k_guidance.hip only.
#pragma once
#include "common.h"
#include "launch.h"
#include "source.h"
#include "tail_math.h"

namespace dmx {

// ---------------------------------------------------------------------------
// CFG rescale (include/dmx.h dmx_guidance): eg = eu + g*(ec-eu) scaled per sample by
// r[n] = 1 + phi*(std(ec[n])/std(eg[n]) - 1).  The reduction over a sample's C*HW elements sits
// between the out head and the update, so the rescaled step replaces the one tail launch by
//   cfg_stats4_kernel / cfg_stats_kernel: head + CFG mix as the tails compute them; eg to the
//     arena (NCHW) and, per block, mean and centred sum of squares of ec and eg in double;
//   cfg_scale_kernel: every block combines its sample's partials in block order (the sample mean,
//     then the blocks' M2 plus their means' spread about it), forms r and scales its slice of eg
//     in place;
//   step_tail_kernel (kernels.h) on the scaled eg (its precomputed-eps form).
// They live in a translation unit of their own (k_guidance.hip; launchers in launch.h): the code
// object of engine.hip, which holds the tails, gains no kernel.
// No atomics; a sample's partials depend on that sample alone, so its result does not depend on
// the batch.  A constant sample gives exactly zero deviations in every block and hence r = 1.
// ---------------------------------------------------------------------------
// (the moments go through block_sum2, tail_math.h)
// r from the centred sums of squares of ec and eg over the same element count (which cancels):
// formed in double, rounded to fp32 once; 1 where std(eg) is not a positive finite number.
DMX_DEV float rescale_ratio(double m2c, double m2g, float phi) {
  const double sg = sqrt(m2g);
  if (phi == 0.f || !(sg > 0.0 && sg <= 1.7976931348623157e308)) return 1.f;
  return (float)(1.0 + (double)phi * (sqrt(m2c) / sg - 1.0));
}

// Head path with Co = 4: step_tail4_kernel's loads and DPP reduction (16 lanes per pixel, 16 pixels
// per block); grid (cdiv(HW, 16), B).  p.cfg is 1 here.  part: [B][gridDim.x][4] doubles =
// (mean ec, M2 ec, mean eg, M2 eg) of the block's 4 * min(16, HW - 16 blockIdx.x) values.
static __global__ __launch_bounds__(256) void cfg_stats4_kernel(const CfgHeadParams p, float* eg_out, double* part) {
  __shared__ double sh[512];
  const int sub = threadIdx.x & 15, pix = blockIdx.x * 16 + (threadIdx.x >> 4), n = blockIdx.y;
  const bool valid = pix < p.HW;
  const int pc = valid ? pix : 0;
  const floatx4 a = ld4(p.feat + ((size_t)n * p.HW + pc) * 64 + 4 * sub);
  const floatx4 bb = ld4(p.feat + ((size_t)(n + p.B) * p.HW + pc) * 64 + 4 * sub);
  float eu[4], ec[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const floatx4 w = ld4(p.w + c * 64 + 4 * sub);
    float su = 0.f, sc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      su += w[j] * a[j];
      sc += w[j] * bb[j];
    }
    eu[c] = p.b[c] + group_sum16(su);
    ec[c] = p.b[c] + group_sum16(sc);
  }
  const bool mine = valid && sub < 4;  // lanes 0..3 of the group finish channel c = lane
  const float u = sub == 0 ? eu[0] : sub == 1 ? eu[1] : sub == 2 ? eu[2] : eu[3];
  const float v = sub == 0 ? ec[0] : sub == 1 ? ec[1] : sub == 2 ? ec[2] : ec[3];
  const float e = u + rnd(p.guidance * rnd(v - u));
  if (mine) {
    flag_nonfinite(p.range_flag, e);
    eg_out[((size_t)n * 4 + sub) * p.HW + pix] = e;
  }
  const int rem = p.HW - blockIdx.x * 16;
  const double cnt = 4.0 * (rem < 16 ? rem : 16);
  double sc = mine ? (double)v : 0.0, sg = mine ? (double)e : 0.0;
  block_sum2(sc, sg, sh);
  const double mc = sc / cnt, mg = sg / cnt;
  double dc = mine ? (double)v - mc : 0.0, dg = mine ? (double)e - mg : 0.0;
  dc *= dc;
  dg *= dg;
  block_sum2(dc, dg, sh);
  if (threadIdx.x == 0) {
    double* out = part + ((size_t)n * gridDim.x + blockIdx.x) * 4;
    out[0] = mc;
    out[1] = dc;
    out[2] = mg;
    out[3] = dg;
  }
}

// Generic head path (Co < 4): step_tail_kernel's loads, one pixel per thread and 256 pixels per
// block; grid (cdiv(HW, 256), B).  part as above with Co * min(256, HW - 256 blockIdx.x) values.
static __global__ __launch_bounds__(256) void cfg_stats_kernel(const CfgHeadParams p, float* eg_out, double* part) {
  __shared__ double sh[512];
  const int pix = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y, Co = p.Co;
  const bool valid = pix < p.HW;
  const int pc = valid ? pix : 0;
  const float* fu = p.feat + ((size_t)n * p.HW + pc) * 64;
  const float* fc = p.feat + ((size_t)(n + p.B) * p.HW + pc) * 64;
  float eu[4], ec[4], eg[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) eu[c] = ec[c] = c < Co ? p.b[c] : 0.f;
  for (int k = 0; k < 64; k += 4) {
    const floatx4 fa = ld4(fu + k), fb = ld4(fc + k);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < Co) {
        const floatx4 w = ld4(p.w + c * 64 + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          eu[c] += w[j] * fa[j];
          ec[c] += w[j] * fb[j];
        }
      }
    }
  }
  double sc = 0.0, sg = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    eg[c] = eu[c] + rnd(p.guidance * rnd(ec[c] - eu[c]));
    if (valid && c < Co) {
      flag_nonfinite(p.range_flag, eg[c]);
      eg_out[((size_t)n * Co + c) * p.HW + pix] = eg[c];
      sc += (double)ec[c];
      sg += (double)eg[c];
    }
  }
  const int rem = p.HW - blockIdx.x * 256;
  const double cnt = (double)Co * (rem < 256 ? rem : 256);
  block_sum2(sc, sg, sh);
  const double mc = sc / cnt, mg = sg / cnt;
  double dc = 0.0, dg = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (valid && c < Co) {
      const double da = (double)ec[c] - mc, db = (double)eg[c] - mg;
      dc += da * da;
      dg += db * db;
    }
  }
  block_sum2(dc, dg, sh);
  if (threadIdx.x == 0) {
    double* out = part + ((size_t)n * gridDim.x + blockIdx.x) * 4;
    out[0] = mc;
    out[1] = dc;
    out[2] = mg;
    out[3] = dg;
  }
}

// Stage 2: grid (cdiv(Co*HW, 1024), B).  Every block combines the sample's nb = cdiv(HW, pixb) block
// partials in the same fixed order (block b holds Co * min(pixb, HW - b*pixb) values), so every
// block of a sample scales by the same r; eg is scaled in place, four elements per thread.
static __global__ __launch_bounds__(256) void cfg_scale_kernel(float* eg, const double* part, int nb, int pixb, int Co,
                                                               int HW, float phi, float* ratio_out) {
  __shared__ double sh[512];
  const int n = blockIdx.y;
  const double* q = part + (size_t)n * nb * 4;
  // M2 = sum_b M2_b + sum_b cnt_b (mean_b - mean)^2 with mean = sum_b cnt_b mean_b / (Co HW): thread t
  // takes blocks t, t + 256, ..., and the threads' sums go through the fixed tree of block_sum2
  double sc = 0.0, sg = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) {
    const int rem = HW - b * pixb;
    const double cb = (double)Co * (rem < pixb ? rem : pixb);
    sc += cb * q[4 * b];
    sg += cb * q[4 * b + 2];
  }
  block_sum2(sc, sg, sh);
  const double cnt = (double)Co * HW, mc = sc / cnt, mg = sg / cnt;
  double m2c = 0.0, m2g = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) {
    const int rem = HW - b * pixb;
    const double cb = (double)Co * (rem < pixb ? rem : pixb);
    const double dc = q[4 * b] - mc, dg = q[4 * b + 2] - mg;
    m2c += q[4 * b + 1] + cb * (dc * dc);
    m2g += q[4 * b + 3] + cb * (dg * dg);
  }
  block_sum2(m2c, m2g, sh);
  const float r = rescale_ratio(m2c, m2g, phi);
  if (ratio_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) ratio_out[n] = r;
  const int total = Co * HW;
  float* e = eg + (size_t)n * total;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = blockIdx.x * 1024 + k * 256 + threadIdx.x;
    if (i < total) e[i] = rnd(e[i] * r);
  }
}

// Standalone form (dmx_cfg_rescale; no feature map, no arena): one block per sample over its
// `total` = c*h*w elements — mean, then centred squares, then the scaling, eg recomputed each pass.
// eps may alias eu or ec (each element is read and written by the same thread, in the last pass).
static __global__ __launch_bounds__(256) void cfg_rescale_kernel(const float* eu, const float* ec, float g, float phi,
                                                                 float* eps, float* ratio_out, int64_t total) {
  __shared__ double sh[512];
  const size_t base = (size_t)blockIdx.x * (size_t)total;
  double sc = 0.0, sg = 0.0;
  for (int64_t i = threadIdx.x; i < total; i += 256) {
    const float u = eu[base + i], v = ec[base + i];
    sc += (double)v;
    sg += (double)(u + rnd(g * rnd(v - u)));
  }
  block_sum2(sc, sg, sh);
  const double mc = sc / (double)total, mg = sg / (double)total;
  double dc = 0.0, dg = 0.0;
  for (int64_t i = threadIdx.x; i < total; i += 256) {
    const float u = eu[base + i], v = ec[base + i];
    const double da = (double)v - mc, db = (double)(u + rnd(g * rnd(v - u))) - mg;
    dc += da * da;
    dg += db * db;
  }
  block_sum2(dc, dg, sh);
  const float r = rescale_ratio(dc, dg, phi);
  if (ratio_out != nullptr && threadIdx.x == 0) ratio_out[blockIdx.x] = r;
  for (int64_t i = threadIdx.x; i < total; i += 256) {
    const float u = eu[base + i], v = ec[base + i];
    eps[base + i] = rnd((u + rnd(g * rnd(v - u))) * r);
  }
}

}  // namespace dmx
