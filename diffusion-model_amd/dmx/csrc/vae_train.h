// dmx — kernels of the VAE training step (train_vae.py: `_, _, loss, _ = vae(x); loss.backward()`
// over models/vae.py:51-76) that the U-Net step (train.h) does not already have:
//   the encoder tail with a tape (raw mu / logvar, the NHWC decoder input), its adjoint (heads +
//   reparameterisation + clamp + KL), the GroupNorm(8) + GELU adjoint, the sigmoid adjoint and the
//   direct gradients of the two convs with 3 / 4 channels on one side (dec.18: weight and data
//   gradient, dec.0: data gradient).
// Layout and conventions as train.h: NHWC fp32 activations, every reduction in a fixed order.
#pragma once
#include "common.h"

namespace dmx {

// ---------------------------------------------------------------------------
// Encoder tail of the training forward: vae_enc_tail_kernel (kernels.h, same arithmetic and launch
// geometry) that also records what the backward reads — heads[row][8] = mu (0-3) and the unclamped
// logvar (4-7) per latent pixel row = n HW + pix, and zin[row][4] = z / scale, the decoder's NHWC input.
// The KL terms and their sums are taken in double (klp[n][block], summed in block order by
// vae_train_kl_kernel), so that kl[n] is the fp32 rounding of the sum and not a neighbour of it: a
// per-sample scalar has no other samples to average a summation ulp over.
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void vae_train_heads_kernel(const float* in, const float* wmu, const float* bmu,
                                                                     const float* wlv, const float* blv, const float* eps,
                                                                     float* z, double* klp, int HW, float scale,
                                                                     int* range_flag, float* heads, float* zin) {
  __shared__ __attribute__((aligned(16))) float ws[8][256];  // rows 0-3: to_mu, 4-7: to_logvar ([out][in])
  __shared__ double red[4];
  for (int i = threadIdx.x; i < 8 * 256; i += 256) ws[i / 256][i % 256] = i < 1024 ? wmu[i] : wlv[i - 1024];
  __syncthreads();
  const int n = blockIdx.y, l8 = threadIdx.x & 7, pix = blockIdx.x * 32 + (threadIdx.x >> 3);
  float a[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) a[o] = 0.f;
  if (pix < HW) {
    const float* src = in + ((size_t)n * HW + pix) * 256 + 4 * l8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const floatx4 v = ld4(src + 32 * i);
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        const floatx4 w = *reinterpret_cast<const floatx4*>(&ws[o][32 * i + 4 * l8]);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[o] += v[j] * w[j];
      }
    }
  }
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    a[o] += __shfl_xor(a[o], 1, 64);
    a[o] += __shfl_xor(a[o], 2, 64);
    a[o] += __shfl_xor(a[o], 4, 64);
  }
  double kacc = 0.0;
  if (l8 == 0 && pix < HW) {
    const size_t row = (size_t)n * HW + pix;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const float mu0 = a[o] + bmu[o], lv0 = a[o + 4] + blv[o];
      flag_nonfinite(range_flag, mu0 + lv0);
      const float mu = mu0, lv = fminf(fmaxf(lv0, -30.f), 20.f);
      const size_t idx = ((size_t)n * 4 + o) * HW + pix;
      const float zz = (mu + eps[idx] * expf(0.5f * lv)) * scale;
      z[idx] = zz;
      zin[row * 4 + o] = zz / scale;
      heads[row * 8 + o] = mu0;
      heads[row * 8 + 4 + o] = lv0;
      kacc += ((exp((double)lv) + (double)mu * (double)mu) - 1.0) - (double)lv;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kacc += __shfl_xor(kacc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = kacc;
  __syncthreads();
  if (threadIdx.x == 0) klp[(size_t)n * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// kl[n] = 0.5 sum_b klp[n][b] / (h w): the block partials in block order, in double, rounded to fp32 once
static __global__ void vae_train_kl_kernel(const double* klp, int nb, int N, double px, float* kl) {
  for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
    double sacc = 0.0;
    for (int b = 0; b < nb; ++b) sacc += klp[(size_t)n * nb + b];
    kl[n] = (float)(0.5 * sacc / px);
  }
}

// Adjoint of the tail (models/vae.py:52-61).  With u = mu + eps std, z = u scale, zin = z / scale and
// kl_n = 0.5 sum(e^lv + mu^2 - 1 - lv) / (h w):  g = (d_z + dzin / scale) scale,
//   dmu = g + d_kl_n mu / (h w),   dlogvar = g eps std / 2 + d_kl_n (e^lv - 1) / (2 h w),
// dlogvar = 0 where the unclamped logvar lies outside [-30, 20] (torch's clamp gradient).
// dheads[row][8] = dmu (0-3) | dlogvar (4-7); d_z (NCHW) and d_kl (n) may be null (zero).
static __global__ void vae_heads_bwd_kernel(const float* heads, const float* eps, const float* d_z, const float* dzin,
                                            const float* d_kl, int N, int HW, float scale, float inv_px, float* dheads) {
  const size_t total = (size_t)N * HW * 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t row = i >> 2;
    const int o = (int)(i & 3), n = (int)(row / HW), pix = (int)(row - (size_t)n * HW);
    const size_t idx = ((size_t)n * 4 + o) * HW + pix;
    const float mu = heads[row * 8 + o], lv0 = heads[row * 8 + 4 + o];
    const float lv = fminf(fmaxf(lv0, -30.f), 20.f);
    const float g = ((d_z != nullptr ? d_z[idx] : 0.f) + dzin[i] / scale) * scale;
    const float dk = d_kl != nullptr ? d_kl[n] * inv_px : 0.f;
    const float sd = expf(0.5f * lv);
    float dlv = g * eps[idx] * 0.5f * sd + dk * 0.5f * (expf(lv) - 1.f);
    if (lv0 < -30.f || lv0 > 20.f) dlv = 0.f;
    dheads[row * 8 + o] = g + dk * mu;
    dheads[row * 8 + 4 + o] = dlv;
  }
}

// ---------------------------------------------------------------------------
// Sigmoid adjoint folded into the staging of the tail conv's dY: dpre[row][3] (NHWC, row = n HW + pix)
// = d_recon s (1 - s) from the NCHW cotangent and the taped NCHW sigmoid output.
// ---------------------------------------------------------------------------
static __global__ void vae_sigmoid_bwd_kernel(const float* d_recon, const float* s, int N, int HW, float* dpre) {
  const size_t total = (size_t)N * HW * 3;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t row = i / 3;
    const int co = (int)(i - row * 3), n = (int)(row / HW), pix = (int)(row - (size_t)n * HW);
    const size_t idx = ((size_t)n * 3 + co) * HW + pix;
    const float sv = s[idx];
    dpre[i] = d_recon[idx] * sv * (1.f - sv);
  }
}

// Data gradient of the tail conv3x3 64 -> 3 (dec.18, w [3][64][3][3]): da[n][y][x][c] =
// sum over taps, co of dpre[n][y - ty][x - tx][co] w[co][c][tap].  16 pixels x 16 channel quads per
// block (27 FMAs per output: VALU, exact fp32).
static __global__ __launch_bounds__(256) void vae_tail_dgrad_kernel(const float* dpre, const float* w, int N, int H,
                                                                    int W, float* da) {
  __shared__ __attribute__((aligned(16))) float ws[9 * 3 * 64];  // [tap][co][c]
  for (int i = threadIdx.x; i < 9 * 3 * 64; i += 256) {
    const int c = i & 63, co = (i >> 6) % 3, tap = i / 192;
    ws[i] = w[(co * 64 + c) * 9 + tap];
  }
  __syncthreads();
  const size_t M = (size_t)N * H * W, row = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (row >= M) return;
  const int c = (threadIdx.x & 15) * 4, HW = H * W;
  const int n = (int)(row / HW), rr = (int)(row - (size_t)n * HW), y = rr / W, x = rr - y * W;
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int tap = 0; tap < 9; ++tap) {
    const int sy = y - (tap / 3 - 1), sx = x - (tap % 3 - 1);
    if (sy < 0 || sx < 0 || sy >= H || sx >= W) continue;
    const float* d = dpre + (((size_t)n * H + sy) * W + sx) * 3;
#pragma unroll
    for (int co = 0; co < 3; ++co) {
      const float dv = d[co];
      const floatx4 wv = *reinterpret_cast<const floatx4*>(&ws[(tap * 3 + co) * 64 + c]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(dv, wv[j], acc[j]);
    }
  }
  *reinterpret_cast<floatx4*>(da + row * 64 + c) = acc;
}

// Weight gradient of the tail conv (dW[co][c][tap] = sum over pixels p of dpre[p - tap offset][co]
// a[p][c], 1728 outputs over N H W pixels): three output channels fill 3 / 64 of an MFMA tile, so it
// runs on the VALU.  Block b takes pixels [b ppb, (b + 1) ppb); thread -> (4 channels, pixel slot tid / 16);
// each a[p] float4 is loaded once and meets the 9 x 3 dpre values around p (108 accumulators); the 16
// pixel slots are added in slot order and the block's slab part[b][co][tap 64 + c] goes to
// wgrad_finish_kernel (slabs in a fixed order).
static __global__ __launch_bounds__(256) void vae_tail_wgrad_kernel(const float* dpre, const float* a, int N, int H,
                                                                    int W, int ppb, float* part) {
  __shared__ float red[16][64 + 1];
  const int tid = threadIdx.x, slot = tid >> 4, c = (tid & 15) * 4, HW = H * W;
  const size_t M = (size_t)N * HW, pbeg = (size_t)blockIdx.x * ppb, pend = min(M, pbeg + (size_t)ppb);
  float acc[9][3][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int co = 0; co < 3; ++co)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][co][j] = 0.f;
  for (size_t p = pbeg + slot; p < pend; p += 16) {
    const int n = (int)(p / HW), rr = (int)(p - (size_t)n * HW), y = rr / W, x = rr - y * W;
    const floatx4 av = ld4(a + p * 64 + c);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int oy = y - (t / 3 - 1), ox = x - (t % 3 - 1);  // the output pixel whose tap t reads p
      if (oy < 0 || ox < 0 || oy >= H || ox >= W) continue;
      const float* d = dpre + (((size_t)n * H + oy) * W + ox) * 3;
#pragma unroll
      for (int co = 0; co < 3; ++co) {
        const float dv = d[co];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][co][j] = fmaf(dv, av[j], acc[t][co][j]);
      }
    }
  }
  float* dst = part + (size_t)blockIdx.x * 3 * 576;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int co = 0; co < 3; ++co) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) red[slot][c + j] = acc[t][co][j];
      __syncthreads();
      if (tid < 64) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += red[k][tid];
        dst[co * 576 + t * 64 + tid] = s;
      }
    }
}

// Data gradient of the decoder's first conv3x3 4 -> 256 (dec.0, w [256][4][3][3]) into its NHWC input:
// dzin[row][c] = sum over taps, co of d0[n][y - ty][x - tx][co] w[co][c][tap].  One wave per latent
// pixel: lane l takes co 4 l .. 4 l + 3 (coalesced float4 rows of d0), then a fixed shuffle tree.
static __global__ __launch_bounds__(256) void vae_dec0_dgrad_kernel(const float* d0, const float* w, int N, int H, int W,
                                                                    float* dzin) {
  __shared__ __attribute__((aligned(16))) float ws[9 * 4 * 256];  // [tap][c][co]
  for (int i = threadIdx.x; i < 9 * 4 * 256; i += 256) {
    const int co = i & 255, c = (i >> 8) & 3, tap = i >> 10;
    ws[i] = w[(co * 4 + c) * 9 + tap];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const size_t M = (size_t)N * H * W, row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;  // (whole waves leave together: the shuffles below see all 64 lanes)
  const int HW = H * W, n = (int)(row / HW), rr = (int)(row - (size_t)n * HW), y = rr / W, x = rr - y * W;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int tap = 0; tap < 9; ++tap) {
    const int sy = y - (tap / 3 - 1), sx = x - (tap % 3 - 1);
    if (sy < 0 || sx < 0 || sy >= H || sx >= W) continue;
    const floatx4 dv = ld4(d0 + (((size_t)n * H + sy) * W + sx) * 256 + 4 * lane);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const floatx4 wv = *reinterpret_cast<const floatx4*>(&ws[(tap * 4 + c) * 256 + 4 * lane]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[c] = fmaf(dv[j], wv[j], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
  if (lane == 0) *reinterpret_cast<floatx4*>(dzin + row * 4) = floatx4{acc[0], acc[1], acc[2], acc[3]};
}

// ---------------------------------------------------------------------------
// GroupNorm(8, C) + GELU backward (every VAE stage, models/vae.py:17-48): a = GELU(GN8(r)) with the
// forward's (mean, rstd) per (sample, group) taped.  The sibling of gn_bwd_reduce_kernel /
// gn_bwd_apply_kernel (GroupNorm(1, C), whose instances keep their code path) with per-group sums:
// pass A (grid (chunks, N)): dy = dout GELU'(y); block partials of S1_g = sum(gamma dy), S2_g =
// sum(gamma dy xhat) per group and of dgamma = sum(dy xhat), dbeta = sum(dy) per channel;
// pass B (grid (achunks, N)): the partials in chunk order, then
//   dr = rstd_g (gamma dy - S1_g / cnt - xhat S2_g / cnt),  cnt = HW C / 8,
// and the per-block max |dr| for the x3 gradient GEMMs that read dr next (gn8_bwd's AbsMax).
// C / 4 divides 256 and C / 8 is a multiple of 4: a thread's float4 lies in one group.
// ---------------------------------------------------------------------------
struct Gn8BwdParams {
  const float* r;        // raw conv output [N][HW][C]
  const float2* stats;   // [N][8] (mean, rstd) of the forward (gn_finalize_kernel)
  const float* gamma; const float* beta;
  const float* dout;     // [N][HW][C]
  int C, HW;
  float* dr;             // [N][HW][C]
  float* chpart;         // [N][2][C]: per-sample dgamma, dbeta sums (pass B out)
  int chunks, ppb;       // pass A: blocks per sample, pixels per block
  double* bsum;          // [N][chunks][8][2] block partials of S1_g, S2_g
  float* bch;            // [N][chunks][2][C] block partials of dgamma, dbeta
  unsigned* amax_part;   // or null: per-block max |dr| ([N][gridDim.x], absmax_part_kernel's format)
};

static __global__ __launch_bounds__(256) void gn8_bwd_reduce_kernel(const Gn8BwdParams p) {
  __shared__ float tg[2][4][256];
  __shared__ float ts[2][256];
  __shared__ double qd[2][64];
  const int n = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  const int L4 = p.C / 4, c4 = tid % L4, p0 = tid / L4, pstep = 256 / L4, c = 4 * c4, cpg = p.C / 8;
  const float2 st = p.stats[n * 8 + c / cpg];
  const size_t base = (size_t)n * p.HW * p.C;
  const int pbeg = b * p.ppb, pend = min(p.HW, pbeg + p.ppb);
  const floatx4 g4 = *reinterpret_cast<const floatx4*>(p.gamma + c), bt4 = *reinterpret_cast<const floatx4*>(p.beta + c);
  float s1 = 0.f, s2 = 0.f;
  floatx4 g1 = {0.f, 0.f, 0.f, 0.f}, b1 = g1;
  for (int pix = pbeg + p0; pix < pend; pix += pstep) {
    const size_t idx = base + (size_t)pix * p.C + c;
    const floatx4 r4 = *reinterpret_cast<const floatx4*>(p.r + idx), d4 = *reinterpret_cast<const floatx4*>(p.dout + idx);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xh = (r4[j] - st.x) * st.y;
      const float dy = d4[j] * gelu_grad(xh * g4[j] + bt4[j]);
      const float gd = g4[j] * dy;
      s1 += gd;
      s2 += gd * xh;
      g1[j] += dy * xh;
      b1[j] += dy;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    tg[0][j][tid] = g1[j];
    tg[1][j][tid] = b1[j];
  }
  ts[0][tid] = s1;
  ts[1][tid] = s2;
  __syncthreads();
  const size_t blk = (size_t)n * p.chunks + b;
  // per-channel sums over the threads sharing a channel quad, in thread order (deterministic)
  for (int cc = tid; cc < p.C; cc += 256) {
    const int q = cc >> 2, j = cc & 3;
    float a0 = 0.f, a1 = 0.f;
    for (int t = q; t < 256; t += L4) {
      a0 += tg[0][j][t];
      a1 += tg[1][j][t];
    }
    float* o = p.bch + blk * 2 * p.C;
    o[cc] = a0;
    o[p.C + cc] = a1;
  }
  // per-group sums: the threads of a quad in thread order, then the quads of a group in order
  if (tid < L4) {
    double a0 = 0.0, a1 = 0.0;
    for (int t = tid; t < 256; t += L4) {
      a0 += (double)ts[0][t];
      a1 += (double)ts[1][t];
    }
    qd[0][tid] = a0;
    qd[1][tid] = a1;
  }
  __syncthreads();
  if (tid < 8) {
    const int qpg = L4 / 8;
    double a0 = 0.0, a1 = 0.0;
    for (int q = tid * qpg; q < (tid + 1) * qpg; ++q) {
      a0 += qd[0][q];
      a1 += qd[1][q];
    }
    p.bsum[(blk * 8 + tid) * 2] = a0;
    p.bsum[(blk * 8 + tid) * 2 + 1] = a1;
  }
}

static __global__ __launch_bounds__(256) void gn8_bwd_apply_kernel(const Gn8BwdParams p) {
  __shared__ float s12[8][2];
  __shared__ float wm[4];
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int gi = 0; gi < 2; ++gi) {  // wave wv: groups 2 wv, 2 wv + 1; lanes over the chunks, fixed shuffle tree
    const int g = 2 * wv + gi;
    double a = 0.0, b = 0.0;
    for (int k = lane; k < p.chunks; k += 64) {
      const size_t o = (((size_t)n * p.chunks + k) * 8 + g) * 2;
      a += p.bsum[o];
      b += p.bsum[o + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, 64);
      b += __shfl_xor(b, o, 64);
    }
    if (lane == 0) {
      s12[g][0] = (float)a;
      s12[g][1] = (float)b;
    }
  }
  if (blockIdx.x == 0) {
    for (int c = tid; c < p.C; c += 256) {
      float a0 = 0.f, a1 = 0.f;
      for (int k = 0; k < p.chunks; ++k) {
        const float* o = p.bch + ((size_t)n * p.chunks + k) * 2 * p.C;
        a0 += o[c];
        a1 += o[p.C + c];
      }
      p.chpart[((size_t)n * 2 + 0) * p.C + c] = a0;
      p.chpart[((size_t)n * 2 + 1) * p.C + c] = a1;
    }
  }
  __syncthreads();
  const int cpg = p.C / 8;
  const float cnt = (float)p.HW * (float)cpg;
  const size_t base = (size_t)n * p.HW * p.C;
  const int per = p.HW * p.C;
  float mx = 0.f;
  for (int i4 = blockIdx.x * 256 + tid; i4 < per / 4; i4 += gridDim.x * 256) {  // float4 along the rows
    const int c = (4 * i4) % p.C, g = c / cpg;
    const float2 st = p.stats[n * 8 + g];
    const float m1 = s12[g][0] / cnt, m2 = s12[g][1] / cnt;
    const size_t idx = base + 4 * (size_t)i4;
    const floatx4 r4 = *reinterpret_cast<const floatx4*>(p.r + idx), d4 = *reinterpret_cast<const floatx4*>(p.dout + idx);
    const floatx4 g4 = *reinterpret_cast<const floatx4*>(p.gamma + c), bt4 = *reinterpret_cast<const floatx4*>(p.beta + c);
    floatx4 o4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xh = (r4[j] - st.x) * st.y;
      const float dy = d4[j] * gelu_grad(xh * g4[j] + bt4[j]);
      o4[j] = st.y * (g4[j] * dy - m1 - xh * m2);
      mx = fmaxf(mx, fabsf(o4[j]));
    }
    *reinterpret_cast<floatx4*>(p.dr + idx) = o4;
  }
  if (p.amax_part != nullptr) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) wm[wv] = mx;
    __syncthreads();
    if (tid == 0)
      p.amax_part[(size_t)n * gridDim.x + blockIdx.x] = __float_as_uint(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3])));
  }
}

}  // namespace dmx
