// dmx — the training objective around the network (include/dmx.h dmx_train_noise, dmx_objective_loss,
// dmx_objective_seed): forward diffusion with its draws and the CFG dropout in front of the forward,
// the weighted loss behind it, and the loss's gradient that seeds dmx_train_backward.  Included by
// k_objective.hip only (launchers in launch.h): the code object of engine.hip gains no kernel.
#pragma once
#include "common.h"
#include "dmx.h"
#include "source.h"
#include "tail_math.h"

namespace dmx {

// ---------------------------------------------------------------------------
// Plain bandwidth-bound kernels.  The (B, C, h, w) tensors are walked in quads of four consecutive
// elements of one sample, Q = cdiv(chw, 4) per sample and one per thread; the <true> instantiations
// (chw a multiple of 4, every base pointer 16-byte aligned: objective_aligned16) move a quad with one
// 16-byte access, the others element by element with the last quad cut at chw.  No LDS beyond the
// block sums, no atomics.  Table reads clamp t to [1, T]: a bad timestep cannot reach past a table.
// ---------------------------------------------------------------------------
DMX_DEV int table_row(int64_t t, int T) { return (int)(t < 1 ? 1 : (t > T ? T : t)) - 1; }

DMX_DEV void st4g(float* p, floatx4 v) { *reinterpret_cast<floatx4*>(p) = v; }

// first word of the Philox block of (seed, stream, index): the per-sample draws
DMX_DEV uint32_t philox_word(uint64_t seed, uint64_t stream, uint64_t index) {
  return philox4x32(make_uint4((uint32_t)index, (uint32_t)(index >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)),
                    make_uint2((uint32_t)seed, (uint32_t)(seed >> 32))).x;
}
// t uniform on [1, T] by multiply-high: floor(word * T / 2^32) takes each value either floor(2^32 / T)
// or that plus one times, so a timestep's probability is off by at most T / 2^32 relative (2.3e-7 at
// T = 1000) — no rejection loop for that.
DMX_DEV int64_t draw_t(uint64_t seed, uint64_t row, int T) {
  return 1 + (int64_t)__umulhi(philox_word(seed, DMX_DRAW_T, row), (uint32_t)T);
}
// u = 24 bits * 2^-24 in [0, 1 - 2^-24], exact in fp32: u < 0 never, u < 1 always
DMX_DEV bool draw_drop(uint64_t seed, uint64_t row, float p) {
  return (float)(philox_word(seed, DMX_DRAW_DROP, row) >> 8) * 5.9604644775390625e-08f < p;
}

// z_noisy = sa[t] z + s1[t] noise (diff.py:18-30: torch.sqrt(ab) * x_0 + torch.sqrt(1 - ab) * noise):
// two products and a sum, one rounding each (rnd keeps the products out of an FMA), so given t and
// noise the bits are torch's.  Grid cdiv(B * Q, 256).  Every thread of a sample derives the same t_n
// and drop_n (each read, or drawn from the sample's global row, by its bit of a.draw); the thread of quad 0 stores them and the
// label, and the sample's threads share its gd value / mask columns (column j: quad j mod Q).
// target (null: not written): the v-prediction target sa[t] noise - s1[t] z of the same operands, two
// products and a difference with one rounding each — one more store per quad.
template <bool VEC>
static __global__ __launch_bounds__(256) void train_noise_kernel(const dmx_noise_args a, float* target, int64_t chw,
                                                                 int64_t Q, int64_t total) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int64_t n = id / Q, q = id - n * Q;
  const uint64_t row = (uint64_t)(a.sample_offset + n);
  const bool draws_t = a.draw & DMX_DRAWS_T, draws_nz = a.draw & DMX_DRAWS_NOISE, draws_drop = a.draw & DMX_DRAWS_DROP;
  const int64_t t = draws_t ? draw_t(a.seed, row, a.T) : a.t[n];
  const bool drop = draws_drop ? draw_drop(a.seed, row, a.cfg_drop_prob) : (a.drop != nullptr && a.drop[n] != 0);
  if (q == 0) {
    if (draws_t) a.t[n] = t;
    if (draws_drop) a.drop[n] = drop ? 1 : 0;
    if (a.y != nullptr) a.y_used[n] = drop ? a.null_label : a.y[n];
  }
  if (a.vals != nullptr) {
    for (int64_t j = q; j < a.gd; j += Q) {
      const int64_t k = n * a.gd + j;
      a.vals_used[k] = drop ? 0.f : a.vals[k];
      a.mask_used[k] = drop ? 0.f : a.mask[k];
    }
  }
  const int r = table_row(t, a.T);
  const float ca = a.sa[r], cb = a.s1[r];
  const int64_t base = n * chw + 4 * q;
  floatx4 nz = {0.f, 0.f, 0.f, 0.f};
  if (draws_nz) nz = normal4(a.seed, DMX_DRAW_NOISE, row * (uint64_t)Q + (uint64_t)q);
  if (VEC) {
    const floatx4 z = ld4(a.z + base);
    if (!draws_nz) nz = ld4(a.noise + base);
    floatx4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = rnd(ca * z[k]) + rnd(cb * nz[k]);
    st4g(a.z_noisy + base, o);
    if (draws_nz) st4g(a.noise + base, nz);
    if (target != nullptr) {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = rnd(ca * nz[k]) - rnd(cb * z[k]);
      st4g(target + base, o);
    }
  } else {
    const int64_t left = chw - 4 * q;
    const int cnt = left < 4 ? (int)left : 4;
    for (int k = 0; k < cnt; ++k) {
      const float e = draws_nz ? nz[k] : a.noise[base + k];
      const float zk = a.z[base + k];
      a.z_noisy[base + k] = rnd(ca * zk) + rnd(cb * e);
      if (draws_nz) a.noise[base + k] = e;
      if (target != nullptr) target[base + k] = rnd(ca * e) - rnd(cb * zk);
    }
  }
}

// One block per sample: part[n] = (sum_i (eps - noise)^2, sum_j m (g - v)^2, sum_j m).  Difference,
// square and mask product in fp32 (one rounding each), accumulated in double: thread k takes quads
// (elements) k, k + 256, .. in ascending order and the threads' sums meet in block_sum2's fixed tree.
template <bool VEC>
static __global__ __launch_bounds__(256) void objective_loss_kernel(const dmx_objective_args a, int64_t chw) {
  __shared__ double sh[512];
  const int64_t n = blockIdx.x;
  const float* e = a.eps + n * chw;
  const float* z = a.noise + n * chw;
  double s = 0.0;
  if (VEC) {
    for (int64_t q = threadIdx.x; q < chw / 4; q += 256) {
      const floatx4 x = ld4(e + 4 * q), y = ld4(z + 4 * q);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = x[k] - y[k];
        s += (double)rnd(d * d);
      }
    }
  } else {
    for (int64_t i = threadIdx.x; i < chw; i += 256) {
      const float d = e[i] - z[i];
      s += (double)rnd(d * d);
    }
  }
  double num = 0.0, ms = 0.0, none = 0.0;
  if (a.geom != nullptr) {
    for (int j = threadIdx.x; j < a.gd; j += 256) {
      const int64_t k = n * a.gd + j;
      const float d = a.geom[k] - a.vals[k], m = a.mask[k];
      num += (double)rnd(m * rnd(d * d));
      ms += (double)m;
    }
  }
  block_sum2(s, num, sh);
  block_sum2(ms, none, sh);
  if (threadIdx.x == 0) {
    a.part[3 * n] = s;
    a.part[3 * n + 1] = num;
    a.part[3 * n + 2] = ms;
  }
}

// One block: per_sample and the three scalars.  The B partials are staged 256 at a time and added by
// thread 0 in index order, in double; each output is rounded to fp32 once.  A NaN denominator stays
// NaN (torch's clamp_min).
static __global__ __launch_bounds__(256) void objective_finish_kernel(const dmx_objective_args a, int64_t chw) {
  __shared__ double sh[3][256];
  double sn = 0.0, sg = 0.0, sm = 0.0;
  for (int64_t b0 = 0; b0 < a.B; b0 += 256) {
    const int64_t n = b0 + threadIdx.x;
    __syncthreads();
    if (n < a.B) {
      const double w = a.weight != nullptr ? (double)a.weight[table_row(a.t[n], a.T)] : 1.0;
      const double ps = w * (a.part[3 * n] / (double)chw);
      a.per_sample[n] = (float)ps;
      sh[0][threadIdx.x] = ps;
      sh[1][threadIdx.x] = a.part[3 * n + 1];
      sh[2][threadIdx.x] = a.part[3 * n + 2];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int cnt = a.B - b0 < 256 ? (int)(a.B - b0) : 256;
      for (int i = 0; i < cnt; ++i) {
        sn += sh[0][i];
        sg += sh[1][i];
        sm += sh[2][i];
      }
    }
  }
  if (threadIdx.x == 0) {
    const double nl = sn / (double)a.B;
    double dn = a.denom != nullptr ? (double)*a.denom : sm;
    dn = dn < 1e-6 ? 1e-6 : dn;
    const double gl = a.geom != nullptr ? sg / dn : 0.0;
    a.out[0] = (float)(nl + (double)a.geom_lambda * gl);
    a.out[1] = (float)nl;
    a.out[2] = (float)gl;
    a.out[3] = (float)dn;
  }
}

// The loss's gradient, scaled by the upstream scalar read from the device: grid cdiv(B * Q, 256),
// quads and geometry columns shared out as in train_noise_kernel.  Each coefficient is formed in
// double and rounded once, then difference and product in fp32: three roundings per element (the
// mask product is a fourth where the mask is not 0 / 1).  A power-of-two *up scales every output
// exactly.
template <bool VEC>
static __global__ __launch_bounds__(256) void objective_seed_kernel(const dmx_objective_args a, const float* up,
                                                                    float* d_eps, float* d_geom, int64_t chw,
                                                                    int64_t Q, int64_t total) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int64_t n = id / Q, q = id - n * Q;
  const double u = (double)*up;
  const double w = a.weight != nullptr ? (double)a.weight[table_row(a.t[n], a.T)] : 1.0;
  const float ce = (float)(u * 2.0 * w / ((double)a.B * (double)chw));
  const int64_t base = n * chw + 4 * q;
  if (VEC) {
    const floatx4 x = ld4(a.eps + base), y = ld4(a.noise + base);
    floatx4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = ce * (x[k] - y[k]);
    st4g(d_eps + base, o);
  } else {
    const int64_t left = chw - 4 * q;
    const int cnt = left < 4 ? (int)left : 4;
    for (int k = 0; k < cnt; ++k) d_eps[base + k] = ce * (a.eps[base + k] - a.noise[base + k]);
  }
  if (d_geom != nullptr) {
    const float cg = (float)(u * (double)a.geom_lambda * 2.0 / (double)a.out[3]);
    for (int64_t j = q; j < a.gd; j += Q) {
      const int64_t k = n * a.gd + j;
      d_geom[k] = cg * (a.mask[k] * (a.geom[k] - a.vals[k]));
    }
  }
}

}  // namespace dmx
