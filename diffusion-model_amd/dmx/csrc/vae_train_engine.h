// dmx — training step of the VAE (train_vae.py: `_, _, loss, _ = vae(x); loss.backward()` over
// models/vae.py:51-76; the loss expression and Adam stay in torch).
//
// Forward = vae_enc_body + vae_body (engine.hip) in the training forward's arithmetic (x3 split GEMMs
// with device-split weight planes whatever the model's precision, exact-fp32 GEMMs for the two convs
// with 4 input channels, erf GELU), every stage's raw conv output, GroupNorm(8) statistics and
// activation kept in the tape, plus the raw mu / logvar, the decoder's NHWC input and the sigmoid output.
// Backward (vae_train.h + train.h kernels): sigmoid adjoint -> tail conv -> per stage GroupNorm(8) + GELU
// adjoint, weight gradient (wgrad, the 16-tap stride-2 gather for Conv2d / ConvTranspose2d 4x4 s2) and
// data gradient (conv3x3: flipped conv; Conv2d s2: the 4-phase ConvT GEMM; ConvT: the conv4x4-s2 GEMM —
// both read the forward weight tensor as it lies, the channel roles swap by reinterpretation) -> heads /
// reparameterisation / clamp / KL adjoint -> encoder stages.  No gradient for x.
// The pass's state is train_engine.h's: one Bwd per pass, and each stage's dY scale as the AbsMax that
// gn8_bwd returns, handed to the stage's wgrad and dgrad.
//
// Included by engine.hip after train_engine.h (same translation unit).
#pragma once

namespace dmx {

struct VStage {  // one conv -> GN(8) -> GELU stage
  const float* in = nullptr;  // NHWC input [N][H][W][cin]
  float* r = nullptr;         // raw conv output [N][Ho][Wo][cout]
  float2* st = nullptr;       // [N][8] (mean, rstd)
  float* a = nullptr;         // GELU(GN(r))
  int H = 0, W = 0, Ho = 0, Wo = 0, cin = 0, cout = 0;
};

struct VaeTape {
  int64_t id = 0;
  int n = 0, h = 0, w = 0;
  float *xin = nullptr, *eps = nullptr, *heads = nullptr, *zin = nullptr, *recon = nullptr;
  VStage enc[6], dec[6];
};

static const int kVaeEncCin[6] = {3, 64, 64, 128, 128, 256}, kVaeEncCout[6] = {64, 64, 128, 128, 256, 256};
static const int kVaeDecCin[6] = {4, 256, 256, 128, 128, 64}, kVaeDecCout[6] = {256, 256, 128, 128, 64, 64};

// Conv2d 4x4 s2 p1 [cout][cin][4][4] -> its data gradient, a ConvTranspose2d 4x4 s2 p1 of dY: the same
// tensor read as a ConvT weight [in = cout][out = cin][4][4] (RepackJob kind 2, the 4-phase layout)
static ConvW pack_dgrad_conv4s2(Packer& P, const std::string& wname, int cin, int cout) {
  ConvW c;
  c.cin = cout;
  c.cout = cin;
  c.taps = 4;
  c.phases = 4;
  c.kpad = rup(4 * cout, 64);
  c.npad = rup(cin, 128);
  c.B = P.alloc((size_t)4 * c.npad * c.kpad);
  P.repack(c.B, P.in(wname).first, 2, 4, c.npad, c.kpad, cin, cout, 4);
  P.split_dev(c);
  return c;
}

// ConvTranspose2d 4x4 s2 p1 [cin][cout][4][4] -> its data gradient, a Conv2d 4x4 s2 p1 over dY: the same
// tensor read as a conv weight [out = cin][in = cout][4][4] (RepackJob kind 0)
static ConvW pack_dgrad_convt(Packer& P, const std::string& wname, int cin, int cout) {
  ConvW c;
  c.cin = cout;
  c.cout = cin;
  c.taps = 16;
  c.kpad = rup(16 * cout, 64);
  c.npad = rup(cin, 128);
  c.B = P.alloc((size_t)c.npad * c.kpad);
  P.repack(c.B, P.in(wname).first, 0, 1, c.npad, c.kpad, cin, cout, 4);
  P.split_dev(c);
  return c;
}

// fwd_x3_weight for the VAE's layers: the ConvT's four phase matrices are split under one scale
static ConvW vae_x3_weight(Packer& P, const ConvW& c) {
  ConvW t = c;
  t.Bh = t.Bl = t.Fh = t.Fl = t.Uh = t.Ul = nullptr;
  t.inv_dev = nullptr;
  t.amax_dev = nullptr;
  if (c.cin >= 64) P.split_dev(t);
  return t;
}

static void ensure_vae_train(dmx_model* m, hipStream_t st) {
  if (m->train_ready) return;
  Packer P{m, st};
  for (int i = 0; i < 6; ++i) {
    const std::string w = "enc." + std::to_string(3 * i) + ".weight";
    m->venc_t[i] = vae_x3_weight(P, m->venc[i]);
    if (i == 0) continue;  // the image takes no gradient
    m->venc_d[i] = (i & 1) ? pack_dgrad_conv4s2(P, w, kVaeEncCin[i], kVaeEncCout[i])
                           : pack_dgrad_conv(P, w, kVaeEncCin[i], kVaeEncCout[i]);
  }
  for (int s = 0; s < 6; ++s) {
    const std::string w = "dec." + std::to_string(3 * s) + ".weight";
    m->vdec_t[s] = vae_x3_weight(P, (s & 1) ? m->vconvt[s / 2] : m->vconv[s / 2]);
    if (s == 0) continue;  // dec.0's data gradient (4 channels): vae_dec0_dgrad_kernel
    m->vdec_d[s] = (s & 1) ? pack_dgrad_convt(P, w, kVaeDecCin[s], kVaeDecCout[s])
                           : pack_dgrad_conv(P, w, kVaeDecCin[s], kVaeDecCout[s]);
  }
  run_split_jobs(m, st);
  HIPCHK(hipStreamSynchronize(st));
  m->train_ready = true;
}

// ---------------------------------------------------------------------------
// training forward
// ---------------------------------------------------------------------------
// conv (3x3 | 4x4 s2 | ConvT 4x4 s2) + row statistics -> GN(8) finalize -> GN + GELU materialised.
// H x W: the input map; kind 0 conv3x3, 1 conv4x4 s2 (rows = output pixels), 2 ConvT (rows = input pixels)
static VStage vae_train_stage(Run& R, const ConvW& cw, const Vec& g, const Vec& b, const float* in, int n, int H,
                              int W, int kind) {
  VStage t;
  t.in = in;
  t.H = H;
  t.W = W;
  t.Ho = kind == 1 ? H / 2 : kind == 2 ? 2 * H : H;
  t.Wo = kind == 1 ? W / 2 : kind == 2 ? 2 * W : W;
  t.cin = cw.cin;
  t.cout = cw.cout;
  const int G = 8, Mo = n * t.Ho * t.Wo, seg = std::min(32, cw.cout / G);
  t.r = R.ws.get<float>((size_t)Mo * cw.cout);
  float2* rp = R.ws.get<float2>((size_t)Mo * (cw.cout / seg));
  t.st = R.ws.get<float2>((size_t)n * G);
  t.a = R.ws.get<float>((size_t)Mo * cw.cout);
  const int gh = kind == 1 ? t.Ho : H, gw = kind == 1 ? t.Wo : W;  // the GEMM's row grid
  const int rr = gemm(R, plain_src(in, cw.cin), SRC_PLAIN, n, gh, gw, cw, EPI_STATS, t.r, nullptr, rp, seg);
  gn_finalize(R, rp, t.st, n, rr, cw.cout / seg, G, cw.cout, t.Ho * t.Wo);
  NormParams np = norm_params(t.r, nullptr, 0, 0, g.p, b.p, cw.cout, t.Ho * t.Wo, t.a);
  np.stats = t.st;
  np.G = G;
  np.act = 1;
  norm(R, np, n);
  return t;
}

static void vae_train_fwd_body(Run& R, VaeTape& T, const float* x, const float* eps, float* x_recon, float* z,
                               float* kl, int n, int h, int w) {
  dmx_model* m = R.m;
  T.n = n;
  T.h = h;
  T.w = w;
  const int hl = h / 8, wl = w / 8, HWl = hl * wl;
  T.xin = R.ws.get<float>((size_t)n * h * w * 4);
  T.eps = R.ws.get<float>((size_t)n * 4 * HWl);
  T.heads = R.ws.get<float>((size_t)n * HWl * 8);
  T.zin = R.ws.get<float>((size_t)n * HWl * 4);
  T.recon = R.ws.get<float>((size_t)n * 3 * h * w);
  if (!R.plan) {
    R.layer = "vae.train.in";
    nchw_to_nhwc_kernel<<<ew_blocks((size_t)n * h * w * 4), 256, 0, R.st>>>(x, T.xin, n, 3, 4, h * w);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(T.eps, eps, (size_t)n * 4 * HWl * sizeof(float), hipMemcpyDeviceToDevice, R.st));
  }
  const float* cur = T.xin;
  int H = h, W = w;
  for (int i = 0; i < 6; ++i) {
    R.layer = "vae.train.enc" + std::to_string(i);
    T.enc[i] = vae_train_stage(R, m->venc_t[i], m->veg[i], m->veb[i], cur, n, H, W, (i & 1) ? 1 : 0);
    cur = T.enc[i].a;
    H = T.enc[i].Ho;
    W = T.enc[i].Wo;
  }
  const int nb = cdiv(HWl, 32);
  double* klp = R.ws.get<double>((size_t)n * nb);
  if (!R.plan) {
    R.layer = "vae.train.heads";
    R.begin("vae_train_heads_kernel", 2.0 * n * HWl * 8 * 256, 4.0 * (double)n * HWl * (256 + 4 + 4 + 12));
    vae_train_heads_kernel<<<dim3(nb, n), 256, 0, R.st>>>(cur, m->wmu, m->bmu, m->wlv, m->blv, T.eps, z, klp, HWl,
                                                           m->cfg.scale, m->range_flag, T.heads, T.zin);
    vae_train_kl_kernel<<<cdiv(n, 64), 64, 0, R.st>>>(klp, nb, n, (double)h * (double)w, kl);
    R.end();
    HIPCHK(hipGetLastError());
  }
  cur = T.zin;
  for (int s = 0; s < 6; ++s) {
    R.layer = "vae.train.dec" + std::to_string(s);
    T.dec[s] = vae_train_stage(R, m->vdec_t[s], m->vg[s], m->vb[s], cur, n, H, W, (s & 1) ? 2 : 0);
    cur = T.dec[s].a;
    H = T.dec[s].Ho;
    W = T.dec[s].Wo;
  }
  if (R.plan) return;
  R.layer = "vae.train.tail";
  R.begin("vae_tail_kernel", 2.0 * n * H * W * 3 * 576, 4.0 * (double)n * H * W * (64 + 3));
  vae_tail_kernel<<<dim3(cdiv(H * W, 256), n), 256, 0, R.st>>>(cur, m->vconv[3].B, m->vconv[3].bias, n, H, W, x_recon,
                                                               nullptr, m->range_flag);
  R.end();
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(T.recon, x_recon, (size_t)n * 3 * h * w * sizeof(float), hipMemcpyDeviceToDevice, R.st));
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// GroupNorm(8) + GELU adjoint (vae_train.h): dout -> dr, dgamma / dbeta through colsum_pair; want_absmax and the
// returned scale of dr as gn_bwd
static AbsMax gn8_bwd(Run& R, Bwd& B, const VStage& t, const Vec& g, const Vec& b, const float* dout, int N, float* dr,
                      float* ggamma, float* gbeta, bool want_absmax) {
  const int C = t.cout, HW = t.Ho * t.Wo;
  if (C % 32 != 0 || C / 4 > 64 || 256 % (C / 4) != 0) throw Error(DMX_E_INTERNAL, "gn8_bwd: C must be 64, 128 or 256");
  const int chunks = std::max(1, std::min(cdiv(512, N), cdiv(HW, 16)));
  const int ppb = cdiv(HW, chunks);
  float* chpart = R.ws.get<float>((size_t)N * 2 * C);
  double* bsum = R.ws.get<double>((size_t)N * chunks * 16);
  float* bch = R.ws.get<float>((size_t)N * chunks * 2 * C);
  const int achunks = gn_bwd_achunks(HW, C);
  unsigned* amax = want_absmax ? R.ws.get<unsigned>((size_t)N * achunks) : nullptr;
  if (!R.plan) {
    Gn8BwdParams p;
    std::memset(&p, 0, sizeof(p));
    p.r = t.r;
    p.stats = t.st;
    p.gamma = g.p;
    p.beta = b.p;
    p.dout = dout;
    p.C = C;
    p.HW = HW;
    p.dr = dr;
    p.chpart = chpart;
    p.chunks = cdiv(HW, ppb);
    p.ppb = ppb;
    p.bsum = bsum;
    p.bch = bch;
    p.amax_part = amax;
    R.begin("gn8_bwd_reduce_kernel", 0.0, 4.0 * (double)N * HW * C * 2);
    gn8_bwd_reduce_kernel<<<dim3(p.chunks, N), 256, 0, R.st>>>(p);
    R.end();
    HIPCHK(hipGetLastError());
    R.begin("gn8_bwd_apply_kernel", 0.0, 4.0 * (double)N * HW * C * 3);
    gn8_bwd_apply_kernel<<<dim3(achunks, N), 256, 0, R.st>>>(p);
    R.end();
    HIPCHK(hipGetLastError());
  }
  colsum_pair(R, B, chpart, N, C, 2 * (size_t)C, ggamma, gbeta);
  return want_absmax ? AbsMax{amax, N * achunks} : AbsMax{};
}

// One stage backward: dout (gradient of the stage's activation) -> parameter gradients of the conv
// (`p`.weight / .bias) and its GroupNorm (`pn`), and the gradient of the stage's input (returned; null
// when dw == nullptr: the caller computes it, or the input takes none).
// kind 0 conv3x3, 1 conv4x4 s2, 2 ConvT 4x4 s2; cin_real: channels of the reference's weight tensor.
static float* vae_stage_bwd(Run& R, Bwd& B, const VStage& t, const std::string& p, const std::string& pn,
                            const Vec& g, const Vec& b, const ConvW* dw, int kind, int cin_real, const float* dout,
                            int N, float** dr_out = nullptr) {
  const int C = t.cout, Mo = N * t.Ho * t.Wo;
  float* dr = R.ws.get<float>((size_t)Mo * C);
  if (dr_out != nullptr) *dr_out = dr;
  // dr's scale: read by the x3 weight gradient and by the data gradient
  const bool fast = kind == 2 ? wgrad_fast(C, t.cin) : wgrad_fast(t.cin, C);
  const AbsMax s = gn8_bwd(R, B, t, g, b, dout, N, dr, B.grad(pn + ".weight"), B.grad(pn + ".bias"), fast || dw != nullptr);
  if (kind == 2) {
    // rows = the input map's pixels, "dY" operand = the layer input, gathered operand = dY (2H x 2W)
    wgrad(R, B, t.in, dr, N, t.H, t.W, C, t.cin, 16, C, B.grad(p + ".weight"), nullptr, s, 2);
  } else {
    wgrad(R, B, dr, t.in, N, t.Ho, t.Wo, t.cin, C, kind == 1 ? 16 : 9, cin_real, B.grad(p + ".weight"),
          B.grad(p + ".bias"), s, kind);
  }
  float* dx = nullptr;
  if (dw != nullptr) {
    dx = R.ws.get<float>((size_t)N * t.H * t.W * t.cin);
    // conv3x3: flipped conv on dY's grid; conv s2: 4-phase ConvT GEMM, rows = dY's pixels; ConvT: conv4x4-s2
    // GEMM, rows = the input map's pixels (dY on the 2H x 2W map)
    if (kind == 2) dgrad(R, dr, C, N, t.H, t.W, *dw, dx, false, s);
    else dgrad(R, dr, C, N, t.Ho, t.Wo, *dw, dx, false, s);
  }
  if (kind == 2) bias_grad(R, B, dr, Mo, C, B.grad(p + ".bias"));
  return dx;
}

static void vae_train_bwd_body(Run& R, VaeTape& T, const GradMap& G, const float* d_recon, const float* d_z,
                               const float* d_kl) {
  dmx_model* m = R.m;
  Bwd B{G, false, !R.plan};
  const int N = T.n, H = T.h, W = T.w, HW = H * W, M = N * HW;
  const int hl = H / 8, wl = W / 8, HWl = hl * wl, Ml = N * HWl;
  // tail: sigmoid adjoint folded into the staging of dec.18's dY, its weight / bias and data gradients
  R.layer = "vae.train.tail.bwd";
  float* dpre = R.ws.get<float>((size_t)M * 3);
  float* dcur = R.ws.get<float>((size_t)M * 64);
  if (!R.plan) {
    if (d_recon != nullptr) {
      vae_sigmoid_bwd_kernel<<<ew_blocks((size_t)M * 3), 256, 0, R.st>>>(d_recon, T.recon, N, HW, dpre);
      HIPCHK(hipGetLastError());
    } else {
      HIPCHK(hipMemsetAsync(dpre, 0, (size_t)M * 3 * sizeof(float), R.st));
    }
  }
  {  // dec.18's weight gradient on the VALU (3 output channels), slabs summed by wgrad_finish_kernel
    const int ppb = cdiv(M, std::min(1024, cdiv(M, 16))), nb = cdiv(M, ppb);
    float* part = R.ws.get<float>((size_t)nb * 3 * 576);
    if (!R.plan) {
      R.begin("vae_tail_wgrad_kernel", 2.0 * M * 3.0 * 576.0, 4.0 * ((double)M * (64 + 3) + (double)nb * 1728));
      vae_tail_wgrad_kernel<<<nb, 256, 0, R.st>>>(dpre, T.dec[5].a, N, H, W, ppb, part);
      R.end();
      HIPCHK(hipGetLastError());
      wgrad_finish_kernel<<<cdiv(3 * 576, 64), 256, 0, R.st>>>(part, nb, 3, 64, 64, 9, B.grad("dec.18.weight"));
      HIPCHK(hipGetLastError());
    }
    bias_grad(R, B, dpre, M, 3, B.grad("dec.18.bias"));
  }
  if (!R.plan) {
    R.begin("vae_tail_dgrad_kernel", 2.0 * M * 64.0 * 27.0, 4.0 * (double)M * (64 + 3));
    vae_tail_dgrad_kernel<<<(unsigned)cdiv(M, 16), 256, 0, R.st>>>(dpre, srcp(m, "dec.18.weight"), N, H, W, dcur);
    R.end();
    HIPCHK(hipGetLastError());
  }
  float* d0 = nullptr;
  for (int s = 5; s >= 0; --s) {
    R.layer = "vae.train.dec" + std::to_string(s) + ".bwd";
    const std::string p = "dec." + std::to_string(3 * s), pn = "dec." + std::to_string(3 * s + 1);
    dcur = vae_stage_bwd(R, B, T.dec[s], p, pn, m->vg[s], m->vb[s], s > 0 ? &m->vdec_d[s] : nullptr, (s & 1) ? 2 : 0,
                         kVaeDecCin[s], dcur, N, &d0);
  }
  // dec.0's data gradient into the decoder input, then the heads / reparameterisation / KL adjoint
  R.layer = "vae.train.heads.bwd";
  float* dzin = R.ws.get<float>((size_t)Ml * 4);
  float* dheads = R.ws.get<float>((size_t)Ml * 8);
  float* dact = R.ws.get<float>((size_t)Ml * 256);
  if (!R.plan) {
    R.begin("vae_dec0_dgrad_kernel", 2.0 * Ml * 256.0 * 36.0, 4.0 * (double)Ml * (256 + 4));
    vae_dec0_dgrad_kernel<<<(unsigned)cdiv(Ml, 4), 256, 0, R.st>>>(d0, srcp(m, "dec.0.weight"), N, hl, wl, dzin);
    R.end();
    vae_heads_bwd_kernel<<<ew_blocks((size_t)Ml * 4), 256, 0, R.st>>>(T.heads, T.eps, d_z, dzin, d_kl, N, HWl,
                                                                      m->cfg.scale, 1.0f / ((float)H * (float)W), dheads);
    HIPCHK(hipGetLastError());
  }
  const float* act = T.enc[5].a;
  dense_dw(R, B, dheads, 8, act, 256, Ml, 4, 256, B.grad("to_mu.weight"), nullptr);
  dense_dw(R, B, dheads + 4, 8, act, 256, Ml, 4, 256, B.grad("to_logvar.weight"), nullptr);
  colsum_pair(R, B, dheads, Ml, 4, 8, B.grad("to_mu.bias"), B.grad("to_logvar.bias"));
  dense_dx(R, dheads, 8, srcp(m, "to_mu.weight"), Ml, 4, 256, dact, 256, false);
  dense_dx(R, dheads + 4, 8, srcp(m, "to_logvar.weight"), Ml, 4, 256, dact, 256, true);
  dcur = dact;
  for (int i = 5; i >= 0; --i) {
    R.layer = "vae.train.enc" + std::to_string(i) + ".bwd";
    const std::string p = "enc." + std::to_string(3 * i), pn = "enc." + std::to_string(3 * i + 1);
    dcur = vae_stage_bwd(R, B, T.enc[i], p, pn, m->veg[i], m->veb[i], i > 0 ? &m->venc_d[i] : nullptr, (i & 1) ? 1 : 0,
                         kVaeEncCin[i], dcur, N);
  }
  if (!R.plan) colsum_flush(R, B);
}

}  // namespace dmx
