// dmx — sampling on the host side: one denoising step (U-Net trunk + the tail's update, in every
// mode of step_mode.h), its argument rules, the eager / hipGraph sample loop, and the launches of
// the standalone updates and the known-region blend.  The C ABI entries in engine.hip fill a
// StepMode and call sample_step / sample_loop.
//
// Included by engine.hip after the inference engine (same translation unit).
#pragma once

namespace dmx {

// The blend's launch (kernels.h known_blend_kernel): float4 lanes where the rows and every pointer allow.
static void launch_known_blend(const float* x, float* x_out, const int64_t* pos, int pos_stride,
                               const dmx_known_sched& kn, int n, int c, int hw, hipStream_t st) {
  KnownBlendParams p;
  std::memset(&p, 0, sizeof(p));
  p.x = x;
  p.x_out = x_out;
  p.z0 = kn.z0;
  p.e0 = kn.e0;
  p.mask = kn.mask;
  p.q_a = kn.q_a;
  p.q_e = kn.q_e;
  p.pos = pos;
  p.pos_stride = pos_stride;
  p.S = kn.S;
  p.HW = hw;
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)x_out | (uintptr_t)kn.z0 | (uintptr_t)kn.e0 | (uintptr_t)kn.mask;
  if (hw % 4 == 0 && bits % 16 == 0)
    known_blend_kernel<true><<<dim3(cdiv(hw / 4, 256), c, n), 256, 0, st>>>(p);
  else
    known_blend_kernel<false><<<dim3(cdiv(hw, 256), c, n), 256, 0, st>>>(p);
}

// The strided form of the tail: positions in [1, S], one table row per position.
static void set_sched(StepTailParams& p, const dmx_ddim_sched& sc) {
  p.tmax = sc.S;
  p.t_map = sc.t_map;
  p.k_e = sc.k_e;
  p.k_a = sc.k_a;
  p.k_s = sc.k_s;
  p.k_d = sc.k_d;
  p.k_n = sc.k_n;
}

// The DPM-Solver++(2M) form: positions as above, its own three tables and the history buffer.
static void set_sched(StepTailParams& p, const dmx_dpm_sched& dp) {
  p.tmax = dp.S;
  p.t_map = dp.t_map;
  p.k_e = dp.k_e;
  p.k_a = dp.k_a;
  p.k_x = dp.k_x;
  p.k_c = dp.k_c;
  p.k_p = dp.k_p;
  p.hist = dp.hist;
}

// The inversion form: countdown positions over the S rows; the tail reads the position's source latent
// where the other rules read x (kernels.h), and stores into the same buffer on adv rows.
static void set_sched(StepTailParams& p, const dmx_invert_sched& iv) {
  p.tmax = iv.S;
  p.t_map = iv.t_map;
  p.i_x = iv.i_x;
  p.i_e = iv.i_e;
  p.adv = iv.adv;
  p.src = iv.src;
}

// The tail's launch: the instance of the update rule; head4 = the network head path with Co = 4
// (16 pixels per block), else one pixel per thread; comp: the composed head4 tail (launch.h).
// p.p_o given (a v-model): the PRED_V instances of the same kernels; p.d_s too (its x0-form): the PRED_X0
// instances, except in inversion, which has no x0 and no division and runs PRED_V.
static void launch_step_tail(const StepTailParams& p, Rule rule, bool head4, dim3 grid, hipStream_t st,
                             const ComposeParams* comp = nullptr) {
  if (comp != nullptr) {
    if (!head4) throw Error(DMX_E_INTERNAL, "the composed tail is the Co = 4 head tail");
    if (rule == Rule::INVERT) throw Error(DMX_E_INTERNAL, "there is no composed inversion tail");
    launch_compose_tail4(p, *comp, rule == Rule::DDIM, rule == Rule::DPM, grid, st);
  } else if (p.p_o != nullptr && p.d_s != nullptr && rule != Rule::INVERT) {  // a v-model in x0-form
    if (!head4) {
      if (rule == Rule::DPM) step_tail_kernel<false, true, false, PRED_X0><<<grid, 256, 0, st>>>(p);
      else if (rule == Rule::DDIM) step_tail_kernel<true, false, false, PRED_X0><<<grid, 256, 0, st>>>(p);
      else step_tail_kernel<false, false, false, PRED_X0><<<grid, 256, 0, st>>>(p);
    } else {
      if (rule == Rule::DPM) step_tail4_kernel<false, true, false, PRED_X0><<<grid, 256, 0, st>>>(p);
      else if (rule == Rule::DDIM) step_tail4_kernel<true, false, false, PRED_X0><<<grid, 256, 0, st>>>(p);
      else step_tail4_kernel<false, false, false, PRED_X0><<<grid, 256, 0, st>>>(p);
    }
  } else if (p.p_o != nullptr) {  // a v-model: the converting instances
    if (!head4) {
      if (rule == Rule::INVERT) step_tail_kernel<false, false, true, PRED_V><<<grid, 256, 0, st>>>(p);
      else if (rule == Rule::DPM) step_tail_kernel<false, true, false, PRED_V><<<grid, 256, 0, st>>>(p);
      else if (rule == Rule::DDIM) step_tail_kernel<true, false, false, PRED_V><<<grid, 256, 0, st>>>(p);
      else step_tail_kernel<false, false, false, PRED_V><<<grid, 256, 0, st>>>(p);
    } else {
      if (rule == Rule::INVERT) step_tail4_kernel<false, false, true, PRED_V><<<grid, 256, 0, st>>>(p);
      else if (rule == Rule::DPM) step_tail4_kernel<false, true, false, PRED_V><<<grid, 256, 0, st>>>(p);
      else if (rule == Rule::DDIM) step_tail4_kernel<true, false, false, PRED_V><<<grid, 256, 0, st>>>(p);
      else step_tail4_kernel<false, false, false, PRED_V><<<grid, 256, 0, st>>>(p);
    }
  } else if (!head4) {
    if (rule == Rule::INVERT) step_tail_kernel<false, false, true><<<grid, 256, 0, st>>>(p);
    else if (rule == Rule::DPM) step_tail_kernel<false, true><<<grid, 256, 0, st>>>(p);
    else if (rule == Rule::DDIM) step_tail_kernel<true><<<grid, 256, 0, st>>>(p);
    else step_tail_kernel<false><<<grid, 256, 0, st>>>(p);
  } else {
    if (rule == Rule::INVERT) step_tail4_kernel<false, false, true><<<grid, 256, 0, st>>>(p);
    else if (rule == Rule::DPM) step_tail4_kernel<false, true><<<grid, 256, 0, st>>>(p);
    else if (rule == Rule::DDIM) step_tail4_kernel<true><<<grid, 256, 0, st>>>(p);
    else step_tail4_kernel<false><<<grid, 256, 0, st>>>(p);
  }
}

// A step's place in a multi-step sample-loop graph: t_next is where the embedding kernel stores the
// step's t - 1; cond_cached = the conditioning MLP rows of the graph's first step are still valid.
struct GraphStep {
  int64_t* t_next = nullptr;
  bool cond_cached = false;
};

// One step, validated by validate().  With mode.rescale() > 0 the tail becomes three launches
// (guidance.h, through launch.h) whose eg and block partials come from the arena, in the dry run as
// in the real one; they read the position scalar the tail reads, through step_tail_kernel.  The
// known-region blend follows the tail as a launch of its own, on a.x_out in place, at the position
// the tail read.  A composed step (mode.comp) runs K + 1 branch-major rows through the trunk and the
// composed tail; with Co < 4 the head, the mix and the update are three launches whose predictions
// come from the arena.  With mode.perturb the trailing branches of the composition run the identity
// core in the chosen attention blocks (engine.hip attention_rows); the arena and the tail are the
// composed step's.  A geometry-guided step (mode.geom; geom.h) runs, after the trunk, the taped
// training forward of the B conditional rows, the loss seed and the data-only backward
// (train_engine.h) in the same arena — nothing is allocated outside the plan, so the step captures
// like any other — then materialises the CFG eps as the rescaled step does, mixes the input
// gradient into it and runs the rule's tail on the mixed eps.  kind: the step's part in a
// feature-cached call (StepMode::cache_kind) — the trunk stores or reads the model's deep feature
// (unet_trunk); the head and the tail are the same either way.
static void step_body(Run& R, const dmx_step_args& a, const StepMode& mode, GraphStep gs = {},
                      StepMode::Kind kind = StepMode::PLAIN) {
  dmx_model* m = R.m;
  const dmx_compose* comp = mode.comp;
  const bool cfg = comp == nullptr && m->kind != DMX_UNET && a.guidance > 0.f && a.y != nullptr;
  const bool resc = mode.rescale() > 0.f;
  const dmx_geom_guide* gg = mode.geom;
  const Rule rule = mode.rule();
  const int N = comp != nullptr ? (comp->K + 1) * a.n : cfg ? 2 * a.n : a.n;
  FwdIn in{a.x_in, a.n, a.t, a.t_stride, a.y, cfg ? 1 : 0, a.null_label, a.vals, a.mask, a.n};
  if (comp != nullptr) {  // every row of the forward has its own label and condition row
    in.y = comp->y;
    in.y_null = 0;
    in.vals = comp->vals;
    in.mask = comp->mask;
    in.cond_rows = N;
  }
  if (mode.perturb != nullptr) {  // the trailing branches k0..K: the rows [k0 n, (K + 1) n) of the forward
    const int k0 = __builtin_ctz(mode.perturb->branches);
    in.perturb = Perturb{mode.perturb->blocks, k0 * a.n, N};
  }
  in.t_next = gs.t_next;
  in.cond_cached = gs.cond_cached;
  if (kind != StepMode::PLAIN) {
    in.cache = (int)kind;
    in.dcache = m->dcache;
  }
  if (rule != Rule::DDPM) {
    in.t_map = mode.t_map();
    in.n_pos = mode.positions(a);
  }
  float* feat = unet_trunk(R, in, N, a.h, a.w);
  const int pixb = m->in_ch == 4 ? 16 : 256;  // pixels per block of the rescaled tail's first stage
  const int nb = cdiv(a.h * a.w, pixb);
  const bool mat = resc || gg != nullptr;  // the guided eps goes through the arena
  float* eg = mat ? R.ws.get<float>((size_t)a.n * m->in_ch * a.h * a.w) : nullptr;
  double* part = mat ? R.ws.get<double>((size_t)a.n * nb * 4) : nullptr;
  const bool comp3 = comp != nullptr && m->in_ch != 4;  // head, mix, update as three launches
  float* eall = comp3 ? R.ws.get<float>((size_t)N * m->in_ch * a.h * a.w) : nullptr;
  float* emix = comp3 ? R.ws.get<float>((size_t)a.n * m->in_ch * a.h * a.w) : nullptr;
  float* gx = nullptr;  // dL/dx of a geometry-guided step
  if (gg != nullptr) {
    const int gd = m->cfg.gdim;
    gx = R.ws.get<float>((size_t)a.n * m->in_ch * a.h * a.w);
    float* teps = R.ws.get<float>((size_t)a.n * m->in_ch * a.h * a.w);
    float* geom = R.ws.get<float>((size_t)a.n * gd);
    float* seed = R.ws.get<float>((size_t)a.n * gd);
    // The model's training tape is replaced (its record now points into this arena) under an id no
    // caller holds: a backward pending on an earlier forward is refused as stale.
    if (m->tape == nullptr) m->tape = new Tape();
    Tape& T = *m->tape;
    T.id = 0;
    TrainArgs ta{a.x_in, a.t, a.y, a.vals, a.mask, a.n, a.h, a.w, teps, geom, a.t_stride, mode.t_map(),
                 mode.positions(a)};
    const std::string layer = R.layer;
    with_fp32(m, [&] {
      train_fwd_body(R, T, ta);
      if (!R.plan) {
        R.layer = "geom.seed";
        R.begin("geom_seed_kernel", 6.0 * a.n * gd, 4.0 * 5.0 * a.n * gd);
        launch_geom_seed(geom, a.vals, a.mask, a.n, gd, nullptr, seed, R.st);
        R.end();
        HIPCHK(hipGetLastError());
      }
      train_bwd_body(R, T, GradMap{}, nullptr, seed, gx);
    });
    R.layer = layer;
    if (!R.plan) T.id = ++m->tape_id;
  }
  if (R.plan) return;
  StepTailParams p;
  std::memset(&p, 0, sizeof(p));
  p.feat = feat;
  p.w = m->out_w;
  p.b = m->out_b;
  p.Co = m->in_ch;
  p.B = a.n;
  p.HW = a.h * a.w;
  p.cfg = cfg ? 1 : 0;
  p.guidance = a.guidance;
  p.x = a.x_in;
  p.x_out = a.x_out;
  p.t = a.t;
  p.t_stride = a.t_stride;
  p.noise = a.noise;
  p.seed = a.seed;
  p.sample_offset = a.sample_offset;
  p.range_flag = m->range_flag;
  if (m->pred != DMX_PRED_EPS) {  // every tail below converts its mixed output (tail_math.h tail_eps / tail_x0)
    p.p_o = m->pred_tab;
    p.p_x = m->pred_tab + m->pred_T;
    p.pred_T = m->pred_T;
    p.x_net = a.x_in;  // the buffer the trunk read: in an inversion's refinement rows y, not the source latent
    if (m->pred == DMX_PRED_V_X0) {
      p.d_s = m->pred_tab + 2 * (size_t)m->pred_T;
      p.d_d = m->pred_tab + 3 * (size_t)m->pred_T;
    }
  }
  if (rule == Rule::INVERT) {
    set_sched(p, *mode.invert);
    p.x = mode.invert->src;  // (the latent the network saw, a.x_in, is an operand of the update in v-mode alone)
  } else if (rule == Rule::DPM) {
    set_sched(p, *mode.dpm);
  } else if (rule == Rule::DDIM) {
    set_sched(p, *mode.ddim);
  } else {
    p.tmax = a.T;
    p.c1 = a.c1;
    p.c2 = a.c2;
    p.sd = a.sd;
  }
  R.layer = rule == Rule::INVERT ? "out+cfg+invert"
            : rule == Rule::DPM  ? "out+cfg+dpm"
            : rule == Rule::DDIM ? "out+cfg+ddim"
                                 : "out+cfg+ddpm";
  const double el = (double)a.n * p.Co * p.HW;
  const double head_flops = 2.0 * N * p.HW * 64.0 * p.Co, head_bytes = 4.0 * ((double)N * p.HW * 64 + 3.0 * el);
  if (comp != nullptr) {
    const ComposeParams cq{comp->K, comp->weight};
    p.cfg = 0;
    p.guidance = 0.f;
    if (!comp3) {
      R.begin("compose_tail4_kernel", head_flops, head_bytes);
      launch_step_tail(p, rule, true, dim3(cdiv(p.HW, 16), a.n), R.st, &cq);
    } else {
      R.begin("out_head_kernel", head_flops, 4.0 * ((double)N * p.HW * 64 + (double)N * p.Co * p.HW));
      out_head_kernel<<<dim3(cdiv(p.HW, 256), N), 256, 0, R.st>>>(feat, m->out_w, m->out_b, eall, p.Co, p.HW,
                                                                 m->range_flag);
      R.end();
      HIPCHK(hipGetLastError());
      R.begin("compose_eps_kernel", 3.0 * comp->K * el, 4.0 * (comp->K + 2.0) * el);
      launch_compose_eps(eall, comp->weight, comp->K, a.n, (int64_t)p.Co * p.HW, emix, R.st);
      R.end();
      HIPCHK(hipGetLastError());
      p.feat = nullptr;
      p.eps_u = emix;
      R.begin("step_tail_kernel", 8.0 * el, 4.0 * 4.0 * el);
      launch_step_tail(p, rule, false, dim3(cdiv(p.HW, 256), a.n), R.st);
    }
  } else if (mat) {
    R.begin(p.Co == 4 ? "cfg_stats4_kernel" : "cfg_stats_kernel", head_flops, 4.0 * ((double)N * p.HW * 64 + el));
    CfgHeadParams hp{p.feat, p.w, p.b, p.Co, p.B, p.HW, p.guidance, p.range_flag};
    launch_cfg_stats(hp, eg, part, nb, R.st);
    R.end();
    HIPCHK(hipGetLastError());
    if (resc) {
      R.begin("cfg_scale_kernel", el, 8.0 * el);
      launch_cfg_scale(eg, part, nb, pixb, p.Co, p.HW, a.n, mode.rescale(), nullptr, R.st);
    } else {  // (the block moments of the stats kernel are not read here)
      R.begin("geom_mix_kernel", 3.0 * el, 12.0 * el);
      launch_geom_mix(eg, gx, *gg, a.t, a.t_stride, a.n, (int64_t)p.Co * p.HW, eg, p.range_flag, R.st);
    }
    R.end();
    HIPCHK(hipGetLastError());
    // the update on the scaled eg: the tail's precomputed-eps form (it raises the range flag on it)
    p.feat = nullptr;
    p.cfg = 0;
    p.eps_u = eg;
    R.begin("step_tail_kernel", 8.0 * el, 4.0 * 4.0 * el);
    launch_step_tail(p, rule, false, dim3(cdiv(p.HW, 256), a.n), R.st);
  } else if (p.Co == 4 && p.feat != nullptr) {
    R.begin("step_tail4_kernel", head_flops, head_bytes);
    launch_step_tail(p, rule, true, dim3(cdiv(p.HW, 16), a.n), R.st);
  } else {
    R.begin("step_tail_kernel", head_flops, head_bytes);
    launch_step_tail(p, rule, false, dim3(cdiv(p.HW, 256), a.n), R.st);
  }
  R.end();
  HIPCHK(hipGetLastError());
  if (mode.known != nullptr) {
    R.layer = "known_blend";
    R.begin("known_blend_kernel", 5.0 * a.n * p.Co * p.HW, 4.0 * (4.0 * p.Co + 1.0) * a.n * p.HW);
    launch_known_blend(a.x_out, a.x_out, a.t, a.t_stride, *mode.known, a.n, p.Co, p.HW, R.st);
    R.end();
    HIPCHK(hipGetLastError());
  }
}

// ---------------------------------------------------------------------------
// Argument rules
// ---------------------------------------------------------------------------
static void check_sched(const dmx_ddim_sched* sc) {
  REQUIRE(sc != nullptr, "null schedule");
  REQUIRE(sc->S >= 1, "schedule needs S >= 1 positions");
  REQUIRE(sc->t_map && sc->k_e && sc->k_a && sc->k_s && sc->k_d && sc->k_n, "null table in schedule");
}

static void check_sched(const dmx_dpm_sched* dp) {
  REQUIRE(dp != nullptr, "null schedule");
  REQUIRE(dp->S >= 1, "schedule needs S >= 1 positions");
  REQUIRE(dp->t_map && dp->k_e && dp->k_a && dp->k_x && dp->k_c && dp->k_p, "null table in schedule");
  REQUIRE(dp->hist != nullptr, "DPM schedule needs a history buffer");
}

static void check_sched(const dmx_invert_sched* iv) {
  REQUIRE(iv != nullptr, "null schedule");
  REQUIRE(iv->S >= 1, "schedule needs S >= 1 rows");
  REQUIRE(iv->t_map && iv->i_x && iv->i_e && iv->adv, "null table in schedule");
  REQUIRE(iv->src != nullptr, "inversion schedule needs a source buffer");
}

static void check_known(const dmx_known_sched* kn, const float* x_out) {
  REQUIRE(kn != nullptr, "null known-region schedule");
  REQUIRE(kn->S >= 1, "known-region schedule needs S >= 1 positions");
  REQUIRE(kn->z0 && kn->e0 && kn->q_a && kn->q_e, "null tensor in known-region schedule");
  REQUIRE(kn->z0 != x_out && kn->e0 != x_out && kn->mask != x_out, "z0 / e0 / mask must not alias x_out");
}

// Every rule of a step (for_loop: of a sample loop) in `mode`; a null member of mode is a part not
// asked for.  The parts are checked before the model's state, the step args after it.
static void validate(dmx_model* m, const dmx_step_args* a, const StepMode& mode, bool for_loop) {
  REQUIRE(m != nullptr, "null model");
  REQUIRE(a != nullptr, "null step args");
  const bool cfg = m->kind != DMX_UNET && a->guidance > 0.f && a->y != nullptr;
  if (const char* why = mode.invert_conflict()) throw Error(DMX_E_ARG, why);
  if (const char* why = mode.cache_conflict()) throw Error(DMX_E_ARG, why);
  if (mode.cached()) REQUIRE(mode.cache->phase >= 0, "cache phase must be >= 0");
  if (mode.comp != nullptr) {
    const dmx_compose& c = *mode.comp;
    REQUIRE(c.K >= 1 && c.K <= DMX_COMPOSE_MAX, "compose K must lie in [1, DMX_COMPOSE_MAX]");
    REQUIRE(c.y != nullptr && c.weight != nullptr, "compose needs y and weight");
    REQUIRE((c.vals == nullptr) == (c.mask == nullptr), "compose vals and mask must be given together");
    REQUIRE(m->kind == DMX_UNET_COND_GEOM || m->kind == DMX_UNET_COND, "compose needs a conditional model");
    REQUIRE(mode.rescale() == 0.f, "composed steps take no guidance rescale");
    REQUIRE(a->n <= 65535, "composed steps take at most 65535 samples");
    const void* xo = a->x_out;
    REQUIRE(c.y != xo && c.vals != xo && c.mask != xo && c.weight != xo, "compose tables must not alias x_out");
  }
  if (mode.gd != nullptr) {
    REQUIRE(mode.gd->rescale >= 0.f && mode.gd->rescale <= 1.f, "guidance rescale must lie in [0, 1]");
    if (mode.rescale() > 0.f) {
      REQUIRE(cfg, "guidance rescale needs a CFG step (guidance > 0, y given, a conditional model)");
      REQUIRE(a->n <= 65535, "rescaled steps take at most 65535 samples");
    }
  }
  if (mode.geom != nullptr) {
    const dmx_geom_guide& g = *mode.geom;
    REQUIRE(g.scale != nullptr && g.sig != nullptr, "geometry guidance needs the scale and sig tables");
    REQUIRE(m->kind == DMX_UNET_COND_GEOM, "geometry guidance needs a model with a GeomHead");
    REQUIRE(mode.comp == nullptr, "geometry guidance takes no composition");
    REQUIRE(mode.rescale() == 0.f, "geometry guidance takes no guidance rescale");
    REQUIRE(a->guidance > 0.f && a->y != nullptr, "geometry guidance needs a CFG step (guidance > 0, y given)");
    REQUIRE(a->vals != nullptr && a->mask != nullptr, "geometry guidance needs vals and mask (its target)");
    REQUIRE(g.S == mode.positions(*a), "geometry guidance S differs from the schedule's");
    REQUIRE(a->n <= 65535, "geometry-guided steps take at most 65535 samples");
    const void* xo = a->x_out;
    REQUIRE(g.scale != xo && g.sig != xo, "geometry guidance tables must not alias x_out");
  }
  if (mode.perturb != nullptr) {
    const dmx_perturb& p = *mode.perturb;
    REQUIRE(mode.comp != nullptr, "perturbed-attention guidance needs a composition");
    REQUIRE(p.blocks >= 1u && p.blocks < 64u, "perturb blocks must lie in [1, 63] (bit i: sa(i+1))");
    // a non-empty run of set bits that ends at bit K: branches + its lowest set bit == 2^(K+1)
    REQUIRE(p.branches != 0u && (p.branches >> mode.comp->K) == 1u &&
                ((p.branches + (p.branches & (0u - p.branches))) == (1u << (mode.comp->K + 1))),
            "perturb branches must be a non-empty trailing run of the branches 0..K");
    REQUIRE(mode.geom == nullptr, "perturbed-attention guidance takes no geometry guidance");
    REQUIRE(mode.rescale() == 0.f, "perturbed-attention guidance takes no guidance rescale");
  }
  REQUIRE(mode.ddim == nullptr || mode.dpm == nullptr, "at most one of the DDIM and DPM schedules");
  if (mode.ddim != nullptr) check_sched(mode.ddim);
  if (mode.dpm != nullptr) check_sched(mode.dpm);
  if (mode.invert != nullptr) check_sched(mode.invert);
  if (mode.known != nullptr) {  // its tables must cover the positions of the step's schedule
    check_known(mode.known, a->x_out);
    REQUIRE(mode.known->mask != nullptr, "a known-region step needs a mask");
    REQUIRE(a->n <= 65535, "known-region steps take at most 65535 samples");
    REQUIRE(mode.known->S == mode.positions(*a), "known-region S differs from the schedule's");
  }
  check_shapes(m, a->n, a->h, a->w);
  REQUIRE(a->x_in && a->x_out && a->t, "null tensor in step args");
  if (mode.rule() == Rule::INVERT) {
    REQUIRE(a->noise == nullptr, "inversion takes no noise (noise must be NULL)");
    REQUIRE(mode.invert->src != a->x_in && mode.invert->src != a->x_out, "src must not alias x");
  } else if (mode.rule() == Rule::DPM) {
    REQUIRE(a->noise == nullptr, "the DPM solver takes no noise (noise must be NULL)");
    REQUIRE(mode.dpm->hist != a->x_in && mode.dpm->hist != a->x_out, "hist must not alias x");
  } else if (mode.rule() == Rule::DDPM) {  // (the strided steps ignore these)
    REQUIRE(a->c1 && a->c2 && a->sd, "null tensor in step args");
    REQUIRE(a->T >= 1, "T must be >= 1");
  }
  REQUIRE(m->in_ch <= 4, "in_ch must be <= 4");
  if (mode.comp == nullptr && m->kind != DMX_UNET && a->guidance > 0.f) REQUIRE(a->y != nullptr, "CFG needs y");
  if (mode.comp == nullptr && (m->kind == DMX_UNET_COND_GEOM || m->kind == DMX_UNET_COND))
    REQUIRE((a->vals == nullptr) == (a->mask == nullptr), "vals and mask must be given together");
  if (for_loop) {
    REQUIRE(a->x_in == a->x_out, "sample loop runs in place (x_in == x_out)");
    REQUIRE(a->t_stride == 0, "sample loop needs a device scalar t (t_stride 0)");
    REQUIRE(a->noise == nullptr, "sample loop draws on-device Philox noise (noise must be NULL)");
  }
}

// A v-model's step or loop (validated) converts with the rows t - 1 of the model's tables: the largest
// network timestep its schedule names must lie inside them.  The DDPM rule names 1..T of its own
// tables; a strided rule's timesteps are its t_map, device memory, read back here — one small copy
// and a wait for st per call, in v-mode only.  Nothing has been launched when this throws.
static void check_prediction(const dmx_model* m, const dmx_step_args& a, const StepMode& mode, hipStream_t st) {
  if (m->pred == DMX_PRED_EPS) return;
  int64_t t_max = a.T;
  if (mode.rule() != Rule::DDPM) {
    std::vector<int64_t> tm((size_t)mode.positions(a));
    HIPCHK(hipMemcpyAsync(tm.data(), mode.t_map(), tm.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    t_max = 0;
    for (int64_t v : tm) t_max = v > t_max ? v : t_max;
  }
  const char* bad = prediction_range_error(t_max, m->pred_T);
  REQUIRE(bad == nullptr, bad);
}

// ---------------------------------------------------------------------------
// Feature caching: the model's deep-feature buffer and what it belongs to
// ---------------------------------------------------------------------------
// Rows of the trunk in a (validated, uncomposed) step: 2n under CFG batching, else n.
static int trunk_rows(const dmx_model* m, const dmx_step_args& a) {
  return m->kind != DMX_UNET && a.guidance > 0.f && a.y != nullptr ? 2 * a.n : a.n;
}

// Room for the deep feature of a step with these args, before a refresh step is planned.  Growing
// an existing buffer waits for the stream's earlier work, and drops every captured graph and the
// stored feature: the graphs of cached loops hold the old pointer.  The first allocation drops
// nothing — no graph can hold a pointer that did not exist.
static void ensure_dcache(dmx_model* m, const dmx_step_args& a, hipStream_t st) {
  const size_t el = (size_t)trunk_rows(m, a) * (a.h / 2) * (a.w / 2) * m->up[1].cout;
  if (el <= m->dcache_cap) return;
  if (m->dcache != nullptr) {
    HIPCHK(hipStreamSynchronize(st));
    m->owned_bytes.erase(reinterpret_cast<const char*>(m->dcache));
    HIPCHK(hipFree(m->dcache));
    drop_graph(m);
  }
  m->dcache = nullptr;
  m->dcache_cap = 0;
  m->dtag.valid = false;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&m->dcache), el * sizeof(float)));
  m->dcache_cap = el;
  m->owned_bytes[reinterpret_cast<const char*>(m->dcache)] = el * sizeof(float);  // DMX_CHECK ranges
}

// A reuse step with these args may read the stored feature; else DMX_E_STATE naming what differs.
static void check_dcache(const dmx_model* m, const dmx_step_args& a) {
  const dmx_model::DTag& g = m->dtag;
  auto stale = [](const std::string& why) {
    throw Error(DMX_E_STATE, "reuse step without a matching cached feature: " + why);
  };
  if (!g.valid || m->dcache == nullptr) stale("no refresh step has run (or its buffer was reallocated)");
  if (g.gen != m->weights_gen) stale("the weights changed since the refresh step (finalize / refresh)");
  if (g.prec != m->prec)
    stale("the precision mode changed since the refresh step (" + std::to_string(g.prec) + " -> " +
          std::to_string(m->prec) + ")");
  if (g.h != a.h || g.w != a.w)
    stale("the map size differs (" + std::to_string(g.h) + "x" + std::to_string(g.w) + " stored, " +
          std::to_string(a.h) + "x" + std::to_string(a.w) + " asked)");
  const int rows = trunk_rows(m, a);
  if (g.n != a.n)
    stale("the batch differs (" + std::to_string(g.n) + " samples stored, " + std::to_string(a.n) + " asked)");
  if (g.rows != rows)
    stale("the step kind differs (" + std::to_string(g.rows) + " rows stored, " + std::to_string(rows) +
          " asked: CFG and unguided steps do not share a feature)");
}

static void tag_dcache(dmx_model* m, const dmx_step_args& a) {
  m->dtag = dmx_model::DTag{true, trunk_rows(m, a), a.n, a.h, a.w, m->prec, m->weights_gen};
}

// ---------------------------------------------------------------------------
// The step and the loop behind the dmx_step* / dmx_sample_loop* entries
// ---------------------------------------------------------------------------
static void sample_step(dmx_model* m, const dmx_step_args* a, const StepMode& mode, hipStream_t st) {
  validate(m, a, mode, false);
  check_prediction(m, *a, mode, st);
  const StepMode::Kind kind = mode.cache_kind(0);
  if (kind == StepMode::REUSE) check_dcache(m, *a);  // (before anything is launched)
  ensure_planes(m, st);
  if (mode.geom != nullptr) ensure_train(m, st);
  if (kind == StepMode::REFRESH) {
    ensure_dcache(m, *a, st);
    m->dtag.valid = false;  // until the step below has been enqueued
  }
  run_planned(m, st, [&](Run& R) { step_body(R, *a, mode, {}, kind); });
  if (kind == StepMode::REFRESH) tag_dcache(m, *a);
}

// Capture what `body` launches on st into *graph and instantiate it as *exec (both owned by a graph
// slot of m from the moment they are stored).  Any failure on the way drops every slot.
template <typename F>
static void capture(dmx_model* m, hipStream_t st, F&& body, hipGraph_t* graph, hipGraphExec_t* exec) {
  HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  try {
    body();
  } catch (...) {
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(st, &g);
    if (g) (void)hipGraphDestroy(g);
    drop_graph(m);
    throw;
  }
  const hipError_t ec = hipStreamEndCapture(st, graph);
  const hipError_t ei = ec == hipSuccess ? hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0) : ec;
  if (ei != hipSuccess) {
    drop_graph(m);
    HIPCHK(ei);
  }
}

static constexpr int kGraphSteps = 8;

// The loop of a feature-cached call (validated, planes ensured): step k is a refresh or a reuse step
// (StepMode::cache_kind).  Graph replay keeps one slot per kind, each a one-step graph (step +
// decrement; no 8-step graph: a refresh never repeats, and a run of reuse steps is at most
// interval - 1 long), and launches them in the pattern.  The two kinds walk different arenas — a
// reuse step allocates less — so neither graph can use the other's cond-MLP rows: every captured step
// computes its own.  Both arenas are planned before either kind is captured: a capture that grew
// the workspace would drop the slot captured just before it.
static void cached_loop(dmx_model* m, const dmx_step_args* a, const StepMode& mode, int steps, int use_graph,
                        hipStream_t st) {
  if (steps == 0) return;
  int64_t* tdev = const_cast<int64_t*>(a->t);
  bool need[3] = {false, false, false};
  for (int k = 0; k < steps && !(need[StepMode::REFRESH] && need[StepMode::REUSE]); ++k)
    need[mode.cache_kind(k)] = true;
  if (mode.cache_kind(0) == StepMode::REUSE) check_dcache(m, *a);  // (later reuse steps follow a refresh of this call)
  if (need[StepMode::REFRESH]) {
    ensure_dcache(m, *a, st);
    m->dtag.valid = false;  // until every step has been enqueued
  }
  if (!use_graph) {
    for (int i = 0; i < steps; ++i) {
      const StepMode::Kind kind = mode.cache_kind(i);
      run_planned(m, st, [&](Run& R) { step_body(R, *a, mode, {}, kind); });
      decrement_t_kernel<<<1, 64, 0, st>>>(tdev);
      HIPCHK(hipGetLastError());
    }
  } else {
    const StepMode::Kind kinds[2] = {StepMode::REFRESH, StepMode::REUSE};
    GraphSlot* slot[3] = {nullptr, nullptr, nullptr};
    auto find_all = [&] {
      bool all = true;
      for (StepMode::Kind kd : kinds) {
        slot[kd] = need[kd] ? m->graphs.find(make_graph_key(*a, mode, m->ctx->table_gen, kd)) : nullptr;
        all = all && (!need[kd] || slot[kd] != nullptr);
      }
      return all;
    };
    if (!find_all()) {
      // the refresh kind's arena is the larger one (a reuse step runs a subset of its blocks); it is
      // planned even where this call holds no refresh step, so a later one grows nothing (the buffer
      // exists: this call refreshes, or check_dcache has accepted a stored feature)
      for (StepMode::Kind kd : {StepMode::REUSE, StepMode::REFRESH})
        plan_ws(m, st, m->ws, [&](Run& R) { step_body(R, *a, mode, {}, kd); });
      find_all();  // (a grown arena dropped them all)
      for (StepMode::Kind kd : kinds) {
        if (!need[kd] || slot[kd] != nullptr) continue;
        const size_t cap = m->ws.cap;
        plan_ws(m, st, m->ws, [&](Run& R) { step_body(R, *a, mode, {}, kd); });
        if (m->ws.cap != cap) throw Error(DMX_E_INTERNAL, "cached loop: the arena grew between its two captures");
        GraphSlot* s = m->graphs.victim();  // free, or the least recently used: never the other kind's, found or
        drop_slot(m, s);                    // claimed a moment ago
        capture(m, st, [&] {
          Run R{m, st, false, m->ws.a};
          step_body(R, *a, mode, {}, kd);
          decrement_t_kernel<<<1, 64, 0, st>>>(tdev);
        }, &s->val.graph, &s->val.gexec);
        m->graphs.claim(s, make_graph_key(*a, mode, m->ctx->table_gen, kd));
        ++m->graph_captures;
        slot[kd] = s;
      }
    }
    for (int i = 0; i < steps; ++i) HIPCHK(hipGraphLaunch(slot[mode.cache_kind(i)]->val.gexec, st));
  }
  if (need[StepMode::REFRESH]) tag_dcache(m, *a);
}

// `steps` in-place steps.  The scalar a->t counts down by one per step in every mode — timesteps in
// the DDPM loop, positions of the schedule in the strided ones.  The DPM history buffer is updated
// in place by every step and the known-region blend reads the position scalar its tail read, so
// neither needs more than t's ping-pong inside the multi-step graph.  An inversion counts its rows
// down the same way and updates its source buffer in place, as the DPM loop its history.
static void sample_loop(dmx_model* m, const dmx_step_args* a, const StepMode& mode, int steps, int use_graph,
                        hipStream_t st) {
  validate(m, a, mode, true);
  REQUIRE(steps >= 0, "steps must be >= 0");
  check_prediction(m, *a, mode, st);
  ensure_planes(m, st);
  if (mode.geom != nullptr) ensure_train(m, st);  // (packs and synchronises: before any capture)
  int64_t* tdev = const_cast<int64_t*>(a->t);
  if (mode.cached()) return cached_loop(m, a, mode, steps, use_graph, st);
  if (!use_graph) {
    for (int i = 0; i < steps; ++i) {
      run_planned(m, st, [&](Run& R) { step_body(R, *a, mode); });
      decrement_t_kernel<<<1, 64, 0, st>>>(tdev);
      HIPCHK(hipGetLastError());
    }
    return;
  }
  const GraphKey key = make_graph_key(*a, mode, m->ctx->table_gen);
  GraphSlot* slot = m->graphs.find(key);
  if (slot == nullptr) {
    // plan + allocate outside capture (a grown arena drops every slot: their graphs point into the
    // old one), then capture the real launches
    plan_ws(m, st, m->ws, [&](Run& R) { step_body(R, *a, mode); });
    slot = m->graphs.victim();
    drop_slot(m, slot);  // a free slot, or the least recently used pair makes room
    GraphPair& gp = slot->val;
    capture(m, st, [&] {
      Run R{m, st, false, m->ws.a};
      step_body(R, *a, mode);
      decrement_t_kernel<<<1, 64, 0, st>>>(tdev);
    }, &gp.graph, &gp.gexec);
    // kGraphSteps consecutive steps in one graph: the gap between two graph launches (≈9 µs of
    // idle GPU per step in the replay trace) is paid once per kGraphSteps steps.  Inside it, t
    // alternates between the caller's scalar and a scratch scalar: step k reads one and its
    // embedding kernel stores t - 1 in the other (no one-thread decrement launch per step; an even
    // kGraphSteps ends in the caller's scalar).  The noise is keyed by (seed, t, sample), so the
    // captured steps compute what kGraphSteps replays of the one-step graph compute.
    static_assert(kGraphSteps % 2 == 0, "t ping-pong must end in the caller's buffer");
    int64_t* tscr = m->t_scratch;
    capture(m, st, [&] {
      for (int k = 0; k < kGraphSteps; ++k) {
        m->ws.a.rewind();
        Run R{m, st, false, m->ws.a};
        dmx_step_args ak = *a;
        ak.t = (k & 1) ? tscr : tdev;
        step_body(R, ak, mode, {(k & 1) ? tdev : tscr, k > 0});  // cond MLP rows from step 0 of the graph
      }
    }, &gp.graph_k, &gp.gexec_k);
    // the slot is not `used` (no key can find it) until both graphs are instantiated
    m->graphs.claim(slot, key);
    ++m->graph_captures;
  }
  int i = 0;
  for (; i + kGraphSteps <= steps; i += kGraphSteps) HIPCHK(hipGraphLaunch(slot->val.gexec_k, st));
  for (; i < steps; ++i) HIPCHK(hipGraphLaunch(slot->val.gexec, st));
}

// ---------------------------------------------------------------------------
// Standalone updates (dmx_ddpm_update / dmx_ddim_update / dmx_dpm_update / dmx_invert_update): the
// tail on given eps
// ---------------------------------------------------------------------------
// What the three have in common; the caller adds its tables (and noise, where its rule draws).
static StepTailParams update_params(const float* x, float* x_out, const float* eu, const float* ec, float guidance,
                                    const int64_t* t, int t_stride, int n, int c, int h, int w) {
  REQUIRE(x && x_out && eu && t, "null tensor");
  REQUIRE(n >= 1 && c >= 1 && c <= 4 && h >= 1 && w >= 1, "bad shape");
  StepTailParams p;
  std::memset(&p, 0, sizeof(p));
  p.Co = c;
  p.B = n;
  p.HW = h * w;
  p.cfg = ec != nullptr ? 1 : 0;
  p.guidance = guidance;
  p.eps_u = eu;
  p.eps_c = ec;
  p.x = x;
  p.x_out = x_out;
  p.t = t;
  p.t_stride = t_stride;
  return p;
}

static void launch_update(const StepTailParams& p, Rule rule, hipStream_t st) {
  launch_step_tail(p, rule, false, dim3(cdiv(p.HW, 256), p.B), st);
  HIPCHK(hipGetLastError());
}

}  // namespace dmx
