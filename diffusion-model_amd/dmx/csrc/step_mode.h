// What kind of step a sampling call runs, and the key its captured graphs are kept under
// (sample_engine.h).  Host C++ only — no HIP type or call appears here — so the key's rules are
// exercised by a stand-alone program as well (tools/step_mode_check.cpp).
#pragma once
#include <cstring>

#include "dmx.h"

namespace dmx {

enum class Rule { DDPM, DDIM, DPM, INVERT };  // the tail's update

// The optional parts of a step (include/dmx.h); all null: the plain DDPM step.
struct StepMode {
  const dmx_ddim_sched* ddim = nullptr;    // strided sampling: a.t holds positions, a.c1 / c2 / sd / T are not read
  const dmx_dpm_sched* dpm = nullptr;      // the same with the DPM-Solver++(2M) update (at most one of ddim / dpm)
  const dmx_known_sched* known = nullptr;  // the known-region blend follows the tail
  const dmx_guidance* gd = nullptr;        // guidance controls beyond the scale
  const dmx_compose* comp = nullptr;       // composed guidance: K + 1 branches; a.y / vals / mask / guidance /
                                           // null_label are not read
  const dmx_geom_guide* geom = nullptr;    // geometry guidance: the GeomHead's input gradient joins the CFG eps
  const dmx_perturb* perturb = nullptr;    // perturbed-attention guidance: identity attention in the trailing
                                           // branches of comp
  const dmx_invert_sched* invert = nullptr;  // DDIM inversion: a.t holds countdown positions over the rows; no
                                             // other part may be given (invert_conflict)
  const dmx_cache* cache = nullptr;  // feature caching: refresh and reuse steps (cache_kind); interval <= 1 is
                                     // no request at all, as rescale == 0 is no rescale

  Rule rule() const {
    return invert != nullptr ? Rule::INVERT : dpm != nullptr ? Rule::DPM : ddim != nullptr ? Rule::DDIM : Rule::DDPM;
  }
  // The part an inversion step cannot be combined with, as the message of its DMX_E_ARG; null: none.
  // (A guidance struct with rescale == 0 is no part, as everywhere.)
  const char* invert_conflict() const {
    if (invert == nullptr) return nullptr;
    if (ddim != nullptr) return "an inversion step takes no DDIM schedule (its rows are its schedule)";
    if (dpm != nullptr) return "an inversion step takes no DPM schedule";
    if (known != nullptr) return "an inversion step takes no known region";
    if (rescale() > 0.f) return "an inversion step takes no guidance rescale";
    if (comp != nullptr) return "an inversion step takes no composition";
    if (geom != nullptr) return "an inversion step takes no geometry guidance";
    if (perturb != nullptr) return "an inversion step takes no perturbed-attention guidance";
    return nullptr;
  }
  // Is the deep feature cached?  The one place that decides that interval <= 1 is no request.
  bool cached() const { return cache != nullptr && cache->interval > 1; }
  // The kind of step k of a call (k = 0: the one-step entry): PLAIN without a request, else REFRESH
  // where (phase + k) % interval == 0 and REUSE elsewhere.
  enum Kind { PLAIN = 0, REFRESH = 1, REUSE = 2 };
  Kind cache_kind(int k) const {
    if (!cached()) return PLAIN;
    return (int)(((long long)cache->phase + k) % cache->interval) == 0 ? REFRESH : REUSE;
  }
  // The part a cached step cannot be combined with, as the message of its DMX_E_ARG; null: none.
  const char* cache_conflict() const {
    if (!cached()) return nullptr;
    if (invert != nullptr) return "a cached step (cache interval > 1) takes no inversion";
    if (comp != nullptr) return "a cached step (cache interval > 1) takes no composition";
    if (perturb != nullptr) return "a cached step (cache interval > 1) takes no perturbed-attention guidance";
    if (geom != nullptr) return "a cached step (cache interval > 1) takes no geometry guidance";
    return nullptr;
  }
  // phi of a rescaled CFG step, else 0.  The one place that decides that a guidance struct with
  // rescale == 0 is no guidance struct at all: launches and graph key are those of the plain call.
  float rescale() const { return gd != nullptr && gd->rescale > 0.f ? gd->rescale : 0.f; }
  // positions of the step's schedule, and their timesteps (null: the position is the timestep)
  int positions(const dmx_step_args& a) const {
    return invert != nullptr ? invert->S : dpm != nullptr ? dpm->S : ddim != nullptr ? ddim->S : a.T;
  }
  const int64_t* t_map() const {
    return invert != nullptr ? invert->t_map : dpm != nullptr ? dpm->t_map : ddim != nullptr ? ddim->t_map : nullptr;
  }
};

// Compared bytewise, so every byte is zero unless make_graph_key sets it.
struct GraphKey {
  dmx_step_args a;
  dmx_ddim_sched sched;  // strided loops: the schedule the graphs read (all zero: the DDPM loop)
  dmx_dpm_sched dpm;     // DPM-Solver++ loops: tables, history buffer and S (all zero otherwise)
  dmx_known_sched known; // known-region loops: z0, e0, mask, tables and S (all zero otherwise)
  dmx_guidance gd;       // rescaled loops: phi (all zero otherwise, rescale == 0 included)
  dmx_compose comp;      // composed loops: K and the four tables (all zero otherwise)
  dmx_geom_guide geom;   // geometry-guided loops: the two tables and S (all zero otherwise)
  dmx_perturb perturb;   // perturbed loops: the block and branch bits (all zero otherwise)
  dmx_invert_sched inv;  // inversion loops: tables, source buffer and S = rows (all zero otherwise)
  int table_gen;  // dmx_ctx::table_gen at capture
  int cache_kind; // cached loops: StepMode::REFRESH or REUSE, the kind of the one step the graph holds (zero otherwise)
  bool operator==(const GraphKey& o) const { return std::memcmp(this, &o, sizeof(GraphKey)) == 0; }
};

// The key of a loop: everything its graphs hold.  The step args enter as the caller's bytes; the
// optional structs enter member by member, so their padding stays zero.  A validated schedule has
// S >= 1, which keeps the keys of the four rules, and known-region keys from plain ones, apart;
// a validated composition has K >= 1, which keeps composed keys from plain ones; validated geometry
// guidance has non-null tables and S >= 1, which keeps its keys from plain ones; a validated
// perturbation has blocks >= 1, which keeps perturbed keys from composed ones.  kind: the step kind of
// a cached loop's graph (StepMode::cache_kind); neither the interval nor the phase enters the key, so
// every pattern over the same loop replays the same two graphs, and kind PLAIN — every loop without a
// cache request, interval <= 1 included — leaves the key what it was.
inline GraphKey make_graph_key(const dmx_step_args& a, const StepMode& mode, int table_gen,
                               StepMode::Kind kind = StepMode::PLAIN) {
  GraphKey key;
  std::memset(&key, 0, sizeof(key));
  std::memcpy(&key.a, &a, sizeof(dmx_step_args));
  if (mode.rule() != Rule::DDPM) {  // the strided graphs read the schedule instead of these
    key.a.c1 = key.a.c2 = key.a.sd = nullptr;
    key.a.T = 0;
  }
  if (mode.rule() == Rule::DDIM) {
    key.sched.t_map = mode.ddim->t_map;
    key.sched.k_e = mode.ddim->k_e;
    key.sched.k_a = mode.ddim->k_a;
    key.sched.k_s = mode.ddim->k_s;
    key.sched.k_d = mode.ddim->k_d;
    key.sched.k_n = mode.ddim->k_n;
    key.sched.S = mode.ddim->S;
  } else if (mode.rule() == Rule::DPM) {
    key.a.seed = 0;  // (not read: the solver draws nothing)
    key.dpm.t_map = mode.dpm->t_map;
    key.dpm.k_e = mode.dpm->k_e;
    key.dpm.k_a = mode.dpm->k_a;
    key.dpm.k_x = mode.dpm->k_x;
    key.dpm.k_c = mode.dpm->k_c;
    key.dpm.k_p = mode.dpm->k_p;
    key.dpm.hist = mode.dpm->hist;  // read and written by every step
    key.dpm.S = mode.dpm->S;
  } else if (mode.rule() == Rule::INVERT) {
    key.a.seed = 0;  // (not read: inversion draws nothing)
    key.inv.t_map = mode.invert->t_map;
    key.inv.i_x = mode.invert->i_x;
    key.inv.i_e = mode.invert->i_e;
    key.inv.adv = mode.invert->adv;
    key.inv.src = mode.invert->src;  // read by every row, written by the last row of a position
    key.inv.S = mode.invert->S;
  }
  if (mode.known != nullptr) {  // the blend's launches are in the graphs too
    key.known.z0 = mode.known->z0;
    key.known.e0 = mode.known->e0;
    key.known.mask = mode.known->mask;
    key.known.q_a = mode.known->q_a;
    key.known.q_e = mode.known->q_e;
    key.known.S = mode.known->S;
  }
  key.gd.rescale = mode.rescale();
  if (mode.comp != nullptr) {  // the branch tables stand where these would
    key.a.y = nullptr;
    key.a.vals = key.a.mask = nullptr;
    key.a.guidance = 0.f;
    key.a.null_label = 0;
    key.comp.K = mode.comp->K;
    key.comp.y = mode.comp->y;
    key.comp.vals = mode.comp->vals;
    key.comp.mask = mode.comp->mask;
    key.comp.weight = mode.comp->weight;
  }
  if (mode.geom != nullptr) {  // the seed, backward and mix launches are in the graphs too
    key.geom.scale = mode.geom->scale;
    key.geom.sig = mode.geom->sig;
    key.geom.S = mode.geom->S;
  }
  if (mode.perturb != nullptr) {  // the identity launches and the sub-range cores are in the graphs too
    key.perturb.blocks = mode.perturb->blocks;
    key.perturb.branches = mode.perturb->branches;
  }
  key.table_gen = table_gen;
  key.cache_kind = mode.cached() ? (int)kind : 0;
  return key;
}

}  // namespace dmx
