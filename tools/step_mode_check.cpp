// Stand-alone check of the sample-loop graph key's rules (dmx/csrc/step_mode.h).
// Host C++ only; build it with the host compiler and sanitizers and run it:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       -I diffusion-model_amd/dmx/csrc tools/step_mode_check.cpp -o step_mode_check && ./step_mode_check
// The pointers are dummies: the key holds their values and nothing dereferences them.
#include <cstdio>
#include <cstring>

#include "step_mode.h"

using namespace dmx;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);       \
      ++fails;                                                    \
    }                                                             \
  } while (0)

static float mem[64];
static int64_t imem[8];
static int amem[4];

// Every struct is filled over `fill` bytes first: what its padding then holds.
struct Inputs {
  dmx_step_args a;
  dmx_ddim_sched ddim;
  dmx_dpm_sched dpm;
  dmx_known_sched known;
  dmx_guidance gd;
  dmx_compose comp;
  dmx_geom_guide geom;
  dmx_perturb perturb;
  dmx_invert_sched inv;
  explicit Inputs(int fill = 0) {
    std::memset(&a, 0, sizeof(a));  // (the step args enter the key as the caller's bytes)
    a.x_in = a.x_out = mem;
    a.t = imem;
    a.y = imem + 1;
    a.null_label = 3;
    a.vals = mem + 1;
    a.mask = mem + 2;
    a.guidance = 3.f;
    a.c1 = mem + 3;
    a.c2 = mem + 4;
    a.sd = mem + 5;
    a.T = 1000;
    a.seed = 7;
    a.sample_offset = 64;
    a.n = 2;
    a.h = a.w = 8;
    std::memset(&ddim, fill, sizeof(ddim));
    ddim.t_map = imem + 2;
    ddim.k_e = mem + 6;
    ddim.k_a = mem + 7;
    ddim.k_s = mem + 8;
    ddim.k_d = mem + 9;
    ddim.k_n = mem + 10;
    ddim.S = 3;
    std::memset(&dpm, fill, sizeof(dpm));
    dpm.t_map = imem + 2;
    dpm.k_e = mem + 6;
    dpm.k_a = mem + 7;
    dpm.k_x = mem + 8;
    dpm.k_c = mem + 9;
    dpm.k_p = mem + 10;
    dpm.hist = mem + 11;
    dpm.S = 3;
    std::memset(&known, fill, sizeof(known));
    known.z0 = mem + 12;
    known.e0 = mem + 13;
    known.mask = mem + 14;
    known.q_a = mem + 15;
    known.q_e = mem + 16;
    known.S = 3;
    std::memset(&gd, fill, sizeof(gd));
    gd.rescale = 0.f;
    std::memset(&comp, fill, sizeof(comp));
    comp.K = 2;
    comp.y = imem + 3;
    comp.vals = mem + 17;
    comp.mask = mem + 18;
    comp.weight = mem + 19;
    std::memset(&geom, fill, sizeof(geom));
    geom.scale = mem + 20;
    geom.sig = mem + 21;
    geom.S = 3;
    std::memset(&perturb, fill, sizeof(perturb));
    perturb.blocks = 4;    // sa3
    perturb.branches = 4;  // branch 2 of K = 2
    std::memset(&inv, fill, sizeof(inv));
    inv.t_map = imem + 4;
    inv.i_x = mem + 22;
    inv.i_e = mem + 23;
    inv.adv = amem;
    inv.src = mem + 24;
    inv.S = 3;
  }
  // an inversion: alone, or (for the rules that refuse it) beside one other part
  StepMode inv_mode(int with = 0) const {
    StepMode m;
    m.invert = &inv;
    if (with == 1) m.ddim = &ddim;
    if (with == 2) m.dpm = &dpm;
    if (with == 3) m.known = &known;
    if (with == 4) m.gd = &gd;
    if (with == 5) m.comp = &comp;
    if (with == 6) m.geom = &geom;
    if (with == 7) m.perturb = &perturb;
    return m;
  }
  GraphKey inv_key(int table_gen = 1) const { return make_graph_key(a, inv_mode(), table_gen); }
  GraphKey key(bool use_ddim, bool use_dpm, bool use_known = false, bool use_gd = false, int table_gen = 1,
               bool use_comp = false, bool use_geom = false, bool use_perturb = false) const {
    return make_graph_key(a, StepMode{use_ddim ? &ddim : nullptr, use_dpm ? &dpm : nullptr,
                                      use_known ? &known : nullptr, use_gd ? &gd : nullptr,
                                      use_comp ? &comp : nullptr, use_geom ? &geom : nullptr,
                                      use_perturb ? &perturb : nullptr}, table_gen);
  }
};

// Does the key of the given mode differ from `base` once `edit` has changed one member of the inputs?
template <typename Edit>
static bool moved(const GraphKey& base, bool ddim, bool dpm, bool known, Edit&& edit) {
  Inputs in;
  edit(in);
  return !(in.key(ddim, dpm, known) == base);
}
#define MOVES(ddim, dpm, known, stmt) \
  CHECK(moved(Inputs().key(ddim, dpm, known), ddim, dpm, known, [](Inputs& in) { stmt; }))
#define STAYS(ddim, dpm, known, stmt) \
  CHECK(!moved(Inputs().key(ddim, dpm, known), ddim, dpm, known, [](Inputs& in) { stmt; }))

int main() {
  // 1. the DDPM key holds the tables, T and the seed
  MOVES(false, false, false, in.a.c1 = mem + 40);
  MOVES(false, false, false, in.a.c2 = mem + 40);
  MOVES(false, false, false, in.a.sd = mem + 40);
  MOVES(false, false, false, in.a.T = 999);
  MOVES(false, false, false, in.a.seed = 8);
  // 2. a DDIM key holds its schedule and the seed instead of the tables and T
  STAYS(true, false, false, in.a.c1 = mem + 40);
  STAYS(true, false, false, in.a.c2 = nullptr);
  STAYS(true, false, false, in.a.sd = mem + 40);
  STAYS(true, false, false, in.a.T = 0);
  MOVES(true, false, false, in.ddim.t_map = imem + 5);
  MOVES(true, false, false, in.ddim.k_e = mem + 40);
  MOVES(true, false, false, in.ddim.k_a = mem + 40);
  MOVES(true, false, false, in.ddim.k_s = mem + 40);
  MOVES(true, false, false, in.ddim.k_d = mem + 40);
  MOVES(true, false, false, in.ddim.k_n = mem + 40);
  MOVES(true, false, false, in.ddim.S = 4);
  MOVES(true, false, false, in.a.seed = 8);
  // 3. a DPM key holds neither those nor the seed; it holds its schedule and the history buffer
  STAYS(false, true, false, in.a.c1 = mem + 40);
  STAYS(false, true, false, in.a.c2 = mem + 40);
  STAYS(false, true, false, in.a.sd = nullptr);
  STAYS(false, true, false, in.a.T = 0);
  STAYS(false, true, false, in.a.seed = 8);
  MOVES(false, true, false, in.dpm.hist = mem + 40);
  MOVES(false, true, false, in.dpm.t_map = imem + 5);
  MOVES(false, true, false, in.dpm.k_e = mem + 40);
  MOVES(false, true, false, in.dpm.k_a = mem + 40);
  MOVES(false, true, false, in.dpm.k_x = mem + 40);
  MOVES(false, true, false, in.dpm.k_c = mem + 40);
  MOVES(false, true, false, in.dpm.k_p = mem + 40);
  MOVES(false, true, false, in.dpm.S = 4);
  // 4. no guidance struct, rescale 0 and the plain mode are one key; every phi > 0 is its own
  for (int mode = 0; mode < 3; ++mode) {
    const bool ddim = mode == 1, dpm = mode == 2;
    Inputs in;
    const GraphKey plain = in.key(ddim, dpm);
    CHECK(in.key(ddim, dpm, false, true) == plain);
    CHECK(plain == make_graph_key(in.a, StepMode{ddim ? &in.ddim : nullptr, dpm ? &in.dpm : nullptr}, 1));
    in.gd.rescale = 0.25f;
    const GraphKey quarter = in.key(ddim, dpm, false, true);
    in.gd.rescale = 0.5f;
    const GraphKey half = in.key(ddim, dpm, false, true);
    CHECK(!(quarter == plain) && !(half == plain) && !(quarter == half));
  }
  CHECK(StepMode{}.rescale() == 0.f);
  // 5. a known region is part of the key, member by member
  CHECK(!(Inputs().key(false, false, true) == Inputs().key(false, false)));
  CHECK(!(Inputs().key(true, false, true) == Inputs().key(true, false)));
  MOVES(true, false, true, in.known.z0 = mem + 40);
  MOVES(true, false, true, in.known.e0 = mem + 40);
  MOVES(true, false, true, in.known.mask = mem + 40);
  MOVES(true, false, true, in.known.q_a = mem + 40);
  MOVES(true, false, true, in.known.q_e = mem + 40);
  MOVES(true, false, true, in.known.S = 4);
  // 6. the three rules never share a key
  {
    const GraphKey ddpm = Inputs().key(false, false), ddim = Inputs().key(true, false), dpm = Inputs().key(false, true);
    CHECK(!(ddpm == ddim) && !(ddpm == dpm) && !(ddim == dpm));
    CHECK(StepMode{}.rule() == Rule::DDPM);
  }
  // 7. the generation of the context's time table
  CHECK(!(Inputs().key(false, false, false, false, 2) == Inputs().key(false, false)));
  CHECK(!(Inputs().key(true, false, false, false, 2) == Inputs().key(true, false)));
  // 8. the padding of the optional structs stays out of the key
  for (int mode = 0; mode < 3; ++mode) {
    const bool ddim = mode == 1, dpm = mode == 2;
    CHECK(Inputs(0xAA).key(ddim, dpm, true, true) == Inputs(0).key(ddim, dpm, true, true));
  }
  // 9. composed guidance: its own keys, member by member; the step args it replaces stay out
  for (int mode = 0; mode < 3; ++mode) {
    const bool ddim = mode == 1, dpm = mode == 2;
    const GraphKey plain = Inputs().key(ddim, dpm), composed = Inputs().key(ddim, dpm, false, false, 1, true);
    CHECK(!(composed == plain));
    auto moved_c = [&](auto&& edit) {
      Inputs in;
      edit(in);
      return !(in.key(ddim, dpm, false, false, 1, true) == composed);
    };
    CHECK(moved_c([](Inputs& in) { in.comp.K = 3; }));
    CHECK(moved_c([](Inputs& in) { in.comp.y = imem + 5; }));
    CHECK(moved_c([](Inputs& in) { in.comp.vals = mem + 40; }));
    CHECK(moved_c([](Inputs& in) { in.comp.mask = mem + 40; }));
    CHECK(moved_c([](Inputs& in) { in.comp.weight = mem + 40; }));
    CHECK(!moved_c([](Inputs& in) { in.a.y = imem + 5; }));
    CHECK(!moved_c([](Inputs& in) { in.a.vals = nullptr; }));
    CHECK(!moved_c([](Inputs& in) { in.a.mask = mem + 40; }));
    CHECK(!moved_c([](Inputs& in) { in.a.guidance = 0.f; }));
    CHECK(!moved_c([](Inputs& in) { in.a.null_label = 0; }));
    CHECK(moved_c([](Inputs& in) { in.a.x_in = in.a.x_out = mem + 40; }));  // (what it still reads stays in)
    CHECK(moved_c([](Inputs& in) { in.a.sample_offset = 0; }));
    // a plain key's compose member is all zero, and so are the other paths'
    const dmx_compose zero{};
    for (int kn = 0; kn < 2; ++kn)
      for (int gd = 0; gd < 2; ++gd) {
        const GraphKey k = Inputs(0xAA).key(ddim, dpm, kn != 0, gd != 0);
        CHECK(std::memcmp(&k.comp, &zero, sizeof(zero)) == 0);
      }
    // its padding stays out of the key
    CHECK(Inputs(0xAA).key(ddim, dpm, true, true, 1, true) == Inputs(0).key(ddim, dpm, true, true, 1, true));
  }
  // 10. geometry guidance: its own keys, member by member; all zero when absent
  for (int mode = 0; mode < 3; ++mode) {
    const bool ddim = mode == 1, dpm = mode == 2;
    const GraphKey plain = Inputs().key(ddim, dpm), guided = Inputs().key(ddim, dpm, false, false, 1, false, true);
    CHECK(!(guided == plain));
    CHECK(!(guided == Inputs().key(ddim, dpm, false, false, 1, true)));  // (nor a composed loop's)
    auto moved_g = [&](auto&& edit) {
      Inputs in;
      edit(in);
      return !(in.key(ddim, dpm, false, false, 1, false, true) == guided);
    };
    CHECK(moved_g([](Inputs& in) { in.geom.scale = mem + 40; }));
    CHECK(moved_g([](Inputs& in) { in.geom.sig = mem + 40; }));
    CHECK(moved_g([](Inputs& in) { in.geom.S = 4; }));
    // the step args it reads stay in: the target is the call's own condition
    CHECK(moved_g([](Inputs& in) { in.a.y = imem + 5; }));
    CHECK(moved_g([](Inputs& in) { in.a.vals = mem + 40; }));
    CHECK(moved_g([](Inputs& in) { in.a.mask = mem + 40; }));
    CHECK(moved_g([](Inputs& in) { in.a.guidance = 2.f; }));
    // with a known region it is still its own key
    CHECK(!(Inputs().key(ddim, dpm, true, false, 1, false, true) == Inputs().key(ddim, dpm, true)));
    // a key without it holds zeros there, whatever the other paths
    const dmx_geom_guide zero{};
    for (int kn = 0; kn < 2; ++kn)
      for (int cp = 0; cp < 2; ++cp) {
        const GraphKey k = Inputs(0xAA).key(ddim, dpm, kn != 0, true, 1, cp != 0);
        CHECK(std::memcmp(&k.geom, &zero, sizeof(zero)) == 0);
      }
    // its padding stays out of the key
    CHECK(Inputs(0xAA).key(ddim, dpm, true, false, 1, false, true) == Inputs(0).key(ddim, dpm, true, false, 1, false, true));
  }
  CHECK(StepMode{}.geom == nullptr);
  // 11. perturbed-attention guidance: a perturbed key is not the composed key; both members count;
  // all zero when absent
  for (int mode = 0; mode < 3; ++mode) {
    const bool ddim = mode == 1, dpm = mode == 2;
    const GraphKey composed = Inputs().key(ddim, dpm, false, false, 1, true);
    const GraphKey perturbed = Inputs().key(ddim, dpm, false, false, 1, true, false, true);
    CHECK(!(perturbed == composed));
    CHECK(!(perturbed == Inputs().key(ddim, dpm)));
    auto moved_p = [&](auto&& edit) {
      Inputs in;
      edit(in);
      return !(in.key(ddim, dpm, false, false, 1, true, false, true) == perturbed);
    };
    CHECK(moved_p([](Inputs& in) { in.perturb.blocks = 63; }));
    CHECK(moved_p([](Inputs& in) { in.perturb.branches = 6; }));
    CHECK(moved_p([](Inputs& in) { in.comp.weight = mem + 40; }));  // (the composition stays in)
    CHECK(!moved_p([](Inputs& in) { in.a.guidance = 0.f; }));
    // with a known region it is still its own key
    CHECK(!(Inputs().key(ddim, dpm, true, false, 1, true, false, true) == Inputs().key(ddim, dpm, true, false, 1, true)));
    // a key without it holds zeros there, whatever the other paths
    const dmx_perturb zero{};
    for (int kn = 0; kn < 2; ++kn)
      for (int cp = 0; cp < 2; ++cp)
        for (int gg = 0; gg < 2; ++gg) {
          const GraphKey k = Inputs(0xAA).key(ddim, dpm, kn != 0, true, 1, cp != 0, gg != 0);
          CHECK(std::memcmp(&k.perturb, &zero, sizeof(zero)) == 0);
        }
    CHECK(Inputs(0xAA).key(ddim, dpm, true, true, 1, true, false, true) ==
          Inputs(0).key(ddim, dpm, true, true, 1, true, false, true));
  }
  CHECK(StepMode{}.perturb == nullptr);
  // 12. DDIM inversion: a rule of its own with a key of its own, member by member, src included; neither the
  // DDPM tables, T nor the seed are in it; it combines with no other part
  {
    const GraphKey inverted = Inputs().inv_key();
    CHECK(Inputs().inv_mode().rule() == Rule::INVERT);
    CHECK(StepMode{}.invert == nullptr && StepMode{}.invert_conflict() == nullptr);
    CHECK(!(inverted == Inputs().key(false, false)) && !(inverted == Inputs().key(true, false)) &&
          !(inverted == Inputs().key(false, true)));
    auto moved_i = [&](auto&& edit) {
      Inputs in;
      edit(in);
      return !(in.inv_key() == inverted);
    };
    CHECK(moved_i([](Inputs& in) { in.inv.t_map = imem + 5; }));
    CHECK(moved_i([](Inputs& in) { in.inv.i_x = mem + 40; }));
    CHECK(moved_i([](Inputs& in) { in.inv.i_e = mem + 40; }));
    CHECK(moved_i([](Inputs& in) { in.inv.adv = amem + 1; }));
    CHECK(moved_i([](Inputs& in) { in.inv.src = mem + 40; }));
    CHECK(moved_i([](Inputs& in) { in.inv.S = 4; }));
    CHECK(!moved_i([](Inputs& in) { in.a.c1 = mem + 40; }));
    CHECK(!moved_i([](Inputs& in) { in.a.c2 = nullptr; }));
    CHECK(!moved_i([](Inputs& in) { in.a.sd = mem + 40; }));
    CHECK(!moved_i([](Inputs& in) { in.a.T = 0; }));
    CHECK(!moved_i([](Inputs& in) { in.a.seed = 8; }));
    CHECK(moved_i([](Inputs& in) { in.a.x_in = in.a.x_out = mem + 40; }));  // (what it still reads stays in)
    CHECK(moved_i([](Inputs& in) { in.a.guidance = 0.f; }));
    CHECK(moved_i([](Inputs& in) { in.a.y = imem + 5; }));
    CHECK(!(Inputs().inv_key(2) == inverted));
    // the tables of a DDIM schedule at the same addresses are still another key: the member differs
    {
      Inputs in;
      in.ddim.t_map = in.inv.t_map;
      in.ddim.k_e = in.inv.i_x;
      in.ddim.k_a = in.inv.i_e;
      CHECK(!(in.key(true, false) == inverted));
    }
    // every other key holds zeros there, and the inversion key holds zeros in every other member
    const dmx_invert_sched zero{};
    for (int mode = 0; mode < 3; ++mode)
      for (int kn = 0; kn < 2; ++kn)
        for (int cp = 0; cp < 2; ++cp) {
          const GraphKey k = Inputs(0xAA).key(mode == 1, mode == 2, kn != 0, true, 1, cp != 0, false, cp != 0);
          CHECK(std::memcmp(&k.inv, &zero, sizeof(zero)) == 0);
        }
    const dmx_ddim_sched zd{};
    const dmx_dpm_sched zp{};
    const dmx_known_sched zk{};
    CHECK(std::memcmp(&inverted.sched, &zd, sizeof(zd)) == 0 && std::memcmp(&inverted.dpm, &zp, sizeof(zp)) == 0 &&
          std::memcmp(&inverted.known, &zk, sizeof(zk)) == 0);
    // its padding stays out of the key
    CHECK(Inputs(0xAA).inv_key() == Inputs(0).inv_key());
    // alone, or beside a guidance struct with rescale 0, it is legal; beside anything else it is refused with a message
    CHECK(Inputs().inv_mode().invert_conflict() == nullptr);
    CHECK(Inputs().inv_mode(4).invert_conflict() == nullptr);
    CHECK(make_graph_key(Inputs().a, Inputs().inv_mode(4), 1) == inverted);
    const int others[6] = {1, 2, 3, 5, 6, 7};
    for (int with : others) {
      const Inputs in;
      const char* why = in.inv_mode(with).invert_conflict();
      CHECK(why != nullptr && std::strlen(why) > 0);
    }
    {
      Inputs in;
      in.gd.rescale = 0.5f;
      CHECK(in.inv_mode(4).invert_conflict() != nullptr);
    }
  }
  // 13. feature caching: no request, interval <= 1 and kind PLAIN leave every key what it was; a cached
  // loop has one key per step kind, which hold neither the interval nor the phase; the step kinds follow
  // (phase + k) % interval; the excluded parts are refused with a message
  for (int mode = 0; mode < 3; ++mode) {
    const bool ddim = mode == 1, dpm = mode == 2;
    Inputs in;
    const GraphKey plain = in.key(ddim, dpm, true, true);
    StepMode sm{ddim ? &in.ddim : nullptr, dpm ? &in.dpm : nullptr, &in.known, &in.gd};
    CHECK(plain.cache_kind == 0);
    dmx_cache c{1, 0};
    sm.cache = &c;
    CHECK(!sm.cached() && sm.cache_kind(0) == StepMode::PLAIN && sm.cache_conflict() == nullptr);
    CHECK(make_graph_key(in.a, sm, 1) == plain);
    CHECK(make_graph_key(in.a, sm, 1, StepMode::REFRESH) == plain);  // (a kind without a request is no kind)
    c.interval = 0;
    CHECK(!sm.cached() && make_graph_key(in.a, sm, 1, StepMode::REUSE) == plain);
    c.interval = -3;
    CHECK(!sm.cached() && make_graph_key(in.a, sm, 1, StepMode::REUSE) == plain);
    c.interval = 3;
    CHECK(sm.cached());
    const GraphKey refresh = make_graph_key(in.a, sm, 1, StepMode::REFRESH);
    const GraphKey reuse = make_graph_key(in.a, sm, 1, StepMode::REUSE);
    CHECK(!(refresh == plain) && !(reuse == plain) && !(refresh == reuse));
    CHECK(refresh.cache_kind == (int)StepMode::REFRESH && reuse.cache_kind == (int)StepMode::REUSE);
    c.interval = 5;
    c.phase = 2;
    CHECK(make_graph_key(in.a, sm, 1, StepMode::REFRESH) == refresh);
    CHECK(make_graph_key(in.a, sm, 1, StepMode::REUSE) == reuse);
    // everything else the loop's graphs hold stays in both keys
    in.known.z0 = mem + 40;
    CHECK(!(make_graph_key(in.a, sm, 1, StepMode::REFRESH) == refresh));
    CHECK(!(make_graph_key(in.a, sm, 1, StepMode::REUSE) == reuse));
    CHECK(!(make_graph_key(Inputs().a, sm, 2, StepMode::REUSE) == reuse));
  }
  {
    const Inputs in;
    dmx_cache c{3, 0};
    StepMode sm;
    sm.cache = &c;
    const int want3[7] = {1, 2, 2, 1, 2, 2, 1};
    for (int k = 0; k < 7; ++k) CHECK((int)sm.cache_kind(k) == want3[k]);
    c.phase = 2;
    const int want32[5] = {2, 1, 2, 2, 1};
    for (int k = 0; k < 5; ++k) CHECK((int)sm.cache_kind(k) == want32[k]);
    c.interval = 2;
    c.phase = 2147483647;  // (the sum does not overflow)
    CHECK(sm.cache_kind(0) == StepMode::REUSE && sm.cache_kind(1) == StepMode::REFRESH);
    CHECK(StepMode{}.cache == nullptr && StepMode{}.cache_kind(0) == StepMode::PLAIN && !StepMode{}.cached());
    // alone, or beside a schedule, a known region and a rescale, it is legal; beside the rest it is refused
    c = dmx_cache{3, 0};
    CHECK(sm.cache_conflict() == nullptr);
    sm.ddim = &in.ddim;
    sm.known = &in.known;
    sm.gd = &in.gd;
    CHECK(sm.cache_conflict() == nullptr);
    const char* words[4] = {"composition", "geometry", "perturbed", "inversion"};
    for (int part = 0; part < 4; ++part) {
      StepMode bad;
      bad.cache = &c;
      if (part == 0) bad.comp = &in.comp;
      if (part == 1) bad.geom = &in.geom;
      if (part == 2) bad.perturb = &in.perturb;
      if (part == 3) bad.invert = &in.inv;
      const char* why = bad.cache_conflict();
      CHECK(why != nullptr && std::strstr(why, "cached") != nullptr && std::strstr(why, words[part]) != nullptr);
      c.interval = 1;  // without a request there is nothing to refuse
      CHECK(bad.cache_conflict() == nullptr);
      c.interval = 3;
    }
  }
  if (fails == 0) std::puts("step_mode_check: ok");
  return fails == 0 ? 0 : 1;
}
