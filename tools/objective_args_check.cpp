// Stand-alone check of the training objective's argument checks (dmx/csrc/objective_args.h): what
// dmx_train_noise, dmx_objective_loss and dmx_objective_seed refuse with DMX_E_ARG before any launch.
// Host C++ only; build it with the host compiler and sanitizers and run it:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       -I diffusion-model_amd/dmx/csrc tools/objective_args_check.cpp -o objective_args_check && ./objective_args_check
// (or through hipcc with -Xarch_host -fsanitize=address,undefined).  The pointers are dummies: the
// checks look at them and at the numbers, and dereference nothing.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "objective_args.h"

using namespace dmx;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);       \
      ++fails;                                                    \
    }                                                             \
  } while (0)

static float f32[64] __attribute__((aligned(16)));
static int64_t i64[8];
static uint8_t u8[8];
static double f64[8];

static dmx_noise_args good_noise() {
  dmx_noise_args a;
  std::memset(&a, 0, sizeof(a));
  a.z = f32;
  a.sa = f32;
  a.s1 = f32;
  a.T = 1000;
  a.draw = DMX_DRAWS_T | DMX_DRAWS_NOISE | DMX_DRAWS_DROP;
  a.t = i64;
  a.noise = f32;
  a.drop = u8;
  a.cfg_drop_prob = 0.1f;
  a.gd = 12;
  a.y = i64;
  a.vals = f32;
  a.mask = f32;
  a.z_noisy = f32;
  a.y_used = i64;
  a.vals_used = f32;
  a.mask_used = f32;
  a.B = 2;
  a.C = 4;
  a.h = 8;
  a.w = 8;
  return a;
}

static dmx_objective_args good_objective() {
  dmx_objective_args a;
  std::memset(&a, 0, sizeof(a));
  a.eps = f32;
  a.noise = f32;
  a.t = i64;
  a.weight = f32;
  a.T = 1000;
  a.geom = f32;
  a.vals = f32;
  a.mask = f32;
  a.gd = 12;
  a.geom_lambda = 0.5f;
  a.part = f64;
  a.per_sample = f32;
  a.out = f32;
  a.B = 2;
  a.C = 4;
  a.h = 8;
  a.w = 8;
  return a;
}

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  {
    dmx_noise_args a = good_noise();
    CHECK(train_noise_error(&a) == nullptr);
    CHECK(train_noise_error(nullptr) != nullptr);
    a.z = nullptr;
    CHECK(train_noise_error(&a) != nullptr);
    a = good_noise();
    for (int b : {0, -1, std::numeric_limits<int>::min()}) {
      a.B = b;
      CHECK(train_noise_error(&a) != nullptr);
    }
    a = good_noise();
    for (int t : {0, -5}) {
      a.T = t;
      CHECK(train_noise_error(&a) != nullptr);
    }
    a = good_noise();
    for (float p : {-0.1f, 1.5f, nan, inf, -inf}) {
      a.cfg_drop_prob = p;
      CHECK(train_noise_error(&a) != nullptr);
    }
    for (float p : {0.f, 1.f, 0.5f}) {
      a.cfg_drop_prob = p;
      CHECK(train_noise_error(&a) == nullptr);
    }
    a.cfg_drop_prob = 7.f;  // not read when drop is given
    a.draw = DMX_DRAWS_T | DMX_DRAWS_NOISE;
    CHECK(train_noise_error(&a) == nullptr);
    a.drop = nullptr;  // given, none dropped
    CHECK(train_noise_error(&a) == nullptr);
    a.draw = DMX_DRAWS_DROP;
    a.cfg_drop_prob = 0.5f;
    CHECK(train_noise_error(&a) != nullptr);  // a drawn drop has nowhere to go
    a = good_noise();
    for (int d : {-1, 8, 1 << 20}) {
      a.draw = d;
      CHECK(train_noise_error(&a) != nullptr);
    }
    a = good_noise();
    a.C = 0;
    CHECK(train_noise_error(&a) != nullptr);
    a = good_noise();
    a.h = -3;
    CHECK(train_noise_error(&a) != nullptr);
    a = good_noise();
    a.B = a.C = a.h = a.w = 1 << 15;  // 2^60 elements
    CHECK(train_noise_error(&a) != nullptr);
    a = good_noise();
    a.sample_offset = -1;
    CHECK(train_noise_error(&a) != nullptr);
    a.sample_offset = std::numeric_limits<int64_t>::max();
    CHECK(train_noise_error(&a) != nullptr);
    a.draw = 0;  // nothing drawn: the offset is not read
    CHECK(train_noise_error(&a) == nullptr);
    a = good_noise();
    a.sa = nullptr;
    CHECK(train_noise_error(&a) != nullptr);
    a = good_noise();
    a.t = nullptr;
    CHECK(train_noise_error(&a) != nullptr);
    a = good_noise();
    a.z_noisy = nullptr;
    CHECK(train_noise_error(&a) != nullptr);
    a = good_noise();
    a.mask = nullptr;  // vals without mask
    CHECK(train_noise_error(&a) != nullptr);
    a.vals = nullptr;  // neither: fine, gd is not read
    a.gd = -7;
    CHECK(train_noise_error(&a) == nullptr);
    a = good_noise();
    for (int gd : {0, -1, 4097}) {
      a.gd = gd;
      CHECK(train_noise_error(&a) != nullptr);
    }
    a = good_noise();
    a.vals_used = nullptr;
    CHECK(train_noise_error(&a) != nullptr);
    a = good_noise();
    a.y_used = nullptr;
    CHECK(train_noise_error(&a) != nullptr);
    a.y = nullptr;
    CHECK(train_noise_error(&a) == nullptr);
  }
  {
    dmx_objective_args a = good_objective();
    CHECK(objective_error(&a) == nullptr);
    CHECK(objective_error(nullptr) != nullptr);
    CHECK(objective_seed_error(&a, f32, f32, f32) == nullptr);
    CHECK(objective_seed_error(&a, f32, f32, nullptr) == nullptr);
    CHECK(objective_seed_error(&a, nullptr, f32, f32) != nullptr);
    CHECK(objective_seed_error(&a, f32, nullptr, f32) != nullptr);
    CHECK(objective_seed_error(nullptr, f32, f32, f32) != nullptr);
    a.eps = nullptr;
    CHECK(objective_error(&a) != nullptr);
    a = good_objective();
    a.B = 0;
    CHECK(objective_error(&a) != nullptr && objective_seed_error(&a, f32, f32, f32) != nullptr);
    a = good_objective();
    a.w = 0;
    CHECK(objective_error(&a) != nullptr);
    a = good_objective();
    a.t = nullptr;  // a weight table without timesteps
    CHECK(objective_error(&a) != nullptr);
    a.weight = nullptr;
    a.T = 0;
    CHECK(objective_error(&a) == nullptr);
    a = good_objective();
    a.T = 0;
    CHECK(objective_error(&a) != nullptr);
    a = good_objective();
    a.mask = nullptr;
    CHECK(objective_error(&a) != nullptr);
    a = good_objective();
    for (int gd : {0, -1, 4097}) {
      a.gd = gd;
      CHECK(objective_error(&a) != nullptr);
    }
    a.geom = nullptr;  // no geometry term: gd is not read
    CHECK(objective_error(&a) == nullptr);
    CHECK(objective_seed_error(&a, f32, f32, f32) != nullptr);  // d_geom of a term that is not there
    CHECK(objective_seed_error(&a, f32, f32, nullptr) == nullptr);
    a = good_objective();
    for (float l : {-1.f, nan, inf}) {
      a.geom_lambda = l;
      CHECK(objective_error(&a) != nullptr);
    }
    a.geom_lambda = 0.f;
    CHECK(objective_error(&a) == nullptr);
    a = good_objective();
    a.part = nullptr;
    CHECK(objective_error(&a) != nullptr);
    a = good_objective();
    a.out = nullptr;
    CHECK(objective_error(&a) != nullptr);
  }
  {
    const void* p[3] = {f32, f32 + 4, nullptr};
    CHECK(objective_aligned16(256, p, 3));
    CHECK(!objective_aligned16(189, p, 3));
    p[1] = f32 + 1;
    CHECK(!objective_aligned16(256, p, 3));
    CHECK(objective_aligned16(256, p, 1));
  }
  if (fails == 0) std::printf("objective_args_check: ok\n");
  return fails == 0 ? 0 : 1;
}
