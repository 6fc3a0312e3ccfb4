// Stand-alone check of the v-prediction entries' argument checks (dmx/csrc/prediction_args.h): what
// dmx_model_set_prediction, dmx_model_set_prediction_x0, dmx_pred_to_eps and dmx_pred_split refuse with
// DMX_E_ARG before any launch, and the timestep range of a v-model's step or loop.  Host C++ only; build it with the host compiler and
// sanitizers and run it:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       -I diffusion-model_amd/dmx/csrc tools/prediction_args_check.cpp -o prediction_args_check && ./prediction_args_check
// (or through hipcc with -Xarch_host -fsanitize=address,undefined).  The pointers are dummies: the
// checks look at them and at the numbers, and dereference nothing.
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "prediction_args.h"

using namespace dmx;

// the feature is additive: no struct of the ABI changes size
static_assert(sizeof(dmx_noise_args) == 160, "dmx_noise_args changed size");
static_assert(sizeof(dmx_objective_args) == 128, "dmx_objective_args changed size");
static_assert(sizeof(dmx_step_args) == 144, "dmx_step_args changed size");

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);       \
      ++fails;                                                    \
    }                                                             \
  } while (0)

static float f32[64];
static float g32[64];
static int64_t i64[8];

int main() {
  const int imin = std::numeric_limits<int>::min(), imax = std::numeric_limits<int>::max();
  {  // dmx_model_set_prediction
    CHECK(set_prediction_error(DMX_PRED_V, f32, g32, 1000) == nullptr);
    CHECK(set_prediction_error(DMX_PRED_V, f32, g32, 1) == nullptr);
    CHECK(set_prediction_error(DMX_PRED_V, f32, f32, imax) == nullptr);  // (one table twice: the caller's business)
    for (int kind : {-1, 2, 7, imin, imax}) CHECK(set_prediction_error(kind, f32, g32, 1000) != nullptr);
    CHECK(set_prediction_error(DMX_PRED_V, nullptr, g32, 1000) != nullptr);
    CHECK(set_prediction_error(DMX_PRED_V, f32, nullptr, 1000) != nullptr);
    CHECK(set_prediction_error(DMX_PRED_V, nullptr, nullptr, 1000) != nullptr);
    for (int T : {0, -1, imin}) CHECK(set_prediction_error(DMX_PRED_V, f32, g32, T) != nullptr);
    // eps reads neither table nor T
    CHECK(set_prediction_error(DMX_PRED_EPS, nullptr, nullptr, 0) == nullptr);
    CHECK(set_prediction_error(DMX_PRED_EPS, f32, nullptr, -5) == nullptr);
  }
  {  // dmx_pred_to_eps
    auto ok = [&](const float* out, const float* x, const int64_t* t, int ts, const float* po, const float* px, int T,
                  int n, int c, int h, int w, const float* eo) {
      return pred_to_eps_error(out, x, t, ts, po, px, T, n, c, h, w, eo) == nullptr;
    };
    CHECK(ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, f32 + 32));
    CHECK(ok(f32, g32, i64, 0, f32, g32, 1, 1, 1, 1, 1, f32));   // eps_out may alias out
    CHECK(ok(f32, g32, i64, 3, f32, g32, 1000, 2, 3, 9, 7, f32)); // a strided t, any c*h*w
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, g32));  // not x
    CHECK(!ok(nullptr, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, f32));
    CHECK(!ok(f32, nullptr, i64, 1, f32, g32, 1000, 2, 4, 2, 2, f32));
    CHECK(!ok(f32, g32, nullptr, 1, f32, g32, 1000, 2, 4, 2, 2, f32));
    CHECK(!ok(f32, g32, i64, 1, nullptr, g32, 1000, 2, 4, 2, 2, f32));
    CHECK(!ok(f32, g32, i64, 1, f32, nullptr, 1000, 2, 4, 2, 2, f32));
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, nullptr));
    for (int T : {0, -1, imin}) CHECK(!ok(f32, g32, i64, 1, f32, g32, T, 2, 4, 2, 2, f32));
    for (int ts : {-1, imin}) CHECK(!ok(f32, g32, i64, ts, f32, g32, 1000, 2, 4, 2, 2, f32));
    for (int bad : {0, -1, imin}) {
      CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, bad, 4, 2, 2, f32));
      CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, bad, 2, 2, f32));
      CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, bad, 2, f32));
      CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, bad, f32));
    }
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 1 << 15, 1 << 15, 1 << 15, 1 << 15, f32));  // 2^60 elements
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, imax, imax, imax, imax, f32));              // (no integer overflow)
    CHECK(ok(f32, g32, i64, 1, f32, g32, 1000, 1 << 10, 1 << 10, 1 << 9, 1 << 9, f32));     // 2^38: the largest power
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 1 << 10, 1 << 10, 1 << 10, 1 << 9, f32));   // 2^39
  }
  {  // dmx_model_set_prediction_x0: four tables and T >= 1
    CHECK(set_prediction_x0_error(f32, g32, f32 + 16, g32 + 16, 1000) == nullptr);
    CHECK(set_prediction_x0_error(f32, g32, f32, g32, 1) == nullptr);
    CHECK(set_prediction_x0_error(f32, g32, f32, g32, imax) == nullptr);
    CHECK(set_prediction_x0_error(nullptr, g32, f32, g32, 1000) != nullptr);
    CHECK(set_prediction_x0_error(f32, nullptr, f32, g32, 1000) != nullptr);
    CHECK(set_prediction_x0_error(f32, g32, nullptr, g32, 1000) != nullptr);
    CHECK(set_prediction_x0_error(f32, g32, f32, nullptr, 1000) != nullptr);
    CHECK(set_prediction_x0_error(nullptr, nullptr, nullptr, nullptr, 1000) != nullptr);
    for (int T : {0, -1, imin}) CHECK(set_prediction_x0_error(f32, g32, f32, g32, T) != nullptr);
    // DMX_PRED_V_X0 has an entry of its own: it is no kind of dmx_model_set_prediction
    CHECK(set_prediction_error(DMX_PRED_V_X0, f32, g32, 1000) != nullptr);
  }
  {  // dmx_pred_split
    auto ok = [&](const float* out, const float* x, const int64_t* t, int ts, const float* po, const float* px, int T,
                  int n, int c, int h, int w, const float* x0o, const float* eo) {
      return pred_split_error(out, x, t, ts, po, px, T, n, c, h, w, x0o, eo) == nullptr;
    };
    CHECK(ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, g32 + 32, f32 + 32));
    CHECK(ok(f32, g32, i64, 0, f32, g32, 1, 1, 1, 1, 1, g32 + 32, f32));    // eps_out may alias out
    CHECK(ok(f32, g32, i64, 3, f32, g32, 1000, 2, 3, 9, 7, g32 + 32, f32));  // a strided t, any c*h*w
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, g32 + 32, g32));  // eps_out: not x
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, g32, f32 + 32));  // x0_out: not x
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, f32, f32 + 32));  // x0_out: not out
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, f32 + 32, f32 + 32));  // not each other
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, f32, f32));
    CHECK(!ok(nullptr, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, g32 + 32, f32));
    CHECK(!ok(f32, nullptr, i64, 1, f32, g32, 1000, 2, 4, 2, 2, g32 + 32, f32));
    CHECK(!ok(f32, g32, nullptr, 1, f32, g32, 1000, 2, 4, 2, 2, g32 + 32, f32));
    CHECK(!ok(f32, g32, i64, 1, nullptr, g32, 1000, 2, 4, 2, 2, g32 + 32, f32));
    CHECK(!ok(f32, g32, i64, 1, f32, nullptr, 1000, 2, 4, 2, 2, g32 + 32, f32));
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, nullptr, f32));
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, 2, g32 + 32, nullptr));
    for (int T : {0, -1, imin}) CHECK(!ok(f32, g32, i64, 1, f32, g32, T, 2, 4, 2, 2, g32 + 32, f32));
    for (int ts : {-1, imin}) CHECK(!ok(f32, g32, i64, ts, f32, g32, 1000, 2, 4, 2, 2, g32 + 32, f32));
    for (int bad : {0, -1, imin}) {
      CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, bad, 4, 2, 2, g32 + 32, f32));
      CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, bad, 2, 2, g32 + 32, f32));
      CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, bad, 2, g32 + 32, f32));
      CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 2, 4, 2, bad, g32 + 32, f32));
    }
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, imax, imax, imax, imax, g32 + 32, f32));             // (no integer overflow)
    CHECK(ok(f32, g32, i64, 1, f32, g32, 1000, 1 << 10, 1 << 10, 1 << 9, 1 << 9, g32 + 32, f32));    // 2^38
    CHECK(!ok(f32, g32, i64, 1, f32, g32, 1000, 1 << 10, 1 << 10, 1 << 10, 1 << 9, g32 + 32, f32));  // 2^39
  }
  {  // the schedule's largest timestep against the stored T
    CHECK(prediction_range_error(1000, 1000) == nullptr);
    CHECK(prediction_range_error(1, 1000) == nullptr);
    CHECK(prediction_range_error(0, 1) == nullptr);  // (below 1: clamped like every table read, not this check's)
    CHECK(prediction_range_error(1001, 1000) != nullptr);
    CHECK(prediction_range_error(std::numeric_limits<int64_t>::max(), imax) != nullptr);
    CHECK(prediction_range_error(2, 1) != nullptr);
  }
  if (fails == 0) std::printf("prediction_args_check: ok\n");
  return fails == 0 ? 0 : 1;
}
