// Stand-alone check of the optimizer's host tables (dmx/csrc/optim_table.h).
// Host C++ only; build it with the host compiler and sanitizers and run it:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       -I diffusion-model_amd/dmx/csrc tools/optim_table_check.cpp -o optim_table_check && ./optim_table_check
// The pointers are dummies: the rows hold their values and nothing dereferences them.
#include <cstdio>
#include <cstring>
#include <vector>

#include "optim_table.h"

using namespace dmx;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);       \
      ++fails;                                                    \
    }                                                             \
  } while (0)

// Every element of every tensor lies in exactly one chunk and no chunk reaches past its tensor.
static void check_cover(const std::vector<int64_t>& numel) {
  const std::vector<dmx_optim_chunk> c = optim_chunks((int)numel.size(), numel.data());
  std::vector<std::vector<unsigned char>> hit;
  for (int64_t n : numel) hit.emplace_back((size_t)n, 0);
  int last_tensor = -1;
  int64_t last_end = 0;
  for (const dmx_optim_chunk& k : c) {
    CHECK(k.tensor >= 0 && k.tensor < (int)numel.size());
    if (k.tensor < 0 || k.tensor >= (int)numel.size()) return;
    CHECK(k.len >= 1 && k.len <= DMX_OPTIM_CHUNK);
    CHECK(k.offset >= 0 && k.offset % DMX_OPTIM_CHUNK == 0);
    CHECK(k.offset + k.len <= numel[k.tensor]);
    if (k.offset < 0 || k.len < 1 || k.offset + k.len > numel[k.tensor]) return;
    CHECK(k.tensor > last_tensor || (k.tensor == last_tensor && k.offset == last_end));  // tensor order, no gap
    last_tensor = k.tensor;
    last_end = k.offset + k.len;
    for (int64_t i = k.offset; i < k.offset + k.len; ++i) ++hit[k.tensor][(size_t)i];
  }
  for (const auto& h : hit)
    for (unsigned char x : h) CHECK(x == 1);
}

static float mem[64] __attribute__((aligned(16)));

int main() {
  const int64_t C = DMX_OPTIM_CHUNK;
  check_cover({0, 1, 3, 4, C - 1, C, C + 1, 2 * C + 5});
  check_cover({});
  check_cover({0, 0, 0});
  check_cover({7 * C, 0, 1});
  CHECK(optim_chunks(1, std::vector<int64_t>{0}.data()).empty());
  CHECK(optim_chunks(1, std::vector<int64_t>{2 * C + 5}.data()).size() == 3);
  {  // offsets past 2^31 elements stay exact (table only: nothing that large is allocated)
    const int64_t big = ((int64_t)1 << 31) + 5;
    const std::vector<dmx_optim_chunk> c = optim_chunks(1, &big);
    CHECK((int64_t)c.size() == big / C + 1);
    CHECK(c.back().offset == ((int64_t)1 << 31) && c.back().len == 5);
  }

  dmx_optim_tensor r;
  std::memset(&r, 0xFF, sizeof(r));  // (flags and reserved arrive dirty)
  r.p = mem;
  r.g = mem + 4;
  r.m = mem + 8;
  r.v = mem + 12;
  r.ema = nullptr;
  r.flags = DMX_OPTIM_DECOUPLED;
  CHECK(optim_row(r).flags == (DMX_OPTIM_ALIGNED | DMX_OPTIM_DECOUPLED) && optim_row(r).reserved == 0);
  r.flags = DMX_OPTIM_ALIGNED;  // the caller's bit is not trusted
  r.g = mem + 5;
  CHECK(optim_row(r).flags == 0);
  r.g = mem + 4;
  r.ema = mem + 17;
  CHECK(optim_row(r).flags == 0);
  r.ema = mem + 16;
  CHECK(optim_row(r).flags == DMX_OPTIM_ALIGNED);
  r.p = mem + 2;  // 8-byte aligned only
  CHECK(optim_row(r).flags == 0);
  r.p = mem;

  CHECK(optim_row_error(r, 4) == nullptr);
  r.g = nullptr;  // skipped: nothing else is looked at
  r.m = nullptr;
  CHECK(optim_row_error(r, 4) == nullptr);
  r.g = mem + 4;
  CHECK(optim_row_error(r, 4) != nullptr);
  CHECK(optim_row_error(r, 0) == nullptr);  // an empty tensor runs no block
  r.m = mem + 8;
  r.g = (const float*)((const char*)mem + 18);
  CHECK(optim_row_error(r, 4) != nullptr);  // not 4-byte aligned
  r.g = mem;
  CHECK(optim_row_error(r, 4) != nullptr);  // aliases p

  if (fails == 0) std::printf("optim_table_check: ok\n");
  return fails == 0 ? 0 : 1;
}
