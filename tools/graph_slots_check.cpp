// Stand-alone check of the graph slots' least-recently-used bookkeeping (dmx/csrc/graph_slots.h).
// Host C++ only; build it with the host compiler and sanitizers and run it:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I diffusion-model_amd/dmx/csrc tools/graph_slots_check.cpp -o graph_slots_check && ./graph_slots_check
// The values stand for the graph handles the engine owns: heap blocks here, so a slot released
// without freeing its value, or freed twice, is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "graph_slots.h"

struct Key {
  int a;
  char pad_after;  // (padding follows: keys are compared bytewise, as the engine's are)
  double b;
  bool operator==(const Key& o) const { return std::memcmp(this, &o, sizeof(Key)) == 0; }
};
struct Val {
  int* handle;
};
using Slots = dmx::LruSlots<Key, Val, 4>;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);       \
      ++fails;                                                    \
    }                                                             \
  } while (0)

static Key key(int a) {
  Key k;
  std::memset(&k, 0, sizeof(k));
  k.a = a;
  k.b = 0.5 * a;
  return k;
}

static void drop(Slots& s, Slots::Slot* sl) {  // the engine's drop_slot
  delete sl->val.handle;
  s.release(sl);
}

// The engine's lookup-or-capture: -> the slot, *captured = a new value was made.
static Slots::Slot* use(Slots& s, int a, bool* captured) {
  const Key k = key(a);
  Slots::Slot* sl = s.find(k);
  *captured = sl == nullptr;
  if (sl == nullptr) {
    sl = s.victim();
    drop(s, sl);
    sl->val.handle = new int(a);
    s.claim(sl, k);
  }
  return sl;
}

int main() {
  Slots s;
  bool cap = false;
  CHECK(s.live() == 0 && s.find(key(1)) == nullptr);
  // guided, unguided, guided again, rescaled: 1, 1, 0, 1 captures
  const int order[] = {1, 2, 1, 3};
  const bool want[] = {true, true, false, true};
  for (int i = 0; i < 4; ++i) {
    Slots::Slot* sl = use(s, order[i], &cap);
    CHECK(cap == want[i] && *sl->val.handle == order[i]);
  }
  CHECK(s.live() == 3);
  use(s, 4, &cap);
  CHECK(cap && s.live() == 4);
  // a fifth key evicts the least recently used one: key 2 (1 was touched after it)
  use(s, 5, &cap);
  CHECK(cap && s.live() == 4);
  CHECK(s.find(key(2)) == nullptr);
  CHECK(s.find(key(1)) != nullptr && s.find(key(3)) != nullptr && s.find(key(4)) != nullptr);
  // find() refreshes: after touching 1, 3, 4 above the oldest is 5
  use(s, 6, &cap);
  CHECK(cap && s.find(key(5)) == nullptr && s.find(key(1)) != nullptr);
  // a key that differs only in its second member is another key
  Key k = key(1);
  k.b = 7.0;
  CHECK(s.find(k) == nullptr);
  // dropping everything (arena moved, precision changed): nothing is found, every value freed once
  for (Slots::Slot& sl : s.slot) drop(s, &sl);
  CHECK(s.live() == 0 && s.find(key(1)) == nullptr);
  use(s, 1, &cap);
  CHECK(cap && s.live() == 1);
  for (Slots::Slot& sl : s.slot) drop(s, &sl);
  if (fails == 0) std::puts("graph_slots_check: ok");
  return fails == 0 ? 0 : 1;
}
