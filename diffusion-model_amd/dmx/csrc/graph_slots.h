// Least-recently-used bookkeeping of a model's captured sample-loop graphs (engine.hip): which of a
// few slots holds the graphs of which key, and which slot the next capture replaces.  Host C++
// only — no HIP type or call appears here, the slot's value is opaque — so it is exercised by a
// stand-alone program as well (tools/graph_slots_check.cpp).
#pragma once
#include <cstdint>
#include <cstring>

namespace dmx {

// Key: trivially copyable, compared with ==.  Val: trivially copyable handles the caller owns; a
// slot's value is released by the caller before release() / a new claim().
template <typename Key, typename Val, int N>
struct LruSlots {
  struct Slot {
    Key key;
    Val val;
    uint64_t stamp;
    bool used;
  };
  Slot slot[N];
  uint64_t clock = 0;

  LruSlots() {
    for (Slot& s : slot) {
      std::memset(static_cast<void*>(&s.key), 0, sizeof(Key));
      s.val = Val{};
      s.stamp = 0;
      s.used = false;
    }
  }

  // The slot that holds `key`, now the most recently used one; nullptr: not held.
  Slot* find(const Key& key) {
    for (Slot& s : slot)
      if (s.used && s.key == key) {
        s.stamp = ++clock;
        return &s;
      }
    return nullptr;
  }

  // Where the next key goes: a free slot, else the least recently used one (still `used`: the
  // caller frees what its value owns, then calls release()).
  Slot* victim() {
    Slot* v = nullptr;
    for (Slot& s : slot) {
      if (!s.used) return &s;
      if (v == nullptr || s.stamp < v->stamp) v = &s;
    }
    return v;
  }

  // The slot now holds `key` (bytewise copy: keys compared bytewise keep their zeroed padding).
  void claim(Slot* s, const Key& key) {
    std::memcpy(static_cast<void*>(&s->key), static_cast<const void*>(&key), sizeof(Key));
    s->used = true;
    s->stamp = ++clock;
  }

  void release(Slot* s) {
    s->used = false;
    s->val = Val{};
    s->stamp = 0;
  }

  int live() const {
    int n = 0;
    for (const Slot& s : slot) n += s.used ? 1 : 0;
    return n;
  }
};

}  // namespace dmx
