// The optimizer's host tables (include/dmx.h dmx_optim): the chunk table of a parameter set and the
// checks of a step's per-tensor rows.  Host C++ only — no HIP type or call appears here — so both
// are exercised by a stand-alone program as well (tools/optim_table_check.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "dmx.h"

namespace dmx {

// Tensor i of numel[i] elements becomes ceil(numel[i] / DMX_OPTIM_CHUNK) chunks in tensor order, each
// starting at a multiple of DMX_OPTIM_CHUNK (so a chunk of a 16-byte aligned tensor starts 16-byte
// aligned) and all but a tensor's last one full.  An empty tensor has no chunk.  Offsets are 64-bit:
// one tensor may pass 2^31 elements; a chunk's length never passes DMX_OPTIM_CHUNK.
inline std::vector<dmx_optim_chunk> optim_chunks(int n, const int64_t* numel) {
  std::vector<dmx_optim_chunk> out;
  for (int i = 0; i < n; ++i)
    for (int64_t off = 0; off < numel[i]; off += DMX_OPTIM_CHUNK) {
      const int64_t left = numel[i] - off;
      out.push_back(dmx_optim_chunk{off, i, (int32_t)(left < DMX_OPTIM_CHUNK ? left : DMX_OPTIM_CHUNK)});
    }
  return out;
}

inline bool optim_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The row as the kernels read it: the 16-byte bit is derived from the pointers here, never taken
// from the caller (ema counts only where it is set).
inline dmx_optim_tensor optim_row(dmx_optim_tensor r) {
  const bool al = optim_aligned16(r.p) && optim_aligned16(r.g) && optim_aligned16(r.m) && optim_aligned16(r.v) &&
                  optim_aligned16(r.ema);
  r.flags = (r.flags & ~(uint32_t)DMX_OPTIM_ALIGNED) | (al ? DMX_OPTIM_ALIGNED : 0u);
  r.reserved = 0;
  return r;
}

// null: the row can be run; else what is wrong with it.  A row without a gradient is skipped by the
// kernels whatever else it holds.
inline const char* optim_row_error(const dmx_optim_tensor& r, int64_t numel) {
  if (r.g == nullptr || numel == 0) return nullptr;
  if (r.p == nullptr || r.m == nullptr || r.v == nullptr) return "optimizer row with a gradient needs p, m and v";
  if (((uintptr_t)r.p | (uintptr_t)r.g | (uintptr_t)r.m | (uintptr_t)r.v | (uintptr_t)r.ema) & 3u)
    return "optimizer tensors must be 4-byte aligned";
  if ((const float*)r.p == r.g || (const float*)r.m == r.g || (const float*)r.v == r.g || (const float*)r.ema == r.g)
    return "the gradient buffer is read only and may not alias p, m, v or ema";
  return nullptr;
}

}  // namespace dmx
