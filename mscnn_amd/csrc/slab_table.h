// Bookkeeping of the InnerProduct stream-K slab buffers (gemm.hip: reserve_slabs): which buffer belongs to which stream.
// Plain C++ without a HIP call, so that a host program can exercise it (tests/slab_table_main.cpp).
//
// One table per (host thread, device).  A slot ties one stream handle to one buffer; calls on the same stream are ordered by the
// stream and share a buffer, calls on different streams may be in flight at once and never do.  When every slot is taken the
// least recently used one is handed out again: the caller frees its buffer (hipFree waits for the device, so no kernel of the
// evicted stream still reads it) and allocates a new one.
#pragma once
#include <cstddef>

namespace mscnn {

constexpr int kSlabSlots = 4;

struct SlabSlot {
  const void* stream = nullptr;      // the key; meaningful while live
  void* p = nullptr;                 // the caller's buffer (nullptr: none yet, or freed)
  size_t bytes = 0;
  unsigned long long used = 0;       // the table's clock at the slot's last hand-out
  bool live = false;
};

struct SlabTable {
  SlabSlot slot[kSlabSlots];
  unsigned long long clock = 0;
};

// The slot of `stream`: its own if it has one, else a slot never used, else the least recently used one, re-keyed to `stream`.
// In the last case the slot still holds the evicted stream's buffer (p, bytes), which is the caller's to free or to grow; which
// case it was is returned in *evicted (may be null).
inline SlabSlot* slab_slot(SlabTable& t, const void* stream, bool* evicted = nullptr) {
  if (evicted) *evicted = false;
  ++t.clock;
  SlabSlot* pick = nullptr;
  for (SlabSlot& s : t.slot) {
    if (s.live && s.stream == stream) { s.used = t.clock; return &s; }
    if (!s.live) { if (!pick || pick->live) pick = &s; }
    else if (!pick || (pick->live && s.used < pick->used)) pick = &s;
  }
  if (pick->live && evicted) *evicted = true;
  pick->live = true; pick->stream = stream; pick->used = t.clock;
  return pick;
}

}  // namespace mscnn
