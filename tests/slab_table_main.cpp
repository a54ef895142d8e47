// Host-side exercise of mscnn_amd/csrc/slab_table.h (the bookkeeping behind reserve_slabs of gemm.hip): a stand-alone program,
// built by tests/test_slab_table_cpu.py with -fsanitize=address,undefined.  Buffers are malloc'ed stand-ins for hipMalloc, handled
// the way reserve_slabs handles them, so the sanitizer sees a double free, a leak or a use after free in that protocol.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "slab_table.h"

using namespace mscnn;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

// reserve_slabs without HIP: the slot of `stream`, its buffer grown or (after an eviction) replaced
static unsigned char* reserve(SlabTable& t, const void* stream, size_t need, int* frees) {
  bool evicted = false;
  SlabSlot& w = *slab_slot(t, stream, &evicted);
  if (need > w.bytes || evicted) {
    void* old = w.p;
    w.p = nullptr; w.bytes = 0;
    if (old) { std::free(old); ++*frees; }
    w.p = std::malloc(need);
    w.bytes = need;
  }
  std::memset(w.p, 0x5A, need);      // the whole buffer is the caller's
  return static_cast<unsigned char*>(w.p);
}

static const void* S(uintptr_t i) { return reinterpret_cast<const void*>(i * 0x1000); }      // S(0) is the NULL stream

int main() {
  SlabTable t;
  int frees = 0;

  // one stream: one slot, the same buffer until it has to grow
  unsigned char* a = reserve(t, S(0), 1000, &frees);
  EXPECT(reserve(t, S(0), 1000, &frees) == a && reserve(t, S(0), 10, &frees) == a && frees == 0);
  reserve(t, S(0), 5000, &frees);
  EXPECT(frees == 1);

  // kSlabSlots streams: a buffer each, none shared, none freed
  unsigned char* p[kSlabSlots + 2] = {};
  for (int i = 0; i < kSlabSlots; ++i) p[i] = reserve(t, S(i), 4096, &frees);
  for (int i = 0; i < kSlabSlots; ++i)
    for (int j = 0; j < i; ++j) EXPECT(p[i] != p[j]);
  for (int i = 0; i < kSlabSlots; ++i) EXPECT(reserve(t, S(i), 4096, &frees) == p[i]);
  EXPECT(frees == 1);

  // more streams than slots: the least recently used slot goes, its buffer is freed even where it is large enough
  reserve(t, S(0), 16, &frees);                                     // stream 1 is now the least recently used
  bool evicted = false;
  SlabSlot* victim = nullptr;
  for (SlabSlot& s : t.slot) if (s.live && s.stream == S(1)) victim = &s;
  EXPECT(victim != nullptr);
  reserve(t, S(kSlabSlots), 16, &frees);
  EXPECT(frees == 2 && victim->stream == S(kSlabSlots) && victim->bytes == 16);
  for (SlabSlot& s : t.slot) EXPECT(s.stream != S(1));
  // ... the evicted stream comes back through the slot that is oldest by then (stream 2's), never through a live one it shares
  reserve(t, S(1), 64, &frees);
  EXPECT(frees == 3);
  int live = 0;
  for (SlabSlot& s : t.slot) { live += s.live; EXPECT(s.stream != S(2)); }
  EXPECT(live == kSlabSlots);

  // a rotation over twice as many streams as slots: every call evicts, two streams in the table never share a buffer
  for (int round = 0; round < 50; ++round)
    for (int i = 0; i < 2 * kSlabSlots; ++i) {
      unsigned char* q = reserve(t, S(100 + i), 256 + 16 * i, &frees);
      for (SlabSlot& s : t.slot) EXPECT(!s.live || s.stream == S(100 + i) || s.p != q);
      int same_key = 0;
      for (SlabSlot& s : t.slot) same_key += s.live && s.stream == S(100 + i);
      EXPECT(same_key == 1);
    }

  // the hit path reports no eviction and does not move a slot
  SlabSlot* h0 = slab_slot(t, S(100 + 2 * kSlabSlots - 1), &evicted);
  EXPECT(!evicted && h0 == slab_slot(t, S(100 + 2 * kSlabSlots - 1), nullptr));

  for (SlabSlot& s : t.slot) std::free(s.p);      // (a thread's tables live as long as the thread; here the leak checker watches)
  std::printf(failures ? "slab table: %d FAILED\n" : "slab table ok\n", failures);
  return failures ? 1 : 0;
}
