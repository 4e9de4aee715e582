// vxu::Buf (voxel-slam_amd/csrc/vxba_buf.hpp) over a memory policy that records the live blocks and refuses the k-th allocation: one scripted life
// of a handle's buffers for every k, from "never" down to the first allocation.  A stand-alone program, built with the address and undefined-behaviour
// sanitizers by tests/test_dev_buf_cpu.py; the blocks are real malloc blocks, written over their whole capacity, so the sanitizer sees an owner that
// reports more than it holds.  One line per k on stdout; any broken promise ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "../../voxel-slam_amd/csrc/vxba_buf.hpp"

namespace {

[[noreturn]] void broken(const char* what, int line) {
  std::printf("FAILED line %d: %s\n", line, what);
  std::exit(1);
}
#define CHECK(c) do { if (!(c)) broken(#c, __LINE__); } while (0)

struct Fake {
  using status = int;
  static std::set<void*> live;
  static int allocs, refuse_at, frees;      // refuse_at 0: never
  static status alloc(void** p, size_t bytes) {
    CHECK(bytes > 0);
    if (++allocs == refuse_at) { *p = nullptr; return 2; }
    *p = std::malloc(bytes);
    CHECK(*p && live.insert(*p).second);
    return 0;
  }
  static status free(void* p) {
    if (live.erase(p) != 1) broken("a block is freed twice, or freed without being live", __LINE__);
    std::free(p);
    ++frees;
    return 0;
  }
};
std::set<void*> Fake::live;
int Fake::allocs = 0, Fake::refuse_at = 0, Fake::frees = 0;

struct Rec { double a[3]; int k; };      // 28 -> 32 bytes: an element that is no power-of-two multiple of a word
using B = vxu::Buf<Rec, Fake>;

void inv(const B& b) {
  CHECK((b.get() == nullptr) == (b.capacity() == 0));
  CHECK((Rec*)b == b.get());
  if (b.get()) CHECK(Fake::live.count(b.get()) == 1);
}

// one reserve and everything it promises: nothing happens while the elements fit; a growth is one allocation of max(need, grown) elements after the
// old block went; a refused growth leaves the owner empty and returns the error
void reserve(B& b, size_t need, size_t grown) {
  const int before = Fake::allocs;
  const bool fits = need <= b.capacity();
  Rec* const old = b.get();
  const size_t old_cap = b.capacity(), held = Fake::live.size();
  const int s = b.reserve(need, grown);
  inv(b);
  if (fits) {
    CHECK(s == 0 && Fake::allocs == before && b.get() == old && b.capacity() == old_cap && Fake::live.size() == held);
    return;
  }
  CHECK(Fake::allocs == before + 1);
  if (Fake::allocs == Fake::refuse_at) {
    CHECK(s != 0 && b.get() == nullptr && b.capacity() == 0 && Fake::live.size() == held - (old ? 1 : 0));
  } else {
    CHECK(s == 0 && b.capacity() == (grown > need ? grown : need) && b.capacity() >= 1 && Fake::live.size() == held - (old ? 1 : 0) + 1);
    std::memset((void*)b.get(), 0xab, b.capacity() * sizeof(Rec));
  }
}

void life() {
  {
    B a;
    inv(a);
    CHECK(a.reserve(0) == 0 && a.get() == nullptr && Fake::allocs == 0);      // nothing asked, nothing held
    reserve(a, 100, 100 + 100 / 4 + 64);                                      // 1. with growth
    reserve(a, 10, 10);                                                       // 2. smaller: no allocation (unless 1. was refused)
    reserve(a, 1000, 2048);                                                   // 3. larger
    reserve(a, 2048, 2048);                                                   //    exactly the capacity
    Rec* const pa = a.get();
    const size_t ca = a.capacity();
    B b(std::move(a));                                                        // 4. move-construct: the source is empty
    inv(a); inv(b);
    CHECK(a.get() == nullptr && b.get() == pa && b.capacity() == ca);
    B c;
    reserve(c, 50, 50);
    const size_t held = Fake::live.size(), c_held = c.get() ? 1 : 0;
    c = std::move(b);                                                         //    move-assign onto a target that holds a block: that block goes
    inv(b); inv(c);
    CHECK(b.get() == nullptr && c.get() == pa && c.capacity() == ca && Fake::live.size() == held - c_held);
    B d;
    d = std::move(c);                                                         //    and onto an empty one
    inv(c); inv(d);
    CHECK(c.get() == nullptr && d.get() == pa && d.capacity() == ca);
    reserve(a, 3, 3);                                                         //    a moved-from owner is an empty owner
    reserve(b, 5, 2);                                                         //    a growth rule below the need: the need
    std::vector<B> v;                                                         // 5. a vector of owners that reallocates
    for (size_t i = 0; i < 9; i++) {
      v.emplace_back();
      reserve(v.back(), i + 1, 2 * i + 3);
      for (const B& e : v) inv(e);
    }
    size_t owned = 0;
    for (const B* e : {&a, &b, &c, &d}) owned += e->get() ? 1 : 0;
    for (const B& e : v) owned += e.get() ? 1 : 0;
    CHECK(owned == Fake::live.size());                                        // no block without an owner, none owned twice
    const size_t gone = v[2].get() ? 1 : 0;
    v.erase(v.begin() + 2);                                                   //    shifts by move-assignment onto owners that hold blocks
    for (const B& e : v) inv(e);
    CHECK(Fake::live.size() == owned - gone);
    d.release();                                                              // 6. release twice
    inv(d);
    CHECK(d.get() == nullptr);
    d.release();
    inv(d);
    reserve(d, 7, 7);                                                         //    and a released owner serves again
  }                                                                           // 7. scope exit
  CHECK(Fake::live.empty());
}

int run(int refuse_at) {
  Fake::allocs = Fake::frees = 0;
  Fake::refuse_at = refuse_at;
  life();
  return Fake::allocs;
}

}  // namespace

int main() {
  const int n = run(0);
  std::printf("refuse never: %d allocations, %d frees, 0 live\n", n, Fake::frees);
  for (int k = n; k >= 1; k--) {
    const int m = run(k);
    CHECK(m >= k);
    std::printf("refuse %d: %d allocations, %d frees, 0 live\n", k, m, Fake::frees);
  }
  return 0;
}
