// The memory of a handle that outlives a call: one block of `count` elements of T and its capacity in one move-only object, so that the two cannot
// disagree and no block is without an owner.  Mem is the kind of memory: `status`, an integer type whose zero is success, and
//   static status alloc(void** p, size_t bytes);   static status free(void* p);
// vxba_dev.hpp has the real ones (vxu::Dev<T>: device memory, vxu::Pin<T>: pinned host memory, and the mapped, coherent and fine-grained kinds).  Nothing of HIP is included here: the host check
// (tests/hostmath/buf_hostcheck.cpp) runs this header over a policy that refuses allocations.
//
// RULE: a Buf frees in its destructor, so it is for handle members and locals.  An object with static storage (vxba_downsample.hip's per-device table,
// Lease's slots, and the Arena they hold) keeps its explicit release(): its destructor would run after the HIP runtime has shut down.
#pragma once
#include <cstddef>

namespace vxu {

template <class T, class Mem>
class Buf {
 public:
  using status = typename Mem::status;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~Buf() { release(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }         // a kernel argument or a copy's end; the owner itself cannot be copied
  size_t capacity() const { return cap_; }   // elements

  // Room for `need` elements.  Nothing happens while they fit.  Otherwise the old block is freed first -- the caller has waited for whatever still
  // used it -- and one of `grown` elements (the call site's growth rule; at least `need`) takes its place: the contents are not kept.  When the
  // allocation is refused the owner is empty, pointer and capacity together, and the error is returned.
  status reserve(size_t need, size_t grown) {
    if (need <= cap_) return status();
    release();
    if (grown < need) grown = need;
    void* p = nullptr;
    const status e = Mem::alloc(&p, grown * sizeof(T));
    if (e != status()) return e;
    p_ = (T*)p; cap_ = grown;
    return e;
  }
  status reserve(size_t need) { return reserve(need, need); }
  void release() {
    if (p_) Mem::free(p_);
    p_ = nullptr; cap_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace vxu
