// Host side of the front-end units (tfra_frontend.hip, tfra_unique.hip, tfra_combine.hip, tfra_partition.hip, tfra_sorted.hip)
// and of the plan's layout (tfra_csr.hip): scratch is carved out of one allocation in 256-byte steps, and a layout is
// written ONCE — as a function of a Carver — and run twice, dry for the bytes it needs and over the buffer for its pointers.
#pragma once
#include <cstddef>

#include "tfra_host.h"

namespace tfra {

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// carve helper; p == nullptr: dry (take returns null, `used` counts all the same)
struct Carver {
  unsigned char* p = nullptr;
  size_t used = 0;
  template <class T> T* take(size_t n) {
    T* r = p ? reinterpret_cast<T*>(p + used) : nullptr;
    used += align_up(n * sizeof(T));
    return r;
  }
};

// the workspace's scratch laid out by `layout(Carver&)`: sized by a dry run, grown if need be, then carved
template <class Layout>
int carve(tfra_workspace* ws, hipStream_t s, Layout&& layout) {
  Carver dry;
  layout(dry);
  const int rc = ws->ensure(dry.used, s);
  if (rc) return rc;
  Carver c{(unsigned char*)ws->buf};
  layout(c);
  return TFRA_OK;
}

}  // namespace tfra
