// cspm_pool.h -- DevPool: the owner of a set of device allocations that share one lifetime (DESIGN.md "Context memory").
// Plain host C++ without a HIP header: the allocator pair comes in at construction (cspm_api.hip passes hipMalloc / hipFree, the CPU
// test a counting fake).  An entry is {base, slot, bytes}.  `slot` is where the caller keeps its pointer: a set slot means "held", so
// get() is idempotent, and whatever frees the entry nulls the slot.  Freeing goes by `base`, never by the slot's content: a caller may
// swap the contents of two slots of one pool, or keep base + lead in the slot, and every base is still freed exactly once.
// A slot must outlive its entry (a member of the heap-allocated context does, a local does not: add() records none).
#pragma once

#include <cstddef>
#include <cstring>
#include <vector>

namespace cspm {

class DevPool {
 public:
  typedef int (*AllocFn)(void **, size_t);  // 0 = ok, anything else is handed back to the caller as it is
  typedef void (*FreeFn)(void *);
  typedef size_t Mark;

  DevPool(AllocFn alloc, FreeFn free) : alloc_(alloc), free_(free) {}
  DevPool(const DevPool &) = delete;
  DevPool &operator=(const DevPool &) = delete;
  ~DevPool() { release(); }

  // *slot = max(n, 1) elements behind `lead` more, unless it is set already.  On failure nothing is recorded and *slot stays null.
  template <class T>
  int get(T **slot, size_t n, size_t lead = 0) {
    return *slot ? 0 : take(slot, slot, n, lead);
  }
  // the same for a pointer the pool does not remember (a local, a derived field): always allocates, nothing is nulled on release
  template <class T>
  int add(T **out, size_t n, size_t lead = 0) {
    *out = nullptr;
    return take(out, nullptr, n, lead);
  }

  Mark mark() const { return entries_.size(); }
  // frees the entries made since `m`, newest first
  void rewind(Mark m) {
    while (entries_.size() > m) {
      give_back(entries_.back());
      entries_.pop_back();
    }
  }
  // frees the entry of `slot`, if there is one
  template <class T>
  void drop(T **slot) {
    for (size_t i = 0; i < entries_.size(); ++i)
      if (entries_[i].slot == (const void *)slot) {
        give_back(entries_[i]);
        entries_.erase(entries_.begin() + (std::ptrdiff_t)i);
        return;
      }
  }
  void release() { rewind(0); }
  size_t bytes() const { return bytes_; }  // what the live entries asked of the allocator

 private:
  struct Entry {
    void *base;
    void *slot;  // the address of the caller's pointer, or null
    size_t bytes;
  };
  template <class T>
  int take(T **out, void *slot, size_t n, size_t lead) {
    const size_t bytes = ((n ? n : 1) + lead) * sizeof(T);
    void *base = nullptr;
    if (const int rc = alloc_(&base, bytes)) return rc;
    entries_.push_back(Entry{base, slot, bytes});
    bytes_ += bytes;
    *out = (T *)base + lead;
    return 0;
  }
  void give_back(const Entry &e) {
    free_(e.base);
    bytes_ -= e.bytes;
    if (e.slot) std::memset(e.slot, 0, sizeof(void *));  // bytewise: the slot's pointer type is not known here, a null pointer is all zero bits
  }

  AllocFn alloc_;
  FreeFn free_;
  std::vector<Entry> entries_;
  size_t bytes_ = 0;
};

}  // namespace cspm
