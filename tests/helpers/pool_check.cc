// pool_check.cc -- DevPool (crossscalepatchmatch_amd/csrc/cspm_pool.h) over a fake allocator that counts its live blocks and fails the
// k-th call on request (tests/test_pool.py builds and runs this stand-alone, once more under AddressSanitizer and UBSan).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <type_traits>
#include <utility>

#include "cspm_pool.h"

using cspm::DevPool;
static_assert(!std::is_copy_constructible<DevPool>::value && !std::is_copy_assignable<DevPool>::value, "two owners of one allocation");

namespace {

std::map<void *, size_t> g_live;  // base -> the size asked for
int g_calls = 0, g_fail_at = 0, g_frees = 0, g_bad_frees = 0;
size_t g_last_bytes = 0;
const int kStatus = 2;  // what a failing call answers: the pool hands it back as it is

int fake_alloc(void **p, size_t bytes) {
  g_last_bytes = bytes;
  if (++g_calls == g_fail_at) return kStatus;
  *p = malloc(bytes);
  g_live[*p] = bytes;
  return 0;
}
void fake_free(void *p) {
  ++g_frees;
  if (!g_live.erase(p)) ++g_bad_frees;  // not a base, or freed twice
  else free(p);
}
size_t live_bytes() {
  size_t s = 0;
  for (const auto &e : g_live) s += e.second;
  return s;
}
void reset() { g_calls = g_fail_at = g_frees = g_bad_frees = 0; }

int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);       \
      ++g_failed;                                                           \
    }                                                                       \
  } while (0)
// at the end of every case: nothing live, no free of a non-base or of a base twice
#define CASE_END() CHECK(g_live.empty() && g_bad_frees == 0)

struct Slots {
  double *a = nullptr;
  unsigned char *b = nullptr;
  int *c = nullptr;
  const unsigned int *d = nullptr;
};
int get_all(DevPool &p, Slots &s) {
  int rc;
  if ((rc = p.get(&s.a, 10)) || (rc = p.get(&s.b, 7)) || (rc = p.get(&s.c, 3)) || (rc = p.get(&s.d, 5))) return rc;
  return 0;
}
const size_t kAll = 10 * sizeof(double) + 7 + 3 * sizeof(int) + 5 * sizeof(unsigned int);

void case_get_is_idempotent() {
  reset();
  DevPool p(fake_alloc, fake_free);
  Slots s;
  CHECK(p.bytes() == 0);
  CHECK(get_all(p, s) == 0 && g_calls == 4 && g_live.size() == 4);
  CHECK(s.a && s.b && s.c && s.d);
  CHECK(p.bytes() == kAll && live_bytes() == kAll);
  double *a = s.a;
  CHECK(get_all(p, s) == 0 && g_calls == 4 && s.a == a);  // every slot is set: no allocator call
  CHECK(p.bytes() == kAll);
  p.release();
  CHECK(g_frees == 4 && !s.a && !s.b && !s.c && !s.d && p.bytes() == 0);
  p.release();  // an empty pool: nothing
  CHECK(g_frees == 4);
  CASE_END();
}

void case_failure_and_retry() {
  for (int k = 1; k <= 4; ++k) {
    reset();
    DevPool p(fake_alloc, fake_free);
    Slots s;
    g_fail_at = k;
    CHECK(get_all(p, s) == kStatus);
    CHECK(g_calls == k && (int)g_live.size() == k - 1);  // the earlier entries stay owned
    void *slots[4] = {s.a, s.b, s.c, (void *)s.d};
    for (int i = 0; i < 4; ++i) CHECK((slots[i] != nullptr) == (i < k - 1));  // the failing slot and the ones behind it are null
    CHECK(p.bytes() == live_bytes());
    double *a = s.a;
    CHECK(get_all(p, s) == 0);  // the whole sequence again: exactly the missing ones
    CHECK(g_calls == k + (4 - (k - 1)) && g_live.size() == 4 && p.bytes() == kAll);
    if (k > 1) CHECK(s.a == a);
    p.release();
    CHECK(g_frees == 4 && !s.a && !s.b && !s.c && !s.d);
    CASE_END();
  }
}

void case_release_goes_by_base() {
  reset();
  DevPool p(fake_alloc, fake_free);
  unsigned char *x = nullptr, *y = nullptr;
  double *vol = nullptr;
  CHECK(p.get(&x, 16) == 0 && p.get(&y, 16) == 0);
  unsigned char *x0 = x, *y0 = y;
  std::swap(x, y);  // the median filter's double buffer
  CHECK(p.get(&x, 16) == 0 && p.get(&y, 16) == 0 && g_calls == 2);  // both still set
  CHECK(p.get(&vol, 12, 4) == 0 && g_last_bytes == 16 * sizeof(double) && g_calls == 3);  // 12 elements behind 4 more
  CHECK(g_live.count(vol - 4) == 1 && g_live.count(vol) == 0);
  vol[-4] = 1.0;
  vol[11] = 2.0;  // both ends are inside the block (the sanitizer build would say otherwise)
  CHECK(p.bytes() == 32 + 16 * sizeof(double));
  p.release();
  CHECK(g_frees == 3 && g_bad_frees == 0 && !x && !y && !vol);
  CHECK(g_live.count(x0) == 0 && g_live.count(y0) == 0);
  CASE_END();
}

void case_add_rewind_drop() {
  reset();
  DevPool p(fake_alloc, fake_free);
  Slots s;
  CHECK(get_all(p, s) == 0);
  const DevPool::Mark m = p.mark();
  double *v0 = (double *)8, *v1 = nullptr;  // add() does not read what the pointer held
  int *kept = nullptr;
  CHECK(p.add(&v0, 100) == 0 && p.add(&v1, 50, 2) == 0 && p.get(&kept, 1) == 0);
  CHECK(g_live.count(v0) == 1 && g_live.count(v1 - 2) == 1);
  CHECK(p.bytes() == kAll + 152 * sizeof(double) + sizeof(int));
  g_fail_at = g_calls + 1;
  double *v2 = (double *)8;
  CHECK(p.add(&v2, 10) == kStatus && v2 == nullptr && p.bytes() == kAll + 152 * sizeof(double) + sizeof(int));
  p.rewind(m);  // only the entries behind the mark, only their slots
  CHECK(g_frees == 3 && g_live.size() == 4 && p.bytes() == kAll && !kept);
  CHECK(v0 && v1 && s.a && s.b && s.c && s.d);  // a pointer add() filled is the caller's to reset
  p.rewind(m);
  CHECK(g_frees == 3);
  p.drop(&s.b);
  CHECK(g_frees == 4 && !s.b && s.a && s.c && s.d && p.bytes() == kAll - 7);
  p.drop(&s.b);  // no entry: nothing
  CHECK(g_frees == 4);
  CHECK(p.get(&s.b, 9) == 0 && p.bytes() == kAll + 2);  // a dropped slot is allocated afresh
  p.release();
  CHECK(g_frees == 8 && !s.a && !s.b && !s.c && !s.d);
  CASE_END();
}

void case_zero_elements_and_destructor() {
  reset();
  Slots s;
  {
    DevPool p(fake_alloc, fake_free);
    CHECK(p.get(&s.a, 0) == 0 && g_last_bytes == sizeof(double) && p.bytes() == sizeof(double));  // n == 0: one element
    CHECK(p.get(&s.c, 0, 3) == 0 && g_last_bytes == 4 * sizeof(int));
    CHECK(p.get(&s.b, 5) == 0);
    CHECK(g_live.size() == 3);
  }  // the destructor releases
  CHECK(g_frees == 3 && !s.a && !s.b && !s.c);
  CASE_END();
}

}  // namespace

int main() {
  case_get_is_idempotent();
  case_failure_and_retry();
  case_release_goes_by_base();
  case_add_rewind_drop();
  case_zero_elements_and_destructor();
  if (g_failed) return 1;
  printf("pool_check ok\n");
  return 0;
}
