// Stand-alone driver of the handle's memory-ownership rule (multidronesim_amd/csrc/mds_devmem.hpp) for tests/test_devmem_cpu.py: built
// with g++ (-fsanitize=address,undefined), run as a subprocess.  No HIP anywhere: the allocator is a malloc that counts its live blocks,
// fills fresh memory with a non-zero byte and fails its k-th alloc or k-th zero call on request.  Exit status 0 and "ok" on stdout when
// every statement below holds; the first one that does not is printed with its line and ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../multidronesim_amd/csrc/mds_devmem.hpp"

namespace {

constexpr unsigned char kPoison = 0xA5;
constexpr int kFailed = -7;                     // the fake's failure status: DevMem must hand it back unchanged

long g_live = 0, g_alloc_calls = 0, g_zero_calls = 0, g_free_calls = 0;
long g_fail_alloc_at = 0, g_fail_zero_at = 0;   // 1-based index of the call that fails, counted from arm(); 0: none

int fake_alloc(void** out, size_t bytes) {
  if (++g_alloc_calls == g_fail_alloc_at) return kFailed;
  void* p = malloc(bytes ? bytes : 1);
  if (!p) abort();
  memset(p, kPoison, bytes);
  *out = p;
  ++g_live;
  return 0;
}
void fake_free(void* p) {
  ++g_free_calls;
  --g_live;
  free(p);
}
int fake_zero(void* p, size_t bytes) {
  if (++g_zero_calls == g_fail_zero_at) return kFailed;
  memset(p, 0, bytes);
  return 0;
}
const mds::DevAllocator kFake = {fake_alloc, fake_free, fake_zero};

void arm(long fail_alloc_at, long fail_zero_at) {
  g_alloc_calls = g_zero_calls = 0;
  g_fail_alloc_at = fail_alloc_at;
  g_fail_zero_at = fail_zero_at;
}

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("devmem_main.cpp:%d: CHECK(%s) failed\n", __LINE__, #cond); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

bool all_bytes(const void* p, size_t n, unsigned char v) {
  for (size_t k = 0; k < n; ++k)
    if (((const unsigned char*)p)[k] != v) return false;
  return true;
}

// five fields of the types the handle has
struct Fields {
  void* a = nullptr;
  double* b = nullptr;
  int* c = nullptr;
  void* d[2] = {nullptr, nullptr};
  void* at(int k) const { return k == 0 ? a : k == 1 ? (void*)b : k == 2 ? (void*)c : d[k - 3]; }
  bool is_null(int k) const { return at(k) == nullptr; }
};
constexpr size_t kBytes[5] = {24, 8 * sizeof(double), 5 * sizeof(int), 1, 100};

std::vector<mds::DevMem::Want> group_of(Fields& f, int n, unsigned zero_mask) {
  std::vector<mds::DevMem::Want> g;
  for (int k = 0; k < n; ++k) {
    const bool z = (zero_mask >> k) & 1;
    if (k == 0) g.push_back({&f.a, kBytes[0], z});
    if (k == 1) g.push_back({&f.b, kBytes[1], z});
    if (k == 2) g.push_back({&f.c, kBytes[2], z});
    if (k >= 3) g.push_back({&f.d[k - 3], kBytes[k], z});
  }
  return g;
}

// A group of n, field `pre` (or none: -1) allocated beforehand with contents of its own.  The fail_alloc-th alloc or fail_zero-th zero call
// of the group fails: every field the call would have filled is null afterwards, the earlier one and its contents are as they were, and
// exactly as many blocks are live as before the call.
void group_failure(int n, int pre, unsigned zero_mask, long fail_alloc, long fail_zero) {
  const long live0 = g_live;
  {
    Fields f;
    mds::DevMem mem(kFake);
    void* before = nullptr;
    if (pre >= 0) {
      arm(0, 0);
      CHECK(mem.alloc_all({group_of(f, n, 0)[pre]}) == 0);
      before = f.at(pre);
      CHECK(before != nullptr);
      memset(before, 0x3C, kBytes[pre]);
    }
    const long live_before = g_live;
    arm(fail_alloc, fail_zero);
    CHECK(mem.alloc_all(group_of(f, n, zero_mask)) == kFailed);
    CHECK(g_live == live_before);
    for (int k = 0; k < n; ++k) {
      if (k == pre) {
        CHECK(f.at(k) == before);
        CHECK(all_bytes(before, kBytes[k], 0x3C));
      } else {
        CHECK(f.is_null(k));
      }
    }
    // the same call once the allocator works again: the whole group exists, the earlier field still untouched
    arm(0, 0);
    CHECK(mem.alloc_all(group_of(f, n, zero_mask)) == 0);
    CHECK(g_live == live_before + n - (pre >= 0 ? 1 : 0));
    for (int k = 0; k < n; ++k) {
      CHECK(!f.is_null(k));
      if (k == pre) CHECK(f.at(k) == before && all_bytes(before, kBytes[k], 0x3C));
      else CHECK(all_bytes(f.at(k), kBytes[k], ((zero_mask >> k) & 1) ? 0 : kPoison));
    }
  }                                             // ~DevMem frees what is left
  CHECK(g_live == live0);
}

void groups() {
  for (int n = 1; n <= 5; ++n) {
    const unsigned all = (1u << n) - 1;
    for (int pre = -1; pre < n; ++pre) {
      const int fresh = n - (pre >= 0 ? 1 : 0);             // blocks the call has to allocate
      const unsigned pre_bit = pre >= 0 ? 1u << pre : 0;
      for (long k = 1; k <= fresh; ++k) {
        group_failure(n, pre, 0, k, 0);                     // the k-th allocation fails, nothing zero-filled
        group_failure(n, pre, all, k, 0);                   // ... every field zero-filled
        group_failure(n, pre, all, 0, k);                   // the k-th zero-fill fails
        group_failure(n, pre, 0x15 & all, k, 0);            // ... fields 0, 2, 4 zero-filled only
      }
      long zeros = 0;
      for (int j = 0; j < n; ++j) zeros += ((0x15 & all & ~pre_bit) >> j) & 1;
      for (long k = 1; k <= zeros; ++k) group_failure(n, pre, 0x15 & all, 0, k);
      if (fresh == 0) {                                     // a group that is already there allocates nothing and succeeds
        Fields f;
        mds::DevMem mem(kFake);
        arm(0, 0);
        CHECK(mem.alloc(&f.a, kBytes[0]) == 0);
        arm(1, 1);
        CHECK(mem.alloc_all(group_of(f, 1, 1)) == 0 && g_alloc_calls == 0 && g_zero_calls == 0);
      }
    }
  }
}

void single_alloc() {
  Fields f;
  mds::DevMem mem(kFake);
  arm(0, 0);
  CHECK(mem.alloc(&f.b, kBytes[1], true) == 0 && f.b && all_bytes(f.b, kBytes[1], 0));        // zeroed: all zero bytes
  CHECK(mem.alloc(&f.c, kBytes[2]) == 0 && f.c && all_bytes(f.c, kBytes[2], kPoison));        // (not zeroed: as the allocator left it)
  CHECK(g_live == 2);
  // a second alloc on a field that has its block allocates nothing, zero-fills nothing and keeps the pointer and the contents
  double* const b0 = f.b;
  f.b[3] = 1.5;
  arm(0, 0);
  CHECK(mem.alloc(&f.b, 4 * kBytes[1], true) == 0);
  CHECK(g_alloc_calls == 0 && g_zero_calls == 0 && f.b == b0 && f.b[3] == 1.5 && g_live == 2);
  // a failed alloc / zero-fill of a single field: null, nothing live
  arm(1, 0);
  CHECK(mem.alloc(&f.a, kBytes[0], true) == kFailed && !f.a && g_live == 2);
  arm(0, 1);
  CHECK(mem.alloc(&f.a, kBytes[0], true) == kFailed && !f.a && g_live == 2);
}

void replacing() {
  Fields f;
  mds::DevMem mem(kFake);
  arm(0, 0);
  // on a null field replace is an allocation
  auto nothing = [](void*) { return 0; };
  CHECK(mem.replace(&f.b, 4 * sizeof(double), nothing) == 0 && f.b && g_live == 1);
  for (int k = 0; k < 4; ++k) f.b[k] = 10.0 + k;
  double* const old = f.b;
  // success: the fill sees the new block while the field still shows the old one; then the old block is freed, once
  const long frees0 = g_free_calls;
  int rc = mem.replace(&f.b, 6 * sizeof(double), [&](void* fresh) {
    CHECK(fresh != old && f.b == old && f.b[2] == 12.0 && g_live == 2);
    for (int k = 0; k < 6; ++k) ((double*)fresh)[k] = 20.0 + k;
    return 0;
  });
  CHECK(rc == 0 && f.b != old && f.b[5] == 25.0);
  CHECK(g_free_calls == frees0 + 1 && g_live == 1);
  // failure in the allocation: field, contents and live count untouched, fill never called
  double* const cur = f.b;
  arm(1, 0);
  bool called = false;
  rc = mem.replace(&f.b, 64, [&](void*) { called = true; return 0; });
  CHECK(rc == kFailed && !called && f.b == cur && f.b[5] == 25.0 && g_live == 1);
  // failure in the fill (an upload that fails): the new block is freed, the old one stays
  arm(0, 0);
  rc = mem.replace(&f.b, 64, [&](void* fresh) { memset(fresh, 0, 64); return -4; });
  CHECK(rc == -4 && f.b == cur && f.b[0] == 20.0 && f.b[5] == 25.0 && g_live == 1);
  CHECK(mem.replace(&f.b, 16, nothing) == 0 && f.b != nullptr && g_live == 1);
}

void releasing() {
  {
    Fields f;
    mds::DevMem mem(kFake);
    arm(0, 0);
    CHECK(mem.alloc_all(group_of(f, 5, 0x1f)) == 0 && g_live == 5);
    mem.release(&f.c);
    CHECK(!f.c && g_live == 4);
    mem.release(&f.c);                           // twice: nothing happens
    CHECK(!f.c && g_live == 4);
    mem.release(&f.d[1]);
    // two fields that have traded their blocks since (the double-buffered state): each block is still freed once
    void* t = f.a; f.a = f.d[0]; f.d[0] = t;
    mem.release_all();                           // after some fields were released by hand
    CHECK(g_live == 0);
    for (int k = 0; k < 5; ++k) CHECK(f.is_null(k));
    mem.release_all();                           // twice
    CHECK(g_live == 0);
    // the owner goes on working after release_all
    CHECK(mem.alloc(&f.a, 8) == 0 && g_live == 1);
    int* never = nullptr;
    mem.release(&never);                         // a field it has never seen, null: nothing happens
    CHECK(g_live == 1);
  }
  CHECK(g_live == 0);                            // the destructor released the rest
}

}  // namespace

int main() {
  groups();
  single_alloc();
  replacing();
  releasing();
  CHECK(g_live == 0);
  printf("ok\n");
  return 0;
}
