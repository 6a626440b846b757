// Who owns the device memory behind a handle's pointer fields.  The fields stay the raw pointers every launch site reads; a DevMem
// beside them records which fields (their addresses: "slots") own a block, and is the only code that allocates or frees one.
//
//   - a field is non-null only once its block exists completely (allocated and, where asked for, zero-filled);
//   - a group (alloc_all) comes into being as a whole or not at all: a failure leaves every field it would have filled null, every
//     field that was there before untouched, and nothing allocated;
//   - replace() builds the new block, contents included, before it gives up the old one;
//   - release_all() frees whatever the registered fields hold at that moment (fields may have swapped their pointers since).
//
// The allocator is a parameter (three functions returning 0 on success), so the rule compiles with plain g++ and no HIP header:
// csrc/mds_api.hip binds it to the HIP runtime, tests/devmem_main.cpp to a malloc that can be told to fail.  A non-zero status of the
// allocator is returned to the caller as it is.  Not thread-safe, like the handle it lives in.
#pragma once
#include <stddef.h>
#include <string.h>

#include <vector>

namespace mds {

struct DevAllocator {
  int (*alloc)(void** out, size_t bytes);       // on failure *out stays as it was
  void (*free)(void* p);
  int (*zero)(void* p, size_t bytes);
};

class DevMem {
 public:
  // one field of a group: where the pointer lives, how many bytes it gets, whether they start as zeros
  struct Want {
    void** field;
    size_t bytes;
    bool zeroed;
    template <typename P> Want(P** f, size_t b, bool z = false) : field(slot(f)), bytes(b), zeroed(z) {}
  };

  explicit DevMem(DevAllocator a) : a_(a) {}
  ~DevMem() { release_all(); }
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;

  // Allocates the fields of the group that are null (a field that already has a block is left alone).  All of them or none.
  int alloc_all(const std::vector<Want>& group) {
    for (const Want& w : group) note(w.field);
    std::vector<void*> fresh(group.size(), nullptr);
    int rc = 0;
    for (size_t k = 0; k < group.size() && rc == 0; ++k) {
      if (get(group[k].field)) continue;
      rc = a_.alloc(&fresh[k], group[k].bytes);
      if (rc == 0 && group[k].zeroed && fresh[k]) rc = a_.zero(fresh[k], group[k].bytes);
    }
    for (size_t k = 0; k < group.size(); ++k) {
      if (!fresh[k]) continue;
      if (rc == 0) set(group[k].field, fresh[k]);
      else a_.free(fresh[k]);
    }
    return rc;
  }
  template <typename P> int alloc(P** field, size_t bytes, bool zeroed = false) { return alloc_all({Want(field, bytes, zeroed)}); }

  // A new block of `bytes` for a field that may hold one: fill(new block) -> 0 writes its contents while the old block still serves;
  // only then the old block is freed and the field points to the new one.  Any failure: the field and the old block stay.
  template <typename P, typename Fill> int replace(P** field, size_t bytes, Fill&& fill) {
    void** s = slot(field);
    note(s);
    void* fresh = nullptr;
    int rc = a_.alloc(&fresh, bytes);
    if (rc != 0) return rc;
    rc = fill(fresh);
    if (rc != 0) {
      if (fresh) a_.free(fresh);
      return rc;
    }
    release(field);
    set(s, fresh);
    return 0;
  }

  template <typename P> void release(P** field) {
    void** s = slot(field);
    if (void* p = get(s)) a_.free(p);
    set(s, nullptr);
  }
  void release_all() {
    for (void** s : slots_) release(s);
  }

 private:
  // the fields are void*, double*, int*: their common representation is read and written as bytes
  template <typename P> static void** slot(P** f) { return reinterpret_cast<void**>(f); }
  static void* get(void** s) {
    void* p;
    memcpy(&p, s, sizeof(p));
    return p;
  }
  static void set(void** s, void* p) { memcpy(s, &p, sizeof(p)); }
  void note(void** s) {
    for (void** k : slots_)
      if (k == s) return;
    slots_.push_back(s);
  }

  DevAllocator a_;
  std::vector<void**> slots_;
};

}  // namespace mds
