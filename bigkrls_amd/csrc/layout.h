// The packed layout of a post-estimation entry (csrc/margeff.hip, inteff.hip, grpeff.hip, pdep.hip, condeff.hip): one
// workspace slot carved into regions, the first of them staged in the context's pinned buffer in the same order and
// uploaded by ONE copy. An entry declares every region once, in order; the offsets, the upload size, the slot size and
// the read-back size all follow from that one list. Pure pointer arithmetic: no HIP call, nothing but <cstdint> -- what
// tests/layout_check.cpp compiles on its own. Internal and header-only, as hostprep.h.
#pragma once
#include <cstdint>

namespace bk {

// a region of the slot, in doubles from its start. A region aliased to another is that region's value (no length of its
// own): `const Region Zs = h_newdata ? L.up(u * p) : Xs;`
struct Region {
  int64_t off = 0, len = 0;
};

class Layout {
 public:
  // uploaded: staged on the host at the same offset. Every uploaded region precedes all others (valid() otherwise false).
  Region up(int64_t doubles) {
    if (total_ != up_) ok_ = false;
    const Region r = add(doubles);
    up_ = total_;
    return r;
  }
  // `count` records of T, uploaded, rounded up to whole doubles
  template <class T>
  Region up_records(int64_t count) { return up((count * (int64_t)sizeof(T) + 7) / 8); }
  // device only
  Region dev(int64_t doubles) { return add(doubles); }
  // read back. The regions read back by ONE copy, from down_off(), must be adjacent (down_adjacent()).
  Region down(int64_t doubles) {
    if (down_ == 0) down_off_ = total_;
    if (doubles > 0 && down_off_ + down_ != total_) adjacent_ = false;
    down_ += doubles;
    return add(doubles);
  }

  int64_t up_doubles() const { return up_; }
  int64_t down_doubles() const { return down_; }
  int64_t down_off() const { return down_off_; }
  int64_t slot_doubles() const { return total_ + 64; }   // (the slack every entry has always asked for)
  int64_t total_doubles() const { return total_; }       // the regions alone (csrc/s2plan.h: slots sized without slack)
  bool valid() const { return ok_; }
  bool down_adjacent() const { return adjacent_; }

  void bind_device(void* base) { dev_ = (double*)base; }
  void bind_host(double* pinned) { pin_ = pinned; }
  template <class T = double>
  T* d(Region r) const { return (T*)(dev_ + r.off); }
  template <class T = double>
  T* h(Region r) const { return (T*)(pin_ + r.off); }     // uploaded regions only
  double* pinned() const { return pin_; }

 private:
  Region add(int64_t doubles) {
    if (doubles < 0) ok_ = false;
    const Region r{total_, doubles};
    total_ += doubles;
    return r;
  }
  int64_t total_ = 0, up_ = 0, down_ = 0, down_off_ = 0;
  bool ok_ = true, adjacent_ = true;
  double *dev_ = nullptr, *pin_ = nullptr;
};

}  // namespace bk
