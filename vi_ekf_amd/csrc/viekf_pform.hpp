// viekf_pform.hpp -- the form of the covariance P between launches and where the live state is: pure host bookkeeping, no HIP and
// no batch handle, so that tests/cpp/pform_model.cpp can search every state on a CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace viekf {

// P is symmetric and the hot kernels keep only its LOWER triangle current.  Ordered by what a reader can tolerate:
//   Full    all of P valid
//   Lower   stale above the diagonal (left by the fused kernels, the matrix-core propagate and the grouped update: all of them
//           read and write the lower triangle only)
//   Packed  not the column-major matrix but the fused kernel's own register and LDS image (ResPack, viekf_instance_rows.hpp),
//           left by a fused launch for the next one -- whole-batch mode only, never under per-filter live slots or a
//           participation mask (a buffer would end up holding filters of both forms)
enum class PForm { Full, Lower, Packed };

// The conversions that bring the live P to at most a requested form: unpack (Packed -> Lower, the fused kernel's own conversion
// launch) and / or mirror (Lower -> Full, the lower triangle copied up), in that order.
struct PPlan {
  bool unpack, mirror;
};

// The book: the live P's form, which buffer is live -- the batch's own ("home", kHome) or a slot of the history ring, or under
// per-filter mode a slot of its own per filter -- and whether each buffer that can hold a whole batch's P is packed.  Launches
// are uniform over the batch, so all of this is host state.  It changes through the events below only; each is named for what
// the caller has just done to the buffers.  (Hidden visibility: the library exports its C ABI, not this class.)
class __attribute__((visibility("hidden"))) PBook {
 public:
  static constexpr int kHome = -1;

  PForm live_form() const { return live_; }
  int live_slot() const { return live_slot_; }   // kHome, or the ring slot that IS the live state (whole-batch mode)
  bool per_filter() const { return per_filter_; }
  bool packed(int buf) const { return buf < 0 ? home_packed_ : slot_packed_[(size_t)buf] != 0; }
  // the stalest CANONICAL form (<= Lower) any launch of this batch has left
  PForm stalest_canonical() const { return ever_; }

  PPlan plan(PForm at_most) const { return {live_ == PForm::Packed && at_most < PForm::Packed, live_ != PForm::Full && at_most == PForm::Full}; }

  // a launch wrote the live P in form f (in every mode: under per-filter mode no single buffer is live and no flag moves)
  void wrote_live(PForm f) {
    live_ = f;
    set_live_flag(f == PForm::Packed);
    ever_ = std::max(ever_, std::min(f, PForm::Lower));
  }
  // a fused launch stored into ring slot s instead of in place; the caller makes the slot live afterwards (select)
  void wrote_slot(int s, bool packed) {
    slot_packed_[(size_t)s] = packed;
    ever_ = PForm::Lower;
  }
  // the live buffer was copied to ring slot s / ring slot s was copied into the live buffer, as it stands: the form travels
  void saved_to(int s) { slot_packed_[(size_t)s] = live_ == PForm::Packed; }
  void restored_from(int s) { became_live(packed(s)); }
  // ring slot s (or kHome) IS now the live buffer
  void select(int s) {
    live_slot_ = s;
    became_live(packed(s));
  }
  // Single filters moved between canonical buffers, or canonical buffers became (part of) the live state.  A canonical buffer
  // carries no form of its own: it is taken to be as stale as anything canonical this batch ever produced.
  void filters_moved() { live_ = std::min(PForm::Lower, std::max(ever_, live_)); }
  // buffer buf was unpacked in place (a buffer that is not live: the live one is converted through plan / wrote_live)
  void unpacked(int buf) { (buf < 0 ? home_packed_ : slot_packed_[(size_t)buf]) = 0; }
  // every filter's live state is a ring slot of its own from now on (the caller has unpacked every buffer)
  void enter_per_filter() { per_filter_ = true; }
  // The ring now has `depth` fresh slots; whatever was live was copied home first, as it stood.
  void resized(int depth) {
    per_filter_ = false;
    if (live_slot_ >= 0) home_packed_ = live_ == PForm::Packed;
    live_slot_ = kHome;
    slot_packed_.assign((size_t)depth, 0);
  }

 private:
  void set_live_flag(bool packed) {
    if (!per_filter_) (live_slot_ >= 0 ? slot_packed_[(size_t)live_slot_] : home_packed_) = packed;
  }
  void became_live(bool packed) {   // (whole-batch mode: the callers refuse per-filter mode)
    if (packed) live_ = PForm::Packed; else filters_moved();
    set_live_flag(packed);
  }

  PForm live_ = PForm::Full, ever_ = PForm::Full;
  unsigned char home_packed_ = 0;
  std::vector<unsigned char> slot_packed_;   // [ring depth]
  int live_slot_ = kHome;
  bool per_filter_ = false;
};

}  // namespace viekf
