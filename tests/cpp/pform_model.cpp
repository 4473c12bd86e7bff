// Exhaustive model check of the book that keeps the form of P and the live-state location (vi_ekf_amd/csrc/viekf_pform.hpp),
// stand-alone on a CPU.  Beside the book runs a ground truth: the true form of every buffer that can hold a whole batch's P --
// the batch's own ("home") and the slots of a ring of 2; under per-filter mode the live truth is the worst form over the ring.
// Every event of the C ABI that touches the book is applied in every reachable state, breadth first, the way viekf_dispatch.hpp /
// viekf_capi.hip drive the book; events the ABI refuses in a state are skipped there.  After every event:
//   (a) each buffer's packed flag in the book equals its true packedness
//   (b) in whole-batch mode the live form is Packed exactly when the live buffer truly is
//   (c) live form >= true form (Full < Lower < Packed)
//   (d) in per-filter mode nothing is packed
//   (e) a mirror is never planned on a truly packed buffer
// and a reader that required a form finds the truth at most that form.  (The image is assumed to fit and the tile family to be
// off: otherwise nothing is ever packed.)
#include <array>
#include <cstdio>
#include <deque>
#include <set>
#include <string>
#include <vector>

#include "../../vi_ekf_amd/csrc/viekf_pform.hpp"

using viekf::PBook;
using viekf::PForm;

namespace {

constexpr int H = 2;   // ring depth
constexpr int kHome = PBook::kHome;

struct World {
  PBook book;
  PForm truth[H + 1] = {PForm::Full, PForm::Full, PForm::Full};   // [0] home, [1 + s] ring slot s
  bool mask = false;     // a participation mask is set
  bool tune = true;      // the packed switch
  int violations = 0;    // raised while an event runs
  std::string why;

  PForm& t(int buf) { return truth[buf + 1]; }
  PForm live_truth() {
    if (!book.per_filter()) return t(book.live_slot());
    PForm w = PForm::Full;
    for (int s = 0; s < H; s++) w = std::max(w, t(s));
    return w;
  }
  void set_live_truth(PForm f) {
    if (!book.per_filter()) { t(book.live_slot()) = f; return; }
    if (f == PForm::Packed) bad("packed store under per-filter mode");
    for (int s = 0; s < H; s++) t(s) = f;
  }
  void bad(const char* what) { violations++; if (why.empty()) why = what; }

  // require_P of viekf_dispatch.hpp: executes the book's plan
  void require(PForm at_most) {
    const viekf::PPlan plan = book.plan(at_most);
    if (plan.unpack) {
      if (live_truth() == PForm::Packed) set_live_truth(PForm::Lower);
      book.wrote_live(PForm::Lower);
    }
    if (plan.mirror) {
      if (live_truth() == PForm::Packed) bad("(e) mirror planned on a packed buffer");
      set_live_truth(PForm::Full);
      book.wrote_live(PForm::Full);
    }
    if (live_truth() > at_most) bad("a reader got a form beyond what it required");
  }
  // canonicalize_all: the live P, then every buffer the book says is packed
  void canonicalize_all() {
    require(PForm::Lower);
    for (int buf : {0, 1, kHome})
      if (book.packed(buf)) {
        if (t(buf) == PForm::Packed) t(buf) = PForm::Lower;
        book.unpacked(buf);
      }
  }
  bool keeps_packed() const { return !book.per_filter() && tune; }   // (the rule of keeps_packed(), viekf_dispatch.hpp)

  void check() {
    for (int buf : {kHome, 0, 1})
      if (book.packed(buf) != (t(buf) == PForm::Packed)) bad("(a) packed flag differs from the truth");
    if (!book.per_filter()) {
      if ((book.live_form() == PForm::Packed) != (live_truth() == PForm::Packed)) bad("(b) live form packed differs from the truth");
    } else {
      if (book.live_form() == PForm::Packed || book.packed(kHome) || book.packed(0) || book.packed(1)) bad("(d) packed under per-filter mode");
    }
    if (book.live_form() < live_truth()) bad("(c) live form below the truth");
  }

  std::array<int, 12> key() const {
    return {(int)book.live_form(), (int)book.stalest_canonical(), book.packed(kHome), book.packed(0), book.packed(1), book.live_slot(),
            book.per_filter(), mask, tune, (int)truth[0], (int)truth[1], (int)truth[2]};
  }
};

// ---- the events; false: the ABI refuses the call in this state ----
bool ev_select(World& w, int s) {
  if (w.book.per_filter()) return false;
  w.book.select(s);
  return true;
}
// launch_resident: in place (dst == -2) or into ring slot dst (viekf_batch_propagate_to / _propagate_n_to)
bool ev_fused(World& w, int dst) {
  const bool in_place = dst == -2 || dst == w.book.live_slot();
  if (!in_place && (w.book.per_filter() || w.mask)) return false;
  const bool store_packed = w.keeps_packed() && !w.mask;
  if (w.book.per_filter() || w.mask) w.require(PForm::Lower);
  if (in_place) {
    w.set_live_truth(store_packed ? PForm::Packed : PForm::Lower);
    w.book.wrote_live(store_packed ? PForm::Packed : PForm::Lower);
  } else {
    w.t(dst) = store_packed ? PForm::Packed : PForm::Lower;
    w.book.wrote_slot(dst, store_packed);
    w.book.select(dst);
  }
  return true;
}
bool ev_stream(World& w) {   // streaming propagate / grouped update
  w.require(PForm::Lower);
  w.set_live_truth(PForm::Lower);
  w.book.wrote_live(PForm::Lower);
  return true;
}
bool ev_read_full(World& w) { w.require(PForm::Full); return true; }
bool ev_read_lower(World& w) { w.require(PForm::Lower); return true; }
bool ev_set_P(World& w) {   // viekf_batch_set_state(P) / viekf_batch_reset
  if (w.book.per_filter()) w.require(PForm::Full);
  w.set_live_truth(PForm::Full);
  w.book.wrote_live(PForm::Full);
  return true;
}
bool ev_snapshot(World& w, int s) {
  if (w.book.per_filter()) return false;
  w.t(s) = w.live_truth();
  w.book.saved_to(s);
  return true;
}
bool ev_restore(World& w, int s) {
  if (w.book.per_filter()) return false;
  w.t(w.book.live_slot()) = w.t(s);
  w.book.restored_from(s);
  return true;
}
bool ev_select_filters(World& w) {
  if (w.book.live_slot() >= 0) return false;
  w.canonicalize_all();
  if (!w.book.per_filter()) w.book.enter_per_filter();
  w.book.filters_moved();
  return true;
}
bool ev_resize(World& w) {
  w.t(kHome) = w.live_truth();   // (per-filter mode: gathered home; a live ring slot: copied home; home live: itself)
  w.book.resized(0);
  w.book.resized(H);
  for (int s = 0; s < H; s++) w.t(s) = PForm::Full;
  return true;
}
bool ev_ring_filters(World& w, bool to_ring) {   // viekf_batch_snapshot_filters / _restore_filters
  if (w.book.live_slot() >= 0) return false;
  w.canonicalize_all();
  if (to_ring) {
    const PForm live = w.live_truth();
    for (int s = 0; s < H; s++) w.t(s) = std::max(w.t(s), live);
  } else {
    w.book.filters_moved();
    if (!w.book.per_filter())
      for (int s = 0; s < H; s++) w.t(kHome) = std::max(w.t(kHome), w.t(s));
  }
  return true;
}
bool ev_mask(World& w, bool on) { w.mask = on; return true; }
bool ev_tune_packed(World& w, bool on) { w.require(PForm::Lower); w.tune = on; return true; }
bool ev_tune_instance(World& w) { w.canonicalize_all(); return true; }

struct Event { const char* name; bool (*fire)(World&); long fired; };
Event kEvents[] = {
    {"fused step in place", [](World& w) { return ev_fused(w, -2); }, 0},
    {"fused propagate into slot 0", [](World& w) { return ev_fused(w, 0); }, 0},
    {"fused propagate into slot 1", [](World& w) { return ev_fused(w, 1); }, 0},
    {"streaming propagate / grouped update", ev_stream, 0},
    {"reader of the whole P", ev_read_full, 0},
    {"reader / in-place writer of the lower triangle", ev_read_lower, 0},
    {"set_state(P) / reset", ev_set_P, 0},
    {"snapshot(0)", [](World& w) { return ev_snapshot(w, 0); }, 0},
    {"snapshot(1)", [](World& w) { return ev_snapshot(w, 1); }, 0},
    {"restore(0)", [](World& w) { return ev_restore(w, 0); }, 0},
    {"restore(1)", [](World& w) { return ev_restore(w, 1); }, 0},
    {"select(home)", [](World& w) { return ev_select(w, kHome); }, 0},
    {"select(0)", [](World& w) { return ev_select(w, 0); }, 0},
    {"select(1)", [](World& w) { return ev_select(w, 1); }, 0},
    {"select_filters", ev_select_filters, 0},
    {"history_resize", ev_resize, 0},
    {"snapshot_filters", [](World& w) { return ev_ring_filters(w, true); }, 0},
    {"restore_filters", [](World& w) { return ev_ring_filters(w, false); }, 0},
    {"mask on", [](World& w) { return ev_mask(w, true); }, 0},
    {"mask off", [](World& w) { return ev_mask(w, false); }, 0},
    {"packed switch off", [](World& w) { return ev_tune_packed(w, false); }, 0},
    {"packed switch on", [](World& w) { return ev_tune_packed(w, true); }, 0},
    {"instance change", ev_tune_instance, 0},
};

}  // namespace

int main() {
  World start;
  start.book.resized(H);
  std::set<std::array<int, 12>> seen = {start.key()};
  std::deque<World> frontier = {start};
  long violations = 0;
  bool slot_live = false, home_live = false, per_filter = false;
  while (!frontier.empty()) {
    const World from = frontier.front();
    frontier.pop_front();
    for (Event& e : kEvents) {
      World w = from;
      if (!e.fire(w)) continue;
      e.fired++;
      w.check();
      if (w.violations) {
        if (violations < 8) std::printf("VIOLATION after '%s': %s\n", e.name, w.why.c_str());
        violations += w.violations;
        continue;
      }
      per_filter |= w.book.per_filter();
      slot_live |= !w.book.per_filter() && w.book.live_slot() >= 0;
      home_live |= !w.book.per_filter() && w.book.live_slot() == kHome;
      if (seen.insert(w.key()).second) frontier.push_back(w);
    }
  }
  bool all_fired = true;
  for (const Event& e : kEvents) {
    std::printf("%-48s fired %ld\n", e.name, e.fired);
    all_fired &= e.fired > 0;
  }
  std::printf("states %zu violations %ld\n", seen.size(), violations);
  if (violations || !all_fired || !slot_live || !home_live || !per_filter) {
    std::printf("pform model: FAILED (all events fired %d, slot live %d, home live %d, per-filter %d)\n", all_fired, slot_live, home_live, per_filter);
    return 1;
  }
  std::printf("pform model: ok\n");
  return 0;
}
