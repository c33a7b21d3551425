// meter_lane_host.cpp -- the host part of the meters' record lane (grav1synth_amd/csrc/meter_op.h: the records a kind holds
// and their hand-over, the count of a frame's units) built with a host compiler alone, as a stand-alone program, and driven
// with a toy record: the capacity rule of every *_finish call.  tests/test_meter_lane_cpu.py compiles it under the address
// and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>

#include "../grav1synth_amd/csrc/meter_op.h"

#ifdef __HIPCC__
#error "this program is the proof that the first part of meter_op.h needs no HIP"
#endif

using namespace g1s_op;

struct Toy {
  uint64_t id, twice;
};

static void require(bool ok, const char *what) {
  if (ok) return;
  std::fprintf(stderr, "meter_lane_host: %s\n", what);
  std::exit(1);
}

static Toy toy(uint64_t id) { return Toy{id, 2 * id}; }
static bool is_toy(const Toy &t, uint64_t id) { return t.id == id && t.twice == 2 * id; }

int main() {
  const uint64_t kUntouched = 0xfeedfaceull;
  Records<Toy> lane;
  size_t n = 99;

  // nothing held: NULL is fine, with and without room, and with no n_out
  require(lane.hand_over(nullptr, 0, &n) == G1S_OK && n == 0, "a hand-over of no records with out == NULL is not OK");
  n = 99;
  require(lane.hand_over(nullptr, 5, &n) == G1S_OK && n == 0, "a hand-over of no records with out == NULL and cap 5 is not OK");
  require(lane.hand_over(nullptr, 0, nullptr) == G1S_OK, "a hand-over of no records without n_out is not OK");

  // three records, as a batch collects them
  const Toy batch[3] = {toy(1), toy(2), toy(3)};
  lane.collect(batch, 3);
  n = 99;
  require(lane.hand_over(nullptr, 3, &n) == G1S_ERR_CAPACITY && n == 3, "NULL with records is not G1S_ERR_CAPACITY with *n_out set");
  require(lane.records.size() == 3, "a refused hand-over (NULL) dropped records");

  Toy out[4] = {toy(kUntouched), toy(kUntouched), toy(kUntouched), toy(kUntouched)};
  n = 99;
  require(lane.hand_over(out, 2, &n) == G1S_ERR_CAPACITY && n == 3, "cap one short is not G1S_ERR_CAPACITY with *n_out set");
  require(lane.records.size() == 3 && is_toy(lane.records[0], 1) && is_toy(lane.records[1], 2) && is_toy(lane.records[2], 3),
          "a refused hand-over (cap one short) changed the records held");
  for (const Toy &t : out) require(is_toy(t, kUntouched), "a refused hand-over wrote to the caller's entries");
  require(lane.hand_over(out, 2, nullptr) == G1S_ERR_CAPACITY && lane.records.size() == 3, "cap one short without n_out");

  n = 99;
  require(lane.hand_over(out, 3, &n) == G1S_OK && n == 3, "exact cap does not hand over");
  require(is_toy(out[0], 1) && is_toy(out[1], 2) && is_toy(out[2], 3) && is_toy(out[3], kUntouched), "exact cap: the entries are not the records in order");
  require(lane.records.empty(), "a hand-over left records behind");
  n = 99;
  require(lane.hand_over(out, 3, &n) == G1S_OK && n == 0 && is_toy(out[0], 1), "a second hand-over is not empty");

  // two collects, one hand-over: in the order they came, into more room than needed
  const Toy first[2] = {toy(10), toy(11)}, second[3] = {toy(12), toy(13), toy(14)};
  lane.collect(first, 2);
  lane.collect(second, 0);  // (a kind without a job in the batch)
  lane.collect(second, 3);
  Toy wide[7];
  for (Toy &t : wide) t = toy(kUntouched);
  n = 99;
  require(lane.hand_over(wide, 7, &n) == G1S_OK && n == 5, "two collects do not hand over as five records");
  for (uint64_t i = 0; i < 5; ++i) require(is_toy(wide[i], 10 + i), "two collects came out of order");
  require(is_toy(wide[5], kUntouched) && is_toy(wide[6], kUntouched) && lane.records.empty(), "the hand-over wrote past the records");

  // the units of a frame: 130 x 260 at 4:2:0 in tiles of 64 x 128 -- 3 x 3, and 2 x 2 a chroma plane
  g1s_frame_t f{};
  f.width = 130, f.height = 260, f.nplanes = 3, f.xdec = 1, f.ydec = 1;
  Units u;
  u.cut(PlaneGeom(f, 1), 64, 128);
  require(u.n[0] == 9 && u.n[1] == 4 && u.n[2] == 4 && u.base[0] == 0 && u.base[1] == 9 && u.base[2] == 13 && u.frame == 17, "Units::cut of 130 x 260 at 4:2:0");
  f.nplanes = 1;
  u.cut(PlaneGeom(f, 2), 256, 128);
  require(u.n[0] == 3 && u.n[1] == 0 && u.n[2] == 0 && u.base[1] == 3 && u.base[2] == 3 && u.frame == 3, "Units::cut of one plane in strips");
  u.n[0] = 0, u.n[1] = 7, u.n[2] = 2;
  u.lay();
  require(u.base[0] == 0 && u.base[1] == 0 && u.base[2] == 7 && u.frame == 9, "Units::lay of counts set by hand");

  std::printf("ok\n");
  return 0;
}
