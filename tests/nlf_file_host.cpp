// nlf_file_host.cpp -- the record arithmetic of the noise levels' file commands (grav1synth_amd/csrc/nlf_file.cpp) built with a
// host compiler alone, as a stand-alone program: a clip's total taken a batch at a time through clip_file.h's take_records
// with nlf.h's sum_records (what that does with a sum that leaves 64 bits and with the signed temporal kind is checked in
// tests/clip_file_host.cpp), and the ordinary record of the frames with a predecessor, the total less the first frame's
// (without_first), which the temporal report's ratio lines are formed from.  tests/test_nlf_t_cpu.py compiles it under the
// address and undefined-behaviour sanitizers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../grav1synth_amd/csrc/clip_file.h"
#include "../grav1synth_amd/csrc/nlf.h"

static void require(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "nlf_file_host: %s\n", what);
    std::exit(1);
  }
}

// a batch of records held by a meter, taken as nlf_file.cpp takes them
template <class Record>
static bool take(std::vector<Record> batch, Record &total) {
  std::vector<Record> scratch;
  auto finish = [&](Record *out, size_t cap, size_t *n) {
    *n = batch.size();
    if (cap < batch.size()) return (int)G1S_ERR_CAPACITY;
    std::copy(batch.begin(), batch.end(), out);
    return (int)G1S_OK;
  };
  return g1s_clip::take_records(finish, g1s_nl::sum_records<Record>, [] { return "the meter failed"; }, g1s_nl::kSumsLeave64, scratch, total).empty();
}

int main() {
  // five frames, frame f with n = f + 1, a = 10 (f + 1), q = 100 (f + 1) in bin f of every plane; batches of two
  std::vector<g1s_nlf_record_t> frames(5);
  std::memset(frames.data(), 0, sizeof(g1s_nlf_record_t) * frames.size());
  for (int f = 0; f < 5; ++f)
    for (int c = 0; c < 3; ++c) frames[f].n[c][f] = f + 1, frames[f].a[c][f] = 10 * (f + 1), frames[f].q[c][f] = 100 * (f + 1);
  g1s_nlf_record_t total;
  std::memset(&total, 0, sizeof total);
  for (size_t at = 0; at < frames.size(); at += 2)
    require(take(std::vector<g1s_nlf_record_t>(frames.begin() + at, frames.begin() + std::min(at + 2, frames.size())), total), "a batch sums");
  g1s_nlf_record_t once;
  require(g1s_nl::sum(frames.data(), frames.size(), &once) && std::memcmp(&once, &total, sizeof once) == 0, "batch by batch is all at once");
  const g1s_nlf_record_t later = g1s_nl::without_first(total, frames[0]);
  g1s_nlf_record_t want;
  require(g1s_nl::sum(frames.data() + 1, frames.size() - 1, &want) && std::memcmp(&want, &later, sizeof want) == 0,
          "the total less the first frame is the sum of the frames with a predecessor");
  require(later.n[2][0] == 0 && later.a[0][0] == 0 && later.q[1][0] == 0 && later.n[1][4] == 5, "the first frame's bin is empty, the last one's whole");
  g1s_nlf_record_t none;
  std::memset(&none, 0, sizeof none);
  const g1s_nlf_record_t same = g1s_nl::without_first(total, none);
  require(std::memcmp(&total, &same, sizeof total) == 0, "a clip without a first record loses nothing");
  // a total at the top of 64 bits: the next batch is refused and the total stays
  total.q[1][7] = ~0ull;
  const g1s_nlf_record_t before = total;
  std::vector<g1s_nlf_record_t> over(1, none);
  over[0].q[1][7] = 1;
  require(!take(over, total) && std::memcmp(&total, &before, sizeof total) == 0, "a sum that leaves 64 bits is refused and the total untouched");
  // the temporal kind through the same code: s is signed
  std::vector<g1s_nlf_trecord_t> pairs(3);
  std::memset(pairs.data(), 0, sizeof(g1s_nlf_trecord_t) * pairs.size());
  pairs[0].s[0][3] = -7, pairs[1].s[0][3] = 4, pairs[2].s[0][3] = -1, pairs[0].n[0][3] = pairs[1].n[0][3] = pairs[2].n[0][3] = 1;
  g1s_nlf_trecord_t ttotal;
  std::memset(&ttotal, 0, sizeof ttotal);
  require(take(std::vector<g1s_nlf_trecord_t>(pairs.begin(), pairs.begin() + 2), ttotal) && take(std::vector<g1s_nlf_trecord_t>(pairs.begin() + 2, pairs.end()), ttotal),
          "temporal batches sum");
  require(ttotal.s[0][3] == -4 && ttotal.n[0][3] == 3, "with their signs");
  std::printf("ok\n");
  return 0;
}
