// clip_file_host.cpp -- what the file commands share (grav1synth_amd/csrc/clip_file.h) built with a host compiler alone, as
// a stand-alone program: the frame pair of two scripted readers, a stub meter's records taken a batch at a time (with
// nlf.h's checked sum for either record kind), the table loader with stub parsers, a text into a file.
// tests/test_ingest_cpu.py compiles it under the address and undefined-behaviour sanitizers.
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../grav1synth_amd/csrc/clip_file.h"
#include "../grav1synth_amd/csrc/nlf.h"

using namespace g1s_clip;

static void require(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "clip_file_host: %s\n", what);
    std::exit(1);
  }
}

// a reader of `frames` frames that then ends, or fails with `code` at frame `fail_at` (negative: never); frame k has width k + 1
struct Reader {
  int frames, fail_at, code, at = 0, calls = 0;
};
static int next(void *user, g1s_frame_t *out) {
  Reader *r = static_cast<Reader *>(user);
  ++r->calls;
  if (r->at == r->fail_at) return r->code;
  if (r->at >= r->frames) return 0;
  std::memset(out, 0, sizeof *out);
  out->width = (uint32_t)++r->at;
  return 1;
}

// the clip of two readers: the pairs before the end or the error, and what ended it
struct Clip {
  int pairs = 0;
  PairRead last;
};
static Clip run(Reader s, Reader d) {
  Clip c;
  for (;;) {
    g1s_frame_t fs, fd;
    c.last = next_pair(next, &s, next, &d, &fs, &fd);
    require(s.calls == d.calls, "a frame from each reader every call, whatever the first returned");
    if (c.last.got <= 0) return c;
    require(fs.width == (uint32_t)c.pairs + 1 && fd.width == fs.width, "pair k is frame k of either reader");
    ++c.pairs;
  }
}

// a meter that holds records and hands them over as g1s_nlf_finish does
template <class Rec>
struct Meter {
  std::vector<Rec> held;
  int finishes = 0, fail = 0;
  int finish(Rec *out, size_t cap, size_t *n) {
    ++finishes;
    if (fail) return fail;
    *n = held.size();
    if (cap < held.size()) return G1S_ERR_CAPACITY;
    std::copy(held.begin(), held.end(), out);
    held.clear();
    return G1S_OK;
  }
};
template <class Rec>
static std::string take(Meter<Rec> &m, std::vector<Rec> batch, std::vector<Rec> &scratch, Rec &total, uint64_t *count = nullptr) {
  m.held = batch;
  return take_records(
      [&](Rec *out, size_t cap, size_t *n) { return m.finish(out, cap, n); }, [](const Rec *r, size_t n, Rec *t) { return g1s_nl::sum_records(r, n, t); },
      [] { return "the meter's text"; }, "the sums leave 64 bits", scratch, total, count);
}

int main() {
  // ---- next_pair
  Clip c = run({5, -1, 0}, {3, -1, 0});
  require(c.pairs == 3 && c.last.got == 0 && c.last.unequal, "(5, 3): three pairs, then the end with unequal");
  c = run({3, -1, 0}, {5, -1, 0});
  require(c.pairs == 3 && c.last.got == 0 && c.last.unequal, "(3, 5): the same");
  c = run({3, -1, 0}, {3, -1, 0});
  require(c.pairs == 3 && c.last.got == 0 && !c.last.unequal, "(3, 3): no unequal");
  c = run({0, -1, 0}, {0, -1, 0});
  require(c.pairs == 0 && c.last.got == 0 && !c.last.unequal, "(0, 0): none");
  c = run({5, 2, G1S_ERR_INVALID}, {5, -1, 0});
  require(c.pairs == 2 && c.last.got == G1S_ERR_INVALID && c.last.failed == 0 && std::string(c.last.side()) == "source", "source failing at pair 2");
  c = run({2, -1, 0}, {5, 2, G1S_ERR_HIP});
  require(c.pairs == 2 && c.last.got == G1S_ERR_HIP && c.last.failed == 1 && std::string(c.last.side()) == "denoised" && !c.last.unequal,
          "denoised failing while the source ends: the error, not the end");
  c = run({5, 1, G1S_ERR_INVALID}, {5, 1, G1S_ERR_HIP});
  require(c.pairs == 1 && c.last.got == G1S_ERR_INVALID && c.last.failed == 0, "both failing: the source's");

  // ---- take_records: five frames, frame f with n = f + 1, a = 10 (f + 1), q = 100 (f + 1) in bin f of every plane; batches of two
  std::vector<g1s_nlf_record_t> frames(5);
  std::memset(frames.data(), 0, sizeof(g1s_nlf_record_t) * frames.size());
  for (int f = 0; f < 5; ++f)
    for (int p = 0; p < 3; ++p) frames[f].n[p][f] = f + 1, frames[f].a[p][f] = 10 * (f + 1), frames[f].q[p][f] = 100 * (f + 1);
  g1s_nlf_record_t total, none;
  std::memset(&total, 0, sizeof total), std::memset(&none, 0, sizeof none);
  Meter<g1s_nlf_record_t> meter;
  std::vector<g1s_nlf_record_t> scratch;
  uint64_t count = 0;
  for (size_t at = 0; at < frames.size(); at += 2) {
    const std::vector<g1s_nlf_record_t> batch(frames.begin() + at, frames.begin() + std::min(at + 2, frames.size()));
    require(take(meter, batch, scratch, total, &count).empty(), "a batch sums");
    require(scratch.size() == batch.size() + 1 && std::memcmp(scratch.data(), batch.data(), sizeof batch[0] * batch.size()) == 0,
            "the batch's records stay in scratch, the total as it was behind them");
  }
  require(count == 5 && meter.finishes == 6 && meter.held.empty(), "every record taken once: a call for the count, a call for the records");
  g1s_nlf_record_t once;
  require(g1s_nl::sum(frames.data(), frames.size(), &once) && std::memcmp(&once, &total, sizeof once) == 0, "batch by batch is all at once");
  require(take(meter, {}, scratch, total, &count).empty() && count == 5 && scratch.size() == 1 && std::memcmp(&once, &total, sizeof once) == 0,
          "a meter that holds nothing adds nothing");
  // a total at the top of 64 bits: the next batch is refused and the total stays
  total.q[1][7] = ~0ull;
  const g1s_nlf_record_t before = total;
  std::vector<g1s_nlf_record_t> over(1, none);
  over[0].q[1][7] = 1;
  require(take(meter, over, scratch, total, &count) == "the sums leave 64 bits" && std::memcmp(&total, &before, sizeof total) == 0 && count == 5,
          "a sum that leaves 64 bits is refused and the total untouched");
  meter.fail = G1S_ERR_HIP;
  require(take(meter, over, scratch, total) == "the meter's text" && std::memcmp(&total, &before, sizeof total) == 0, "a meter that fails: its text");
  // the temporal kind through the same code: s is signed
  std::vector<g1s_nlf_trecord_t> pairs(3);
  std::memset(pairs.data(), 0, sizeof(g1s_nlf_trecord_t) * pairs.size());
  pairs[0].s[0][3] = -7, pairs[1].s[0][3] = 4, pairs[2].s[0][3] = -1, pairs[0].n[0][3] = pairs[1].n[0][3] = pairs[2].n[0][3] = 1;
  g1s_nlf_trecord_t ttotal;
  std::memset(&ttotal, 0, sizeof ttotal);
  Meter<g1s_nlf_trecord_t> tmeter;
  std::vector<g1s_nlf_trecord_t> tscratch;
  require(take(tmeter, std::vector<g1s_nlf_trecord_t>(pairs.begin(), pairs.begin() + 2), tscratch, ttotal).empty() &&
              take(tmeter, std::vector<g1s_nlf_trecord_t>(pairs.begin() + 2, pairs.end()), tscratch, ttotal).empty(),
          "temporal batches sum");
  require(ttotal.s[0][3] == -4 && ttotal.n[0][3] == 3, "with their signs");

  // ---- the table loader
  char path[] = "/tmp/clip_file_host_XXXXXX";
  const int fd = mkstemp(path);
  require(fd >= 0, "a temporary file");
  const std::string body(70000, 't');  // (more than one read of read_text)
  require(write_text(path, body.data(), body.size()).empty(), "write_text writes");
  std::string back;
  require(read_text(path, &back) && back == body, "read_text reads what write_text wrote");
  int calls = 0;
  std::vector<g1s_segment_t> segs;
  std::string why;
  auto wants65 = [&](const char *text, size_t len, g1s_segment_t *out, size_t cap, size_t *n, char *, size_t) {
    ++calls;
    require(len == body.size() && std::memcmp(text, body.data(), len) == 0, "the parser sees the file");
    *n = 65;
    if (cap < 65) return (int)G1S_ERR_CAPACITY;
    for (size_t k = 0; k < 65; ++k) std::memset(&out[k], 0, sizeof out[k]), out[k].start_time = k;
    return (int)G1S_OK;
  };
  require(load_table(path, wants65, segs, "cannot open ", "grain table: ", &why) == G1S_OK && calls == 2 && segs.size() == 65 && segs[64].start_time == 64 &&
              why.empty(),
          "a table of 65 segments: parsed twice, 65 segments");
  calls = 0;
  auto wants3 = [&](const char *, size_t, g1s_segment_t *out, size_t, size_t *n, char *, size_t) {
    ++calls, *n = 3;
    std::memset(out, 0, 3 * sizeof *out);
    return (int)G1S_OK;
  };
  require(load_table(path, wants3, segs, "cannot open ", "grain table: ", &why) == G1S_OK && calls == 1 && segs.size() == 3, "a table of 3: parsed once");
  auto fails = [&](const char *, size_t, g1s_segment_t *, size_t, size_t *, char *err, size_t cap) {
    snprintf(err, cap, "line 3: no");
    return (int)G1S_ERR_STATE;
  };
  require(load_table(path, fails, segs, "cannot open ", "grain prior: ", &why) == G1S_ERR_STATE && why == "grain prior: line 3: no",
          "a parser that fails: its code, its text behind the caller's prefix");
  close(fd), std::remove(path);
  calls = 0;
  require(load_table(path, wants3, segs, "grain prior: cannot open ", "grain prior: ", &why) == G1S_ERR_INVALID && calls == 0 &&
              why == std::string("grain prior: cannot open ") + path,
          "an unreadable path: the caller's cannot-open text, nothing parsed");
  // ---- fill_segments as the three *_finish use it, write_text into a directory that is not there
  calls = 0;
  require(fill_segments(segs, [&](g1s_segment_t *, size_t, size_t *n) { return ++calls, *n = 70, (int)G1S_ERR_CAPACITY; }) == G1S_ERR_CAPACITY && calls == 2,
          "capacity twice: the code, no third call");
  const std::string missing = std::string(path) + "/report.txt";
  require(write_text(missing.c_str(), "x", 1) == "cannot create " + missing, "a path in a missing directory: cannot create");
  char err[8] = "";
  require(refuse(err, sizeof err, G1S_ERR_HIP, "a long text") == G1S_ERR_HIP && std::string(err) == "a long " && refuse(nullptr, 0, -3, "x") == -3,
          "refuse: the code, the text cut to the buffer, no buffer no text");
  std::printf("ok\n");
  return 0;
}
