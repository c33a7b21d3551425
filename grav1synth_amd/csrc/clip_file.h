// clip_file.h -- what the file commands share (`diff`, `measure`, `check`, `render`, `estimate --levels`, `denoise`: ingest.cpp,
// measure_file.cpp, grain_file.cpp, nlf_file.cpp, denoise_file.cpp and frame_op.h's rewrite_y4m): a refusal into the caller's
// buffer, a text file read and written, a grain table loaded with its capacity retry, a meter's records taken a batch at a
// time, a frame pair from two readers and two clips opened together.  Host code only: it calls nothing of HIP and builds
// with a host compiler alone (tests/clip_file_host.cpp).  The texts stay with the callers: what is here returns which case
// it met, or takes the caller's words.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"

namespace g1s_clip {

// a file command's way out when it fails: the text into the caller's buffer, the code returned
inline int refuse(char *err, size_t cap, int code, const std::string &text) {
  if (err && cap) snprintf(err, cap, "%s", text.c_str());
  return code;
}

// the whole file behind *text; false: it cannot be opened
inline bool read_text(const char *path, std::string *text) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  char buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text->append(buf, n);
  std::fclose(f);
  return true;
}

// n bytes into a new file.  "" when fine
inline std::string write_text(const char *path, const char *data, size_t n) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return std::string("cannot create ") + path;
  const bool ok = std::fwrite(data, 1, n, f) == n;
  return std::fclose(f) != 0 || !ok ? std::string("cannot write ") + path : "";
}

// Segments from something that fills a buffer of them and says G1S_ERR_CAPACITY, with the number there are, when it is too
// small (`fill(out, cap, &n)`: g1s_diff_finish, g1s_fold_finish, a parser): room for 64, and once more with room for all.
// Returns fill's code; G1S_OK: `segs` is the segments.
template <class Fill>
int fill_segments(std::vector<g1s_segment_t> &segs, Fill fill) {
  size_t n = 0;
  segs.resize(64);
  int rc = fill(segs.data(), segs.size(), &n);
  if (rc == G1S_ERR_CAPACITY) {
    segs.resize(n);
    rc = fill(segs.data(), segs.size(), &n);
  }
  if (!rc) segs.resize(n);
  return rc;
}

// The segments `fill` hands over (fill_segments) into the grain table at `path`: fill's code with last_error() in *why, or
// g1s_write_tbl's with its text.  G1S_OK: written.
template <class Fill, class LastError>
int write_table(const char *path, Fill fill, LastError last_error, std::string *why) {
  std::vector<g1s_segment_t> segs;
  int rc = fill_segments(segs, fill);
  if (rc) return *why = last_error(), rc;
  if ((rc = g1s_write_tbl(path, segs.data(), segs.size())) != 0) *why = std::string("cannot write ") + path;
  return rc;
}

// The grain table at `path` through `parse` (g1s_parse_tbl's arguments).  A code with *why = cannot_open + path, or parse's
// code with *why = parse_failed + parse's text: the two prefixes are the caller's.
template <class Parse>
int load_table(const char *path, Parse parse, std::vector<g1s_segment_t> &segs, const char *cannot_open, const char *parse_failed, std::string *why) {
  std::string text;
  if (!read_text(path, &text)) return *why = std::string(cannot_open) + path, G1S_ERR_INVALID;
  char perr[256] = "";
  const int rc = fill_segments(segs, [&](g1s_segment_t *out, size_t cap, size_t *n) { return parse(text.data(), text.size(), out, cap, n, perr, sizeof perr); });
  if (rc) *why = std::string(parse_failed) + perr;
  return rc;
}

// The records of one kind that a meter holds, added to `total`: `finish(out, cap, &n)` hands them over (with no room: says
// how many there are), `sum(recs, n, &total)` is true when the sum stayed in 64 bits.  They stay in `scratch`, behind them
// the total as it was; *count (if given) grows by their number.  "" when fine, else last_error() or overflow_text.
template <class Rec, class Finish, class Sum, class LastError>
std::string take_records(Finish finish, Sum sum, LastError last_error, const std::string &overflow_text, std::vector<Rec> &scratch, Rec &total,
                         uint64_t *count = nullptr) {
  size_t n = 0;
  int rc = finish(nullptr, 0, &n);
  if (rc && rc != G1S_ERR_CAPACITY) return last_error();
  scratch.resize(n + 1);
  scratch[n] = total;
  if (n && (rc = finish(scratch.data(), n, &n)) != 0) return last_error();
  if (!sum(scratch.data(), n + 1, &total)) return overflow_text;
  if (count) *count += n;
  return "";
}

// One frame from each of two readers, source first (get_filtered_frame_pair, src/main.rs:615-629).  An error on either side
// wins over an end on the other; one reader at its end ends the clip, one alone: `unequal`.
struct PairRead {
  int got = 0;           // 1: a pair in *s and *d; 0: the clip has ended; negative: the code of the reader that failed
  bool unequal = false;  // (got == 0) one reader ended before the other
  int failed = 0;        // (got < 0) 0: the source reader, 1: the denoised one
  const char *side() const { return failed ? "denoised" : "source"; }
};
inline PairRead next_pair(g1s_next_frame_fn source, void *source_user, g1s_next_frame_fn denoised, void *denoised_user, g1s_frame_t *s, g1s_frame_t *d) {
  const int rs = source(source_user, s), rd = denoised(denoised_user, d);
  PairRead p;
  if (rs < 0 || rd < 0) p.got = rs < 0 ? rs : rd, p.failed = rs < 0 ? 0 : 1;
  else if (rs == 0 || rd == 0) p.unequal = (rs == 0) != (rd == 0);
  else p.got = 1;
  return p;
}

inline bool same_clip_shape(const g1s_y4m_info_t &a, const g1s_y4m_info_t &b) {
  return a.width == b.width && a.height == b.height && a.bit_depth == b.bit_depth && a.xdec == b.xdec && a.ydec == b.ydec && a.nplanes == b.nplanes;
}

// two .y4m readers opened one after the other and closed together; the first is closed when the second does not open
struct TwoClips {
  g1s_y4m_t *a = nullptr, *b = nullptr;
  g1s_y4m_info_t ia{}, ib{};
  TwoClips() = default;
  TwoClips(const TwoClips &) = delete;
  TwoClips &operator=(const TwoClips &) = delete;
  ~TwoClips() { close(); }
  // false: the reader's text is in err
  bool open(const char *path_a, const char *path_b, char *err, size_t cap) {
    if (!(a = g1s_y4m_open(path_a, err, cap))) return false;
    if (!(b = g1s_y4m_open(path_b, err, cap))) return close(), false;
    g1s_y4m_get_info(a, &ia), g1s_y4m_get_info(b, &ib);
    return true;
  }
  // the text of the reader that next_pair says failed
  const char *last_error(const PairRead &p) const { return g1s_y4m_last_error(p.failed ? b : a); }
  void close() {
    if (a) g1s_y4m_close(a);
    if (b) g1s_y4m_close(b);
    a = b = nullptr;
  }
};

}  // namespace g1s_clip
