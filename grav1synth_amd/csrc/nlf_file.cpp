// nlf_file.cpp -- the file commands of the noise levels: `estimate --levels` (g1s_nlf_y4m_file) and `--levels-temporal`
// (g1s_nlf_y4m_file_temporal), which are also the pre-pass of `denoise --auto-*`, and `--table` (g1s_nlf_y4m_file_table).  Host code above the per-frame ABI of
// nlf.hip: it launches no kernel and sees the meter through g1s_nlf_* alone.  The records are taken after every batch of
// frames (frame_op.h's batch_of: the meter's own batch), so the meter never holds more than a batch of them.
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "clip_file.h"
#include "frame_op.h"
#include "nlf.h"
#include "nlf_table.h"

using g1s_clip::refuse;

namespace {

// the records of one kind the meter holds (`finish`: g1s_nlf_finish or g1s_nlf_finish_temporal), added to `total`; they
// stay in `scratch`, behind them the total as it was.  "" when fine
template <class Record, class Finish>
std::string take_from(g1s_nlf_t *m, Finish finish, std::vector<Record> &scratch, Record &total) {
  return g1s_clip::take_records([&](Record *out, size_t cap, size_t *n) { return finish(m, out, cap, n); }, g1s_nl::sum_records<Record>,
                                [&] { return g1s_nlf_last_error(m); }, g1s_nl::kSumsLeave64, scratch, total);
}

std::string write_report(const char *path, const std::string &text) { return g1s_clip::write_text(path, text.data(), text.size()); }

// what `--table` adds to a temporal job: the clip's own table (rules L6 - L9) and the lag report (L10)
struct TableJob {
  const char *out_table, *out_lags;
  uint32_t lag;
  uint64_t min_count;
  g1s_segment_t *segment_out;
};

// a .y4m file through a meter (`temporal`: a temporal one, the file one run; `table`: a lag meter): the reports, the clip's
// records.  A table that is refused is refused before anything is written.
int64_t nlf_y4m_file(const char *source, const char *out_report, const char *out_treport, const g1s_nlf_opts_t *opts, uint64_t max_frames,
                     g1s_nlf_record_t *total_out, g1s_nlf_trecord_t *ttotal_out, bool temporal, char *err, size_t cap, const TableJob *table = nullptr) {
  if (!source) return refuse(err, cap, G1S_ERR_INVALID, "null path");
  g1s_y4m_t *y = g1s_y4m_open(source, err, cap);
  if (!y) return G1S_ERR_INVALID;
  g1s_y4m_info_t info;
  g1s_y4m_get_info(y, &info);
  int rc = G1S_OK;
  std::string why;
  int64_t frames = 0;
  uint64_t pairs = 0;
  g1s_nlf_record_t total, first;  // first: the clip's first frame alone, which has no predecessor
  g1s_nlf_trecord_t ttotal;
  std::memset(&total, 0, sizeof total), std::memset(&first, 0, sizeof first), std::memset(&ttotal, 0, sizeof ttotal);
  bool have_first = false;
  std::vector<g1s_nlf_record_t> scratch;
  std::vector<g1s_nlf_trecord_t> tscratch;
  g1s_nlf_lrecord_t ltotal;
  std::memset(&ltotal, 0, sizeof ltotal);
  std::vector<g1s_nlf_lrecord_t> lscratch;
  const uint32_t batch = g1s_op::batch_of(opts ? opts->batch_frames : 0);
  g1s_nlf_t *m = table ? g1s_nlf_new_lags(info.bit_depth, opts) : temporal ? g1s_nlf_new_temporal(info.bit_depth, opts) : g1s_nlf_new(info.bit_depth, opts);
  auto take_all = [&]() -> std::string {
    std::string no = take_from(m, g1s_nlf_finish, scratch, total);
    if (no.empty() && !have_first && scratch.size() > 1) first = scratch[0], have_first = true;
    if (no.empty() && temporal && (no = take_from(m, g1s_nlf_finish_temporal, tscratch, ttotal)).empty()) pairs += tscratch.size() - 1;
    if (no.empty() && table)
      no = g1s_clip::take_records([&](g1s_nlf_lrecord_t *out, size_t n_cap, size_t *n) { return g1s_nlf_finish_lags(m, out, n_cap, n); }, g1s_nl::sum_lags,
                                  [&] { return g1s_nlf_last_error(m); }, g1s_nl::kSumsLeave64, lscratch, ltotal);
    return no;
  };
  if (!m) rc = G1S_ERR_NO_DEVICE, why = g1s_last_global_error();
  while (!rc && (!max_frames || (uint64_t)frames < max_frames)) {
    g1s_frame_t f;
    const int got = g1s_y4m_next(y, &f);
    if (got < 0) {
      rc = got, why = "frame " + std::to_string(frames) + ": " + g1s_y4m_last_error(y);
      break;
    }
    if (got == 0) break;
    f.on_device = 0;  // (the reader lends the frame until its next call: copied before the call returns)
    if ((rc = g1s_nlf_frame(m, &f)) != 0) {
      why = "frame " + std::to_string(frames) + ": " + g1s_nlf_last_error(m);
      break;
    }
    ++frames;
    if (frames % batch == 0 && !(why = take_all()).empty()) rc = G1S_ERR_INVALID;
  }
  if (!rc && !(why = take_all()).empty()) rc = G1S_ERR_INVALID;
  g1s_segment_t segment;
  if (!rc && table) {
    if (frames < 2) rc = G1S_ERR_INVALID, why = "a table needs two frames";
    else if ((rc = g1s_nlf_table(&ttotal, &ltotal, info.bit_depth, info.xdec, info.ydec, info.nplanes, table->lag, table->min_count, &segment)) != 0)
      why = g1s_last_global_error();
  }
  if (!rc && table && table->out_table) {
    std::string text(4096, '\0');
    const long n = g1s_format_tbl(&segment, 1, &text[0], text.size());
    if (n < 0) rc = G1S_ERR_INVALID, why = "the table does not fit its text";
    else if (!(why = g1s_clip::write_text(table->out_table, text.data(), (size_t)n)).empty()) rc = G1S_ERR_INVALID;
  }
  if (!rc && table && table->out_lags &&
      !(why = write_report(table->out_lags, g1s_nl::lag_report(ltotal, pairs, info.bit_depth, info.nplanes, table->lag, table->min_count))).empty())
    rc = G1S_ERR_INVALID;
  if (!rc && table && table->segment_out) *table->segment_out = segment;
  if (!rc && out_report && !(why = write_report(out_report, g1s_nl::report(total, (uint64_t)frames, info.bit_depth, info.nplanes, 0))).empty())
    rc = G1S_ERR_INVALID;
  if (!rc && out_treport) {
    const g1s_nlf_record_t later = g1s_nl::without_first(total, first);
    if (!(why = write_report(out_treport, g1s_nl::report_t(ttotal, &later, pairs, info.bit_depth, info.nplanes, 0))).empty()) rc = G1S_ERR_INVALID;
  }
  if (!rc && total_out) *total_out = total;
  if (!rc && ttotal_out) *ttotal_out = ttotal;
  g1s_nlf_free(m);
  g1s_y4m_close(y);
  return rc ? refuse(err, cap, rc, why) : frames;
}

}  // namespace

extern "C" {

int64_t g1s_nlf_y4m_file(const char *source, const char *out_report, const g1s_nlf_opts_t *opts, uint64_t max_frames, g1s_nlf_record_t *total_out,
                         char *err, size_t cap) {
  return nlf_y4m_file(source, out_report, nullptr, opts, max_frames, total_out, nullptr, false, err, cap);
}

int64_t g1s_nlf_y4m_file_temporal(const char *source, const char *out_report, const char *out_treport, const g1s_nlf_opts_t *opts, uint64_t max_frames,
                                  g1s_nlf_record_t *total_out, g1s_nlf_trecord_t *ttotal_out, char *err, size_t cap) {
  return nlf_y4m_file(source, out_report, out_treport, opts, max_frames, total_out, ttotal_out, true, err, cap);
}

int64_t g1s_nlf_y4m_file_table(const char *source, const char *out_table, const char *out_report, const char *out_treport, const char *out_lags,
                               const g1s_nlf_opts_t *opts, uint64_t max_frames, uint32_t lag, uint64_t min_count, g1s_segment_t *segment_out, char *err,
                               size_t cap) {
  if (lag < 1 || lag > 3) return refuse(err, cap, G1S_ERR_INVALID, "a table's lag is 1, 2 or 3");
  const TableJob job{out_table, out_lags, lag, min_count, segment_out};
  return nlf_y4m_file(source, out_report, out_treport, opts, max_frames, nullptr, nullptr, true, err, cap, &job);
}

}  // extern "C"
