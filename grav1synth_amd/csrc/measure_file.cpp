// measure_file.cpp -- the file commands of `measure` and `check` (g1s_measure_y4m_files*, g1s_check_y4m_files*).  Host code
// above the per-frame ABI of measure.hip and grain.hip: it launches no kernel and sees the meters and the synthesizer through
// g1s_measure_* and g1s_grain_* and one accessor.  The records are taken after every batch of frames (frame_op.h's batch_of:
// the meter's own batch), so a meter never holds more than a batch of them; the reports are measure_report.cpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "clip_file.h"
#include "fold.h"
#include "frame_op.h"

extern "C" int32_t g1s_measure_device_(const g1s_measure_t *);

using namespace g1s_op;
using namespace g1s_clip;

namespace {

// where the reports of a clip go: the plain one always, the others where a path is given
struct ReportPaths {
  const char *plain, *temporal, *cross, *scales;
};

// a clip's total of one record kind: a meter's records pass through `scratch` and are counted
template <class Rec>
struct KindTotal {
  Rec total;
  std::vector<Rec> scratch;
  uint64_t count = 0;
  KindTotal() { std::memset(&total, 0, sizeof total); }
  // the records of the kind that the meter holds, added to the total.  "" when fine; `kind`: "", "temporal " ... in the text
  template <class Finish, class Sum>
  std::string take(g1s_measure_t *m, Finish finish, Sum sum, const char *kind) {
    return take_records([&](Rec *out, size_t cap, size_t *n) { return finish(m, out, cap, n); },
                        [&](const Rec *recs, size_t n, Rec *t) { return sum(recs, n, t) == 0; }, [&] { return g1s_measure_last_error(m); },
                        std::string("the clip's ") + kind + "sums leave 64 bits", scratch, total, &count);
  }
};

// a clip's totals of the four kinds (temporal.count: the clip's pairs with a predecessor)
struct ClipTotals {
  KindTotal<g1s_measure_record_t> plain;
  KindTotal<g1s_measure_trecord_t> temporal;
  KindTotal<g1s_measure_xrecord_t> cross;
  KindTotal<g1s_measure_srecord_t> scales;
  // what the meter holds of every kind that has a report to go to.  "" when fine
  std::string take(g1s_measure_t *m, const ReportPaths &out) {
    std::string why = plain.take(m, g1s_measure_finish, g1s_measure_sum, "");
    if (why.empty() && out.temporal) why = temporal.take(m, g1s_measure_finish_temporal, g1s_measure_sum_temporal, "temporal ");
    if (why.empty() && out.cross) why = cross.take(m, g1s_measure_finish_cross, g1s_measure_sum_cross, "cross ");
    if (why.empty() && out.scales) why = scales.take(m, g1s_measure_finish_scales, g1s_measure_sum_scales, "scale ");
    return why;
  }
};

// a report as a g1s_format_measure* call left it (n bytes of buf, n < 0: refused) into a file.  "" when fine
std::string write_report(const char *path, const char *buf, long n, const char *kind) {
  return n < 0 ? std::string("formatting the ") + kind + "report failed" : write_text(path, buf, (size_t)n);
}

// the reports of a clip's totals (beside `synth`'s, of the rendered clip, where there is one) into their files.  "" when fine
std::string write_reports(const ReportPaths &out, const ClipTotals &t, const ClipTotals *synth, uint64_t frames, const g1s_y4m_info_t &i) {
  std::vector<char> text(1 << 16);
  char *buf = text.data();
  const size_t cap = text.size();
  const g1s_measure_record_t *plain2 = synth ? &synth->plain.total : nullptr;
  long n = g1s_format_measure(&t.plain.total, plain2, frames, i.bit_depth, i.width, i.height, i.xdec, i.ydec, i.nplanes, buf, cap);
  std::string why = write_report(out.plain, buf, n, "");
  if (why.empty() && out.temporal) {
    n = g1s_format_measure_temporal(&t.temporal.total, synth ? &synth->temporal.total : nullptr, t.temporal.count, i.bit_depth, i.width, i.height,
                                    i.xdec, i.ydec, i.nplanes, buf, cap);
    why = write_report(out.temporal, buf, n, "temporal ");
  }
  if (why.empty() && out.cross) {
    n = g1s_format_measure_cross(&t.cross.total, synth ? &synth->cross.total : nullptr, frames, i.bit_depth, i.width, i.height, i.xdec, i.ydec, buf, cap);
    why = write_report(out.cross, buf, n, "cross ");
  }
  if (why.empty() && out.scales) {
    n = g1s_format_measure_scales(&t.plain.total, &t.scales.total, plain2, synth ? &synth->scales.total : nullptr, frames, i.bit_depth, i.nplanes, buf, cap);
    why = write_report(out.scales, buf, n, "scale ");
  }
  return why;
}

// a meter for the kinds that have a report to go to
g1s_measure_t *meter_for(const ReportPaths &out, uint32_t bit_depth, const g1s_measure_opts_t *opts) {
  const uint32_t modes = (out.temporal ? G1S_MEASURE_TEMPORAL : 0u) | (out.cross ? G1S_MEASURE_CROSS : 0u);
  return out.scales ? g1s_measure_new_scales(bit_depth, opts, modes) : g1s_measure_new_modes(bit_depth, opts, modes);
}

// what either command refuses of its two clips before it asks for a device
int clips_refusal(const TwoClips &clips, const ReportPaths &out, std::string *why) {
  if (!same_clip_shape(clips.ia, clips.ib)) return *why = "the two clips differ in geometry or bit depth", G1S_ERR_DIM_MISMATCH;
  if (out.cross && clips.ib.nplanes != 3) return *why = "--cross compares chroma with luma: the clip has no chroma planes", G1S_ERR_INVALID;
  return G1S_OK;
}

// the next frame pair of the two clips: 1, or 0 at the end of the shorter one (one alone: the warning of `diff` through
// *unequal), or the failing reader's code with its text behind the pair's index in *why
int next_clip_pair(const TwoClips &clips, int64_t frames, g1s_frame_t *a, g1s_frame_t *b, int *unequal, std::string *why) {
  const PairRead p = next_pair(g1s_y4m_next, clips.a, g1s_y4m_next, clips.b, a, b);
  if (p.got < 0) *why = "frame " + std::to_string(frames) + ": " + clips.last_error(p);
  if (p.got == 0 && unequal) *unequal = p.unequal;
  return p.got;
}

}  // namespace

extern "C" {

int64_t g1s_measure_y4m_files(const char *noisy, const char *clean, const char *out_report, const g1s_measure_opts_t *opts, int *unequal, char *err,
                              size_t cap) {
  return g1s_measure_y4m_files_temporal(noisy, clean, out_report, nullptr, opts, unequal, err, cap);
}

int64_t g1s_measure_y4m_files_temporal(const char *noisy, const char *clean, const char *out_report, const char *out_treport,
                                       const g1s_measure_opts_t *opts, int *unequal, char *err, size_t cap) {
  return g1s_measure_y4m_files_modes(noisy, clean, out_report, out_treport, nullptr, opts, unequal, err, cap);
}

int64_t g1s_measure_y4m_files_modes(const char *noisy, const char *clean, const char *out_report, const char *out_treport, const char *out_xreport,
                                    const g1s_measure_opts_t *opts, int *unequal, char *err, size_t cap) {
  return g1s_measure_y4m_files_scales(noisy, clean, out_report, out_treport, out_xreport, nullptr, opts, unequal, err, cap);
}

int64_t g1s_measure_y4m_files_scales(const char *noisy, const char *clean, const char *out_report, const char *out_treport, const char *out_xreport,
                                     const char *out_sreport, const g1s_measure_opts_t *opts, int *unequal, char *err, size_t cap) {
  if (unequal) *unequal = 0;
  if (!noisy || !clean || !out_report) return refuse(err, cap, G1S_ERR_INVALID, "null path");
  TwoClips clips;
  if (!clips.open(noisy, clean, err, cap)) return G1S_ERR_INVALID;
  g1s_measure_t *m = nullptr;
  std::string why;
  int64_t frames = 0;
  const ReportPaths out{out_report, out_treport, out_xreport, out_sreport};
  const uint32_t batch = batch_of(opts ? opts->batch_frames : 0);
  ClipTotals totals;
  int rc = clips_refusal(clips, out, &why);
  if (!rc && !(m = meter_for(out, clips.ia.bit_depth, opts))) rc = G1S_ERR_NO_DEVICE, why = g1s_last_global_error();
  while (!rc) {
    g1s_frame_t fa, fb;
    const int got = next_clip_pair(clips, frames, &fa, &fb, unequal, &why);
    if (got <= 0) {
      rc = got;
      break;
    }
    fa.on_device = fb.on_device = 0;  // (the readers lend the frames until their next call: copied before the call returns)
    if ((rc = g1s_measure_frame(m, &fa, &fb)) != 0) {
      why = "frame " + std::to_string(frames) + ": " + g1s_measure_last_error(m);
      break;
    }
    ++frames;
    if (frames % batch == 0 && !(why = totals.take(m, out)).empty()) rc = G1S_ERR_INVALID;
  }
  if (!rc && !(why = totals.take(m, out)).empty()) rc = G1S_ERR_INVALID;
  if (!rc && !(why = write_reports(out, totals, nullptr, (uint64_t)frames, clips.ia)).empty()) rc = G1S_ERR_INVALID;
  g1s_measure_free(m);
  return rc ? refuse(err, cap, rc, why) : frames;
}

int64_t g1s_check_y4m_files(const char *source, const char *denoised, const char *tbl, const char *out_report, const g1s_measure_opts_t *opts,
                            const g1s_grain_opts_t *gopts, int *unequal, char *err, size_t cap) {
  return g1s_check_y4m_files_temporal(source, denoised, tbl, out_report, nullptr, opts, gopts, unequal, err, cap);
}

int64_t g1s_check_y4m_files_temporal(const char *source, const char *denoised, const char *tbl, const char *out_report, const char *out_treport,
                                     const g1s_measure_opts_t *opts, const g1s_grain_opts_t *gopts, int *unequal, char *err, size_t cap) {
  return g1s_check_y4m_files_modes(source, denoised, tbl, out_report, out_treport, nullptr, opts, gopts, unequal, err, cap);
}

int64_t g1s_check_y4m_files_modes(const char *source, const char *denoised, const char *tbl, const char *out_report, const char *out_treport,
                                  const char *out_xreport, const g1s_measure_opts_t *opts, const g1s_grain_opts_t *gopts, int *unequal, char *err,
                                  size_t cap) {
  return g1s_check_y4m_files_scales(source, denoised, tbl, out_report, out_treport, out_xreport, nullptr, opts, gopts, unequal, err, cap);
}

int64_t g1s_check_y4m_files_scales(const char *source, const char *denoised, const char *tbl, const char *out_report, const char *out_treport,
                                   const char *out_xreport, const char *out_sreport, const g1s_measure_opts_t *opts, const g1s_grain_opts_t *gopts,
                                   int *unequal, char *err, size_t cap) {
  if (unequal) *unequal = 0;
  if (!source || !denoised || !tbl || !out_report) return refuse(err, cap, G1S_ERR_INVALID, "null path");
  std::vector<g1s_segment_t> segs;
  std::string why;
  int rc = load_table(tbl, g1s_parse_tbl, segs, "cannot open ", "grain table: ", &why);
  if (rc) return refuse(err, cap, rc, why);
  TwoClips clips;
  if (!clips.open(source, denoised, err, cap)) return G1S_ERR_INVALID;
  const g1s_y4m_info_t &id = clips.ib;
  const PlaneGeom pg(id);
  const Layout lay = staging_layout(pg);
  g1s_measure_t *ms = nullptr, *mr = nullptr;  // source - denoised; rendered - denoised
  g1s_grain_t *gr = nullptr;
  DevBuf<uint8_t> d_src, d_den, d_ren;  // a group of frames each: the source, the denoised, the rendered
  int64_t frames = 0;
  uint32_t in_group = 0;
  const uint32_t group = batch_of(opts ? opts->batch_frames : 0);
  const ReportPaths out{out_report, out_treport, out_xreport, out_sreport};
  ClipTotals total_s, total_r;
  rc = clips_refusal(clips, out, &why);
  if (!rc && (!(ms = meter_for(out, id.bit_depth, opts)) || !(mr = meter_for(out, id.bit_depth, opts)))) rc = G1S_ERR_NO_DEVICE, why = g1s_last_global_error();
  if (!rc) {
    g1s_grain_opts_t go{};
    if (gopts) go = *gopts;
    go.struct_size = sizeof go, go.device = g1s_measure_device_(ms), go.batch_frames = group;  // one device, one group size
    if (!(gr = g1s_grain_new(id.bit_depth, &go))) rc = G1S_ERR_NO_DEVICE, why = g1s_last_global_error();
  }
  if (!rc) {
    (void)hipSetDevice(g1s_measure_device_(ms));
    if (hipMalloc((void **)&d_src.p, lay.frame * group) != hipSuccess || hipMalloc((void **)&d_den.p, lay.frame * group) != hipSuccess ||
        hipMalloc((void **)&d_ren.p, lay.frame * group) != hipSuccess)
      rc = G1S_ERR_HIP, why = "hipMalloc of the frame buffers failed";
  }
  auto slot = [&](const DevBuf<uint8_t> &buf, uint32_t k) { return device_frame(pg, lay, buf + lay.frame * k); };
  // a group is through: its renders complete (the synthesizer has a stream of its own) before the meters read them, both
  // meters' batches out and waited for, so that the group's buffers are free again
  auto end_group = [&]() {
    if ((rc = g1s_grain_sync(gr)) != 0) why = std::string("render: ") + g1s_grain_last_error(gr);
    for (uint32_t k = 0; k < in_group && !rc; ++k) {
      const g1s_frame_t s = slot(d_src, k), d = slot(d_den, k), r = slot(d_ren, k);
      if ((rc = g1s_measure_frame(ms, &s, &d)) != 0) why = std::string("measure: ") + g1s_measure_last_error(ms);
      else if ((rc = g1s_measure_frame(mr, &r, &d)) != 0) why = std::string("measure: ") + g1s_measure_last_error(mr);
    }
    // (a temporal meter keeps a copy of the group's last pair on the device: the group's buffers are free again all the same)
    if (!rc && !(why = total_s.take(ms, out)).empty()) rc = G1S_ERR_INVALID;
    if (!rc && !(why = total_r.take(mr, out)).empty()) rc = G1S_ERR_INVALID;
    in_group = 0;
  };
  while (!rc) {
    g1s_frame_t fs, fd;
    const int got = next_clip_pair(clips, frames, &fs, &fd, unequal, &why);
    if (got <= 0) {
      rc = got;
      break;
    }
    // both frames to the device, once (the readers lend them until their next call)
    const g1s_frame_t s = slot(d_src, in_group), d = slot(d_den, in_group);
    g1s_frame_t r = slot(d_ren, in_group);
    if (!upload_frame(fs, s) || !upload_frame(fd, d)) {
      rc = G1S_ERR_HIP, why = "copy of a frame pair to the device failed";
      break;
    }
    // the table's lookup at the frame's presentation time, as `render` makes it; no segment: rendered = denoised
    const long si = g1s_tbl_segment_for(segs.data(), segs.size(), g1s::frame_time((uint64_t)frames, id.fps_num, id.fps_den));
    if ((rc = g1s_grain_frame(gr, si < 0 ? nullptr : &segs[(size_t)si], &d, &r)) != 0) {
      why = "frame " + std::to_string(frames) + ": render: " + g1s_grain_last_error(gr);
      break;
    }
    ++frames;
    if (++in_group == group) end_group();
  }
  if (!rc && in_group) end_group();
  if (!rc && !(why = write_reports(out, total_s, &total_r, (uint64_t)frames, id)).empty()) rc = G1S_ERR_INVALID;
  if (ms) (void)hipSetDevice(g1s_measure_device_(ms));
  g1s_grain_free(gr);
  g1s_measure_free(mr);
  g1s_measure_free(ms);
  return rc ? refuse(err, cap, rc, why) : frames;
}

}  // extern "C"
