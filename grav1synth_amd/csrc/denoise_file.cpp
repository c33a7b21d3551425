// denoise_file.cpp -- the file commands of `denoise`: `denoise INPUT -o OUTPUT` (g1s_denoise_y4m_file*) and `diff SOURCE --denoise
// -o TABLE` (g1s_diff_y4m_file_denoised*).  Host code above the per-frame ABI of denoise.hip: it launches no kernel and
// sees the denoiser through g1s_denoise_* and two accessors.  Every exported rung fills a FileSpec with its defaults; one
// recipe (Recipe::prepare) makes the grain prior and the effective options for both commands, one runner each does the rest.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <deque>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "clip_file.h"
#include "curve.h"
#include "frame_op.h"
#include "nlf.h"

extern "C" int32_t g1s_diff_device_(const g1s_diff_t *);
extern "C" uint32_t g1s_diff_frames_in_flight_max_(const g1s_diff_t *);
extern "C" uint32_t g1s_denoise_batch_(const g1s_denoise_t *);
extern "C" uint32_t g1s_denoise_temporal_radius_(const g1s_denoise_t *);
extern "C" void g1s_denoise_levels_refusal_(const g1s_denoise_opts_t *, uint32_t coarse_levels, double coarse_ratio, char *err, size_t cap);

using namespace g1s_op;
using g1s_clip::refuse;

namespace {

// what a file command takes beyond its paths and its opts: what the last rung of either ladder takes, with the values an
// earlier rung stands for
struct FileSpec {
  uint32_t temporal_radius = 0, flags = 0;
  const char *prior_tbl = nullptr;
  uint32_t prior_range = 0;
  int32_t prior_segment = -1;
  uint32_t motion_range = 0, auto_flags = 0;
  uint64_t profile_frames = 0, min_count = 0;
  uint32_t chroma_prior = 0;
  uint32_t coarse_levels = 0;
  double coarse_ratio = 0.0;
  uint32_t auto_temporal = 0;
};

// A grain prior as the file commands take it: the table at `path`, its segment `segment` alone or (negative) the mean of
// all of them, range R (0 = the default).  load() reads and parses; make() is g1s_denoise_curve for the clip's depth.
// measure() is the other way to one: the noise levels of the clip itself (rules N5 - N6) through g1s_denoise_curve_sigma.
struct Prior {
  std::vector<g1s_segment_t> segs;
  uint32_t range = 0;
  std::vector<uint16_t> pair_fwd, pair_inv;  // a curve that is there already (a measured prior): make() hands it on
  bool chroma = false;         // the prior extends to chroma (rules 21 - 24): load() and measure() also make the gain
  std::vector<uint16_t> gain;  // m[256] then; else empty
  std::string load(const char *path, uint32_t range_, int32_t segment) {
    range = range_;
    std::string why;
    if (g1s_clip::load_table(path, g1s_parse_tbl, segs, "grain prior: cannot open ", "grain prior: ", &why)) return why;
    const size_t nseg = segs.size();
    if (segment >= 0 && (size_t)segment >= nseg)
      return "grain prior: segment " + std::to_string(segment) + " is not in the table (" + std::to_string(nseg) + " segments)";
    if (segment >= 0) segs = {segs[(size_t)segment]};
    if (chroma) {  // rule 22 on the segments in hand, rule 21
      gain.assign(g1s_cv::kGainEntries, 0);
      return g1s_cv::build_gain(segs.data(), segs.size(), range, gain.data());
    }
    return "";
  }
  std::string make(uint32_t bit_depth, std::vector<uint16_t> &fwd, std::vector<uint16_t> &inv) const {
    if (!pair_fwd.empty()) {
      fwd = pair_fwd, inv = pair_inv;
      return "";
    }
    fwd.assign((size_t)1 << (bit_depth <= 12 ? bit_depth : 12), 0), inv.assign(g1s_cv::kInvEntries, 0);
    return g1s_cv::build(segs.data(), segs.size(), bit_depth, range, fwd.data(), inv.data());
  }
  // `luma_s(s)` and `chroma_s(s)`: the two scaling functions of the clip's record, the ordinary one's (N6, N9) or the
  // temporal one's (T7)
  template <class LumaS, class ChromaS>
  std::string measure(uint32_t bit_depth, uint32_t range_, LumaS luma_s, ChromaS chroma_s) {
    std::string why = g1s_cv::check_depth_range(bit_depth, range_);
    if (!why.empty()) return why;
    std::vector<uint8_t> sg((size_t)1 << bit_depth);
    if (!(why = luma_s(sg.data())).empty()) return why;
    pair_fwd.assign((size_t)1 << bit_depth, 0), pair_inv.assign(g1s_cv::kInvEntries, 0);
    if (!(why = g1s_cv::build_sigma(sg.data(), bit_depth, range_, pair_fwd.data(), pair_inv.data())).empty() || !chroma) return why;
    uint8_t sc[g1s_cv::kGainEntries];  // rule 23 on the same record, rule 21
    if (!(why = chroma_s(sc)).empty()) return why;
    gain.assign(g1s_cv::kGainEntries, 0);
    return g1s_cv::gain_from_s(sc, range_, gain.data());
  }
};

// The pre-pass of the auto flags: their refusals, the noise levels of the first profile_frames frames of `source` on
// `device`, then the prior's curve into *prior (G1S_AUTO_PRIOR) and the two strengths into *d (G1S_AUTO_STRENGTH).
// Under auto_temporal the meter is a temporal one and the values are rule T7's.  "" when fine.
std::string auto_prepass(const char *source, int32_t device, const FileSpec &s, Prior *prior, g1s_denoise_opts_t *d) {
  if (s.auto_flags & ~(G1S_AUTO_PRIOR | G1S_AUTO_STRENGTH)) return "unknown auto flags";
  if ((s.auto_flags & G1S_AUTO_PRIOR) && s.prior_tbl) return "an auto prior does not combine with a grain prior table";
  if ((s.auto_flags & G1S_AUTO_STRENGTH) && (d->strength != 0.0 || d->chroma_strength != 0.0)) return "an auto strength does not combine with a given strength";
  if (!source) return "null path";
  struct stat st;
  if (stat(source, &st) == 0 && !S_ISREG(st.st_mode)) return std::string(source) + " cannot be read twice (not a regular file): the auto flags need a pre-pass";
  g1s_nlf_opts_t no{};
  no.struct_size = sizeof no, no.device = device;
  g1s_nlf_record_t total;
  g1s_nlf_trecord_t ttotal;
  char err[512] = "";
  const int64_t n = s.auto_temporal ? g1s_nlf_y4m_file_temporal(source, nullptr, nullptr, &no, s.profile_frames, nullptr, &ttotal, err, sizeof err)
                                    : g1s_nlf_y4m_file(source, nullptr, &no, s.profile_frames, &total, err, sizeof err);
  if (n < 0) return err;
  if (s.auto_temporal && n < 2) return "temporal noise levels need two frames";
  g1s_y4m_t *y = g1s_y4m_open(source, err, sizeof err);
  if (!y) return err;
  g1s_y4m_info_t info;
  g1s_y4m_get_info(y, &info);
  g1s_y4m_close(y);
  const uint32_t bd = info.bit_depth;
  const bool t = s.auto_temporal != 0;
  if (s.auto_flags & G1S_AUTO_PRIOR) {
    const std::string why = prior->measure(
        bd, s.prior_range, [&](uint8_t *sg) { return t ? g1s_nl::sigma_t(ttotal, 0, bd, s.min_count, sg) : g1s_nl::sigma(total, bd, s.min_count, sg); },
        [&](uint8_t *sc) { return t ? g1s_nl::sigma_t(ttotal, 1, 8, s.min_count, sc) : g1s_nl::chroma_sigma(total, s.min_count, sc); });
    if (!why.empty()) return why;
  }
  if (s.auto_flags & G1S_AUTO_STRENGTH) {
    auto strength = [&](uint32_t plane_class, double *h) {
      return t ? g1s_nl::strength_t(ttotal, bd, s.min_count, plane_class, h) : g1s_nl::strength(total, bd, s.min_count, plane_class, h);
    };
    const std::string why = strength(0, &d->strength);
    if (!why.empty()) return why;
    double hc = 0;  // (where the chroma strength is refused: the luma strength)
    if (strength(1, &hc).empty()) d->chroma_strength = hc;
  }
  return "";
}

// the refusals of a chroma prior that need neither the table nor the clip.  "" when fine.
std::string chroma_prior_refusal(const FileSpec &s) {
  if (s.chroma_prior > 1) return "chroma_prior is 0 or 1";
  if (!s.prior_tbl && !(s.auto_flags & G1S_AUTO_PRIOR)) return "a chroma prior needs a grain prior (a table or the clip's own levels)";
  if (!(s.flags & G1S_DENOISE_JOINT_CHROMA)) return "a chroma gain needs joint chroma";
  return "";
}

// What a file command runs with: the prior (or none) and the effective opts, and how to make the denoiser from them.
struct Recipe {
  FileSpec s;
  Prior prior;
  bool has_prior = false;
  g1s_denoise_opts_t own{};                  // the caller's opts with the measured strengths, where a flag asks for a copy
  const g1s_denoise_opts_t *opts = nullptr;  // &own, or the caller's as they came: then struct_size is the constructor's to check
  // `prepass_device`: where the pre-pass runs; null: on the effective opts' device.  Returns the refusal's text, "" when fine.
  // Without chroma_prior and auto flags only the table is loaded.  Under either, in this order: the chroma prior's own
  // refusals, struct_size, the pre-pass with its refusals, the table.
  std::string prepare(const char *source, const g1s_denoise_opts_t *caller, const int32_t *prepass_device) {
    opts = caller, has_prior = s.prior_tbl || s.chroma_prior || (s.auto_flags & G1S_AUTO_PRIOR);
    if (s.auto_temporal > 1) return "auto_temporal is 0 or 1";
    if (s.auto_temporal && !s.auto_flags) return "temporal noise levels need an auto flag (an auto prior or an auto strength)";
    if (s.chroma_prior || s.auto_flags) {
      std::string why = s.chroma_prior ? chroma_prior_refusal(s) : "";
      if (!why.empty()) return why;
      if (caller && caller->struct_size != sizeof(g1s_denoise_opts_t)) return "g1s_denoise_opts_t.struct_size mismatch";
      prior.chroma = s.chroma_prior != 0;
      if (caller) own = *caller;
      own.struct_size = sizeof own;
      if (!caller) own.device = -1;
      opts = &own;
      if (s.auto_flags && !(why = auto_prepass(source, prepass_device ? *prepass_device : own.device, s, &prior, &own)).empty()) return why;
    }
    return s.prior_tbl ? prior.load(s.prior_tbl, s.prior_range, s.prior_segment) : "";
  }
  // the denoiser for a clip of this depth on `device` (negative: the effective opts'); NULL with the global error text set
  g1s_denoise_t *open(uint32_t bit_depth, int32_t device = -1) const {
    g1s_denoise_opts_t d{};
    if (device >= 0) {
      if (opts) d = *opts;
      d.struct_size = sizeof d, d.device = device;
    }
    std::vector<uint16_t> fwd, inv;
    const std::string why = has_prior ? prior.make(bit_depth, fwd, inv) : "";
    if (!why.empty()) {
      g1s_set_global_error_(why.c_str());
      return nullptr;
    }
    return g1s_denoise_new_levels(bit_depth, device >= 0 ? &d : opts, s.temporal_radius, s.flags, has_prior ? fwd.data() : nullptr,
                                  has_prior ? inv.data() : nullptr, s.motion_range, prior.gain.empty() ? nullptr : prior.gain.data(), s.coarse_levels,
                                  s.coarse_ratio);
  }
};

// `denoise INPUT -o OUTPUT`
int64_t denoise_y4m_file(const char *in, const char *out, const g1s_denoise_opts_t *opts, const FileSpec &s, char *err, size_t cap) {
  Recipe r{s};
  const std::string why = r.prepare(in, opts, nullptr);
  if (!why.empty()) return refuse(err, cap, G1S_ERR_INVALID, why);
  // a ring of output frames in pinned memory: denoised, waited for, written.  The file is one clip: between two drains a
  // batch is handed over, and the denoiser holds the last D frames back, so batch + D frames can be unwritten
  struct Driver {
    const Recipe &r;
    g1s_denoise_t *g = nullptr;
    const int new_failed = G1S_ERR_INVALID;
    bool open(const g1s_y4m_info_t &i) { return (g = r.open(i.bit_depth)) != nullptr; }
    uint32_t batch() const { return g1s_denoise_batch_(g); }
    uint32_t ring() const { return g1s_denoise_batch_(g) + g1s_denoise_temporal_radius_(g); }
    int frame(int64_t, const g1s_frame_t *fin, g1s_frame_t *fout) { return g1s_denoise_frame(g, fin, fout); }
    int drain(bool end, uint64_t *complete) { return end ? g1s_denoise_sync(g) : g1s_denoise_drain(g, complete); }
    const char *last_error() const { return g1s_denoise_last_error(g); }
    void close() { g1s_denoise_free(g); }
  };
  return rewrite_y4m(in, out, err, cap, Driver{r});
}

// `diff SOURCE --denoise -o TABLE`: the source is read once and copied to the device once; the denoiser writes its
// output beside it and the generator takes the pair as device frames.  A pair's two buffers belong to the generator
// until g1s_diff_frames_released() covers the frame, and its source buffer is a neighbour of the D frames after it until the
// denoiser is past those; then they are used again.  The file is one clip: the denoiser is drained once a group, not
// synchronised, and only the frames it has completed go on to the generator.
int diff_y4m_file_denoised(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts, const g1s_denoise_opts_t *dopts,
                           const FileSpec &spec, uint64_t *frames_out, char *err, size_t cap) {
  if (frames_out) *frames_out = 0;
  if (!source || !out_tbl) return refuse(err, cap, G1S_ERR_INVALID, "null path");
  if (spec.flags & ~G1S_DENOISE_JOINT_CHROMA) return refuse(err, cap, G1S_ERR_INVALID, "unknown denoise flags");
  {  // (rule 28's refusals need no device either; the generator is made before the denoiser, so they are looked at here)
    char no[160] = "";
    g1s_denoise_levels_refusal_(dopts, spec.coarse_levels, spec.coarse_ratio, no, sizeof no);
    if (no[0]) return refuse(err, cap, G1S_ERR_INVALID, no);
  }
  Recipe recipe{spec};
  const int32_t generator_device = opts ? opts->device : -1;
  std::string why = recipe.prepare(source, dopts, &generator_device);
  if (!why.empty()) return refuse(err, cap, G1S_ERR_INVALID, why);

  const std::string header = y4m_header_line(source);
  g1s_y4m_t *y = g1s_y4m_open(source, err, cap);
  if (!y) return G1S_ERR_INVALID;
  g1s_y4m_info_t info;
  g1s_y4m_get_info(y, &info);
  const PlaneGeom pg(info);
  const Layout lay = packed_layout(pg);
  g1s_diff_t *g = nullptr;
  g1s_denoise_t *dn = nullptr;
  FILE *fk = nullptr;
  PinnedBuf<uint8_t> kbuf;
  struct Pair {
    DevBuf<uint8_t> src, den;
  };
  std::vector<Pair> pairs;                          // every pair of buffers allocated so far
  std::deque<std::pair<uint64_t, size_t>> lent;     // (frame index, pair) handed to the generator, oldest first
  std::deque<size_t> held;                          // pairs of the frames the denoiser has not completed, oldest first
  std::vector<size_t> spare;
  size_t pair_cap = 0;
  uint64_t frames = 0, taken = 0, complete = 0;     // frames handed to the generator; to the denoiser; completed by it
  uint32_t D = 0, batch = 0;
  int rc = G1S_OK;

  g = g1s_diff_new(info.fps_num, info.fps_den, info.bit_depth, info.bit_depth, opts);
  if (!g) {
    rc = G1S_ERR_NO_DEVICE, why = g1s_last_global_error();
    goto done;
  }
  dn = recipe.open(info.bit_depth, g1s_diff_device_(g));  // one device: the pair never leaves it
  if (!dn) {
    rc = G1S_ERR_INVALID, why = g1s_last_global_error();
    goto done;
  }
  (void)hipSetDevice(g1s_diff_device_(g));
  if (keep_denoised) {
    fk = std::fopen(keep_denoised, "wb");
    if (!fk || std::fwrite(header.data(), 1, header.size(), fk) != header.size() ||
        hipHostMalloc((void **)&kbuf.p, lay.frame, hipHostMallocDefault) != hipSuccess) {
      rc = G1S_ERR_INVALID, why = std::string("cannot write ") + keep_denoised;
      goto done;
    }
  }
  // buffers for two groups until the generator has said how many frames it can hold (after the first hand-over), and for
  // the window: the D frames the denoiser holds back and the D before them that are still their neighbours
  D = g1s_denoise_temporal_radius_(dn), batch = g1s_denoise_batch_(dn);
  pair_cap = 2 * (size_t)batch + 2 * D;
  for (bool eof = false; !eof && !rc;) {
    // ---- one group: up to batch_frames frames to the device and to the denoiser
    for (uint32_t in_group = 0; in_group < batch; ++in_group) {
      g1s_frame_t fin;
      const int got = g1s_y4m_next(y, &fin);
      if (got < 0) {
        rc = got, why = "frame " + std::to_string(taken) + ": source reader failed (" + g1s_y4m_last_error(y) + ")";
        break;
      }
      if (got == 0) {
        eof = true;
        break;
      }
      // a pair of buffers: one that the generator has released and the denoiser is past (frame t + D complete), a new one,
      // or -- the ring is full -- wait for the generator
      size_t k;
      uint64_t released = g1s_diff_frames_released(g);
      auto reclaim = [&] {
        while (!lent.empty() && lent.front().first < released && lent.front().first + D < complete) spare.push_back(lent.front().second), lent.pop_front();
      };
      reclaim();
      if (spare.empty() && pairs.size() >= pair_cap) {
        rc = g1s_diff_sync(g);
        if (rc) {
          why = std::string("diff_frame: ") + g1s_diff_last_error(g);
          break;
        }
        released = frames;
        reclaim();
      }
      if (!spare.empty()) {
        k = spare.back(), spare.pop_back();
      } else {
        Pair p;
        if (hipMalloc((void **)&p.src.p, lay.frame) != hipSuccess || hipMalloc((void **)&p.den.p, lay.frame) != hipSuccess) {
          rc = G1S_ERR_HIP, why = "hipMalloc of a frame pair failed";
          break;
        }
        pairs.push_back(std::move(p)), k = pairs.size() - 1;
      }
      // the reader lends the frame until its next call: on the device before that
      const g1s_frame_t s = device_frame(pg, lay, pairs[k].src);
      g1s_frame_t d = device_frame(pg, lay, pairs[k].den);
      if (!upload_frame(fin, s)) {
        rc = G1S_ERR_HIP, why = "copy of a source frame to the device failed";
        break;
      }
      rc = g1s_denoise_frame(dn, &s, &d);
      if (rc) {
        why = "frame " + std::to_string(taken) + ": denoise: " + g1s_denoise_last_error(dn);
        break;
      }
      held.push_back(k), ++taken;
    }
    if (rc) break;
    // the end of the file is the end of the clip; before it the last D frames stay with the denoiser
    rc = eof ? g1s_denoise_sync(dn) : g1s_denoise_drain(dn, &complete);
    if (rc) {
      why = std::string("denoise: ") + g1s_denoise_last_error(dn);
      break;
    }
    if (eof) complete = taken;
    // ---- the completed frames' pairs to the generator, the denoised frames to the kept file
    while (frames < complete) {
      const size_t k = held.front();
      held.pop_front();
      const g1s_frame_t s = device_frame(pg, lay, pairs[k].src), d = device_frame(pg, lay, pairs[k].den);
      rc = g1s_diff_frame(g, &s, &d);
      if (rc) {
        why = "frame " + std::to_string(frames) + ": diff_frame: " + g1s_diff_last_error(g);
        break;
      }
      lent.emplace_back(frames, k);
      if (fk && (hipMemcpy(kbuf, pairs[k].den, lay.frame, hipMemcpyDeviceToHost) != hipSuccess || std::fwrite("FRAME\n", 1, 6, fk) != 6 ||
                 std::fwrite(kbuf, 1, lay.frame, fk) != lay.frame)) {
        rc = G1S_ERR_INVALID, why = std::string("cannot write ") + keep_denoised;
        break;
      }
      ++frames;
    }
    if (rc) break;
    if (const uint32_t inside = g1s_diff_frames_in_flight_max_(g)) pair_cap = std::max(pair_cap, (size_t)batch + inside + inside / 4 + 2 * D);
  }
  if (rc) goto done;
  rc = g1s_clip::write_table(
      out_tbl, [&](g1s_segment_t *out, size_t cap_, size_t *n) { return g1s_diff_finish(g, out, cap_, n); }, [&] { return g1s_diff_last_error(g); }, &why);
done:
  if (fk && std::fclose(fk) != 0 && !rc) rc = G1S_ERR_INVALID, why = std::string("cannot write ") + keep_denoised;
  if (dn) g1s_denoise_free(dn);
  if (g) g1s_diff_free(g);  // (waits for the kernels that read the pairs, which go when this call returns)
  g1s_y4m_close(y);
  if (frames_out) *frames_out = frames;
  if (rc) return refuse(err, cap, rc, why);
  return G1S_OK;
}

}  // namespace

// every rung: the last rung's arguments, the ones it does not take at their defaults
extern "C" {

int64_t g1s_denoise_y4m_file(const char *in, const char *out, const g1s_denoise_opts_t *opts, char *err, size_t cap) {
  return denoise_y4m_file(in, out, opts, {}, err, cap);
}

int64_t g1s_denoise_y4m_file_temporal(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, char *err,
                                      size_t cap) {
  return denoise_y4m_file(in, out, opts, {temporal_radius}, err, cap);
}

int64_t g1s_denoise_y4m_file_ex(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags, char *err,
                                size_t cap) {
  return denoise_y4m_file(in, out, opts, {temporal_radius, flags}, err, cap);
}

int64_t g1s_denoise_y4m_file_curve(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                   const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, char *err, size_t cap) {
  return denoise_y4m_file(in, out, opts, {temporal_radius, flags, prior_tbl, prior_range, prior_segment}, err, cap);
}

int64_t g1s_denoise_y4m_file_motion(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                    const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, char *err, size_t cap) {
  return denoise_y4m_file(in, out, opts, {temporal_radius, flags, prior_tbl, prior_range, prior_segment, motion_range}, err, cap);
}

int64_t g1s_denoise_y4m_file_auto(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                  const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags,
                                  uint64_t profile_frames, uint64_t min_count, char *err, size_t cap) {
  return denoise_y4m_file(in, out, opts, {temporal_radius, flags, prior_tbl, prior_range, prior_segment, motion_range, auto_flags, profile_frames, min_count},
                          err, cap);
}

int64_t g1s_denoise_y4m_file_chroma(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                    const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags,
                                    uint64_t profile_frames, uint64_t min_count, uint32_t chroma_prior, char *err, size_t cap) {
  return denoise_y4m_file(in, out, opts, {temporal_radius, flags, prior_tbl, prior_range, prior_segment, motion_range, auto_flags, profile_frames, min_count,
                                          chroma_prior}, err, cap);
}

int64_t g1s_denoise_y4m_file_levels(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                    const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags,
                                    uint64_t profile_frames, uint64_t min_count, uint32_t chroma_prior, uint32_t coarse_levels, double coarse_ratio, char *err,
                                    size_t cap) {
  return denoise_y4m_file(in, out, opts, {temporal_radius, flags, prior_tbl, prior_range, prior_segment, motion_range, auto_flags, profile_frames, min_count,
                                          chroma_prior, coarse_levels, coarse_ratio}, err, cap);
}

int64_t g1s_denoise_y4m_file_auto_temporal(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                           const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags,
                                           uint64_t profile_frames, uint64_t min_count, uint32_t chroma_prior, uint32_t coarse_levels, double coarse_ratio,
                                           uint32_t auto_temporal, char *err, size_t cap) {
  return denoise_y4m_file(in, out, opts, {temporal_radius, flags, prior_tbl, prior_range, prior_segment, motion_range, auto_flags, profile_frames, min_count,
                                          chroma_prior, coarse_levels, coarse_ratio, auto_temporal}, err, cap);
}

int g1s_diff_y4m_file_denoised(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                               const g1s_denoise_opts_t *dopts, uint64_t *frames_out, char *err, size_t cap) {
  return diff_y4m_file_denoised(source, out_tbl, keep_denoised, opts, dopts, {}, frames_out, err, cap);
}

int g1s_diff_y4m_file_denoised_temporal(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                        const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint64_t *frames_out, char *err, size_t cap) {
  return diff_y4m_file_denoised(source, out_tbl, keep_denoised, opts, dopts, {temporal_radius}, frames_out, err, cap);
}

int g1s_diff_y4m_file_denoised_ex(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                  const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, uint64_t *frames_out, char *err,
                                  size_t cap) {
  return diff_y4m_file_denoised(source, out_tbl, keep_denoised, opts, dopts, {temporal_radius, flags}, frames_out, err, cap);
}

int g1s_diff_y4m_file_denoised_curve(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                     const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                     uint32_t prior_range, int32_t prior_segment, uint64_t *frames_out, char *err, size_t cap) {
  return diff_y4m_file_denoised(source, out_tbl, keep_denoised, opts, dopts, {temporal_radius, flags, prior_tbl, prior_range, prior_segment}, frames_out, err,
                                cap);
}

int g1s_diff_y4m_file_denoised_motion(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                      const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                      uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint64_t *frames_out, char *err,
                                      size_t cap) {
  return diff_y4m_file_denoised(source, out_tbl, keep_denoised, opts, dopts, {temporal_radius, flags, prior_tbl, prior_range, prior_segment, motion_range},
                                frames_out, err, cap);
}

int g1s_diff_y4m_file_denoised_auto(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                    const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                    uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags, uint64_t profile_frames,
                                    uint64_t min_count, uint64_t *frames_out, char *err, size_t cap) {
  return diff_y4m_file_denoised(source, out_tbl, keep_denoised, opts, dopts,
                                {temporal_radius, flags, prior_tbl, prior_range, prior_segment, motion_range, auto_flags, profile_frames, min_count}, frames_out,
                                err, cap);
}

int g1s_diff_y4m_file_denoised_chroma(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                      const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                      uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags, uint64_t profile_frames,
                                      uint64_t min_count, uint32_t chroma_prior, uint64_t *frames_out, char *err, size_t cap) {
  return diff_y4m_file_denoised(source, out_tbl, keep_denoised, opts, dopts,
                                {temporal_radius, flags, prior_tbl, prior_range, prior_segment, motion_range, auto_flags, profile_frames, min_count, chroma_prior},
                                frames_out, err, cap);
}

int g1s_diff_y4m_file_denoised_levels(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                      const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                      uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags, uint64_t profile_frames,
                                      uint64_t min_count, uint32_t chroma_prior, uint32_t coarse_levels, double coarse_ratio, uint64_t *frames_out, char *err,
                                      size_t cap) {
  return diff_y4m_file_denoised(source, out_tbl, keep_denoised, opts, dopts,
                                {temporal_radius, flags, prior_tbl, prior_range, prior_segment, motion_range, auto_flags, profile_frames, min_count, chroma_prior,
                                 coarse_levels, coarse_ratio},
                                frames_out, err, cap);
}

int g1s_diff_y4m_file_denoised_auto_temporal(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                             const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                             uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags, uint64_t profile_frames,
                                             uint64_t min_count, uint32_t chroma_prior, uint32_t coarse_levels, double coarse_ratio, uint32_t auto_temporal,
                                             uint64_t *frames_out, char *err, size_t cap) {
  return diff_y4m_file_denoised(source, out_tbl, keep_denoised, opts, dopts,
                                {temporal_radius, flags, prior_tbl, prior_range, prior_segment, motion_range, auto_flags, profile_frames, min_count, chroma_prior,
                                 coarse_levels, coarse_ratio, auto_temporal},
                                frames_out, err, cap);
}

}  // extern "C"
