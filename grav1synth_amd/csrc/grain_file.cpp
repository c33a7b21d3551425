// grain_file.cpp -- the file command of `render` (g1s_grain_y4m_file): a .y4m file and a grain table into a .y4m file.
// Host code above the per-frame ABI of grain.hip: it launches no kernel and sees the synthesizer through g1s_grain_* alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "clip_file.h"
#include "fold.h"
#include "frame_op.h"

using namespace g1s_op;

extern "C" int64_t g1s_grain_y4m_file(const char *in, const char *tbl, const char *out, const g1s_grain_opts_t *opts, char *err, size_t cap) {
  if (!in || !tbl || !out) return g1s_clip::refuse(err, cap, G1S_ERR_INVALID, "null path");
  std::vector<g1s_segment_t> segs;
  std::string why;
  const int rc = g1s_clip::load_table(tbl, g1s_parse_tbl, segs, "cannot open ", "grain table: ", &why);
  if (rc) return g1s_clip::refuse(err, cap, rc, why);
  // a batch of output frames in pinned memory: rendered, waited for (everything handed over is then complete), written
  struct Driver {
    const g1s_grain_opts_t *opts;
    std::vector<g1s_segment_t> &segs;
    g1s_y4m_info_t info{};
    g1s_grain_t *g = nullptr;
    const int new_failed = G1S_ERR_NO_DEVICE;
    bool open(const g1s_y4m_info_t &i) { return info = i, (g = g1s_grain_new(i.bit_depth, opts)) != nullptr; }
    uint32_t batch() const { return batch_of(opts ? opts->batch_frames : 0); }  // (the synthesizer's own)
    uint32_t ring() const { return batch(); }
    int frame(int64_t n, const g1s_frame_t *fin, g1s_frame_t *fout) {
      const long si = g1s_tbl_segment_for(segs.data(), segs.size(), g1s::frame_time((uint64_t)n, info.fps_num, info.fps_den));
      return g1s_grain_frame(g, si < 0 ? nullptr : &segs[(size_t)si], fin, fout);
    }
    int drain(bool, uint64_t *) { return g1s_grain_sync(g); }
    const char *last_error() const { return g1s_grain_last_error(g); }
    void close() { g1s_grain_free(g); }
  };
  return rewrite_y4m(in, out, err, cap, Driver{opts, segs});
}
