// host_abi.cpp -- the part of the C ABI (include/g1s_diff.h) that needs no device: the worker pools, the record accessors,
// the messages of the frame-shard protocol and their ordered merge, the stand-alone fold handle, latest-state blobs from
// records, the .tbl calls and the thread's global error text.  Builds with a host compiler; what takes a g1s_diff_t * is
// in engine.hip, and what `measure` does with its records on the host is in measure_report.cpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <string>
#include <vector>

#include "../../include/g1s_diff.h"
#include "curve.h"
#include "fold.h"
#include "host_pool.h"
#include "nlf.h"
#include "record.h"

namespace g1s {

// The cores this process may really use: the hardware threads, cut to the cgroup's CPU quota where there is one (a 1-GPU box
// of the pool this was measured on shows 256 hardware threads and `cpu.max` = 16 cores: 32 pool threads there do 80 k frames/s
// of the per-frame half where 16 do 95 k -- the quota's throttling stops every thread of the group, the launching one included;
// profiles/r04_host_budget_8ranks.txt).
unsigned usable_cpus() {
  unsigned hw = std::thread::hardware_concurrency();
  if (!hw) hw = 1;
  long long quota = -1, period = 100000;
  if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
    char q[32] = {0};
    if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
    fclose(f);
  } else if (FILE *f1 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
    if (fscanf(f1, "%lld", &quota) != 1) quota = -1;
    fclose(f1);
    if (FILE *f2 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (fscanf(f2, "%lld", &period) != 1) period = 100000;
      fclose(f2);
    }
  }
  if (quota > 0 && period > 0) hw = std::min<unsigned>(hw, (unsigned)std::max<long long>(1, (quota + period - 1) / period));
  return hw;
}

// One pool per process (creating 30 threads per generator would dominate short jobs).
Pool *shared_pool() {
  static Pool *p = [] {
    unsigned hw = usable_cpus();
    if (const char *e = getenv("G1S_FOLD_THREADS")) hw = (unsigned)atoi(e);
    if (hw > 32) hw = 32;
    return hw > 1 ? new Pool(hw - 1) : nullptr;  // the calling thread participates
  }();
  return p;
}
// The ordered merge of exchanged latest states (rank 0 of a frame-shard job) has a small pool of its own:
// on that rank the shared pool is busy half of the time with the per-frame half of the rank's own batches,
// and a merge that waits for it falls behind the eight GPUs it serves.
Pool *merge_pool() {
  static Pool *p = [] {
    unsigned hw = usable_cpus();
    if (const char *e = getenv("G1S_FOLD_THREADS")) hw = (unsigned)atoi(e);
    unsigned n = std::min(8u, hw / 2);  // (8: 1.5 - 1.6 us a frame, steady; 16 reaches 1.0 but swings to 2 - 8 on a busy host: profiles/r03_fold_budget.txt)
    if (const char *e = getenv("G1S_MERGE_POOL")) n = (unsigned)atoi(e);  // (measurement: the pool's size itself)
    return n > 1 ? new Pool(n - 1) : nullptr;
  }();
  return p;
}

namespace {
std::mutex g_pool_mutex, g_merge_pool_mutex;  // one job on a pool at a time (host_pool.h)
void on_pool(Pool *p, std::mutex &m, int n, const std::function<void(int)> &fn) {
  if (p && n > 1) {
    std::lock_guard<std::mutex> lk(m);
    p->parallel_for(n, fn);
  } else {
    for (int i = 0; i < n; ++i) fn(i);
  }
}
}  // namespace
void on_shared_pool(int n, const std::function<void(int)> &fn) { on_pool(shared_pool(), g_pool_mutex, n, fn); }
void on_merge_pool(int n, const std::function<void(int)> &fn) { on_pool(merge_pool(), g_merge_pool_mutex, n, fn); }

}  // namespace g1s

using namespace g1s;

namespace {

thread_local std::string g_global_error;

// ---- frame-shard rounds: the exchange protocol (what goes into a round's message, which batch, in which order the root
//      merges) lives here; the transport (RCCL / MPI / torch.distributed gather of fixed-size buffers) stays with the host
constexpr uint32_t kShardMagic = 0x4d315347u;  // "GS1M"
constexpr uint32_t kShardNoIndex = 0xffffffffu;  // a message without a batch index: merged in arrival order
struct ShardHeader {
  uint32_t magic, count, lag, batch_frames;
  // which of the SENDING rank's batches this is (0, 1, ...): global batch = local_batch * world + rank.  The root merges
  // by this index, not by arrival: ranks that have fed different numbers of batches (an idle rank in a short last round)
  // send different local batches in the same round
  uint32_t local_batch, reserved;
};

bool rec_layout(const void *rec, RecHeader &h, RecLayout &L) {
  if (!rec) return false;
  std::memcpy(&h, rec, sizeof(h));
  if (h.magic != kRecMagic) return false;
  L = make_layout(h.width, h.height, h.nplanes, h.lag);
  return L.size == h.size_bytes;
}

}  // namespace

struct g1s_fold {
  NoiseFold fold;
  uint32_t lag;
  std::string err;
  bool finished = false;
  std::vector<g1s_segment_t> final_segs;  // what finish() returned (kept: a too-small buffer can be retried)
  std::vector<FrameLatest> latest;
  std::vector<FrameView> views;  // g1s_fold_push_latest: the blobs of a pass, read in place
  // g1s_shard_merge: indexed batches that arrived ahead of the next one in the global order (global batch -> its states)
  std::map<uint64_t, std::vector<uint8_t>> early;
  uint64_t next_batch = 0;
  g1s_fold(int64_t a, int64_t b, uint32_t lag_) : fold(a, b, lag_), lag(lag_) {}
};

// Runs of latest-state blobs, merged in the order given.  The frames of ALL runs are taken in windows of kChunk frames (the
// solves of a window run on the merge pool, fold.cpp: push_latest_many): a round of a frame-shard job -- eight messages of
// one batch each -- is merged as two windows of 256, not eight of 64 (the pool's hand-over per window is what a small
// window pays: 3.8 -> 5.5 us a frame single-threaded at 64, profiles/r04_host_budget_8ranks.txt).
struct BlobRun {
  const uint8_t *base;
  size_t stride, n;
};
static int fold_push_runs(g1s_fold_t *f, const BlobRun *runs, size_t nruns) {
  if (f->finished) return G1S_ERR_STATE;
  constexpr size_t kChunk = 256;  // frames parsed and merged per pass (bounds the staging memory)
  static struct ParseProfile {  // G1S_FOLD_PROFILE=1: the whole call next to the fold's own stage timers
    bool on = getenv("G1S_FOLD_PROFILE") != nullptr;
    double s = 0, all = 0;
    size_t frames = 0;
    ~ParseProfile() {
      if (on && frames) fprintf(stderr, "ordered merge, us per frame: blob headers %.2f, whole call %.2f (%zu frames)\n", s * 1e6 / frames, all * 1e6 / frames, frames);
    }
  } pp;
  if (f->views.size() < kChunk) f->views.resize(kChunk);
  size_t run = 0, at = 0;  // the next frame to take: frame `at` of run `run`
  for (;;) {
    while (run < nruns && at == runs[run].n) {
      ++run;
      at = 0;
    }
    if (run == nruns) return G1S_OK;
    const auto t_p0 = std::chrono::steady_clock::now();
    size_t good = 0;
    int bad_rc = G1S_OK;
    while (good < kChunk && run < nruns) {
      if (at == runs[run].n) {
        ++run;
        at = 0;
        continue;
      }
      const BlobRun &R = runs[run];
      const uint8_t *b = R.base + at * R.stride;
      // The blobs are read where they lie (fold.h, FrameView); only a caller's unaligned buffer is copied first.
      int rc;
      if (!((reinterpret_cast<uintptr_t>(R.base) | R.stride) & 7)) {
        rc = view_of_blob(b, R.stride, f->lag, f->views[good]);
      } else {
        if (f->latest.size() < kChunk) f->latest.resize(kChunk);
        rc = latest_from_blob(b, R.stride, f->lag, f->latest[good]);
        if (!rc) view_of(f->latest[good], f->views[good]);
      }
      if (rc) {
        bad_rc = rc;
        break;
      }
      ++good;
      ++at;
    }
    const auto t_p1 = std::chrono::steady_clock::now();
    const int rc = f->fold.push_latest_many(f->views.data(), good, on_merge_pool);  // (the frames before a bad blob still count)
    if (pp.on) {
      pp.s += std::chrono::duration<double>(t_p1 - t_p0).count();
      pp.all += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_p0).count();
      pp.frames += good;
    }
    if (rc) {
      f->err = f->fold.error();
      return rc;
    }
    if (bad_rc) {
      f->err = "bad latest blob";
      return bad_rc;
    }
  }
}

extern "C" {

const char *g1s_last_global_error(void) { return g_global_error.c_str(); }
// (frame_op.h) the *_new calls of the generator and the frame operations report through the same thread-local text
void g1s_set_global_error_(const char *text) { g_global_error = text ? text : ""; }

unsigned g1s_usable_cpus(void) { return usable_cpus(); }

size_t g1s_record_size(uint32_t width, uint32_t height, uint32_t xdec, uint32_t ydec, uint32_t nplanes,
                       uint32_t lag) {
  (void)xdec;
  (void)ydec;
  return make_layout(width, height, nplanes, lag).size;
}

int g1s_record_init(void *rec, size_t cap_bytes, uint32_t width, uint32_t height, uint32_t xdec,
                    uint32_t ydec, uint32_t nplanes, uint32_t lag) {
  if (!rec || lag < 1 || lag > 3 || (nplanes != 1 && nplanes != 3)) return G1S_ERR_INVALID;
  const RecLayout L = make_layout(width, height, nplanes, lag);
  if (L.size > cap_bytes) return G1S_ERR_CAPACITY;
  std::memset(rec, 0, L.size);
  const RecHeader h = make_header(L, width, height, xdec, ydec, lag);
  std::memcpy(rec, &h, sizeof(h));
  return G1S_OK;
}

int g1s_record_geometry(const void *rec, uint32_t *nbw, uint32_t *nbh, uint32_t *nplanes, uint32_t *lag) {
  RecHeader h;
  RecLayout L;
  if (!rec_layout(rec, h, L)) return G1S_ERR_INVALID;
  if (nbw) *nbw = h.nbw;
  if (nbh) *nbh = h.nbh;
  if (nplanes) *nplanes = h.nplanes;
  if (lag) *lag = h.lag;
  return G1S_OK;
}
const uint8_t *g1s_record_flat_mask(const void *rec) {
  RecHeader h;
  RecLayout L;
  if (!rec_layout(rec, h, L)) return nullptr;
  return (const uint8_t *)rec + L.off_mask;
}
const float *g1s_record_scores(const void *rec) {
  RecHeader h;
  RecLayout L;
  if (!rec_layout(rec, h, L)) return nullptr;
  return reinterpret_cast<const float *>((const uint8_t *)rec + L.off_scores);
}
int g1s_record_ar_sums(const void *rec, uint32_t c, const int64_t **S, const int64_t **Sb, int64_t *nobs) {
  RecHeader h;
  RecLayout L;
  if (!rec_layout(rec, h, L) || c >= h.nplanes) return G1S_ERR_INVALID;
  const int nc = (int)h.n + (c > 0);
  const int64_t *p = reinterpret_cast<const int64_t *>((const uint8_t *)rec + L.off_ar[c]);
  if (S) *S = p;
  if (Sb) *Sb = p + (size_t)nc * nc;
  if (nobs) *nobs = p[(size_t)nc * nc + nc];
  return nc;
}
int g1s_record_block_stats(const void *rec, uint32_t c, const uint32_t **luma_sum, const int32_t **sum_d,
                           const uint32_t **sum_d2) {
  RecHeader h;
  RecLayout L;
  if (!rec_layout(rec, h, L) || c >= h.nplanes) return G1S_ERR_INVALID;
  const uint8_t *r = (const uint8_t *)rec;
  if (luma_sum) *luma_sum = reinterpret_cast<const uint32_t *>(r + L.off_luma_sum);
  if (sum_d) *sum_d = reinterpret_cast<const int32_t *>(r + L.off_sum_d[c]);
  if (sum_d2) *sum_d2 = reinterpret_cast<const uint32_t *>(r + L.off_sum_d2[c]);
  return (int)L.nblocks;
}

size_t g1s_shard_msg_size(uint32_t ar_coeff_lag, uint32_t batch_frames) {
  return ar_coeff_lag >= 1 && ar_coeff_lag <= 3 ? sizeof(ShardHeader) + (size_t)batch_frames * latest_blob_size(ar_coeff_lag) : 0;
}
int g1s_shard_msg_from_latest_at(const void *blobs, size_t n, uint32_t ar_coeff_lag, uint32_t batch_frames, uint64_t local_batch,
                                 void *msg, size_t cap_bytes) {
  if (!msg || (!blobs && n) || ar_coeff_lag < 1 || ar_coeff_lag > 3 || n > batch_frames) return G1S_ERR_INVALID;
  if (local_batch != G1S_SHARD_NO_INDEX && local_batch >= kShardNoIndex) return G1S_ERR_INVALID;
  const size_t total = g1s_shard_msg_size(ar_coeff_lag, batch_frames), bs = latest_blob_size(ar_coeff_lag);
  if (cap_bytes < total) return G1S_ERR_CAPACITY;
  std::memset(msg, 0, total);
  const ShardHeader h{kShardMagic, (uint32_t)n, ar_coeff_lag, batch_frames,
                      local_batch == G1S_SHARD_NO_INDEX ? kShardNoIndex : (uint32_t)local_batch, 0u};
  std::memcpy(msg, &h, sizeof(h));
  if (n) std::memcpy((uint8_t *)msg + sizeof(h), blobs, n * bs);
  return G1S_OK;
}
int g1s_shard_msg_from_latest(const void *blobs, size_t n, uint32_t ar_coeff_lag, uint32_t batch_frames, void *msg, size_t cap_bytes) {
  return g1s_shard_msg_from_latest_at(blobs, n, ar_coeff_lag, batch_frames, G1S_SHARD_NO_INDEX, msg, cap_bytes);
}

size_t g1s_latest_size(uint32_t ar_coeff_lag) { return ar_coeff_lag >= 1 && ar_coeff_lag <= 3 ? latest_blob_size(ar_coeff_lag) : 0; }

int g1s_latest_from_record(const void *record, size_t size_bytes, uint32_t ar_coeff_lag, void *blob, size_t cap_bytes) {
  if (!record || !blob || ar_coeff_lag < 1 || ar_coeff_lag > 3) return G1S_ERR_INVALID;
  if (cap_bytes < latest_blob_size(ar_coeff_lag)) return G1S_ERR_CAPACITY;
  FrameLatest fl;
  compute_latest((const uint8_t *)record, size_bytes, ar_coeff_lag, fl);  // a failure travels inside the blob
  latest_to_blob(fl, ar_coeff_lag, (uint8_t *)blob);
  return G1S_OK;
}

// The per-frame half of a batch of records on the process' per-frame pool (G1S_FOLD_THREADS; the calling thread takes part):
// what a generator's drainer does with a batch, as a call of its own -- a host that runs the half next to a foreign transport,
// and tools/host_budget_8ranks.py, which replays eight ranks' worth of it.
int g1s_latest_from_records(const void *records, size_t stride_bytes, size_t n, uint32_t ar_coeff_lag, void *blobs, size_t blob_stride_bytes) {
  if ((!records || !blobs) && n) return G1S_ERR_INVALID;
  if (ar_coeff_lag < 1 || ar_coeff_lag > 3) return G1S_ERR_INVALID;
  const size_t bs = latest_blob_size(ar_coeff_lag);
  if (blob_stride_bytes < bs) return G1S_ERR_CAPACITY;
  on_shared_pool((int)n, [&](int i) {
    static thread_local FrameLatest fl;  // (kept per thread: its vectors are sized once, not once a frame)
    compute_latest((const uint8_t *)records + (size_t)i * stride_bytes, stride_bytes, ar_coeff_lag, fl);
    latest_to_blob(fl, ar_coeff_lag, (uint8_t *)blobs + (size_t)i * blob_stride_bytes);
  });
  return G1S_OK;
}

g1s_fold_t *g1s_fold_new(int64_t fps_num, int64_t fps_den, uint32_t lag) {
  if (fps_num <= 0 || fps_den <= 0 || lag < 1 || lag > 3) return nullptr;
  return new g1s_fold(fps_num, fps_den, lag);
}
int g1s_fold_push(g1s_fold_t *f, const void *record, size_t size_bytes) {
  if (!f || !record) return G1S_ERR_INVALID;
  if (f->finished) return G1S_ERR_STATE;
  const int rc = f->fold.push((const uint8_t *)record, size_bytes);
  if (rc) f->err = f->fold.error();
  return rc;
}
int g1s_fold_push_many(g1s_fold_t *f, const void *records, size_t stride_bytes, size_t n) {
  if (!f || (!records && n)) return G1S_ERR_INVALID;
  if (f->finished) return G1S_ERR_STATE;
  const uint8_t *base = (const uint8_t *)records;
  const size_t chunk = 64;
  for (size_t o = 0; o < n; o += chunk) {
    const size_t m = std::min(chunk, n - o);
    if (f->latest.size() < m) f->latest.resize(m);
    on_shared_pool((int)m, [&](int i) { compute_latest(base + (o + i) * stride_bytes, stride_bytes, f->lag, f->latest[i]); });
    for (size_t i = 0; i < m; ++i) {
      const int rc = f->fold.push_latest(f->latest[i]);
      if (rc) {
        f->err = f->fold.error();
        return rc;
      }
    }
  }
  return G1S_OK;
}
int g1s_fold_push_latest(g1s_fold_t *f, const void *blobs, size_t stride_bytes, size_t n) {
  if (!f || (!blobs && n)) return G1S_ERR_INVALID;
  const BlobRun r{(const uint8_t *)blobs, stride_bytes, n};
  return fold_push_runs(f, &r, 1);
}
int g1s_fold_finish(g1s_fold_t *f, g1s_segment_t *out, size_t cap, size_t *n_out) {
  if (!f) return G1S_ERR_INVALID;
  if (!f->early.empty()) {  // (a caller that stopped before the flush rounds, or a rank that skipped a batch)
    f->err = "frame-shard merge: batch " + std::to_string(f->next_batch) + " never arrived (" + std::to_string(f->early.size()) +
             " later batch(es) are waiting for it)";
    return G1S_ERR_STATE;
  }
  if (!f->finished) {
    f->fold.finish(f->final_segs);
    f->finished = true;  // no more records; the segments stay here, so a too-small buffer can be retried
  }
  const int rc = copy_segments(f->final_segs, out, cap, n_out);
  if (rc) f->err = kSegmentsTooSmall;
  return rc;
}
int g1s_shard_merge(g1s_fold_t *f, const void *msgs, size_t stride_bytes, uint32_t world) {
  if (!f || !msgs || !world) return G1S_ERR_INVALID;
  // Global frame order: batch j of the video went to rank j % world, and a message says which of its rank's batches it
  // carries, so global batch = local_batch * world + rank.  Batches are merged strictly in that order; one that arrives
  // before its predecessors (a rank that has fed fewer batches sends an older local batch in the same round) waits here.
  // Messages without an index (g1s_shard_msg_from_latest) are merged as they come: rounds in order, ranks in order.
  for (uint32_t r = 0; r < world; ++r) {  // (validate the whole round before merging any of it)
    const uint8_t *m = (const uint8_t *)msgs + (size_t)r * stride_bytes;
    ShardHeader h;
    std::memcpy(&h, m, sizeof(h));
    if (h.magic != kShardMagic || h.lag != f->lag || h.count > h.batch_frames ||
        stride_bytes < g1s_shard_msg_size(h.lag, h.batch_frames)) {
      f->err = "bad shard message from rank " + std::to_string(r);
      return G1S_ERR_INVALID;
    }
  }
  const size_t bs = latest_blob_size(f->lag);
  // The batches of this round that are next in the global order -- straight from the messages, or from `early` once their
  // predecessors have come -- are collected as runs and merged in one go (fold_push_runs: windows across messages).
  std::vector<BlobRun> runs;
  uint64_t next = f->next_batch;  // the global batch the next run must be
  size_t from_early = 0;          // how many of `early`'s first entries are in `runs`
  auto drain_early = [&] {
    auto it = f->early.begin();
    std::advance(it, from_early);
    while (it != f->early.end() && it->first == next) {
      runs.push_back(BlobRun{it->second.data(), bs, it->second.size() / bs});
      ++it;
      ++from_early;
      ++next;
    }
  };
  auto flush = [&]() -> int {
    const int rc = runs.empty() ? G1S_OK : fold_push_runs(f, runs.data(), runs.size());
    runs.clear();
    f->next_batch = next;
    for (; from_early; --from_early) f->early.erase(f->early.begin());
    return rc;
  };
  for (uint32_t r = 0; r < world; ++r) {
    const uint8_t *m = (const uint8_t *)msgs + (size_t)r * stride_bytes;
    ShardHeader h;
    std::memcpy(&h, m, sizeof(h));
    if (!h.count) continue;
    if (h.local_batch == kShardNoIndex) {
      if (const int rc = flush()) return rc;
      if (!f->early.empty()) {
        f->err = "frame-shard merge: a message without a batch index while indexed batches are waiting";
        return G1S_ERR_STATE;
      }
      const int rc = g1s_fold_push_latest(f, m + sizeof(h), bs, h.count);
      if (rc) return rc;
      continue;
    }
    const uint64_t j = (uint64_t)h.local_batch * world + r;
    if (j < next || f->early.count(j)) {
      flush();
      f->err = "frame-shard merge: batch " + std::to_string(j) + " arrived twice (rank " + std::to_string(r) + ")";
      return G1S_ERR_STATE;
    }
    if (j == next) {
      runs.push_back(BlobRun{m + sizeof(h), bs, h.count});
      ++next;
    } else {
      f->early.emplace(j, std::vector<uint8_t>(m + sizeof(h), m + sizeof(h) + (size_t)h.count * bs));
    }
    drain_early();
  }
  return flush();
}
void g1s_fold_free(g1s_fold_t *f) { delete f; }
const char *g1s_fold_last_error(const g1s_fold_t *f) { return f ? f->err.c_str() : ""; }
uint64_t g1s_fold_frames(const g1s_fold_t *f) { return f ? f->fold.frames() : 0; }

long g1s_format_tbl(const g1s_segment_t *segs, size_t n, char *buf, size_t cap) {
  return format_tbl(segs, n, buf, cap);
}
int g1s_parse_tbl(const char *text, size_t len, g1s_segment_t *out, size_t cap, size_t *n_out, char *err, size_t errcap) {
  if (!text && len) return G1S_ERR_INVALID;
  std::vector<g1s_segment_t> segs;
  std::string msg;
  const int rc = parse_tbl(text, len, segs, msg);
  if (rc) {
    if (err && errcap) snprintf(err, errcap, "%s", msg.c_str());
    return rc;
  }
  if (n_out) *n_out = segs.size();
  if (segs.size() > cap) return G1S_ERR_CAPACITY;
  if (!segs.empty()) std::memcpy(out, segs.data(), sizeof(g1s_segment_t) * segs.size());
  return G1S_OK;
}
long g1s_tbl_segment_for(g1s_segment_t *segs, size_t n, uint64_t packet_ts) {
  if (!segs) return -1;
  for (size_t i = 0; i < n; ++i) {
    if (segs[i].start_time <= packet_ts && packet_ts < segs[i].end_time) {
      segs[i].random_seed = (uint16_t)(segs[i].random_seed + 10956u);  // DEFAULT_GRAIN_SEED, wrapping
      return (long)i;
    }
  }
  return -1;
}
int g1s_write_tbl(const char *path, const g1s_segment_t *segs, size_t n) {
  std::vector<char> buf(1024 + 2048 * n);
  const long k = format_tbl(segs, n, buf.data(), buf.size());
  if (k < 0) return (int)k;
  FILE *f = fopen(path, "wb");
  if (!f) return G1S_ERR_INVALID;
  const size_t w = fwrite(buf.data(), 1, (size_t)k, f);
  const int c = fclose(f);
  return (w == (size_t)k && c == 0) ? G1S_OK : G1S_ERR_INVALID;
}

// rules 12 and 13 of `denoise` (curve.h): needs no device, like the tables of its weights
int g1s_denoise_curve(const g1s_segment_t *segs, size_t n, uint32_t bit_depth, uint32_t range, uint16_t *fwd, uint16_t *inv) {
  const std::string why = !fwd || !inv ? std::string("g1s_denoise_curve needs both output tables") : g1s_cv::build(segs, n, bit_depth, range, fwd, inv);
  if (!why.empty()) {
    g1s_set_global_error_(why.c_str());
    return G1S_ERR_INVALID;
  }
  return G1S_OK;
}

// the same from a scaling function that is given (noise levels, rule N6)
int g1s_denoise_curve_sigma(const uint8_t *s, uint32_t bit_depth, uint32_t range, uint16_t *fwd, uint16_t *inv) {
  const std::string why = !fwd || !inv ? std::string("g1s_denoise_curve_sigma needs both output tables") : g1s_cv::build_sigma(s, bit_depth, range, fwd, inv);
  if (!why.empty()) {
    g1s_set_global_error_(why.c_str());
    return G1S_ERR_INVALID;
  }
  return G1S_OK;
}

// a chroma gain, rules 21 - 23 of `denoise` (curve.h, nlf.h): needs no device either
static int gain_result(const std::string &why) {
  if (why.empty()) return G1S_OK;
  g1s_set_global_error_(why.c_str());
  return G1S_ERR_INVALID;
}

int g1s_denoise_chroma_gain(const g1s_segment_t *segs, size_t n, uint32_t range, uint16_t gain[256]) { return gain_result(g1s_cv::build_gain(segs, n, range, gain)); }

int g1s_nlf_chroma_sigma(const g1s_nlf_record_t *total, uint64_t min_count, uint8_t s[256]) {
  return gain_result(!total || !s ? std::string("g1s_nlf_chroma_sigma needs a record and the output table") : g1s_nl::chroma_sigma(*total, min_count, s));
}

int g1s_denoise_chroma_gain_sigma(const uint8_t s[256], uint32_t range, uint16_t gain[256]) { return gain_result(g1s_cv::gain_from_s(s, range, gain)); }

// noise levels, rules N4 - N8, and temporal noise levels, rules T5 - T8 (nlf.h): what is done with a record of either kind
// needs no device.  A pair of wrappers a rule; the checks of the arguments and the way out are the pair's, `name` its own.
}  // extern "C"

template <class Record>
static int nlf_sum(const Record *recs, size_t n, Record *total) {
  if (!total || (n && !recs)) return G1S_ERR_INVALID;
  return g1s_nl::sum_records(recs, n, total) ? G1S_OK : G1S_ERR_INVALID;
}

template <class Sigma>
static int nlf_sigma(const char *name, bool have, uint32_t bit_depth, Sigma sigma) {
  std::string why = !have ? std::string(name) + " needs a record and the output table" : g1s_cv::check_depth_range(bit_depth, 0);
  if (why.empty()) why = sigma();
  return gain_result(why);
}

template <class Strength>
static int nlf_strength(const char *name, bool have, uint32_t bit_depth, uint32_t plane_class, Strength strength) {
  std::string why;
  if (!have) why = std::string(name) + " needs a record and the output value";
  else if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) why = "noise levels are defined for bit depths 8, 10 and 12";
  else if (plane_class > 1) why = "plane_class is 0 (luma) or 1 (chroma)";
  else why = strength();
  return gain_result(why);
}

template <class Report>
static long nlf_report(bool have, uint32_t bit_depth, uint32_t nplanes, char *buf, size_t cap, Report report) {
  if (!have || (!buf && cap) || (nplanes != 1 && nplanes != 3) || (bit_depth != 8 && bit_depth != 10 && bit_depth != 12)) return G1S_ERR_INVALID;
  const std::string s = report();
  if (s.size() > cap) return G1S_ERR_CAPACITY;
  std::memcpy(buf, s.data(), s.size());
  return (long)s.size();
}

extern "C" {

int g1s_nlf_sum(const g1s_nlf_record_t *recs, size_t n, g1s_nlf_record_t *total) { return nlf_sum(recs, n, total); }
int g1s_nlf_sum_temporal(const g1s_nlf_trecord_t *recs, size_t n, g1s_nlf_trecord_t *total) { return nlf_sum(recs, n, total); }

int g1s_nlf_sigma(const g1s_nlf_record_t *total, uint32_t bit_depth, uint64_t min_count, uint8_t *s) {
  return nlf_sigma("g1s_nlf_sigma", total && s, bit_depth, [&] { return g1s_nl::sigma(*total, bit_depth, min_count, s); });
}
int g1s_nlf_sigma_temporal(const g1s_nlf_trecord_t *total, uint32_t bit_depth, uint64_t min_count, uint8_t *s) {
  return nlf_sigma("g1s_nlf_sigma_temporal", total && s, bit_depth, [&] { return g1s_nl::sigma_t(*total, 0, bit_depth, min_count, s); });
}

int g1s_nlf_chroma_sigma_temporal(const g1s_nlf_trecord_t *total, uint64_t min_count, uint8_t s[256]) {
  return gain_result(!total || !s ? std::string("g1s_nlf_chroma_sigma_temporal needs a record and the output table") : g1s_nl::sigma_t(*total, 1, 8, min_count, s));
}

int g1s_nlf_strength(const g1s_nlf_record_t *total, uint32_t bit_depth, uint64_t min_count, uint32_t plane_class, double *h) {
  return nlf_strength("g1s_nlf_strength", total && h, bit_depth, plane_class, [&] { return g1s_nl::strength(*total, bit_depth, min_count, plane_class, h); });
}
int g1s_nlf_strength_temporal(const g1s_nlf_trecord_t *total, uint32_t bit_depth, uint64_t min_count, uint32_t plane_class, double *h) {
  return nlf_strength("g1s_nlf_strength_temporal", total && h, bit_depth, plane_class,
                      [&] { return g1s_nl::strength_t(*total, bit_depth, min_count, plane_class, h); });
}

long g1s_format_noise_levels(const g1s_nlf_record_t *total, uint64_t frames, uint32_t bit_depth, uint32_t nplanes, uint64_t min_count, char *buf,
                             size_t cap) {
  return nlf_report(total, bit_depth, nplanes, buf, cap, [&] { return g1s_nl::report(*total, frames, bit_depth, nplanes, min_count); });
}
long g1s_format_noise_levels_temporal(const g1s_nlf_trecord_t *total, const g1s_nlf_record_t *ordinary, uint64_t pairs, uint32_t bit_depth,
                                      uint32_t nplanes, uint64_t min_count, char *buf, size_t cap) {
  return nlf_report(total, bit_depth, nplanes, buf, cap, [&] { return g1s_nl::report_t(*total, ordinary, pairs, bit_depth, nplanes, min_count); });
}

}  // extern "C"
