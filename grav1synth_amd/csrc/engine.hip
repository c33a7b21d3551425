// engine.hip -- the generator: host engine + the part of libg1s_diff.so's C ABI (include/g1s_diff.h) that takes a
// g1s_diff_t *.  The ABI that needs no device (records, fold handle, shard messages, .tbl) is host_abi.cpp; the worker
// pools are host_pool.h.
//
// Frames are queued into a slot of `batch_frames` pairs; a full slot is one batch: its schedule is decided once (schedule.h,
// plan_batch), its kernels and the D2H copy of its results follow that plan, the host folds it in frame order (fold.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/g1s_diff.h"
#include "fold.h"
#include "frame_op.h"
#include "host_pool.h"
#include "kernels.hip.h"
#include "k1f.hip.h"
#include "k3m.hip.h"
#include "k3s_params.hip.h"
#include "k3s.hip.h"
#include "k3w.hip.h"
#include "latest_dev.h"
#include "record.h"
#include "schedule.h"

using namespace g1s;
using g1s_op::DevBuf;
using g1s_op::Event;
using g1s_op::PinnedBuf;
using g1s_sched::HostWait;
using g1s_sched::Role;
using g1s_sched::Switches;

namespace {

constexpr uint32_t kDefaultBatch = 32;
constexpr int kK3Chunks = 48;

// The AR accumulation is an exact int8 SYRK on the matrix cores.  G1S_K3 selects the chain:
//   wide (default)    k3w.hip.h: 128-sample units, residuals in 32-bit SWAR, windows as masks on the A operand at multiply time,
//                     entries parked in LDS, ghost units instead of halo loads; the launches scatter the block statistics
//                     themselves, k3w_tail = the partial-system reduction + the exact kernel.  Serves aligned planes of equal depth;
//   stream            k3s.hip.h: round 3's form of the same pass (two-block units, two tile buffers); what `wide` falls back on for
//                     unaligned planes, widths that are not a multiple of 8 samples and mixed depths.
// Both are bit-exact against the oracle; tests/test_gpu_selfcheck.py compares them with each other.  (Rounds 1 and 2's chains --
// the lag-structured v_dot4 kernels behind the pixel pass K0, K0's planes in front of the matrix-core kernel, the 32x32x32 form
// of the fused pass -- were removed in round 4: git history)
//
// The process-wide switches (schedule.h: Switches): read once, when the library first asks for one.
// (Read at every call instead, where they are used: G1S_F_WGS, G1S_W_WGS[_C], G1S_F_REUSE; per generator: G1S_LATEST.)
const Switches &switches() {
  static const Switches s = [] {
    Switches v;
    const char *k3 = getenv("G1S_K3");
    v.wide = !(k3 && std::strcmp(k3, "stream") == 0);
    v.w_off = getenv("G1S_W_OFF") != nullptr;
    v.one_stream = getenv("G1S_ONE_STREAM") != nullptr;
    v.no_defer = getenv("G1S_NO_DEFER") != nullptr;
    v.side2 = getenv("G1S_SIDE2") && atoi(getenv("G1S_SIDE2")) != 0;
    v.w_aside = getenv("G1S_W_ASIDE") != nullptr;
    v.f_serial = getenv("G1S_F_SERIAL") != nullptr;
    v.d2h_sync = getenv("G1S_D2H_SYNC") != nullptr;
    v.w_rev = getenv("G1S_W_REV") ? atoi(getenv("G1S_W_REV")) : 0;
    v.k1_literal = getenv("G1S_K1_LITERAL") ? atoi(getenv("G1S_K1_LITERAL")) : 0;
    return v;
  }();
  return s;
}
constexpr int kMTargetWgs = 1024;  // accumulation workgroups per launch: 4 per CU, one round
// workgroups per frame for a launch of B frames: enough to fill the chip, and few enough units each for int32.
// kind 0: the luma launch, 1: the chroma launch.  The luma launch likes workgroups of ~64 units of the list (4 096 - 6 144
// workgroups for 64 4K frames: 518 / 510 us against 534 at 2 048), the chroma launch 2 048 (372 us against 377 - 383 at 4 096):
// profiles/r03_wgs_sweep.txt.
int m_wgs_per_frame(int nunits, int B, int kind = 1) {
  const int gmin = (nunits + (kMMaxUnits - 16) - 1) / (kMMaxUnits - 16);  // (two lists, each dealt with its own rounding)
  const char *e = getenv("G1S_F_WGS");  // tuning / test aid (read at every call: a test sets it for its own generator)
  // (at least 32 workgroups to a frame: 64-frame launches are two resident rounds)
  int target = std::max(kMTargetWgs, 32 * B);
  if (kind == 0) target = std::max(target, std::min(64 * B, (int)((long long)B * nunits / 64)));
  if (e) target = std::max(8, atoi(e));
  return (std::max(gmin, (target + B - 1) / std::max(B, 1)) + 7) & ~7;  // (a multiple of 8: workgroup b of a frame on XCD b % 8)
}

// the wide chain: workgroups per frame.  A workgroup walks a contiguous slice of the frame's raster-ordered list and forms a
// ghost unit at either end: longer slices, fewer ghosts; at least one resident round (4 to a CU) a launch
int w_wgs_per_frame(int ncell, int B, int kind) {
  const int cap = kind == 1 ? kWMaxUnitsC : kWMaxUnits;
  const int gmin = (ncell + cap - 1) / cap;
  const char *e = getenv(kind ? "G1S_W_WGS_C" : "G1S_W_WGS");  // tuning / test aid
  int target = std::max(kMTargetWgs, (kind ? 16 : 32) * B);
  if (e) {
    // (1 .. 7: that many workgroups a FRAME, as they are: slices of a few units on frames of a handful of units, for the tests of a
    //  slice's ends -- tests/test_gpu_k3w_slices.py; anything else is a launch's workgroups, as it always was)
    const int v = atoi(e);
    if (v >= 1 && v < 8) return std::max(gmin, v);
    target = std::max(8, v);
  }
  int G = (std::max(gmin, (target + B - 1) / std::max(B, 1)) + 7) & ~7;
  // (luma launch of a small frame: slices of at least 64 cells -- a slice pays two ghost units, its entries' parking and a partial
  //  system whatever its length -- as long as a launch still has a workgroup for every slot of the chip.  1080p, 128 frames a
  //  launch: 32 -> 8 workgroups a frame, luma launch 178 -> 168 us, k3w_tail 15 -> 11; 4K (32 a frame) and 8K are where they were.
  //  profiles/r05n_wgs_small_frames.txt)
  if (!e && kind == 0) {
    const int by_cells = ((ncell + 63) / 64 + 7) & ~7, by_slots = ((kMTargetWgs + B - 1) / std::max(B, 1) + 7) & ~7;
    G = std::max(gmin, std::min(G, std::max(by_cells, by_slots)));
    G = (G + 7) & ~7;
  }
  return G;
}

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      char b_[384];                                                                        \
      snprintf(b_, sizeof(b_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return fail_hip(b_);                                                                 \
    }                                                                                      \
  } while (0)

// G1S_LATEST unset: the per-frame half of the fold runs on the device for frames of this many blocks or more.  The device half's solves
// cost the same whatever the frame's size and the host half's cost goes with the blocks: same box, 1080p (2 040 blocks) the host half
// 1.08 - 1.10 x the device half, 4K (8 160 blocks) the device half 1.13 x the host half (profiles/r07_device_latest.txt)
constexpr int kDeviceLatestMinBlocks = 4096;
constexpr int kSlots = 6;  // batches in flight: being filled, finder chain, accumulation, (the per-frame half on the device,) D2H, fold

// A slot's memory: the bytes of every per-slot allocation and, for the buffers that hold several things, where each region
// lies (byte offsets).  set_geometry_alloc works it out once and says there what each region is; whatever
// allocates, zeroes or points a kernel into a slot reads this.
struct SlotLayout {
  size_t planes, records, flags, stage_frame;  // h_planes / d_planes, d_records / h_records, d_flags; d_stage is [batch] x stage_frame
  size_t k1, k1_moments, k1_list, k1_count;
  size_t mu, mu_units, mu_count, mu_any, mu_only, mu_only_bytes, mu_ustats;
  size_t wu, wu_units[2], wu_count, wu_lbad, wu_lbad_bytes;
  size_t mpart, lplane;
  bool operator==(const SlotLayout &o) const { return std::memcmp(this, &o, sizeof(*this)) == 0; }
};
static_assert(std::has_unique_object_representations<SlotLayout>::value, "SlotLayout is compared as bytes: no padding in it");

// A batch's schedule (schedule.h has the table and the decision): filled by plan_batch when the batch is submitted, followed by
// everything that queues work for it.  It lives in the slot: a deferred back half is queued one submit later and follows the
// plan its front half was queued under.
struct BatchPlan {
  Geom g;      // batch_geom
  bool wide;   // the chain: wide_ok(g, batch_far)
  bool timed;  // every kernel of the batch on the main stream, events around them (g1s_diff_set_timing)
  bool chain;  // a timed batch with ONE pair of events, around the batch's whole chain of kernels (g1s_diff_set_timing(g, 2))
  hipStream_t table, finder, accum, rest, latest, d2h;
  bool back_now;
  int after;
  HostWait host_waits;
};

// Per-kernel timing (g1s_diff_set_timing) and the trace (G1S_TRACE): an event in front of each launch on the stream it goes to,
// the name of the kernel it precedes (none: the end of the one before).  A mark that cannot be made is left out.
struct Marks {
  struct Mark { Event ev; std::string name; hipStream_t stream = nullptr; };
  std::vector<Mark> m;
  size_t n = 0;
  // (plan_batch) timed: a timed batch that is not chain-timed -- nothing between two launches of a chain-timed batch;
  // trace: an untimed batch of a generator that writes a trace
  bool timed = false, trace = false;
  void mark(hipStream_t st, const char *name) {
    if (!timed && !trace) return;
    if (n == m.size()) m.emplace_back();
    Mark &k = m[n];
    if ((!k.ev && hipEventCreate(&k.ev.p) != hipSuccess) || hipEventRecord(k.ev, st) != hipSuccess) return;
    k.stream = st, k.name = name ? name : "", ++n;
  }
  // only for the trace: the timed batches' table of kernels stays what it was
  void mark_trace(hipStream_t st, const char *name) { if (trace) mark(st, name); }
};

enum SlotEv { kEvStart, kEvMomStart, kEvMomEnd, kEvFinderEnd, kEvSelectEnd, kEvEnd, kSlotEvs };  // a timed batch's events, as they are recorded

struct Slot {
  PinnedBuf<FramePlanes> h_planes;  // the batch's frame table, as append() fills it
  DevBuf<FramePlanes> d_planes;     // ... uploaded by launch_front
  DevBuf<uint8_t> d_records;        // the batch's records: zeroed, then written by every kernel of the batch
  PinnedBuf<uint8_t> h_records;     // ... on the host (the device half: only the batch's last record)
  DevBuf<uint8_t> d_flags;          // the finder's verdict on each block (k1_certify / the literal kernel -> the select kernel)
  DevBuf<uint8_t> d_k1;             // the finder's moments, literal list and counts (SlotLayout::k1_*)
  DevBuf<uint8_t> d_mu;             // the stream chain's unit lists and statistics, both chains' deferral flags (SlotLayout::mu_*)
  DevBuf<long long> d_mpart;        // partial systems of the accumulation workgroups
  DevBuf<uint8_t> d_wu;             // the wide chain's unit lists, counts and L-outside-int8 flags (SlotLayout::wu_*)
  DevBuf<uint8_t> d_lplane;         // L at chroma resolution, int8 (luma launch -> chroma launch)
  DevBuf<uint8_t> d_stage;          // device copies of host-resident frames (made when the first one comes: append)
  // the per-frame half of the fold on the device (latest.hip): the frames' latest-state blobs and the kernel's scratch
  DevBuf<uint8_t> d_latest, d_lscratch;
  PinnedBuf<uint8_t> h_latest;
  size_t latest_cap = 0, lscratch_cap = 0;
  Event done;            // the batch's results are on the host
  Event ev[kSlotEvs];    // timing: SlotEv
  uint32_t count = 0;
  bool async_in = false;  // the batch holds frames whose H2D copies were queued on the upload stream
  BatchPlan plan{};
  Marks marks;
  // (the device half's buffers: made when a batch first runs that half, made again if one ever asks for more)
  hipError_t ensure_latest(size_t blob_bytes, size_t scratch_bytes) {
    if (latest_cap < blob_bytes) {
      d_latest = {}, h_latest = {}, latest_cap = 0;
      if (hipError_t e = hipMalloc((void **)&d_latest.p, blob_bytes)) return e;
      if (hipError_t e = hipHostMalloc((void **)&h_latest.p, blob_bytes, hipHostMallocDefault)) return e;
      latest_cap = blob_bytes;
    }
    if (lscratch_cap < scratch_bytes) {
      d_lscratch = {}, lscratch_cap = 0;
      if (hipError_t e = hipMalloc((void **)&d_lscratch.p, scratch_bytes)) return e;
      lscratch_cap = scratch_bytes;
    }
    return hipSuccess;
  }
};
static_assert(!std::is_copy_constructible<Slot>::value && std::is_nothrow_move_assignable<Slot>::value,
              "a slot owns what it holds: handed over whole (generator <-> cache), freed by `sl = Slot{}`");

// Process-wide cache of slot buffers: pinned-host and device allocations cost
// hundreds of microseconds each; consecutive generators of the same geometry
// (one per video, or one per bench step) reuse them.
struct CachedSlot {
  int device;
  SlotLayout lay;
  // Not needed for the buffers to fit (the layout says that), and compared all the same: without them slots would move between
  // geometries whose layouts happen to be equal.  What has been examined is reuse at ONE geometry (tests/test_gpu_records.py,
  // every record of every frame against the oracle, both chains): a slot used again inside a generator and a slot handed from a
  // closed generator to the next, going from damaged (deferred blocks, literal lists) and busy content to flat and plane-distinct
  // content and back, full batches followed by short ones.  A slot that moves to ANOTHER geometry of the same layout (the L
  // plane's slack row, the parked entries around a d_wu slice would then hold that geometry's bytes) has not been examined.
  int W, H, xdec, ydec, nplanes;
  Slot slot;
};
std::mutex g_cache_mutex;
// (never destroyed: a parked slot is not freed at exit, when the runtime it would call may be gone already)
std::vector<CachedSlot> &g_slot_cache = *new std::vector<CachedSlot>;

// Streams and their events are process-wide too (0.1-0.2 ms to create each); a generator borrows a set and hands it back
// when it is freed.  What runs on which: schedule.h.  compute is the main stream (the accumulation of one batch after the
// other, back to back), flat the side stream (high priority: the finder chains, next to the accumulation of the batch before),
// copy carries the results' D2H, upload the frame table, k_zero and the queued copies of pinned host frames, ahead of everything.
struct StreamSet {
  int device = -1;
  hipStream_t compute = nullptr, copy = nullptr, flat = nullptr, flat2 = nullptr, upload = nullptr;
  // k4_latest of the even / odd slots where it does NOT run on the main stream (launches of fewer than kLatestWindowMinBatch
  // frames; made when a generator first needs them).  On a stream of its own the kernel's workgroups are not dispatched while
  // another queue's launch still has workgroups to place: 615 us a 64-frame 4K launch in the job whatever the kernel takes
  // alone (343 or 278), 520 us next to k1_moments alone (profiles/r09_latest_window.txt) -- on ONE stream, with the blobs' copy
  // behind it, a batch's half would only start when the half of the batch before had been copied out
  hipStream_t latest = nullptr, latest2 = nullptr;
  hipEvent_t latest_done[kSlots] = {};  // a batch's k4_latest has ended: the blobs' copy waits for it
  int prio_side = 0;
  hipEvent_t kernels_done[kSlots] = {};
  hipEvent_t mask_done[kSlots] = {};
  hipEvent_t table_done[kSlots] = {};
};
std::vector<StreamSet> g_stream_cache;
bool acquire_streams(int device, StreamSet &out) {
  {
    std::lock_guard<std::mutex> lk(g_cache_mutex);
    for (size_t i = 0; i < g_stream_cache.size(); ++i) {
      if (g_stream_cache[i].device == device) {
        out = g_stream_cache[i];
        g_stream_cache.erase(g_stream_cache.begin() + i);
        return true;
      }
    }
  }
  out = StreamSet{};
  out.device = device;
  // the side stream (the finder chain: small latency-bound kernels) outranks the main stream's big kernels, next to which it
  // runs.  The 4 - 6 streams here and the host application's own share the hardware queues the runtime gives the process, by
  // creation order, and kernels of streams on one queue wait for each other (slower, not wrong: 393 - 406 k Mpx/s with every
  // stream in one priority class on 4 queues against 544 - 593 k with the priorities, profiles/r04_streams.txt).  How many
  // queues a process gets is the host's setting and is left alone; the streams only some jobs use (the second side stream,
  // the device half's) are made when they are first needed.
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);  // numerically lower = more urgent
  out.prio_side = prio_hi;
  bool ok = hipStreamCreateWithPriority(&out.compute, hipStreamNonBlocking, prio_lo) == hipSuccess &&
            hipStreamCreateWithFlags(&out.copy, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithPriority(&out.flat, hipStreamNonBlocking, prio_hi) == hipSuccess &&
            (!switches().side2 || hipStreamCreateWithPriority(&out.flat2, hipStreamNonBlocking, prio_hi) == hipSuccess) &&
            hipStreamCreateWithFlags(&out.upload, hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; i < kSlots && ok; ++i)
    ok = hipEventCreateWithFlags(&out.kernels_done[i], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&out.mask_done[i], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&out.table_done[i], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&out.latest_done[i], hipEventDisableTiming) == hipSuccess;
  return ok;
}
// The device half's two streams, when a generator first runs that half outside the window.  Both or none.  In the main stream's
// priority class (the least urgent: the kernel fills in; 4 % better than the runtime's default class and the side stream's,
// profiles/r05_device_latest.txt)
bool ensure_latest_streams(StreamSet &ss) {
  if (ss.latest) return true;
  int plo = 0, phi = 0;
  (void)hipDeviceGetStreamPriorityRange(&plo, &phi);
  hipStream_t made[2] = {nullptr, nullptr};
  bool ok = true;
  for (hipStream_t &st : made) ok = ok && hipStreamCreateWithPriority(&st, hipStreamNonBlocking, plo) == hipSuccess;
  if (!ok) {
    for (hipStream_t st : made)
      if (st) (void)hipStreamDestroy(st);
    return false;
  }
  ss.latest = made[0], ss.latest2 = made[1];
  return true;
}
void release_streams(StreamSet &ss) {
  if (!ss.compute) return;
  std::lock_guard<std::mutex> lk(g_cache_mutex);
  g_stream_cache.push_back(ss);
  ss = StreamSet{};
}

}  // namespace

struct g1s_diff {
  int64_t fps_num, fps_den;
  uint32_t src_bd, den_bd;
  uint32_t lag, n;
  bool luma_only, records_only;
  bool latest_only = false;  // keep the per-frame latest states (blobs) instead of folding them here
  bool device_latest = false;  // the per-frame half of the fold runs on the device (k4_latest): blobs come back, not records
  bool latest_by_size = false;  // G1S_LATEST is unset: set_geometry chooses (kDeviceLatestMinBlocks)
  uint32_t batch;
  bool batch_auto = false;  // no batch size asked for: sized to the frames at the first frame pair
  int device = 0;
  StreamSet ss;                       // borrowed from the process-wide cache
  bool geometry_set = false;
  g1s_frame_t shape{};  // geometry of the first frame
  Geom geom{};
  RecLayout L{};
  FlatConsts fc{};
  double *d_lut = nullptr;
  uint32_t m_lpitch = 0, m_lframe = 0;  // MFMA path: L plane geometry
  int m_nunits = 0;          // MFMA path: chunks per frame
  size_t m_wg_cap = 0;       // ... workgroups (partial systems) the slots hold
  // the wide chain (k3w.hip.h): blocks a chroma unit, cells a block row / a frame per kind, L geometry
  int w_ub_c = 4, w_gx[2] = {0, 0}, w_ncell[2] = {0, 0};
  uint32_t w_lpitch = 0, w_lframe = 0;
  bool wide_ok(const Geom &g, bool far) const;
  bool batch_far(const Slot &sl) const;
  MParams make_mparams(const Slot &sl) const;
  SlotLayout lay{};  // the slots' memory (set_geometry)
  Slot slots[kSlots];
  int cur = 0;
  int pending = -1;  // slot whose front half is queued and whose back half is not (not in the window: submit)
  int last_back = -1;  // slot of the batch whose back half was queued last; -1: none since everything queued was drained
  // The API thread queues frames and launches batches; the drainer thread waits for a batch's records,
  // runs the fold on them and frees the slot.  Everything below dm is shared between the two.
  std::thread drainer;  // waits for a batch's records, runs the per-frame half of the fold on the pool
  std::thread folder;   // the ordered half (merge in frame order), then frees the slot
  std::deque<int> fold_q;  // batches whose per-frame half is done
  std::condition_variable cv_fold;
  bool folder_stop = false;
  std::vector<FrameLatest> latest_s[kSlots];  // per slot: two batches are in the fold at a time
  std::vector<FrameView> views_s[kSlots];     // device_latest: the slot's blobs, read where the copy put them
  std::vector<uint32_t> nflat_s[kSlots];
  std::vector<uint8_t> stage_s[kSlots];
  double ms_fold_front = 0, ms_fold_back = 0;  // (one writer each)
  bool front_failed[kSlots] = {};               // a HIP error in the front stage: the batch is not folded
  std::mutex dm;
  std::condition_variable cv_work, cv_free;
  std::deque<int> in_flight;       // submitted, not yet picked up by the drainer
  bool slot_busy[kSlots] = {};     // submitted and not yet drained
  uint64_t submitted = 0, drained = 0;  // batches
  uint64_t frames_released = 0;         // frame pairs of the drained batches (their inputs are no longer read)
  // asynchronous host -> device copies of pinned frames (on_device == 2): one event per frame pair, in order
  std::mutex h2d_mutex;
  std::deque<std::pair<uint64_t, Event>> h2d_pending;  // (frame pairs handed over up to and including this one, copies done)
  std::vector<Event> h2d_free;
  uint64_t frames_appended = 0;
  Event h2d_order;  // copies -> table upload when the two run on different streams
  bool drainer_stop = false;
  NoiseFold *fold = nullptr;
  std::vector<uint8_t> records_out;
  size_t records_out_frames = 0;
  std::vector<uint8_t> latest_out;  // latest_only: blobs of the drained frames, in frame order
  size_t latest_out_frames = 0;
  std::deque<uint32_t> latest_batches;  // frames per drained, not yet delivered batch
  uint64_t delivered = 0;               // batches handed out by g1s_diff_take_latest
  std::vector<uint8_t> last_record;
  std::string err;
  int deferred = G1S_OK;
  // a fold error, a HIP error or a batch that failed to launch or drain kills the generator: every later call, finish
  // included, returns it (the reference `?`-propagates out of main; a table with frames silently missing is worse)
  std::atomic<int> sticky{G1S_OK};
  bool finished = false;
  std::vector<g1s_segment_t> final_segs;  // what finish() returned (kept: a too-small buffer can be retried)
  bool timing = false;
  bool timing_chain = false;  // timed batches carry one pair of events (first kernel's start, last kernel's end) instead of one a kernel
  int flat_literal = 0;  // flat-block finder: literal f64 evaluation of every block (1: lane per block, 2: wave per block)
  g1s_stats_t stats{};
  std::map<std::string, std::pair<double, uint64_t>> ktimes;  // timed batches: kernel name -> (ms, launches)
  std::mutex ktimes_mutex;
  // G1S_TRACE=file (a measurement aid): the PIPELINED job's own timeline -- an event in front of every launch on the stream it
  // is launched on (its end = the next event of that stream), the host's time at every submit; written at finish
  bool trace = false;
  Event trace_base;
  std::chrono::steady_clock::time_point trace_host0;
  std::vector<std::string> trace_lines;
  std::mutex trace_mutex;
  double trace_now() const { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - trace_host0).count(); }
  void trace_host(const char *what, int si) {
    if (!trace) return;
    char b[96];
    snprintf(b, sizeof(b), "H %12.1f %s slot %d", trace_now(), what, si);
    std::lock_guard<std::mutex> lk(trace_mutex);
    trace_lines.emplace_back(b);
  }

  int fail(int code, const std::string &msg) {
    err = msg;
    return code;
  }
  int fail_hip(const char *msg) {
    err = msg;
    int ok = G1S_OK;
    sticky.compare_exchange_strong(ok, G1S_ERR_HIP);
    return G1S_ERR_HIP;
  }

  int set_geometry(const g1s_frame_t *s, const g1s_frame_t *d);
  int set_geometry_alloc(const g1s_frame_t *s, const g1s_frame_t *d);
  int append(const g1s_frame_t *s, const g1s_frame_t *d);
  uint64_t frames_copied(uint64_t wait_for);
  int submit(int si);        // plan, front half now; back half now or with the next batch's front half
  int plan_batch(int si);    // the batch's schedule: slots[si].plan
  int launch_front(int si);  // frame table, zero fills, flat-block finder, select kernel, unit lists
  int launch_back(int si);   // accumulation kernels, records D2H, hand-over to the drainer; its parts, in order:
  int accumulate_wide(Slot &sl, int si);
  int accumulate_stream(Slot &sl, int si);
  int to_rest(const BatchPlan &p, int si);  // (between a chain's luma and chroma launch)
  int copy_out(Slot &sl, int si);
  static bool wide_gen(const Geom &g);  // the wide chain's general residual form (mixed sample sizes / shifts)
  int flush_pending();
  Geom batch_geom(const Slot &sl) const;
  int drain_front(int si);  // drainer thread
  int drain_back(int si);   // folder thread
  void drainer_main();
  void folder_main();
  int drain_all();          // API thread: wait until everything submitted is drained
  void wait_drained(uint64_t upto);
  void release();
};

// The 3x3 inverse of A^T A for the plane fit, built the way
// FlatBlockFinder::new does (three solves of the normal equations).
static void make_flat_consts(FlatConsts &fc) {
  double AtA[9] = {0};
  for (int y = 0; y < kBlock; ++y) {
    const double yd = ((double)y - kBlock / 2.) / (kBlock / 2.);
    for (int x = 0; x < kBlock; ++x) {
      const double xd = ((double)x - kBlock / 2.) / (kBlock / 2.);
      const double co[3] = {yd, xd, 1};
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) AtA[3 * i + j] += co[i] * co[j];
    }
  }
  for (int i = 0; i < 3; ++i) {
    double A[9], b[3] = {0, 0, 0}, x[3] = {0, 0, 0};
    std::memcpy(A, AtA, sizeof(A));
    b[i] = 1;
    gauss_solve(3, A, b, x);
    for (int j = 0; j < 3; ++j) fc.ata_inv[j * 3 + i] = x[j];
  }
}

// (an allocation that fails half way leaves no half-built slot behind: a retry starts from nothing)
int g1s_diff::set_geometry(const g1s_frame_t *s, const g1s_frame_t *d) {
  const int rc = set_geometry_alloc(s, d);
  if (rc)
    for (Slot &sl : slots) sl = Slot{};
  return rc;
}
int g1s_diff::set_geometry_alloc(const g1s_frame_t *s, const g1s_frame_t *d) {
  shape = *s;
  if (batch_auto) {
    // about 530 Mpixels a launch group (64 4K frames; measured: 32 -> 64 frames a launch +12 % on the 4K job, no gain
    // beyond): the per-launch costs of the small kernels are the same for small frames, so they get more frames per
    // launch (1080p: 128, +6 % over 64 and +13 % over 256; 8K: 32 -- 16 is 5 % slower, 64 the same; 4K: 64 -- 96 and 128 are
    // 5 - 7 % slower: profiles/r04_other_workloads.txt, tools/r4_batch.sh)
    const uint64_t px = (uint64_t)s->width * s->height;
    batch = (uint32_t)std::min<uint64_t>(128, std::max<uint64_t>(32, (530000000ull + px / 2) / std::max<uint64_t>(px, 1)));
  }
  const uint32_t np = luma_only ? 1u : (uint32_t)s->nplanes;
  L = make_layout(s->width, s->height, np, lag);
  Geom &g = geom;
  g.W = (int)s->width;
  g.H = (int)s->height;
  g.xdec = s->xdec;
  g.ydec = s->ydec;
  g.nplanes = (int)np;
  g.nbw = (g.W + kBlock - 1) / kBlock;
  g.nbh = (g.H + kBlock - 1) / kBlock;
  g.nblocks = g.nbw * g.nbh;
  if (latest_by_size) device_latest = !records_only && g.nblocks >= kDeviceLatestMinBlocks;
  g.src_bps = s->bytes_per_sample;
  g.den_bps = d->bytes_per_sample;
  g.src_shift = s->bytes_per_sample == 2 ? (int)src_bd - 8 : 0;
  g.den_shift = d->bytes_per_sample == 2 ? (int)den_bd - 8 : 0;
  g.lag = (int)lag;
  g.n = (int)n;
  g.rec_size = (uint32_t)L.size;
  for (int c = 0; c < 3; ++c) {
    g.off_ar[c] = (uint32_t)L.off_ar[c];
    g.off_sum_d[c] = (uint32_t)L.off_sum_d[c];
    g.off_sum_d2[c] = (uint32_t)L.off_sum_d2[c];
  }
  g.off_luma_sum = (uint32_t)L.off_luma_sum;
  g.off_scores = (uint32_t)L.off_scores;
  g.off_mask = (uint32_t)L.off_mask;

  m_nunits = ((g.nbw + kMUnitBlocks - 1) / kMUnitBlocks) * g.nbh;
  // one partial system per accumulation workgroup and plane: the most workgroups a launch of 1 .. batch frames asks for
  m_wg_cap = 0;
  for (uint32_t b = 1; b <= batch; ++b)
    m_wg_cap = std::max(m_wg_cap, (size_t)b * std::max(m_wgs_per_frame(m_nunits, (int)b, 0), m_wgs_per_frame(m_nunits, (int)b, 1)));
  // L plane of a frame: block rows x chunk columns at chroma resolution (+ a slack row)
  m_lpitch = g.nplanes == 3 ? (uint32_t)((((g.nbw + kMUnitBlocks - 1) / kMUnitBlocks) * kMUnitBlocks * (kBlock >> g.xdec) + 15) & ~15) : 0u;
  m_lframe = m_lpitch * (uint32_t)(g.nbh * (kBlock >> g.ydec) + 1);
  // the wide chain (k3w.hip.h): its own lists and L geometry
  w_ub_c = g.nplanes == 3 ? (kWUnitW / (kBlock >> g.xdec)) : 4;
  w_gx[0] = (g.nbw + 3) / 4;
  w_gx[1] = (g.nbw + w_ub_c - 1) / w_ub_c;
  w_ncell[0] = w_gx[0] * g.nbh;
  w_ncell[1] = g.nplanes == 3 ? w_gx[1] * g.nbh : 0;
  w_lpitch = g.nplanes == 3 ? (uint32_t)((std::max(w_gx[0] * 4 * (kBlock >> g.xdec), w_gx[1] * kWUnitW) + 15) & ~15) : 0u;
  w_lframe = w_lpitch * (uint32_t)(g.nbh * (kBlock >> g.ydec) + 1);
  if (switches().wide)
    for (uint32_t b = 1; b <= batch; ++b)
      m_wg_cap = std::max(m_wg_cap, (size_t)b * std::max(w_wgs_per_frame(w_ncell[0], (int)b, 0), w_wgs_per_frame(std::max(w_ncell[1], 1), (int)b, 1)));
  // Where things lie in a slot: the one place that says so.  Regions of a buffer in the order they are laid down, none re-aligned.
  const size_t B = batch, nblocks = (size_t)g.nblocks;
  lay = SlotLayout{};
  SlotLayout &l = lay;
  l.planes = sizeof(FramePlanes) * B;  // the frame table
  l.records = L.size * B;              // record.h
  l.flags = nblocks * B;               // flat or not, a byte a block
  for (uint32_t c = 0; c < np; ++c) {  // the tight device copy of one host-resident frame pair
    const size_t pw = c ? (s->width >> s->xdec) : s->width, ph = c ? (s->height >> s->ydec) : s->height;
    l.stage_frame += ((pw * s->bytes_per_sample + 15) & ~size_t(15)) * ph;
    l.stage_frame += ((pw * d->bytes_per_sample + 15) & ~size_t(15)) * ph;
  }
  // d_k1, the flat-block finder
  size_t o = 0;
  l.k1_moments = o, o += sizeof(int32_t) * B * nblocks * kMomInts;  // [batch][nblocks][kMomInts], k1_moments -> k1_certify
  l.k1_list = o, o += sizeof(uint32_t) * B * nblocks;               // [batch][nblocks]: the blocks left to the literal kernel
  l.k1_count = o, o += sizeof(uint32_t) * B;                        // [batch]: how many; zeroed per batch
  l.k1 = o;
  // d_mu: the stream chain's unit lists and statistics, around the deferral flags of both chains
  o = 0;
  l.mu_units = o, o += sizeof(uint32_t) * B * m_nunits * kMUnitDwords;  // [batch][nunits][kMUnitDwords], k3m_units -> k3s_fused
  l.mu_count = o, o += sizeof(uint32_t) * 2 * B;                        // [batch][2]: general, plain units; zeroed per batch in one fill with
  l.mu_any = o, o += sizeof(uint32_t) * B;                              // [batch]: the frame has a deferred block
  l.mu_only = o, l.mu_only_bytes = (nblocks * 3 * B + 15) & ~size_t(15), o += l.mu_only_bytes;  // [batch][3][nblocks] bytes: blocks left to the exact kernel; zeroed per batch
  l.mu_ustats = o, o += sizeof(int32_t) * B * m_nunits * kMStatInts;    // [batch][nunits][kMStatInts], k3s_fused -> k3m_finish
  l.mu = o;
  l.mpart = sizeof(long long) * 3 * kMRec * m_wg_cap;  // a partial system per accumulation workgroup and plane
  // d_wu, the wide chain (k3w.hip.h); not allocated under G1S_K3=stream
  o = 64;  // (a workgroup parks the entry in front of its slice too)
  l.wu_units[0] = o, o += sizeof(uint32_t) * B * w_ncell[0] * kWEntry;  // [batch][cells][kWEntry] luma, then chroma: k2w_select_units -> k3w_pass
  l.wu_units[1] = o, o += sizeof(uint32_t) * B * w_ncell[1] * kWEntry;
  l.wu_count = o, o += sizeof(uint32_t) * 2 * B;                        // [batch][2]
  o = ((o + 15) & ~size_t(15)) + 256;  // (a workgroup parks three entries past its slice)
  l.wu_lbad = o, l.wu_lbad_bytes = (B * w_ncell[0] + 15) & ~size_t(15), o += l.wu_lbad_bytes;  // a byte a luma unit: its L left int8; zeroed per batch
  l.wu = switches().wide ? o : 0;
  l.lplane = (size_t)std::max(m_lframe, switches().wide ? w_lframe : 0u) * B;  // L at chroma resolution, int8 (luma launch -> chroma launch)
  for (Slot &sl : slots) {
    {
      std::lock_guard<std::mutex> lk(g_cache_mutex);
      for (size_t i = 0; i < g_slot_cache.size(); ++i) {
        CachedSlot &c = g_slot_cache[i];
        if (c.device == device && c.lay == lay && c.W == g.W && c.H == g.H && c.xdec == g.xdec && c.ydec == g.ydec && c.nplanes == g.nplanes) {
          sl = std::move(c.slot);
          g_slot_cache.erase(g_slot_cache.begin() + i);
          break;
        }
      }
    }
    sl.count = 0;
    if (sl.h_planes) continue;  // reused
    HIP_TRY(hipHostMalloc((void **)&sl.h_planes.p, lay.planes, hipHostMallocDefault));
    HIP_TRY(hipMalloc((void **)&sl.d_planes.p, lay.planes));
    HIP_TRY(hipMalloc((void **)&sl.d_records.p, lay.records));
    HIP_TRY(hipHostMalloc((void **)&sl.h_records.p, lay.records, hipHostMallocDefault));
    HIP_TRY(hipMalloc((void **)&sl.d_flags.p, lay.flags));
    HIP_TRY(hipMalloc((void **)&sl.d_k1.p, lay.k1));
    if (lay.mu) HIP_TRY(hipMalloc((void **)&sl.d_mu.p, lay.mu));
    if (lay.mpart) HIP_TRY(hipMalloc((void **)&sl.d_mpart.p, lay.mpart));
    if (lay.wu) HIP_TRY(hipMalloc((void **)&sl.d_wu.p, lay.wu));
    if (lay.lplane) HIP_TRY(hipMalloc((void **)&sl.d_lplane.p, lay.lplane));
    // (blocking: the drainer SLEEPS until a batch's records have landed instead of spinning on the event -- a core a rank, which an
    //  8-rank node inside a 16-core quota does not have; five more batches are in flight, the wake-up costs the job nothing)
    HIP_TRY(hipEventCreateWithFlags(&sl.done.p, hipEventDisableTiming | hipEventBlockingSync));
    for (Event &e : sl.ev) HIP_TRY(hipEventCreate(&e.p));
  }
  geometry_set = true;
  return G1S_OK;
}

static bool same_shape(const g1s_frame_t &a, const g1s_frame_t &b) {
  return a.width == b.width && a.height == b.height && a.xdec == b.xdec && a.ydec == b.ydec &&
         a.nplanes == b.nplanes;
}

int g1s_diff::append(const g1s_frame_t *s, const g1s_frame_t *d) {
  if (!s || !d) return fail(G1S_ERR_INVALID, "null frame");
  if (!same_shape(*s, *d))
    return fail(G1S_ERR_DIM_MISMATCH, "Source and denoised frame dimensions do not match");
  if ((s->bytes_per_sample != 1 && s->bytes_per_sample != 2) ||
      (d->bytes_per_sample != 1 && d->bytes_per_sample != 2) || (s->nplanes != 1 && s->nplanes != 3) ||
      s->width < 1 || s->height < 1 || s->xdec > 1 || s->ydec > 1)
    return fail(G1S_ERR_INVALID, "unsupported frame format");
  // what the kernels cannot address is refused like a bad plane, and as early (frame_op.h: diff_size_ok, diff_reach)
  auto lost = [&](const std::string &m) {
    int ok = G1S_OK;
    sticky.compare_exchange_strong(ok, G1S_ERR_INVALID);
    return fail(G1S_ERR_INVALID, m);
  };
  if (!g1s_op::diff_size_ok(s->width, s->height))
    return lost("frame of " + std::to_string(s->width) + " x " + std::to_string(s->height) + " samples: diff takes at most 131072 x 131072");
  if ((s->bytes_per_sample == 1) != (src_bd == 8) || (d->bytes_per_sample == 1) != (den_bd == 8))
    return fail(G1S_ERR_INVALID, "bytes_per_sample does not match the bit depth given to g1s_diff_new");
  // what g1s_grain_frame and g1s_denoise_frame refuse for a plane, before anything is allocated, copied or queued: the kernels
  // take the pointer as it is and the stride as a uint32_t.  Sticky: the job has lost a frame, no table from here on.
  for (int side = 0; side < 2; ++side) {
    const g1s_frame_t *f = side ? d : s;
    for (uint32_t c = 0; c < (luma_only ? 1u : (uint32_t)s->nplanes); ++c) {  // (the planes that are read)
      const size_t rowb = (c ? (size_t)(f->width >> f->xdec) : (size_t)f->width) * f->bytes_per_sample;
      const std::string which = std::string(side ? "denoised" : "source") + " frame, plane " + std::to_string(c);
      if (!f->data[c] || f->stride_bytes[c] < rowb || f->stride_bytes[c] > 0xffffffffu || (f->bytes_per_sample == 2 && (f->stride_bytes[c] & 1)))
        return lost(which + ": bad plane pointer or row stride");
      const g1s_op::DiffReach reach = g1s_op::diff_plane_reach(*f, (int)c);
      if (g1s_op::diff_refused(reach)) return lost(which + ": " + g1s_op::diff_refusal_text(reach));
    }
  }
  if (!geometry_set) {
    const int rc = set_geometry(s, d);
    if (rc) return rc;
  } else if (!same_shape(shape, *s) || shape.bytes_per_sample != s->bytes_per_sample) {
    return fail(G1S_ERR_DIM_MISMATCH, "frame geometry changed mid-stream");
  }
  Slot &sl = slots[cur];
  if (sl.count >= batch) return fail(G1S_ERR_STATE, "the previous batch failed to launch");
  FramePlanes &fp = sl.h_planes[sl.count];
  std::memset(&fp, 0, sizeof(fp));
  const uint32_t np = (uint32_t)geom.nplanes;
  const bool any_host = s->on_device != 1 || d->on_device != 1;
  bool any_async = false;
  if (any_host && !sl.d_stage)
    HIP_TRY(hipMalloc((void **)&sl.d_stage.p, lay.stage_frame * batch));
  uint8_t *stage = any_host ? sl.d_stage + lay.stage_frame * sl.count : nullptr;
  for (int side = 0; side < 2; ++side) {
    const g1s_frame_t *f = side ? d : s;
    for (uint32_t c = 0; c < np; ++c) {
      const size_t pw = c ? (f->width >> f->xdec) : f->width, ph = c ? (f->height >> f->ydec) : f->height;
      const uint8_t *ptr;
      uint32_t stride;
      if (f->on_device == 1) {
        ptr = (const uint8_t *)f->data[c];
        stride = (uint32_t)f->stride_bytes[c];
      } else {
        const size_t row = (pw * f->bytes_per_sample + 15) & ~size_t(15);
        if (f->on_device == 2) {
          // pinned host memory the caller keeps valid until g1s_diff_frames_copied() covers this frame: queued on the
          // upload stream (the table upload of the batch follows on that stream, the kernels wait for that), the call
          // returns at once -- file reads, copies and the kernels of earlier batches overlap
          if (f->stride_bytes[c] == row && pw * f->bytes_per_sample == row)
            HIP_TRY(hipMemcpyAsync(stage, f->data[c], row * ph, hipMemcpyHostToDevice, ss.upload));
          else
            HIP_TRY(hipMemcpy2DAsync(stage, row, f->data[c], f->stride_bytes[c], pw * f->bytes_per_sample, ph, hipMemcpyHostToDevice, ss.upload));
          any_async = true;
        } else {
          // the `&Frame` borrow ends when this call returns: copy now
          HIP_TRY(hipMemcpy2D(stage, row, f->data[c], f->stride_bytes[c], pw * f->bytes_per_sample, ph,
                              hipMemcpyHostToDevice));
        }
        ptr = stage;
        stride = (uint32_t)row;
        stage += row * ph;
      }
      if (side) {
        fp.den[c] = ptr;
        fp.den_stride[c] = stride;
      } else {
        fp.src[c] = ptr;
        fp.src_stride[c] = stride;
      }
    }
  }
  {
    std::lock_guard<std::mutex> lk(h2d_mutex);
    ++frames_appended;
    if (any_async) {
      Event e;
      if (!h2d_free.empty()) {
        e = std::move(h2d_free.back());
        h2d_free.pop_back();
      } else {
        HIP_TRY(hipEventCreateWithFlags(&e.p, hipEventDisableTiming));
      }
      HIP_TRY(hipEventRecord(e, ss.upload));
      h2d_pending.emplace_back(frames_appended, std::move(e));
      sl.async_in = true;
    }
  }
  sl.count++;
  if (sl.count == batch) return submit(cur);
  return G1S_OK;
}

// how many frame pairs' host planes are no longer needed (every on_device == 0 frame at once; on_device == 2 frames when
// their queued copies have run); wait_for > 0: block until that many are
uint64_t g1s_diff::frames_copied(uint64_t wait_for) {
  std::lock_guard<std::mutex> lk(h2d_mutex);
  wait_for = std::min(wait_for, frames_appended);
  while (!h2d_pending.empty()) {
    auto &front = h2d_pending.front();
    if (front.first <= wait_for) (void)hipEventSynchronize(front.second);
    else if (hipEventQuery(front.second) != hipSuccess) break;
    h2d_free.push_back(std::move(front.second));
    h2d_pending.pop_front();
  }
  return h2d_pending.empty() ? frames_appended : h2d_pending.front().first - 1;
}

Geom g1s_diff::batch_geom(const Slot &sl) const {
  const uint32_t B = sl.count;
  Geom g = geom;
  int fast = 1;
  for (uint32_t i = 0; i < B; ++i) {
    if (((uintptr_t)sl.h_planes[i].src[0] & 15) || (sl.h_planes[i].src_stride[0] & 15)) fast = 0;
  }
  g.fast_rows = fast;
  int vec_mask = 0x3f;
  for (uint32_t i = 0; i < B; ++i) {
    for (int c = 0; c < g.nplanes; ++c) {
      if (((uintptr_t)sl.h_planes[i].src[c] & 15) || (sl.h_planes[i].src_stride[c] & 15)) vec_mask &= ~(1 << c);
      if (((uintptr_t)sl.h_planes[i].den[c] & 15) || (sl.h_planes[i].den_stride[c] & 15)) vec_mask &= ~(8 << c);
    }
  }
  g.vec_mask = vec_mask;
  return g;
}

// a device plane of the batch reaches past what the wide chain's buffer descriptor covers (frame_op.h: diff_plane_reach; append
// has refused what no chain reaches; staged host frames are tight copies and never do): the batch is the stream chain's
bool g1s_diff::batch_far(const Slot &sl) const {
  const Geom &g = geom;
  for (uint32_t i = 0; i < sl.count; ++i)
    for (int c = 0; c < g.nplanes; ++c) {
      const uint64_t pw = c ? g.W >> g.xdec : g.W, ph = c ? g.H >> g.ydec : g.H;
      if (g1s_op::diff_plane_reach(sl.h_planes[i].src_stride[c], ph, pw * g.src_bps) != g1s_op::DiffReach::kAnyChain ||
          g1s_op::diff_plane_reach(sl.h_planes[i].den_stride[c], ph, pw * g.den_bps) != g1s_op::DiffReach::kAnyChain)
        return true;
    }
  return false;
}

// A batch runs in two halves, each where its plan says (schedule.h has the table; here is why it reads as it does).  Front: the
// frame table and the zero fills, then the finder chain (k1_moments -- the only pass over pixels outside the flat blocks' tiles
// --, certify, the literal blocks, select, the unit lists: small latency-bound kernels).  Back: the accumulation kernels, the
// results' D2H, the hand-over to the drainer.
// Deferred (the default without the device half): back(N) is queued behind front(N + 1), so the main stream runs
// accumulation(N), accumulation(N + 1), ... back to back (the big kernels never share the chip, which only stretches them), and
// the side stream's chain of N + 1 runs next to accumulation(N) and is long done when accumulation(N + 1) comes up.
// The window (the device half, launches of kLatestWindowMinBatch frames or more): nothing is deferred and nothing runs beside
// an accumulation launch.  k4_latest(N) follows the tail of N on the stream that ran it and the finder chain of N + 1 waits for
// kernels_done[N] -- back(N) has to be queued before front(N + 1) can name that event -- so 64 workgroups of serial f64 chains
// run beside a pass over HBM and small kernels: the two want different things and are about as long, 270 and 260 us at 4K.
// Period 850 - 865 us a 64-frame batch against 965 - 985 with the chain beside the luma launch and k4_latest on a stream of
// its own (profiles/r09_latest_window.txt, which also has the three forms that lost).  Not for narrower launches: k4_latest's
// time goes with a frame's blocks (a workgroup a frame), the chain's and the accumulation's with the launch's frames too, so
// there the kernel is the longer side of the window and the chip waits for 32 workgroups -- 8K 4:4:4 in 32-frame launches:
// k4_latest 845 us against a chain of 585, 324 k Mpx/s with the window against 342 - 359 k without.
int g1s_diff::submit(int si) {
  Slot &sl = slots[si];
  if (sl.count == 0) return G1S_OK;
  {
    std::lock_guard<std::mutex> lk(dm);
    slot_busy[si] = true;  // until the drainer has folded it
  }
  trace_host("submit", si);
  int rc = plan_batch(si);
  if (rc) return rc;
  rc = launch_front(si);
  if (rc) return rc;
  trace_host("front queued", si);
  const int prev = pending;
  pending = si;
  if (prev >= 0) {
    rc = launch_back(prev);
    if (rc) return rc;
    trace_host("back queued", prev);
  }
  if (sl.plan.back_now) {
    rc = flush_pending();
    if (rc) return rc;
  }
  {
    // move on to the next slot; wait if the drainer has not freed it yet (back-pressure)
    std::unique_lock<std::mutex> lk(dm);
    cur = (si + 1) % kSlots;
    cv_free.wait(lk, [&] { return !slot_busy[cur]; });
  }
  trace_host("next slot free", cur);
  return G1S_OK;
}

// The batch's schedule, decided once: what the chains depend on (the frame table cannot change once the batch is submitted)
// and the stream of every part (schedule.h).  The only reader of the stream switches and of `timing`.
int g1s_diff::plan_batch(int si) {
  Slot &sl = slots[si];
  BatchPlan &p = sl.plan;
  p.g = batch_geom(sl);
  p.wide = wide_ok(p.g, batch_far(sl));
  p.timed = timing;
  p.chain = timing && timing_chain;
  const g1s_sched::Schedule s = g1s_sched::schedule(switches(), {p.timed, device_latest, p.wide, batch, si, p.g.nplanes, last_back});
  // (the device half's streams: made when a generator first runs that half outside the window)
  if ((s.latest == Role::latest || s.latest == Role::latest2) && !ensure_latest_streams(ss)) return fail_hip("the device half's streams could not be created");
  const hipStream_t of[] = {ss.compute, ss.flat, ss.flat2, ss.copy, ss.upload, ss.latest, ss.latest2};  // (Role's order)
  p.table = of[(int)s.table], p.finder = of[(int)s.finder], p.accum = of[(int)s.accum], p.rest = of[(int)s.rest];
  p.latest = of[(int)s.latest], p.d2h = of[(int)s.d2h];
  p.back_now = s.back_now, p.after = s.after, p.host_waits = s.host_waits;
  sl.marks.n = 0, sl.marks.timed = p.timed && !p.chain, sl.marks.trace = trace && !p.timed;
  return G1S_OK;
}

int g1s_diff::flush_pending() {
  if (pending < 0) return G1S_OK;
  const int si = pending;
  pending = -1;
  return launch_back(si);
}

int g1s_diff::launch_front(int si) {
  Slot &sl = slots[si];
  const BatchPlan &p = sl.plan;
  const Geom &g = p.g;
  const uint32_t B = sl.count;
  // The finder chain's place beside the accumulation of the batch before -- measured and dropped: k1_moments on the main
  // stream in front of that accumulation, the rest of the chain beside it: -3 to -10 % at 4K, +11 % at 1080p, -4 % at 8K
  // (profiles/r04_streams.txt); k1_moments on a stream of its own: profiles/r05o_streams.txt.
  // G1S_SIDE2=1: a batch's chain on the side stream of its slot's parity: the latency-bound tail of a chain (certify, the
  // literal blocks, select, unit lists) then runs next to the moments kernel of the batch after it -- one waits on dependent
  // loads, the other streams through HBM -- instead of in front of it (the timeline shows them overlap either way)
  const hipStream_t up = p.table, fstream = p.finder;
  const FrameTable ft{sl.d_planes};  // pinned host copy -> device on `up`: the upload stream is idle, done long before the main stream gets here
  if (sl.async_in) {  // queued frame copies: on the upload stream; everything below waits for `up`
    if (up != ss.upload) {
      if (!h2d_order) HIP_TRY(hipEventCreateWithFlags(&h2d_order.p, hipEventDisableTiming));
      HIP_TRY(hipEventRecord(h2d_order, ss.upload));
      HIP_TRY(hipStreamWaitEvent(up, h2d_order, 0));
    }
    sl.async_in = false;
  }
  sl.marks.mark_trace(up, "table H2D");
  HIP_TRY(hipMemcpyAsync(sl.d_planes, sl.h_planes, sizeof(FramePlanes) * B, hipMemcpyHostToDevice, up));
  sl.marks.mark_trace(up, "k_zero");
  {
    // all per-batch zero fills in one launch: the records, the counters and flags the kernels add to or set
    ZeroJob z{};
    int nz = 0;
    auto fill = [&](uint8_t *base, size_t off, size_t bytes) { z.ptr[nz] = reinterpret_cast<uint32_t *>(base + off), z.ndw[nz++] = (uint32_t)(bytes / 4); };
    fill(sl.d_records, 0, L.size * B);
    fill(sl.d_mu, lay.mu_count, lay.mu_only - lay.mu_count);  // unit counts (2 lists) and, behind them, the any-deferred flags
    fill(sl.d_mu, lay.mu_only, lay.mu_only_bytes);            // deferred-block flags
    fill(sl.d_k1, lay.k1_count, lay.k1 - lay.k1_count);       // literal-list counts
    if (switches().wide && sl.d_wu) fill(sl.d_wu, lay.wu_lbad, lay.wu_lbad_bytes);  // luma units whose L left int8
    // (on the upload stream too: the slot is free, its buffers can be zeroed while the main stream is still busy
    //  with earlier batches)
    hipLaunchKernelGGL(k_zero, dim3(256), dim3(256), 0, up, z);
  }
  sl.marks.mark_trace(up, nullptr);
  if (up != p.accum) {
    HIP_TRY(hipEventRecord(ss.table_done[si], up));
    HIP_TRY(hipStreamWaitEvent(p.accum, ss.table_done[si], 0));
    HIP_TRY(hipStreamWaitEvent(fstream, ss.table_done[si], 0));  // (the table goes by the upload stream only when the finder chain has a side stream)
  }
  // the window: the chain starts when the accumulation of the batch before has ended (submit)
  if (p.after >= 0) HIP_TRY(hipStreamWaitEvent(fstream, ss.kernels_done[p.after], 0));
  if (p.timed) HIP_TRY(hipEventRecord(sl.ev[kEvStart], fstream));
  {
    // flat-block features: integer moments + certified evaluation; the literal f64 kernel only for
    // the blocks the certificate leaves open (G1S_K1_LITERAL=1 / g1s_diff_set_flat_finder: for every block)
    const int literal_mode = flat_literal ? flat_literal : switches().k1_literal;
    const int force_literal = literal_mode ? 1 : 0;
    int32_t *mom = reinterpret_cast<int32_t *>(sl.d_k1 + lay.k1_moments);
    CertifyLists cl;
    cl.list = reinterpret_cast<uint32_t *>(sl.d_k1 + lay.k1_list);
    cl.count = reinterpret_cast<uint32_t *>(sl.d_k1 + lay.k1_count);
    cl.global = literal_mode == 0 ? 1 : 0;  // (the default chain: one sequence for the launch; "every block literally": per-frame lists)
    // Aligned rows of whole blocks, the default finder: the moments as a pass over column strips that certifies its own
    // blocks (k1_moments_strips); anything else -- unaligned rows, a ragged last block column, the literal modes -- the
    // row-per-lane kernel and k1_certify behind it.  G1S_K1_ROWS=1 (a test and measurement aid, read at every batch): the
    // latter for every batch.
    const char *k1_rows = getenv("G1S_K1_ROWS");
    const bool strips = g.fast_rows && g.W % kBlock == 0 && literal_mode == 0 && !(k1_rows && atoi(k1_rows) != 0);
    if (strips) {
      constexpr int kR2 = G1S_STRIP_ROWS2, kRif = G1S_STRIP_RIF;
      constexpr bool kNt = G1S_STRIP_NT != 0, kFold = G1S_STRIP_FOLD != 0;
      if (p.timed && !p.chain) HIP_TRY(hipEventRecord(sl.ev[kEvMomStart], fstream));
      // (the batch's last luma planes, as many as the last-level cache holds, keep the plain loads; G1S_K1_KEEP_MB: that size, a test
      //  and measurement aid -- 0: the hint on every frame)
      const char *keep_e = getenv("G1S_K1_KEEP_MB");
      const size_t keep_bytes = (size_t)(keep_e ? std::max(atoi(keep_e), 0) : kStripKeepMB) << 20;
      const size_t keep = std::min<size_t>(keep_bytes / ((size_t)g.W * g.src_bps * g.H), B);
      const int nt_frames = kNt ? (int)(B - keep) : 0;
      const dim3 sg((strip_tiles<kR2>(g.nbw, g.nbh) + 3) / 4, B);
      sl.marks.mark(fstream, g.src_bps == 1 ? "k1_moments_strips<1>" : "k1_moments_strips<2>");
      if (g.src_bps == 1)
        hipLaunchKernelGGL((k1_moments_strips<1, kR2, kRif, kNt, kFold>), sg, dim3(256), 0, fstream, ft, g, fc, mom, sl.d_records, sl.d_flags, cl, nt_frames);
      else
        hipLaunchKernelGGL((k1_moments_strips<2, kR2, kRif, kNt, kFold>), sg, dim3(256), 0, fstream, ft, g, fc, mom, sl.d_records, sl.d_flags, cl, nt_frames);
      if (p.timed && !p.chain) HIP_TRY(hipEventRecord(sl.ev[kEvMomEnd], fstream));
    } else {
      // the finder's moments of the luma source: the only pass over pixels that are not in a flat block's tile
      if (p.timed && !p.chain) HIP_TRY(hipEventRecord(sl.ev[kEvMomStart], fstream));
      {  // (also when every block is evaluated literally: the record's luma_sum comes from the moments)
        const dim3 mg((g.nblocks + 7) / 8, B);
        sl.marks.mark(fstream, g.src_bps == 1 ? "k1_moments<1>" : "k1_moments<2>");
        if (g.src_bps == 1) hipLaunchKernelGGL(k1_moments<1>, mg, dim3(256), 0, fstream, ft, g, mom);
        else hipLaunchKernelGGL(k1_moments<2>, mg, dim3(256), 0, fstream, ft, g, mom);
      }
      if (p.timed && !p.chain) HIP_TRY(hipEventRecord(sl.ev[kEvMomEnd], fstream));
    }
    if (!strips || !G1S_STRIP_FOLD) {
      sl.marks.mark(fstream, "k1_certify");
      hipLaunchKernelGGL(k1_certify, dim3((g.nblocks + 255) / 256, B), dim3(256), 0, fstream, g, fc, (const int32_t *)mom,
                         sl.d_records, sl.d_flags, cl, force_literal);
    }
    sl.marks.mark(fstream, literal_mode == 1 ? "k1_flat_features" : "k1_flat_block");
    if (literal_mode == 1) {  // every block: one lane per block
      dim3 grid((g.nblocks + 63) / 64, B);
      if (g.src_bps == 1)
        hipLaunchKernelGGL((k1_flat_features<1, true>), grid, dim3(64), 0, fstream, ft, g, fc, d_lut, sl.d_records, sl.d_flags,
                           (const uint32_t *)cl.list, (const uint32_t *)cl.count);
      else
        hipLaunchKernelGGL((k1_flat_features<2, true>), grid, dim3(64), 0, fstream, ft, g, fc, d_lut, sl.d_records, sl.d_flags,
                           (const uint32_t *)cl.list, (const uint32_t *)cl.count);
    } else {  // the few blocks the certificate leaves open (mode 2, a test aid: every block): one wave per block
      dim3 grid(kFbGrid);
#define G1S_FB(BP, GL) hipLaunchKernelGGL((k1_flat_block<BP, GL>), grid, dim3(64), 0, fstream, ft, g, fc, d_lut, sl.d_records, sl.d_flags, \
                                          (const uint32_t *)cl.list, (const uint32_t *)cl.count, (int)B)
      if (cl.global) {
        if (g.src_bps == 1) G1S_FB(1, true);
        else G1S_FB(2, true);
      } else {
        if (g.src_bps == 1) G1S_FB(1, false);
        else G1S_FB(2, false);
      }
#undef G1S_FB
    }
  }
  if (p.timed && !p.chain) HIP_TRY(hipEventRecord(sl.ev[kEvFinderEnd], fstream));
  const bool w_lists = p.wide;  // the wide chain: the unit lists come out of the select kernel
  WUnitParams wup{};
  if (w_lists) {
    for (int k = 0; k < 2; ++k) {
      wup.units[k] = reinterpret_cast<uint32_t *>(sl.d_wu + lay.wu_units[k]);
      wup.ncell[k] = w_ncell[k];
      wup.gx[k] = w_gx[k];
    }
    wup.count = reinterpret_cast<uint32_t *>(sl.d_wu + lay.wu_count);
    wup.ub[0] = 4;
    wup.ub[1] = w_ub_c;
  }
  sl.marks.mark(fstream, w_lists ? "k2w_select_units" : "k2_flat_select");
  if (w_lists) hipLaunchKernelGGL(k2w_select_units, dim3(B, g.nplanes == 3 ? 2 : 1), dim3(kK2Threads), 0, fstream, g, sl.d_records, (const uint8_t *)sl.d_flags, wup);
  else hipLaunchKernelGGL(k2_flat_select, dim3(B), dim3(kK2Threads), 0, fstream, g, sl.d_records, sl.d_flags);
  if (p.timed && !p.chain) HIP_TRY(hipEventRecord(sl.ev[kEvSelectEnd], fstream));
  if (!w_lists) {
    // the unit lists (chunks with a flat block) need the flat mask (the wide chain: k2w_select_units has built them)
    const MParams mp = make_mparams(sl);
    sl.marks.mark(fstream, "k3m_units");
    hipLaunchKernelGGL(k3m_units, dim3((m_nunits + 255) / 256, B), dim3(256), 0, fstream, g, (const uint8_t *)sl.d_records, mp);
  }
  sl.marks.mark(fstream, nullptr);
  if (fstream != p.accum) HIP_TRY(hipEventRecord(ss.mask_done[si], fstream));
  HIP_TRY(hipGetLastError());
  return G1S_OK;
}

// the wide chain serves: equal sample widths, every plane's rows 16-byte aligned, whole 8-sample words in every plane,
// (unaligned planes, odd widths and mixed depths run the stream chain)
bool g1s_diff::wide_ok(const Geom &g, bool far) const {
  if (!switches().wide || switches().w_off) return false;
  if (g.lag < 1) return false;
  // inputs of one sample size and one narrowing shift <= 4: the residual in place (w_residual); any other pair of depths: the
  // general form (w_residual_gen), built for 4:2:0 and for frames without chroma planes (the other subsamplings of such a pair
  // run the stream chain)
  if (wide_gen(g) && !(g.nplanes != 3 || (g.xdec == 1 && g.ydec == 1))) return false;
  const int need = g.nplanes == 3 ? 0x3f : 0x09;
  if ((g.vec_mask & need) != need) return false;
  if (far) return false;  // a plane of 2 GiB or more from first to last sample (batch_far): the stream chain
  if ((g.W & 7) != 0 || (g.nplanes == 3 && ((g.W >> g.xdec) & 7) != 0)) return false;
  if (g.nbw > 1023 * 4 || g.nbh > 4095) return false;
  return true;
}

bool g1s_diff::wide_gen(const Geom &g) { return g.src_bps != g.den_bps || g.src_shift != g.den_shift || g.src_shift > 4; }

MParams g1s_diff::make_mparams(const Slot &sl) const {
  MParams mp;
  mp.units = reinterpret_cast<uint32_t *>(sl.d_mu + lay.mu_units);
  mp.unit_count = reinterpret_cast<uint32_t *>(sl.d_mu + lay.mu_count);
  mp.only_any = reinterpret_cast<uint32_t *>(sl.d_mu + lay.mu_any);
  mp.only = sl.d_mu + lay.mu_only;
  mp.partials = sl.d_mpart;
  mp.nunits = m_nunits;
  return mp;
}

// the luma launch is queued on plan.accum: the chroma launch and what follows go to plan.rest
int g1s_diff::to_rest(const BatchPlan &p, int si) {
  if (p.rest == p.accum) return G1S_OK;
  HIP_TRY(hipEventRecord(ss.kernels_done[si], p.accum));
  HIP_TRY(hipStreamWaitEvent(p.rest, ss.kernels_done[si], 0));
  return G1S_OK;
}

// the wide chain (k3w.hip.h): luma launch (leaves L behind), chroma launch, k3w_tail = the reducer + the exact kernel for
// deferred blocks
int g1s_diff::accumulate_wide(Slot &sl, int si) {
  const BatchPlan &p = sl.plan;
  const Geom &g = p.g;
  const uint32_t B = sl.count;
  const FrameTable ft{sl.d_planes};  // (uploaded by the front half)
  const MParams mp = make_mparams(sl);
  const bool chroma = g.nplanes == 3;
  WParams wq;
  wq.ft = ft;
  wq.records = sl.d_records;
  wq.partials = mp.partials;
  wq.only = mp.only;
  wq.only_any = mp.only_any;
  wq.lbad = sl.d_wu + lay.wu_lbad;
  wq.lplane = sl.d_lplane;
  wq.lpitch = w_lpitch;
  wq.lframe_bytes = w_lframe;
  wq.ncell_y = w_ncell[0];
  wq.gx_y = w_gx[0];
  wq.frames = (int)B;
  const int w_rev = switches().w_rev;
  int Gk[2] = {w_wgs_per_frame(w_ncell[0], (int)B, 0), w_wgs_per_frame(std::max(w_ncell[1], 1), (int)B, 1)};
  for (int k = 0; k < 2; ++k) {
    if ((size_t)Gk[k] * B <= m_wg_cap) continue;
    // the environment (G1S_W_WGS / G1S_W_WGS_C) changed after the slots were sized: what the slots hold -- but never fewer
    // workgroups than the int32 accumulators and the parked entries of a workgroup allow
    Gk[k] = (int)(m_wg_cap / B) & ~7;
    const int ncell_k = k == 0 ? w_ncell[0] : std::max(w_ncell[1], 1), cap_k = k == 1 ? kWMaxUnitsC : kWMaxUnits;
    if (Gk[k] <= 0 || Gk[k] < (ncell_k + cap_k - 1) / cap_k)
      return fail(G1S_ERR_STATE, "the wide launches' workgroup count was raised (G1S_W_WGS / G1S_W_WGS_C) after this generator's buffers were sized");
  }
  const int G_cap = std::max(Gk[0], Gk[1]);
  wq.wg_cap = G_cap;
  auto set_kind = [&](int k) {
    wq.units = reinterpret_cast<const uint32_t *>(sl.d_wu + lay.wu_units[k]);
    wq.count = reinterpret_cast<const uint32_t *>(sl.d_wu + lay.wu_count) + k;  // (stride 2: see the kernel)
    wq.ncell = w_ncell[k];
    wq.wgs = Gk[k];
  };
#define G1S_WG(KIND, BP, SX, SY, BD, GEN)                                                                              \
  do {                                                                                                                 \
    constexpr int lds_ = w_lds_bytes(KIND, WShape<KIND, SX, SY>::BH);                                                  \
    static const hipError_t attr_ = hipFuncSetAttribute(reinterpret_cast<const void *>(&k3w_pass<KIND, BP, SX, SY, BD, GEN>), \
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, lds_);             \
    (void)attr_;                                                                                                       \
    char kn_[64];                                                                                                      \
    if (GEN) snprintf(kn_, sizeof(kn_), "k3w_pass<%d, %d, %d, %d, %d, true>", KIND, BP, SX, SY, BD);                   \
    else snprintf(kn_, sizeof(kn_), "k3w_pass<%d, %d, %d, %d>", KIND, BP, SX, SY);                                     \
    const hipStream_t st_ = KIND ? p.rest : p.accum;                                                                   \
    sl.marks.mark(st_, kn_);                                                                                           \
    set_kind(KIND);                                                                                                    \
    wq.rev = (w_rev >> KIND) & 1;                                                                                      \
    hipLaunchKernelGGL((k3w_pass<KIND, BP, SX, SY, BD, GEN>), dim3((uint32_t)Gk[KIND] * B), dim3(kWThreads), lds_, st_, g, wq); \
  } while (0)
#define G1S_W(KIND, BP, SX, SY) G1S_WG(KIND, BP, SX, SY, BP, false)
#define G1S_WB(KIND, SX, SY)                   \
  do {                                         \
    if (g.src_bps == 2) G1S_W(KIND, 2, SX, SY); \
    else G1S_W(KIND, 1, SX, SY);               \
  } while (0)
  // (the general form: wide_ok lets it through for 4:2:0 and for frames without chroma planes)
#define G1S_WGEN(KIND, SX, SY)                                              \
  do {                                                                      \
    if (g.src_bps == 2 && g.den_bps == 2) G1S_WG(KIND, 2, SX, SY, 2, true); \
    else if (g.src_bps == 2) G1S_WG(KIND, 2, SX, SY, 1, true);              \
    else G1S_WG(KIND, 1, SX, SY, 2, true); /* (two 8-bit inputs are never general) */ \
  } while (0)
#define G1S_WK(KIND)                                 \
  do {                                               \
    if (g.xdec == 1 && g.ydec == 1) G1S_WB(KIND, 1, 1); \
    else if (g.xdec == 1) G1S_WB(KIND, 1, 0);        \
    else if (g.ydec == 1) G1S_WB(KIND, 0, 1);        \
    else G1S_WB(KIND, 0, 0);                         \
  } while (0)
  const bool gen = wide_gen(g);
  if (!chroma) {
    if (gen) G1S_WGEN(0, -1, -1);
    else G1S_WB(0, -1, -1);
  } else {
    if (gen) G1S_WGEN(0, 1, 1);
    else G1S_WK(0);
    // The chroma launch stays on the main stream behind the luma launch.  Round 3's chain moved it (and what follows) to the
    // copy stream, next to the luma launch of the batch after; with this chain both launches fill every register of the
    // chip and only stretch each other: serial is +2 - 5 % on the 4K job, +10 % at 8K 4:4:4 (profiles/r04_streams.txt).
    // (G1S_W_ASIDE: the chroma launch and what follows next to the luma launch of the batch after)
    if (int rc = to_rest(p, si)) return rc;
    if (gen) G1S_WGEN(1, 1, 1);
    else G1S_WK(1);
  }
#undef G1S_WGEN
#undef G1S_WG
#undef G1S_WK
#undef G1S_WB
#undef G1S_W
  // (the record's block statistics and AR sums: k3_ar_generic adds to / overwrites what the launches and the reduction wrote,
  //  and the exact kernel reads the frame number relative to the launch: frame0 is 0 here)
  sl.marks.mark(p.rest, "k3w_tail");
  hipLaunchKernelGGL(k3w_tail, dim3(kWTailParts + std::min(kWTailChunks, g.nblocks), g.nplanes, B), dim3(kK3Threads), 0, p.rest, ft, g,
                     sl.d_records, (const uint8_t *)mp.only, (const uint32_t *)mp.only_any, (const long long *)mp.partials, G_cap, Gk[0], Gk[1]);
  return G1S_OK;
}

// the stream chain (k3s.hip.h), what the wide chain falls back on: the fused pass -- planes of the flat blocks' tiles ->
// residuals, block statistics, exact int8 SYRK on the matrix cores, one partial system per workgroup; the reducer; then the
// exact int32 kernel for the few blocks next to a residual outside int8
int g1s_diff::accumulate_stream(Slot &sl, int si) {
  const BatchPlan &p = sl.plan;
  const Geom &g = p.g;
  const uint32_t B = sl.count;
  const FrameTable ft{sl.d_planes};  // (uploaded by the front half)
  const MParams mp = make_mparams(sl);
  FParams fq;
  fq.ft = ft;
  fq.units = mp.units;
  fq.unit_count = mp.unit_count;
  fq.partials = mp.partials;
  fq.ustats = reinterpret_cast<int32_t *>(sl.d_mu + lay.mu_ustats);
  fq.nunits = m_nunits;
  int G_kind[2] = {m_wgs_per_frame(m_nunits, (int)B, 0), m_wgs_per_frame(m_nunits, (int)B, 1)};  // luma launch, chroma launch
  for (int &Gk : G_kind)
    if ((size_t)Gk * B > m_wg_cap) Gk = m_wgs_per_frame(m_nunits, 1 << 20);  // (G1S_F_WGS raised after the slots were sized: the fewest that hold the units)
  const int G_cap = std::max(G_kind[0], G_kind[1]);
  int G = G_kind[0];
  const int cbw = g.nplanes == 3 ? (kBlock >> g.xdec) : 0, cbh = g.nplanes == 3 ? (kBlock >> g.ydec) : 0;
  fq.lplane = sl.d_lplane;
  fq.lpitch = m_lpitch;
  fq.lframe_bytes = m_lframe;
  fq.frames = (int)B;
  fq.wgs = G;
  fq.wg_cap = G_cap;
  { const char *e = getenv("G1S_F_REUSE"); fq.reuse = e ? atoi(e) : 1; }  // test / tuning aid (0: every halo word is read)
  dim3 gr((uint32_t)G * B);
  // two launches: the luma plane (which leaves L behind), then the two chroma planes
  // (unaligned planes, odd widths, mixed or deep bit depths: ONE instantiation per format and launch, sample widths at run time)
#define G1S_FS(CW, CH, PL)                                                                                           \
  do {                                                                                                               \
    static const hipError_t attr_rs = hipFuncSetAttribute(reinterpret_cast<const void *>(&k3s_fused<CW, CH, 0, PL>), \
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);   \
    (void)attr_rs;                                                                                                   \
    constexpr size_t lds = s_lds_bytes(CW, CH, PL);                                                                  \
    static_assert(lds <= 144 * 1024, "the tile buffers fit the LDS the kernel may ask for");                         \
    char kn_[64];                                                                                                    \
    snprintf(kn_, sizeof(kn_), "k3s_fused<%d, %d, %d, %d>", CW, CH, 0, PL);                                          \
    const hipStream_t st_ = PL ? p.rest : p.accum;                                                                   \
    sl.marks.mark(st_, kn_);                                                                                         \
    G = G_kind[PL ? 1 : 0];                                                                                          \
    fq.wgs = G;                                                                                                      \
    gr = dim3((uint32_t)G * B);                                                                                      \
    hipLaunchKernelGGL((k3s_fused<CW, CH, 0, PL>), gr, dim3(kFThreads), lds, st_, g, fq);                            \
  } while (0)
  // (the chroma launch, the finisher and what follows go to the copy stream -- next to the luma launch of the batch after --
  //  unless G1S_F_SERIAL)
#define G1S_FP(CW, CH)                      \
  do {                                      \
    G1S_FS(CW, CH, 0);                      \
    if (int rc = to_rest(p, si)) return rc; \
    G1S_FS(CW, CH, 1);                      \
  } while (0)
  if (cbw == 0) G1S_FS(0, 0, 0);
  else if (cbw == 16 && cbh == 16) G1S_FP(16, 16);
  else if (cbw == 16) G1S_FP(16, 32);
  else if (cbh == 32) G1S_FP(32, 32);
  else G1S_FP(32, 16);
#undef G1S_FP
#undef G1S_FS
  sl.marks.mark(p.rest, "k3m_finish");
  hipLaunchKernelGGL(k3m_finish, dim3(kMFinishParts * g.nplanes + kMFinishWgs, B), dim3(256), 0, p.rest, g, mp, G_kind[0], G_kind[1], G_cap,
                     (const int32_t *)fq.ustats, sl.d_records);
  sl.marks.mark(p.rest, "k3_ar_generic");
  hipLaunchKernelGGL(k3_ar_generic, dim3(std::min(kK3Chunks, g.nblocks), g.nplanes, B), dim3(kK3Threads), 0, p.rest, ft, g,
                     sl.d_records, (const uint8_t *)mp.only, (const uint32_t *)mp.only_any);
  return G1S_OK;
}

// the batch's results to the host, on the copy stream behind the tail kernels (the main stream goes straight on to the next
// batch): the records -- or, when the per-frame half of the fold runs on the device, that half and its blobs
int g1s_diff::copy_out(Slot &sl, int si) {
  const BatchPlan &p = sl.plan;
  const uint32_t B = sl.count;
  HIP_TRY(hipEventRecord(ss.kernels_done[si], p.rest));
  HIP_TRY(hipStreamWaitEvent(p.d2h, ss.kernels_done[si], 0));
  if (!device_latest) {
    HIP_TRY(hipMemcpyAsync(sl.h_records, sl.d_records, L.size * B, hipMemcpyDeviceToHost, p.d2h));
    HIP_TRY(hipEventRecord(sl.done, p.d2h));
    return G1S_OK;
  }
  // the per-frame half of the fold where the records lie: the host gets 27 KB of latest state a frame instead of the record
  // (the batch's last record still comes back: g1s_diff_last_record)
  const size_t blob = latest_blob_size(lag), scr = latest_scratch_bytes((uint32_t)L.nblocks);
  HIP_TRY(sl.ensure_latest(blob * batch, scr * batch));
  LatestJob job{};
  job.records = sl.d_records;
  job.L = L;
  job.blobs = sl.d_latest;
  job.blob_bytes = blob;
  job.scratch = sl.d_lscratch;
  job.scratch_bytes = scr;
  job.lag = (int)lag;
  job.n = (int)n;
  job.nplanes = geom.nplanes;
  job.W = geom.W;
  job.H = geom.H;
  job.xdec = geom.xdec;
  job.ydec = geom.ydec;
  job.nbw = geom.nbw;
  job.nbh = geom.nbh;
  // (the window: behind the tail on the stream that ran it, so in the queue ahead of the next batch's finder chain, which waits
  //  for kernels_done[si] -- recorded above, in FRONT of this kernel -- on the side stream)
  if (p.latest != p.rest) HIP_TRY(hipStreamWaitEvent(p.latest, ss.kernels_done[si], 0));  // (why two of them: StreamSet)
  sl.marks.mark(p.latest, latest_kernel_name());
  HIP_TRY(launch_latest(job, B, p.latest));
  sl.marks.mark(p.latest, nullptr);
  HIP_TRY(hipEventRecord(ss.latest_done[si], p.latest));
  HIP_TRY(hipStreamWaitEvent(p.d2h, ss.latest_done[si], 0));
  sl.marks.mark_trace(p.d2h, "blobs D2H");
  HIP_TRY(hipMemcpyAsync(sl.h_latest, sl.d_latest, blob * B, hipMemcpyDeviceToHost, p.d2h));
  HIP_TRY(hipMemcpyAsync(sl.h_records + L.size * (B - 1), sl.d_records + L.size * (B - 1), L.size, hipMemcpyDeviceToHost, p.d2h));
  sl.marks.mark_trace(p.d2h, nullptr);
  HIP_TRY(hipEventRecord(sl.done, p.d2h));
  return G1S_OK;
}

int g1s_diff::launch_back(int si) {
  Slot &sl = slots[si];
  const BatchPlan &p = sl.plan;
  if (p.finder != p.accum) HIP_TRY(hipStreamWaitEvent(p.accum, ss.mask_done[si], 0));  // the mask, the unit lists
  int rc = p.wide ? accumulate_wide(sl, si) : accumulate_stream(sl, si);
  if (rc) return rc;
  sl.marks.mark(p.rest, nullptr);
  if (p.timed) HIP_TRY(hipEventRecord(sl.ev[kEvEnd], p.rest));
  HIP_TRY(hipGetLastError());
  rc = copy_out(sl, si);
  if (rc) return rc;
  // profiling aid (G1S_D2H_SYNC=1, with G1S_ONE_STREAM=1): the records copy has ended before the next batch's first kernel
  // starts -- under rocprofv3 the copy is a blit kernel that otherwise shares the chip with k1_moments and doubles its time
  // A timed batch (g1s_diff_set_timing: every kernel between two events, "alone on the chip") waits for it too: the copy of
  // batch N next to the kernels of batch N + 1 costs the luma launch 4 % at 8K, and on some boxes of the pool the event pair of
  // the batch's last kernel read 280 - 500 us instead of 45 - 75 with it in flight (profiles/r04_rot.txt vs r04_hwq.txt).
  if (p.host_waits == HostWait::copy_stream) HIP_TRY(hipStreamSynchronize(p.d2h));
  else if (p.host_waits == HostWait::done_event) HIP_TRY(hipEventSynchronize(sl.done));  // (the copy's end, whichever stream carried it)
  stats.launches_flat_features++;
  stats.launches_flat_select++;
  stats.launches_ar_accumulate++;
  last_back = si;
  {
    std::unique_lock<std::mutex> lk(dm);
    in_flight.push_back(si);
    ++submitted;
    cv_work.notify_one();
  }
  return G1S_OK;
}

void g1s_diff::drainer_main() {
  (void)hipSetDevice(device);
  for (;;) {
    int si;
    {
      std::unique_lock<std::mutex> lk(dm);
      cv_work.wait(lk, [&] { return drainer_stop || !in_flight.empty(); });
      if (in_flight.empty()) return;  // stop requested and nothing left
      si = in_flight.front();
      in_flight.pop_front();
    }
    const int rc = drain_front(si);
    {
      std::lock_guard<std::mutex> lk(dm);
      if (rc && deferred == G1S_OK) deferred = rc;
      int ok = G1S_OK;
      if (rc) sticky.compare_exchange_strong(ok, rc);  // (the batch is missing from the fold: no table from here on)
      front_failed[si] = rc != G1S_OK;
      fold_q.push_back(si);
    }
    cv_fold.notify_one();
  }
}

void g1s_diff::folder_main() {
  for (;;) {
    int si;
    {
      std::unique_lock<std::mutex> lk(dm);
      cv_fold.wait(lk, [&] { return folder_stop || !fold_q.empty(); });
      if (fold_q.empty()) return;  // stop requested and nothing left
      si = fold_q.front();
      fold_q.pop_front();
    }
    const uint32_t nframes = slots[si].count;  // (drain_back hands the slot back empty)
    const int rc = drain_back(si);
    {
      std::lock_guard<std::mutex> lk(dm);
      if (rc && deferred == G1S_OK) deferred = rc;
      int ok = G1S_OK;
      if (rc) sticky.compare_exchange_strong(ok, rc);
      slot_busy[si] = false;
      ++drained;
      frames_released += nframes;
    }
    cv_free.notify_all();
  }
}

void g1s_diff::wait_drained(uint64_t upto) {
  std::unique_lock<std::mutex> lk(dm);
  cv_free.wait(lk, [&] { return drained >= upto; });
}

int g1s_diff::drain_front(int si) {
  Slot &sl = slots[si];
  std::vector<FrameLatest> &latest = latest_s[si];
  std::vector<uint32_t> &nflat_v = nflat_s[si];
  std::vector<uint8_t> &latest_stage = stage_s[si];
  HIP_TRY(hipEventSynchronize(sl.done));
  const std::vector<Marks::Mark> &km = sl.marks.m;
  const size_t nk = sl.marks.n;
  if (sl.marks.trace && trace_base) {
    std::lock_guard<std::mutex> lk(trace_mutex);
    for (size_t i = 0; i < nk; ++i) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, trace_base, km[i].ev) != hipSuccess) continue;
      char b[160];
      snprintf(b, sizeof(b), "G %12.1f slot %d stream %p %s", ms * 1e3, si, (void *)km[i].stream, km[i].name.empty() ? "-" : km[i].name.c_str());
      trace_lines.emplace_back(b);
    }
    trace_lines.emplace_back(std::string("H ") + std::to_string(trace_now()) + " drained slot " + std::to_string(si));
  }
  if (sl.plan.chain) {
    // (one pair of events around the batch's chain: what the chain takes alone on the chip with nothing between its kernels
    //  but their own dependencies -- the per-kernel events below each put a barrier packet and a signal between two launches)
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, sl.ev[kEvStart], sl.ev[kEvEnd]));
    stats.ms_chain += ms;
    stats.chain_batches += 1;
  } else if (sl.plan.timed) {
    float ms = 0;
    float ms_mom = 0;  // the finder's moments pass
    HIP_TRY(hipEventElapsedTime(&ms_mom, sl.ev[kEvMomStart], sl.ev[kEvMomEnd]));
    HIP_TRY(hipEventElapsedTime(&ms, sl.ev[kEvStart], sl.ev[kEvFinderEnd]));
    stats.ms_flat_features += ms;
    stats.ms_residual += ms_mom;
    HIP_TRY(hipEventElapsedTime(&ms, sl.ev[kEvFinderEnd], sl.ev[kEvSelectEnd]));
    stats.ms_flat_select += ms;
    HIP_TRY(hipEventElapsedTime(&ms, sl.ev[kEvSelectEnd], sl.ev[kEvEnd]));
    stats.ms_ar_accumulate += ms;
    HIP_TRY(hipEventElapsedTime(&ms, sl.ev[kEvStart], sl.ev[kEvEnd]));
    stats.ms_total_gpu += ms;
    {
      std::lock_guard<std::mutex> lk(ktimes_mutex);
      for (size_t i = 0; i + 1 < nk; ++i) {
        if (km[i].name.empty()) continue;  // (the gap between the two halves of a batch)
        HIP_TRY(hipEventElapsedTime(&ms, km[i].ev, km[i + 1].ev));
        auto &kt = ktimes[km[i].name];
        kt.first += ms;
        kt.second += 1;
      }
    }
    {
      std::vector<uint32_t> cnt(batch);
      HIP_TRY(hipMemcpy(cnt.data(), sl.d_k1 + lay.k1_count, sizeof(uint32_t) * batch, hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < sl.count; ++i) stats.literal_blocks += cnt[i];
    }
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (latest.size() < sl.count) latest.resize(sl.count);
  nflat_v.assign(sl.count, 0);
  // ---- per-frame half, concurrent: header, symmetric mirror, latest noise state ----
  const size_t blob = latest_only ? latest_blob_size(lag) : 0;
  if (latest_only) latest_stage.resize(blob * sl.count);
  auto finish_record = [&](int i) {
    uint8_t *rec = sl.h_records + L.size * i;
    RecHeader h = make_header(L, shape.width, shape.height, shape.xdec, shape.ydec, lag);
    const uint8_t *mask = rec + L.off_mask;
    uint32_t nflat = 0;
    for (uint32_t b = 0; b < L.nblocks; ++b) nflat += mask[b] != 0;
    h.status = nflat;
    nflat_v[i] = nflat;
    std::memcpy(rec, &h, sizeof(h));
    // mirror the symmetric AR sums so consumers see full matrices
    for (int c = 0; c < geom.nplanes; ++c) {
      int64_t *S = reinterpret_cast<int64_t *>(rec + L.off_ar[c]);
      const int nc = (int)n + (c > 0);
      for (int a = 0; a < nc; ++a)
        for (int b = a + 1; b < nc; ++b) S[b * nc + a] = S[a * nc + b];
    }
    return rec;
  };
  if (device_latest) {
    // the latest states were computed on the device (k4_latest): nothing per frame is left but reading the headers
    const size_t bl = latest_blob_size(lag);
    std::vector<FrameView> &views = views_s[si];
    if (views.size() < sl.count) views.resize(sl.count);
    int rc = G1S_OK;
    for (uint32_t i = 0; i < sl.count; ++i) {
      uint8_t *b = sl.h_latest + bl * i;
      LatestHeader *h = reinterpret_cast<LatestHeader *>(b);
      nflat_v[i] = h->reserved;
      h->reserved = 0;  // (the kernel's note to this function; the blob a rank sends is the blob the host half would make)
      if (!latest_only && view_of_blob(b, bl, lag, views[i]) != G1S_OK) rc = G1S_ERR_INVALID;
    }
    if (latest_only) latest_stage.assign(sl.h_latest.p, sl.h_latest + bl * sl.count);
    if (sl.count) finish_record((int)sl.count - 1);
    ms_fold_front += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc) {
      std::lock_guard<std::mutex> lk(dm);
      err = "k4_latest wrote a blob the fold does not recognise";
    }
    return rc;
  }
  auto per_frame = [&](int i) {
    uint8_t *rec = finish_record(i);
    if (!records_only) compute_latest(rec, L.size, lag, latest[i]);
    if (latest_only) latest_to_blob(latest[i], lag, latest_stage.data() + (size_t)i * blob);
  };
  on_shared_pool((int)sl.count, per_frame);
  ms_fold_front += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return G1S_OK;
}

// ---- ordered half, serial in frame order; runs next to the per-frame half of the following batch ----
int g1s_diff::drain_back(int si) {
  Slot &sl = slots[si];
  std::vector<FrameLatest> &latest = latest_s[si];
  const std::vector<uint32_t> &nflat_v = nflat_s[si];
  const std::vector<uint8_t> &latest_stage = stage_s[si];
  const size_t blob = latest_only ? latest_blob_size(lag) : 0;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = G1S_OK;
  if (front_failed[si]) {
    sl.count = 0;
    return G1S_OK;  // (the error is already in `deferred`)
  }
  for (uint32_t i = 0; i < sl.count; ++i) {
    uint8_t *rec = sl.h_records + L.size * i;
    stats.frames++;
    stats.blocks += L.nblocks;
    stats.flat_blocks += nflat_v[i];
    if (records_only) {
      std::lock_guard<std::mutex> lk(dm);
      records_out.insert(records_out.end(), rec, rec + L.size);
      records_out_frames++;
    } else if (latest_only) {
      std::lock_guard<std::mutex> lk(dm);
      latest_out.insert(latest_out.end(), latest_stage.begin() + blob * i, latest_stage.begin() + blob * (i + 1));
      latest_out_frames++;
    }
  }
  if (!records_only && !latest_only && sticky == G1S_OK && sl.count) {
    // the ordered merge of the batch: combined-model solves in parallel, tests and commits in order
    // (on the merge pool: the shared pool is busy with the next batch's per-frame half)
    rc = device_latest ? fold->push_latest_many(views_s[si].data(), sl.count, on_merge_pool) : fold->push_latest_many(latest.data(), sl.count, on_merge_pool);
    if (rc) {
      std::lock_guard<std::mutex> lk(dm);
      err = fold->error();
      sticky = rc;
    }
  }
  if (latest_only && sl.count) {
    std::lock_guard<std::mutex> lk(dm);
    latest_batches.push_back(sl.count);
  }
  if (sl.count) last_record.assign(sl.h_records + L.size * (sl.count - 1), sl.h_records + L.size * sl.count);
  sl.count = 0;
  ms_fold_back += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int g1s_diff::drain_all() {
  uint64_t upto;
  {
    std::lock_guard<std::mutex> lk(dm);
    upto = submitted;
  }
  wait_drained(upto);
  return G1S_OK;  // errors of drained batches are in `deferred` / `sticky`
}

void g1s_diff::release() {
  if (drainer.joinable()) {
    {
      std::lock_guard<std::mutex> lk(dm);
      drainer_stop = true;
    }
    cv_work.notify_all();
    drainer.join();  // (it drains whatever was still queued first)
  }
  if (folder.joinable()) {
    {
      std::lock_guard<std::mutex> lk(dm);
      folder_stop = true;
    }
    cv_fold.notify_all();
    folder.join();
  }
  for (hipStream_t st : {ss.compute, ss.copy, ss.latest, ss.latest2, ss.flat, ss.flat2, ss.upload})  // (whichever were made)
    if (st) (void)hipStreamSynchronize(st);
  // (the trace: written when nothing can add to it any more -- the drainer and the folder are joined, the streams idle)
  if (trace) {
    std::lock_guard<std::mutex> lk(trace_mutex);
    if (!trace_lines.empty()) {
      if (FILE *f = fopen(getenv("G1S_TRACE"), "a")) {
        for (const auto &l : trace_lines) fprintf(f, "%s\n", l.c_str());
        fclose(f);
      }
      trace_lines.clear();
    }
  }
  release_streams(ss);
  for (Slot &sl : slots) {
    if (sl.h_planes && geometry_set) {  // park the buffers for the next generator of this geometry
      std::lock_guard<std::mutex> lk(g_cache_mutex);
      if (g_slot_cache.size() < 8) {
        sl.count = 0;
        g_slot_cache.push_back(CachedSlot{device, lay, geom.W, geom.H, geom.xdec, geom.ydec, geom.nplanes, std::move(sl)});
        continue;
      }
    }
    sl = Slot{};  // (frees what the slot holds)
  }
  h2d_pending.clear(), h2d_free.clear(), h2d_order = Event{}, trace_base = Event{};  // (the streams are idle)
  d_lut = nullptr;  // shared per device
  delete fold;
  fold = nullptr;
}

// =============================================================== C ABI =====
extern "C" {

g1s_diff_t *g1s_diff_new(int64_t fps_num, int64_t fps_den, uint32_t source_bit_depth,
                         uint32_t denoised_bit_depth, const g1s_opts_t *opts) {
  g1s_set_global_error_("");
  auto refuse = [](const char *why) -> g1s_diff * {
    g1s_set_global_error_(why);
    return nullptr;
  };
  if (fps_num <= 0 || fps_den <= 0) return refuse("frame rate must be positive");
  // src/main.rs:515-517: "Bit depths not between 8-16 are not currently supported"
  if (source_bit_depth < 8 || source_bit_depth > 16 || denoised_bit_depth < 8 || denoised_bit_depth > 16) return refuse("Bit depths not between 8-16 are not currently supported");
  uint32_t lag = 3, batch = kDefaultBatch;
  bool batch_auto = true;
  bool luma_only = false, records_only = false, latest_only = false;
  int device = -1;
  if (opts) {
    if (opts->struct_size != sizeof(g1s_opts_t)) return refuse("g1s_opts_t.struct_size mismatch");
    if (opts->ar_coeff_lag) lag = opts->ar_coeff_lag;
    if (opts->batch_frames) {
      batch = std::min<uint32_t>(opts->batch_frames, (uint32_t)kMaxBatch);
      batch_auto = false;
    }
    luma_only = opts->luma_only != 0;
    records_only = opts->records_only == 1;
    latest_only = opts->records_only == 2;
    device = opts->device;
  }
  if (lag < 1 || lag > 3) return refuse("ar_coeff_lag must be 1..3");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return refuse("no HIP device available: the diff estimator has no CPU fallback");
  if (device >= 0) {
    if (hipSetDevice(device) != hipSuccess) return refuse("hipSetDevice failed");
  } else if (hipGetDevice(&device) != hipSuccess) {
    return refuse("hipGetDevice failed");
  }
  g1s_diff *g = new g1s_diff();
  g->fps_num = fps_num;
  g->fps_den = fps_den;
  g->src_bd = source_bit_depth;
  g->den_bd = denoised_bit_depth;
  g->lag = lag;
  g->n = num_coeffs(lag);
  g->luma_only = luma_only;
  g->records_only = records_only;
  g->latest_only = latest_only;
  {
    // G1S_LATEST=host|device: where the per-frame half of the fold runs (records_only generators hand out records: host);
    // unset: by the frame's size, once it is known
    const char *e = getenv("G1S_LATEST");
    g->latest_by_size = !e;
    g->device_latest = e && std::string(e) == "device" && !records_only;
  }
  g->batch = batch;
  g->batch_auto = batch_auto;
  g->device = device;
  make_flat_consts(g->fc);
  bool streams_ok = acquire_streams(device, g->ss);  // (a generator without its streams is never handed out: below)
  // the p/255 table is the same for every generator: one device copy per device, kept
  {
    static std::mutex lut_mutex;
    static double *lut_dev[64] = {nullptr};
    std::lock_guard<std::mutex> lk(lut_mutex);
    const int di = device & 63;
    if (!lut_dev[di]) {
      double lut[256];
      for (int i = 0; i < 256; ++i) lut[i] = ((double)i) / 255.0;  // block normalisation, on the host
      if (hipMalloc((void **)&lut_dev[di], sizeof(lut)) != hipSuccess ||
          hipMemcpy(lut_dev[di], lut, sizeof(lut), hipMemcpyHostToDevice) != hipSuccess) {
        lut_dev[di] = nullptr;
        streams_ok = false;
      }
    }
    g->d_lut = lut_dev[di];
  }
  if (!streams_ok) {
    g1s_set_global_error_((std::string("HIP initialisation failed: ") + hipGetErrorString(hipGetLastError())).c_str());
    g->release();
    delete g;
    return nullptr;
  }
  if (!records_only && !latest_only) g->fold = new NoiseFold(fps_num, fps_den, lag);
  if (getenv("G1S_TRACE")) {
    g->trace = hipEventCreate(&g->trace_base.p) == hipSuccess && hipEventRecord(g->trace_base, g->ss.compute) == hipSuccess &&
               hipEventSynchronize(g->trace_base) == hipSuccess;
    g->trace_host0 = std::chrono::steady_clock::now();
  }
  g->drainer = std::thread([g] { g->drainer_main(); });
  g->folder = std::thread([g] { g->folder_main(); });
  return g;
}

// errors of queued frames surface once, on a later call (the drainer thread records them)
static int take_deferred(g1s_diff *g) {
  std::lock_guard<std::mutex> lk(g->dm);
  if (g->sticky) return g->sticky;
  const int rc = g->deferred;
  g->deferred = G1S_OK;
  return rc;
}

int g1s_diff_frame(g1s_diff_t *g, const g1s_frame_t *source, const g1s_frame_t *denoised) {
  if (!g) return G1S_ERR_INVALID;
  if (g->finished) return g->fail(G1S_ERR_STATE, "generator already finished");
  {
    const int pending = take_deferred(g);
    if (pending) return pending;
  }
  (void)hipSetDevice(g->device);
  const int rc = g->append(source, denoised);
  if (rc) return rc;
  return take_deferred(g);
}

int g1s_diff_frames(g1s_diff_t *g, const g1s_frame_t *source, const g1s_frame_t *denoised, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const int rc = g1s_diff_frame(g, source + i, denoised + i);
    if (rc) return rc;
  }
  return G1S_OK;
}

int g1s_diff_sync(g1s_diff_t *g) {
  if (!g) return G1S_ERR_INVALID;
  (void)hipSetDevice(g->device);
  if (g->geometry_set) {
    int rc = g->submit(g->cur);
    if (rc) return rc;
    rc = g->flush_pending();
    if (rc) return rc;
    (void)g->drain_all();
    g->last_back = -1;
  }
  return take_deferred(g);
}

int g1s_diff_finish(g1s_diff_t *g, g1s_segment_t *out, size_t cap, size_t *n_out) {
  if (!g) return G1S_ERR_INVALID;
  if (g->records_only || g->latest_only)
    return g->fail(G1S_ERR_STATE, "records_only / latest_only generator: use g1s_diff_take_* + g1s_fold_*");
  // The segments stay in the object: a call whose buffer is too small reports the count and loses nothing -- the caller
  // sizes the buffer from *n_out and calls again (the reference's Vec has no cap: src/main.rs:524).
  if (!g->finished) {
    const int rc = g1s_diff_sync(g);
    if (rc) return rc;
    g->fold->finish(g->final_segs);
    g->finished = true;  // no more frames
  }
  const int rc = copy_segments(g->final_segs, out, cap, n_out);
  return rc ? g->fail(rc, kSegmentsTooSmall) : G1S_OK;
}

void g1s_diff_free(g1s_diff_t *g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  g->release();
  delete g;
}

const char *g1s_diff_last_error(const g1s_diff_t *g) { return g ? g->err.c_str() : ""; }
// (internal, ingest.cpp: the frame-pair loop prefixes errors with the index of the pair)
uint32_t g1s_diff_source_bit_depth_(const g1s_diff_t *g) { return g ? g->src_bd : 0; }
int32_t g1s_diff_device_(const g1s_diff_t *g) { return g ? g->device : -1; }
// frames the generator can hold at once (its slots x the launch group); 0 until the first frame has set the geometry
uint32_t g1s_diff_frames_in_flight_max_(const g1s_diff_t *g) { return g && g->shape.width ? (uint32_t)kSlots * g->batch : 0; }
void g1s_diff_set_error_text_(g1s_diff_t *g, const char *msg) {
  if (g && msg) g->err = msg;
}

int g1s_diff_take_records(g1s_diff_t *g, void *buf, size_t cap_bytes, size_t *n_frames) {
  if (!g) return G1S_ERR_INVALID;
  if (!g->records_only) return g->fail(G1S_ERR_STATE, "not a records_only generator");
  const int rc = g1s_diff_sync(g);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(g->dm);
  if (n_frames) *n_frames = g->records_out_frames;
  if (g->records_out.size() > cap_bytes) return g->fail(G1S_ERR_CAPACITY, "record buffer too small");
  if (!g->records_out.empty()) std::memcpy(buf, g->records_out.data(), g->records_out.size());
  g->records_out.clear();
  g->records_out_frames = 0;
  return G1S_OK;
}

int g1s_diff_take_latest(g1s_diff_t *g, int sync, void *buf, size_t cap_bytes, size_t *n_frames) {
  if (!g) return G1S_ERR_INVALID;
  if (!g->latest_only) return g->fail(G1S_ERR_STATE, "not a latest_only generator");
  if (sync) {
    const int rc = g1s_diff_sync(g);
    if (rc) return rc;
  } else {
    // everything but the two most recently queued batches has been delivered when this returns
    uint64_t upto;
    {
      std::lock_guard<std::mutex> lk(g->dm);
      upto = g->submitted >= 2 ? g->submitted - 2 : 0;
    }
    g->wait_drained(upto);
  }
  std::lock_guard<std::mutex> lk(g->dm);
  // whole batches, in order: all of them after a sync, otherwise exactly those before the two most recent
  // (so that ranks that run ahead by different amounts still deliver the same batches in the same round)
  const uint64_t upto_batch = sync ? g->delivered + g->latest_batches.size()
                                   : std::min<uint64_t>(g->delivered + g->latest_batches.size(),
                                                        g->submitted >= 2 ? g->submitted - 2 : 0);
  size_t frames = 0;
  uint64_t nb = 0;
  while (g->delivered + nb < upto_batch) frames += g->latest_batches[nb++];
  const size_t bs = latest_blob_size(g->lag);
  if (n_frames) *n_frames = frames;
  if (frames * bs > cap_bytes) return g->fail(G1S_ERR_CAPACITY, "latest buffer too small");
  if (frames) std::memcpy(buf, g->latest_out.data(), frames * bs);
  g->latest_out.erase(g->latest_out.begin(), g->latest_out.begin() + frames * bs);
  g->latest_out_frames -= frames;
  for (uint64_t i = 0; i < nb; ++i) g->latest_batches.pop_front();
  g->delivered += nb;
  return G1S_OK;
}

// ---- frame-shard rounds: a rank's side of the exchange (the messages and the root's merge: host_abi.cpp)
int g1s_shard_pack(g1s_diff_t *g, int flush, void *msg, size_t cap_bytes) {
  if (!g || !msg) return G1S_ERR_INVALID;
  if (!g->latest_only) return g->fail(G1S_ERR_STATE, "not a latest_only generator (records_only = 2)");
  const size_t total = g1s_shard_msg_size(g->lag, g->batch), bs = latest_blob_size(g->lag);
  if (cap_bytes < total) return g->fail(G1S_ERR_CAPACITY, "shard message buffer too small");
  // flush = 0: whatever is ready goes out, nothing is waited for -- the root orders by the batch index in the message, so the
  // ranks need not send the same batch in the same round (they did, and waited for it, when the root merged by arrival: the
  // feeding thread then ran at most two batches ahead of the drain, 3.5 % of a rank's throughput).  A rank is never more than
  // the generator's slots (g1s_shard_flush_rounds) behind with its messages: a round sends nothing only when every unsent batch is still in a slot.
  if (flush) {
    const int rc = g1s_diff_sync(g);
    if (rc) return rc;
  } else {
    const int pending = take_deferred(g);
    if (pending) return pending;
  }
  std::lock_guard<std::mutex> lk(g->dm);
  size_t n = 0;
  uint64_t local_batch = G1S_SHARD_NO_INDEX;
  if (!g->latest_batches.empty()) {  // ONE batch a round, the oldest not sent yet
    n = g->latest_batches.front();
    g->latest_batches.pop_front();
    local_batch = g->delivered;  // (the message says which one: the root orders by it)
    g->delivered += 1;
  }
  const int rc = g1s_shard_msg_from_latest_at(n ? g->latest_out.data() : nullptr, n, g->lag, g->batch, local_batch, msg, cap_bytes);
  if (rc) return rc;
  g->latest_out.erase(g->latest_out.begin(), g->latest_out.begin() + n * bs);
  g->latest_out_frames -= n;
  return G1S_OK;
}

unsigned g1s_shard_flush_rounds(void) { return (unsigned)kSlots; }

int g1s_diff_get_stats(const g1s_diff_t *g, g1s_stats_t *out) {
  if (!g || !out) return G1S_ERR_INVALID;
  *out = g->stats;
  out->ms_host_fold = g->ms_fold_front + g->ms_fold_back;  // (the two stages overlap across batches)
  return G1S_OK;
}
uint64_t g1s_diff_frames_copied(g1s_diff_t *g, uint64_t wait_for) {
  if (!g) return 0;
  (void)hipSetDevice(g->device);
  return g->frames_copied(wait_for);
}
uint64_t g1s_diff_frames_released(g1s_diff_t *g) {
  if (!g) return 0;
  std::lock_guard<std::mutex> lk(g->dm);
  return g->frames_released;
}
long g1s_diff_kernel_times(g1s_diff_t *g, char *buf, size_t cap) {
  if (!g || (!buf && cap)) return G1S_ERR_INVALID;
  std::string out;
  {
    std::lock_guard<std::mutex> lk(g->ktimes_mutex);
    for (const auto &kv : g->ktimes) {
      char line[256];
      snprintf(line, sizeof(line), "%s\t%.6f\t%llu\n", kv.first.c_str(), kv.second.first, (unsigned long long)kv.second.second);
      out += line;
    }
  }
  if (out.size() > cap) return G1S_ERR_CAPACITY;
  std::memcpy(buf, out.data(), out.size());
  return (long)out.size();
}
int g1s_diff_set_flat_finder(g1s_diff_t *g, int mode) {
  if (!g) return G1S_ERR_INVALID;
  if (mode < 0 || mode > 2) return g->fail(G1S_ERR_INVALID, "flat finder mode must be 0, 1 or 2");
  g->flat_literal = mode;
  return G1S_OK;
}
int g1s_diff_set_timing(g1s_diff_t *g, int enable) {
  if (!g) return G1S_ERR_INVALID;
  g->timing = enable != 0;
  g->timing_chain = enable == 2;
  return G1S_OK;
}

int g1s_diff_last_record(const g1s_diff_t *g, void *buf, size_t cap_bytes) {
  if (!g || !buf) return G1S_ERR_INVALID;
  if (g->last_record.empty()) return G1S_ERR_STATE;
  if (g->last_record.size() > cap_bytes) return G1S_ERR_CAPACITY;
  std::memcpy(buf, g->last_record.data(), g->last_record.size());
  return G1S_OK;
}

}  // extern "C"
