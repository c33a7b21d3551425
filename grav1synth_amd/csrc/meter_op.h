// meter_op.h -- the host engine the meters share on top of frame_op.h: measure (measure.hip) and the noise levels (nlf.hip)
// each keep a RecordLane a record kind.  A meter's measuring kernels leave a partial record a unit (a tile, a strip, a
// workgroup); the kind's summing kernel makes a record a job of them; the records come back a batch at a time and
// are held until the caller takes them.  The first part -- the records held and their hand-over, the count of a frame's
// units -- calls nothing of HIP and builds with a host compiler alone (tests/meter_lane_host.cpp drives it); the second part,
// under __HIPCC__, is a batch's queued jobs, the lane, a temporal meter's frame before, and the checks in front of a
// *_finish call.
#pragma once
#include <cstring>
#include <vector>

#include "frame_op.h"

namespace g1s_op {

// The records of a kind since the last hand-over.
template <class Rec>
struct Records {
  std::vector<Rec> records;
  void collect(const Rec *from, size_t n) { records.insert(records.end(), from, from + n); }
  // the records held into the caller's `cap` entries: *n_out says how many there are either way
  int hand_over(Rec *out, size_t cap, size_t *n_out) {
    if (n_out) *n_out = records.size();
    if (records.size() > cap || (!out && !records.empty())) return G1S_ERR_CAPACITY;  // (not sticky: the records stay)
    if (!records.empty()) std::memcpy(out, records.data(), sizeof(Rec) * records.size());
    records.clear();
    return G1S_OK;
  }
};

// How a frame's planes are cut into the units whose partial records a summing launch adds: a plane's count, where its
// partial records start in a job's, a job's count.
struct Units {
  uint32_t n[3] = {0, 0, 0}, base[3] = {0, 0, 0}, frame = 0;
  // n[] is set: the planes' partial records one plane after the other
  void lay() {
    frame = 0;
    for (int c = 0; c < 3; ++c) base[c] = frame, frame += n[c];
  }
  // units of unit_w x unit_h samples over the planes of g (unit_h_chroma: another height for planes 1 and 2; 0 = unit_h)
  void cut(const PlaneGeom &g, int unit_w, int unit_h, int unit_h_chroma = 0) {
    for (int c = 0; c < 3; ++c) {
      const int uh = c && unit_h_chroma ? unit_h_chroma : unit_h;
      n[c] = c < g.nplanes ? (uint32_t)(((g.pw(c) + unit_w - 1) / unit_w) * ((g.ph(c) + uh - 1) / uh)) : 0u;
    }
    lay();
  }
};

}  // namespace g1s_op

#ifdef __HIPCC__

namespace g1s_op {

// What a summing kernel is launched with (km_tail<3>, km_tail<4>, km_tail_s in measure.hip, k_nlf_tail in nlf.hip), grid
// (plane, job): a plane's partial records lie from unit_base[c] of the job's units_frame, units[c] of them
struct TailParams {
  const unsigned long long *partials;  // [job][units_frame][the kind's entries]
  unsigned long long *records;         // [job] the record as 64-bit words
  uint32_t units_frame, units[3], unit_base[3];
};

// the jobs of the batch being filled and their two parameter sets
template <class Job>
struct JobQueue {
  std::vector<Job> jobs;
  ParamSets<Job> sets;
  bool alloc(uint32_t batch) { return sets.alloc(batch); }
  // the queued jobs into set `set` and up on the stream
  hipError_t upload(int set, hipStream_t s) {
    std::memcpy(sets.h[set], jobs.data(), sizeof(Job) * jobs.size());
    return sets.upload(set, jobs.size(), s);
  }
};

// What a record kind owns in a meter, and the steps of a batch that are the same for all kinds.  While the meter is timing,
// INTERVALS + 1 events cut the kind's launches into adjacent intervals: measure has one round a kind's launches (begin, end),
// the noise levels two, luma and chroma (mark).
template <class Rec, int INTERVALS = 1>
struct RecordLane : Records<Rec> {
  bool on = false;  // does the meter make this kind?
  Event ev[INTERVALS + 1];
  DevBuf<unsigned long long> d_partials;
  size_t partials_cap = 0;
  DevBuf<Rec> d_recs;  // a batch's records
  PinnedBuf<Rec> h_recs;
  double ms[INTERVALS] = {};  // in the intervals of the timed batches
  uint64_t timed = 0;         // and the records those made

  // for batches of up to `batch` records (nothing for a kind the meter does not make)
  bool alloc(uint32_t batch) {
    if (!on) return true;
    bool ok = true;
    for (Event &e : ev) ok = ok && hipEventCreate(&e.p) == hipSuccess;
    return ok && hipMalloc((void **)&d_recs.p, sizeof(Rec) * batch) == hipSuccess &&
           hipHostMalloc((void **)&h_recs.p, sizeof(Rec) * batch, hipHostMallocDefault) == hipSuccess;
  }
  // room for `need` words of partial records
  hipError_t size_partials(size_t need) {
    if (!on || need <= partials_cap) return hipSuccess;
    d_partials = DevBuf<unsigned long long>();
    const hipError_t e = hipMalloc((void **)&d_partials.p, need * sizeof(unsigned long long));
    if (e == hipSuccess) partials_cap = need;
    return e;
  }
  // event i, while timing
  hipError_t mark(int i, bool timing, hipStream_t s) { return timing ? hipEventRecord(ev[i], s) : hipSuccess; }
  // a batch of n records begins: zeros (for a summing launch that leaves out the planes a frame does not have), the first event
  hipError_t begin(uint32_t n, bool timing, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(d_recs, 0, sizeof(Rec) * n, s);
    return e != hipSuccess ? e : mark(0, timing, s);
  }
  // the summing launch: the partial records, cut as `u`, into the n records of the batch
  hipError_t sum(void (*kernel)(TailParams), unsigned planes, uint32_t n, unsigned threads, const Units &u, hipStream_t s) {
    TailParams tp{};
    tp.partials = d_partials, tp.records = reinterpret_cast<unsigned long long *>(d_recs.p), tp.units_frame = u.frame;
    for (int c = 0; c < 3; ++c) tp.units[c] = u.n[c], tp.unit_base[c] = u.base[c];
    hipLaunchKernelGGL(kernel, dim3(planes, n), dim3(threads), 0, s, tp);
    return hipGetLastError();
  }
  // the records back
  hipError_t copy_back(uint32_t n, hipStream_t s) { return hipMemcpyAsync(h_recs, d_recs, sizeof(Rec) * n, hipMemcpyDeviceToHost, s); }
  // behind the kind's launches: the last event, the records back
  hipError_t end(uint32_t n, bool timing, hipStream_t s) {
    const hipError_t e = mark(INTERVALS, timing, s);
    return e != hipSuccess ? e : copy_back(n, s);
  }
  // after the wait: the times between the events of a timed batch; then the records to those held
  hipError_t clock(uint32_t n) {
    float t[INTERVALS];
    for (int i = 0; i < INTERVALS; ++i) {
      const hipError_t e = hipEventElapsedTime(&t[i], ev[i], ev[i + 1]);
      if (e != hipSuccess) return e;
    }
    for (int i = 0; i < INTERVALS; ++i) ms[i] += t[i];
    timed += n;
    return hipSuccess;
  }
  void collect(uint32_t n) { Records<Rec>::collect(h_recs.p, n); }
  // the first two intervals' times so far and the records they covered (the noise levels' luma and chroma)
  int times(double *first, double *second, uint64_t *n) const {
    if (first) *first = ms[0];
    if (second) *second = ms[INTERVALS - 1 < 1 ? INTERVALS - 1 : 1];  // (a lane of one interval has no second: its only one)
    if (n) *n = timed;
    return G1S_OK;
  }
};

// The frame before, of a temporal meter's run: SIDES frames a job (measure's noisy and clean, the noise levels' one).  Host
// frames go round input rings of slots(batch) slots, so that the last frame of a batch is still there under the first of the
// next; planes of the frame before that are the caller's are copied into a frame the meter owns (keep) at the moment the
// meter's contract lets the caller have them back.  Where the frame before is read, and when the ring moves on, is the meter's.
template <int SIDES>
struct FrameBefore {
  bool have = false;       // is there one in this run?
  uint32_t next_slot = 0;  // of the rings
  bool callers[SIDES] = {};  // are the planes of side s the caller's (not a ring's, not d_keep's)?
  DevBuf<uint8_t> d_keep[SIDES];
  static uint32_t slots(uint32_t batch) { return batch + 1; }
  void advance(uint32_t batch) { next_slot = (next_slot + 1) % slots(batch); }
  // a new geometry: the run ends, the kept frames go (the rings are made again; where they go on is the meter's)
  void reset() {
    have = false;
    for (int s = 0; s < SIDES; ++s) callers[s] = false, d_keep[s] = DevBuf<uint8_t>();
  }
  // side s, where its planes are the caller's: room for the kept frame, ...
  hipError_t room(int s, const Layout &lay) { return callers[s] && !d_keep[s] ? hipMalloc((void **)&d_keep[s].p, lay.frame) : hipSuccess; }
  // ... the planes copied into it on the stream, device to device, and read from the copy from then on
  hipError_t keep(int s, const PlaneGeom &g, const Layout &lay, const uint8_t *plane[3], uint32_t stride[3], hipStream_t stream) {
    if (!callers[s]) return hipSuccess;
    for (int c = 0; c < g.nplanes; ++c) {
      uint8_t *dst = d_keep[s] + lay.off[c];
      const hipError_t e = hipMemcpy2DAsync(dst, lay.row[c], plane[c], stride[c], g.row_bytes(c), g.ph(c), hipMemcpyDeviceToDevice, stream);
      if (e != hipSuccess) return e;
      plane[c] = dst, stride[c] = (uint32_t)lay.row[c];
    }
    callers[s] = false;
    return hipSuccess;
  }
};

// the not-made text of a kind every meter makes: never set
constexpr const char *kAlwaysMade = nullptr;

// the meter is not of the kind the call is for
template <class Meter>
int not_made(Meter *m, const char *text) {
  m->err = text ? text : "";  // (the text alone, not sticky: err_code stays 0)
  return G1S_ERR_INVALID;
}

// A *_finish call of a kind: the checks, then what the meter does at a hand-over (settle(): what is queued goes out), then
// the lane's records.  `not_made_text`: what a meter without the kind says.
template <class Meter, class Lane, class Rec>
int finish_kind(Meter *m, Lane Meter::*lane, const char *not_made_text, Rec *out, size_t cap, size_t *n_out) {
  if (!m) return G1S_ERR_INVALID;
  if (m->err_code) return m->err_code;
  if (!(m->*lane).on) return not_made(m, not_made_text);
  (void)hipSetDevice(m->device);
  const int rc = m->settle();
  return rc ? rc : (m->*lane).hand_over(out, cap, n_out);
}

}  // namespace g1s_op
#endif  // __HIPCC__
