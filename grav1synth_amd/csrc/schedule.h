// schedule.h -- where the parts of a batch run: the one place that decides it.  Host-only and free of HIP, so that
// tests/test_schedule_cpu.py can pin every row under the host compiler (tests/schedule_host.cpp); engine.hip's plan_batch
// turns the roles into streams, and everything that queues work for the batch follows that plan.
//
// The streams (StreamSet in engine.hip), M = compute, F / F2 = flat / flat2, U = upload, C = copy, L / L2 = latest / latest2.
// With inline = one_stream || timed and window = device_latest && batch >= kLatestWindowMinBatch:
//
//   queued copies of pinned frames   U, always; when table != U the h2d_order event hands over from U to table
//   table   (frame table, k_zero)    M if inline, else U; then table_done[slot] is recorded and M and finder wait for it
//   finder  (the finder chain,       M if inline, else F2 for an odd slot under side2, else F; when finder != M, mask_done[slot]
//            select, unit lists)     is recorded and M waits for it in front of the accumulation
//   after                            the slot whose kernels_done the finder chain waits for: last_back if window, finder != M
//                                    and last_back >= 0, else none (-1)
//   accum   (the luma launch)        M
//   rest    (the chroma launch and   C if !inline, the frames have chroma planes and (wide ? w_aside : !f_serial), else M;
//            what follows, the tail) moving to C goes through kernels_done[slot]
//   latest  (k4_latest; only with    rest if timed || window, else L2 for an odd slot, L for an even one (one_stream alone
//            device_latest)          does not move it); latest != rest waits for kernels_done[slot], the copy for latest_done[slot]
//   d2h     (records / blobs)        C, behind kernels_done[slot]
//   back_now                         one_stream || no_defer || timed || window: the back half is queued with its front half,
//                                    otherwise behind the front half of the batch after
//   host_waits                       d2h_sync: for the copy stream; else timed: for the batch's `done` event; else for nothing
//
// Why each row is what it is, and what was measured: the comments at StreamSet and above g1s_diff::submit in engine.hip.
#pragma once
#include <cstdint>

namespace g1s_sched {

// The process-wide switches: read once, when the library first asks for one (switches() in engine.hip).  Every one selects an
// arrangement that gives the same records as the default, and is here because a test, bench.py or a measurement tool sets it
// (DESIGN.md section 8).
struct Switches {
  bool wide;        // G1S_K3 is not "stream": the wide chain, the stream chain where it does not serve (tests, bench.py)
  bool w_off;       // G1S_W_OFF: the wide chain serves nothing while its buffers and zero fills stay (tests)
  bool one_stream;  // G1S_ONE_STREAM: every kernel of a batch on the main stream, no deferred back half (tests, profiling tools)
  bool no_defer;    // G1S_NO_DEFER: a batch's back half is queued with its own front half (tests)
  bool side2;       // G1S_SIDE2=1: a second side stream, the finder chains of the odd slots on it (tests; no gain: profiles/r03b)
  bool w_aside;     // G1S_W_ASIDE: the wide chain's chroma launch and what follows on the copy stream, round 3's placement (tests)
  bool f_serial;    // G1S_F_SERIAL: the stream chain's chroma launch stays on the main stream (tests)
  bool d2h_sync;    // G1S_D2H_SYNC: launch_back waits for the batch's copy (profiling tools, with G1S_ONE_STREAM)
  int w_rev;        // G1S_W_REV: bit 0 the luma launch, bit 1 the chroma launch of the wide chain walk the frames last to first (tests)
  int k1_literal;   // G1S_K1_LITERAL=1|2: the finder evaluates every block literally, a lane / a wave a block (tests)
};

constexpr uint32_t kLatestWindowMinBatch = 64;  // frames a launch from which k4_latest gets a window of its own (g1s_diff::submit)

enum class Role : uint8_t { compute, flat, flat2, copy, upload, latest, latest2 };
enum class HostWait : uint8_t { none, copy_stream, done_event };

struct Batch {
  bool timed;          // per-kernel or chain timing is on (g1s_diff_set_timing)
  bool device_latest;  // the per-frame half of the fold runs on the device
  bool wide;           // the wide chain serves the batch (wide_ok)
  uint32_t batch;      // frames of a full launch of this generator (not this batch's count)
  int slot, nplanes;
  int last_back;       // slot of the batch whose back half was queued last, or -1
};
struct Schedule {
  Role table, finder, accum, rest, latest, d2h;
  bool back_now;
  int after;
  HostWait host_waits;
};

inline Schedule schedule(const Switches &sw, const Batch &b) {
  const bool in_line = sw.one_stream || b.timed, window = b.device_latest && b.batch >= kLatestWindowMinBatch, odd = (b.slot & 1) != 0;
  Schedule s;
  s.table = in_line ? Role::compute : Role::upload;
  s.finder = in_line ? Role::compute : (odd && sw.side2) ? Role::flat2 : Role::flat;
  s.after = (window && !in_line && b.last_back >= 0) ? b.last_back : -1;
  s.accum = Role::compute;
  s.rest = (!in_line && b.nplanes == 3 && (b.wide ? sw.w_aside : !sw.f_serial)) ? Role::copy : Role::compute;
  // (without the device half nothing runs on `latest`: it names the stream of the tail)
  s.latest = (!b.device_latest || b.timed || window) ? s.rest : odd ? Role::latest2 : Role::latest;
  s.d2h = Role::copy;
  s.back_now = sw.one_stream || sw.no_defer || b.timed || window;
  s.host_waits = sw.d2h_sync ? HostWait::copy_stream : b.timed ? HostWait::done_event : HostWait::none;
  return s;
}

}  // namespace g1s_sched
