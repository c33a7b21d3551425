// A batch's schedule, asked of csrc/schedule.h under the host compiler (test infrastructure; tests/test_schedule_cpu.py builds
// and runs it).  argv: one_stream no_defer side2 w_aside f_serial d2h_sync timed device_latest wide batch slot nplanes last_back
// prints: table finder accum rest latest d2h back_now after host_waits
//         (streams by name; host_waits: none, copy_stream, done_event)
#include <cstdio>
#include <cstdlib>

#include "../grav1synth_amd/csrc/schedule.h"

int main(int argc, char **argv) {
  if (argc != 14) return 2;
  int v[13];
  for (int i = 0; i < 13; ++i) v[i] = std::atoi(argv[1 + i]);
  g1s_sched::Switches sw{};
  sw.wide = true;  // (G1S_K3 unset; which chain serves THIS batch is `wide` below)
  sw.one_stream = v[0], sw.no_defer = v[1], sw.side2 = v[2], sw.w_aside = v[3], sw.f_serial = v[4], sw.d2h_sync = v[5];
  g1s_sched::Batch b{};
  b.timed = v[6], b.device_latest = v[7], b.wide = v[8], b.batch = (uint32_t)v[9], b.slot = v[10], b.nplanes = v[11], b.last_back = v[12];
  const g1s_sched::Schedule s = g1s_sched::schedule(sw, b);
  static_assert((int)g1s_sched::Role::compute == 0 && (int)g1s_sched::Role::latest2 == 6 && (int)g1s_sched::HostWait::done_event == 2, "the names below are in the enums' order");
  static const char *const role[] = {"compute", "flat", "flat2", "copy", "upload", "latest", "latest2"};
  static const char *const wait[] = {"none", "copy_stream", "done_event"};
  std::printf("%s %s %s %s %s %s %d %d %s\n", role[(int)s.table], role[(int)s.finder], role[(int)s.accum], role[(int)s.rest], role[(int)s.latest],
              role[(int)s.d2h], s.back_now ? 1 : 0, s.after, wait[(int)s.host_waits]);
  return 0;
}
