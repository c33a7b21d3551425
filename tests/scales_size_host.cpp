// What a scales meter can sum (rule 21 of `measure`), asked of the host-only half of csrc/frame_op.h (test infrastructure;
// tests/test_measure_s_cpu.py builds and runs it).  argv: bit_depth width height.  prints: ok, and the refusal's text
#include <cstdio>
#include <cstdlib>

#include "../grav1synth_amd/csrc/frame_op.h"

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const uint32_t bd = (uint32_t)std::strtoull(argv[1], nullptr, 10), w = (uint32_t)std::strtoull(argv[2], nullptr, 10),
                 h = (uint32_t)std::strtoull(argv[3], nullptr, 10);
  std::printf("%d\n%s\n", g1s_op::scales_size_ok(bd, w, h) ? 1 : 0, g1s_op::scales_refusal_text());
  return 0;
}
