// What `diff` can address, asked of the host-only half of csrc/frame_op.h (test infrastructure; tests/test_limits_cpu.py
// builds and runs it).  argv: width height bytes_per_sample xdec ydec nplanes stride0 stride1 stride2
// prints: size_ok extent0 extent1 extent2 reach     (reach: 0 either chain, 1 the stream chain, 2 refused for its extent, 3 for its stride)
#include <cstdio>
#include <cstdlib>

#include "../grav1synth_amd/csrc/frame_op.h"

int main(int argc, char **argv) {
  if (argc != 10) return 2;
  g1s_frame_t f{};
  f.width = (uint32_t)std::strtoull(argv[1], nullptr, 10);
  f.height = (uint32_t)std::strtoull(argv[2], nullptr, 10);
  f.bytes_per_sample = (uint8_t)std::atoi(argv[3]);
  f.xdec = (uint8_t)std::atoi(argv[4]);
  f.ydec = (uint8_t)std::atoi(argv[5]);
  f.nplanes = (uint8_t)std::atoi(argv[6]);
  for (int c = 0; c < 3; ++c) f.stride_bytes[c] = (size_t)std::strtoull(argv[7 + c], nullptr, 10);
  std::printf("%d", g1s_op::diff_size_ok(f.width, f.height) ? 1 : 0);
  for (int c = 0; c < 3; ++c) std::printf(" %llu", c < f.nplanes ? (unsigned long long)g1s_op::diff_plane_extent(f, c) : 0ull);
  std::printf(" %d\n", (int)g1s_op::diff_frame_reach(f, f.nplanes));
  return 0;
}
