// The refusals of a surface converter, asked of the host-only half of csrc/frame_op.h (test infrastructure;
// tests/test_surface_cpu.py builds and runs it).  argv: bit_depth unpack(1|0) then NAME=VALUE for every field of the two
// structs that is not 0: s.width s.height s.bps s.xdec s.ydec s.nplanes s.depth s.msb s.data0..2 s.stride0..2, and f.* likewise
// (pointers are numbers: nothing is read through them).  prints: code text
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../grav1synth_amd/csrc/frame_op.h"

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  g1s_surface_t s{};
  g1s_frame_t f{};
  for (int i = 3; i < argc; ++i) {
    const char *eq = std::strchr(argv[i], '=');
    if (!eq || argv[i][1] != '.') return 2;
    const std::string name(argv[i] + 2, (size_t)(eq - argv[i] - 2));
    const unsigned long long v = std::strtoull(eq + 1, nullptr, 0);
    const bool surf = argv[i][0] == 's';
    const int k = name.empty() ? 0 : name.back() - '0';
    if (name == "width") (surf ? s.width : f.width) = (uint32_t)v;
    else if (name == "height") (surf ? s.height : f.height) = (uint32_t)v;
    else if (name == "bps") (surf ? s.bytes_per_sample : f.bytes_per_sample) = (uint8_t)v;
    else if (name == "xdec") (surf ? s.xdec : f.xdec) = (uint8_t)v;
    else if (name == "ydec") (surf ? s.ydec : f.ydec) = (uint8_t)v;
    else if (name == "nplanes") (surf ? s.nplanes : f.nplanes) = (uint8_t)v;
    else if (name == "depth" && surf) s.bit_depth = (uint8_t)v;
    else if (name == "msb" && surf) s.msb_aligned = (uint8_t)v;
    else if (name.compare(0, 4, "data") == 0 && k >= 0 && k < 3) (surf ? s.data[k] : f.data[k]) = reinterpret_cast<const void *>((uintptr_t)v);
    else if (name.compare(0, 6, "stride") == 0 && k >= 0 && k < 3) (surf ? s.stride_bytes[k] : f.stride_bytes[k]) = (size_t)v;
    else return 2;
  }
  const g1s_op::Refusal r = g1s_op::check_surface_pair(s, f, (uint32_t)std::atoi(argv[1]), std::atoi(argv[2]) != 0);
  std::printf("%d %s\n", r.code, r.text.c_str());
  return 0;
}
