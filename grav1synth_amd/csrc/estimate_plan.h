// estimate_plan.h -- how k_estimate_pk's launch is cut into row strips (estimate.hip's flush()).  Host code only, no HIP: a pure
// function of the plane, the batch and the device's numbers, so that the choice can be walked over a grid of them without a
// device (tests/estimate_plan_host.cpp, under the sanitizers).
//
// Output rows per wave strip: chosen so that the launch is a whole number of resident rounds (8 waves a SIMD: 8192 waves on
// the chip): with 64-row strips a 32-frame 4K launch was 8704 waves -- 1.06 rounds, the last 6 % of the waves alone on the chip
// for as long as the first 94 % took.
#pragma once
#include <algorithm>

namespace g1s_est {

constexpr int kPkMaxStripRows = 256;  // (the two 16-bit pixel counters of a lane hold 4 * rows each)
constexpr int kPkMinStripRows = 8;
constexpr int kPkFallbackWgsPerCu = 5;  // where the occupancy query answers below 1
// (strip_walk.hip.h's kWavesPerWg and kColsPerWave: estimate.hip asserts that they are these)
constexpr int kPlanWavesPerWg = 4, kPlanColsPerWave = 62 * 8;

struct StripPlan {
  int strip_rows;  // output rows a wave strip, kPkMinStripRows .. kPkMaxStripRows
  int row_strips;  // strips down a plane: the last one may be short, none is empty
  long rounds;     // k: the resident rounds the height was chosen for; 0 where the height was given
};

// column strips of a plane W samples wide (W >= 2; the second strip begins at W - 1 > 496)
inline int plan_col_strips(int W) { return (W - 1 + kPlanColsPerWave - 1) / kPlanColsPerWave; }

// A plane H rows high (H >= 3) in col_strips column strips, `frames` of them in the launch, on a device of `cus` compute
// units that holds wgs_per_cu workgroups of the kernel each.  forced_rows: 0, or the height to take instead (clamped into
// kPkMinStripRows .. kPkMaxStripRows).
inline StripPlan plan_strips(int H, int col_strips, int frames, int cus, int wgs_per_cu, int forced_rows) {
  StripPlan p;
  const long rows = (long)H - 2;
  if (forced_rows) {
    p.strip_rows = std::min(std::max(forced_rows, kPkMinStripRows), kPkMaxStripRows);
    p.rounds = 0;
  } else {
    // whole resident rounds: k rounds of `resident` waves, the smallest k whose strips are at most kPkMaxStripRows rows
    if (wgs_per_cu < 1) wgs_per_cu = kPkFallbackWgsPerCu;
    const long resident = (long)cus * wgs_per_cu * kPlanWavesPerWg, cols = (long)col_strips * frames;
    int strip_rows;
    long k = 1;
    for (;; ++k) {
      const long rs = std::max(1L, k * resident / cols);  // row strips a frame
      strip_rows = (int)((rows + rs - 1) / rs);
      if (strip_rows <= kPkMaxStripRows) break;
    }
    p.strip_rows = std::max(strip_rows, kPkMinStripRows);
    p.rounds = k;
  }
  p.row_strips = (int)((rows + p.strip_rows - 1) / p.strip_rows);
  return p;
}

}  // namespace g1s_est
