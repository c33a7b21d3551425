// estimate_plan_host.cpp -- the packed estimator's strip plan (grav1synth_amd/csrc/estimate_plan.h) built with a host compiler
// alone, as a stand-alone program: the plan walked over a grid of plane heights, column strips, batches, compute units and
// occupancies, with what must hold at every point; then the heights of three production launches, one line each, for the
// test to compare with its own restatement.  tests/test_estimate_plan_cpu.py compiles it under the address and
// undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../grav1synth_amd/csrc/estimate_plan.h"

using namespace g1s_est;

static long points = 0;

static void require(bool ok, const char *what, int H, int cs, int B, int cus, int occ, int forced, const StripPlan &p) {
  if (ok) return;
  std::fprintf(stderr, "estimate_plan_host: %s at H %d col_strips %d batch %d cus %d wgs_per_cu %d forced %d: strip_rows %d row_strips %d k %ld\n", what,
               H, cs, B, cus, occ, forced, p.strip_rows, p.row_strips, p.rounds);
  std::exit(1);
}

// the height k rounds give before it is raised to the minimum: the definition, written apart from the loop under test
static long rows_at(long k, long rows, long resident, long cols) {
  long rs = k * resident / cols;
  if (rs < 1) rs = 1;
  return (rows + rs - 1) / rs;
}

static void covered(int H, int cs, int B, int cus, int occ, int forced, const StripPlan &p) {
  const long rows = (long)H - 2;
  require(p.strip_rows >= 8 && p.strip_rows <= 256, "strip_rows outside 8 .. 256", H, cs, B, cus, occ, forced, p);
  require((long)p.row_strips * p.strip_rows >= rows, "a row is not covered", H, cs, B, cus, occ, forced, p);
  require((long)(p.row_strips - 1) * p.strip_rows < rows, "an empty strip", H, cs, B, cus, occ, forced, p);
  require(p.row_strips >= 1, "no strip", H, cs, B, cus, occ, forced, p);
}

int main() {
  static_assert(kPkMinStripRows == 8 && kPkMaxStripRows == 256 && kPkFallbackWgsPerCu == 5, "the constants the kernel's comments state");
  std::vector<int> heights;
  for (int H = 3; H <= 600; ++H) heights.push_back(H);
  for (int H : {1080, 2160, 4320, 65535, 65536}) heights.push_back(H);
  const int widths[] = {16, 504, 3840, 7680, 65536}, strips[] = {1, 2, 8, 16, 133};
  const int batches[] = {1, 2, 3, 31, 32}, cu_counts[] = {1, 8, 256, 304};
  for (int wi = 0; wi < 5; ++wi) {
    const int cs = plan_col_strips(widths[wi]);
    if (cs != strips[wi]) {
      std::fprintf(stderr, "estimate_plan_host: width %d has %d column strips, not %d\n", widths[wi], cs, strips[wi]);
      return 1;
    }
    for (int H : heights)
      for (int B : batches)
        for (int cus : cu_counts)
          for (int occ = 0; occ <= 8; ++occ) {
            // (that the loop ends: this call returns; and it ends no later than the k whose strips are surely short enough)
            const StripPlan p = plan_strips(H, cs, B, cus, occ, 0);
            ++points;
            covered(H, cs, B, cus, occ, 0, p);
            const long rows = (long)H - 2, resident = (long)cus * (occ < 1 ? 5 : occ) * 4, cols = (long)cs * B;
            const long need = (rows + 255) / 256;                      // row strips of at most 256 rows
            const long k_enough = (need * cols + resident - 1) / resident;  // k resident / cols >= need
            require(p.rounds >= 1 && p.rounds <= k_enough, "k beyond the first that is surely enough", H, cs, B, cus, occ, 0, p);
            require(rows_at(p.rounds, rows, resident, cols) <= 256, "k does not satisfy the bound", H, cs, B, cus, occ, 0, p);
            const long raw = rows_at(p.rounds, rows, resident, cols);
            require(p.strip_rows == (raw < 8 ? 8 : raw), "strip_rows is not k's height raised to 8", H, cs, B, cus, occ, 0, p);
            // the smallest: no k below it satisfies the bound (all of them up to 64, then every 97th, and always k - 1)
            for (long k = 1; k < p.rounds; k += (k < 64 || k + 97 >= p.rounds) ? 1 : 97)
              require(rows_at(k, rows, resident, cols) > 256, "a smaller k satisfies the bound", H, cs, B, cus, occ, 0, p);
          }
    // a given height: clamped into 8 .. 256, the strips follow from it, whatever the device's numbers are
    for (int H : heights)
      for (int forced : {-3, 1, 7, 8, 9, 10, 11, 17, 85, 86, 255, 256, 257, 100000}) {
        const StripPlan p = plan_strips(H, cs, 5, 256, 8, forced), q = plan_strips(H, cs, 32, 1, 0, forced);
        ++points;
        covered(H, cs, 5, 256, 8, forced, p);
        const int want = forced < 8 ? 8 : forced > 256 ? 256 : forced;
        require(p.strip_rows == want && p.rounds == 0, "a given height was not taken", H, cs, 5, 256, 8, forced, p);
        require(q.strip_rows == p.strip_rows && q.row_strips == p.row_strips, "a given height depends on the device", H, cs, 32, 1, 0, forced, q);
      }
  }
  // the production launches: batch 32 on 256 compute units, occupancy 1 .. 8
  const int prod[3][2] = {{1920, 1080}, {3840, 2160}, {7680, 4320}};
  for (const auto &wh : prod) {
    std::printf("heights %d %d", wh[0], wh[1]);
    for (int occ = 1; occ <= 8; ++occ) {
      const StripPlan p = plan_strips(wh[1], plan_col_strips(wh[0]), 32, 256, occ, 0);
      std::printf(" %d:%d:%ld", p.strip_rows, p.row_strips, p.rounds);
    }
    std::printf("\n");
  }
  std::printf("points %ld\nok\n", points);
  return 0;
}
