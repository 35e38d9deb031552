// Stand-alone check of helicon_amd/csrc/pab_plan.h on the host: every function against a brute-force restatement on small
// random inputs (fixed seed).  Built with -fsanitize=address,undefined and run as a child process by
// tests/test_pab_plan_host.py.  No GPU, no HIP.
#include "pab_plan.h"

#include <cstdio>
#include <random>
#include <set>

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (g_failed < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

static std::mt19937 g_rng(20260412u);
static int draw(int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g_rng); }   // inclusive

// ---- row offsets: bint / bref + the rank of a ray among its operation's rays = where the row goes ------------------------
struct Row { int op, rank, z; };
static void check_row_offsets(bool sliced) {
  const int mz = draw(1, 5), mz1 = mz + 1, n_used = draw(1, 12), chunk = draw(1, 5);
  std::vector<int> cz((size_t)n_used * mz1, 0);
  for (int o = 0; o < n_used; ++o)
    for (int z = 0; z < mz1; ++z)
      cz[(size_t)o * mz1 + z] = z == mz && sliced ? 0 : draw(0, 3);   // (a ray in two slices turns slicing off)
  // the rows in the reference's (operation, ray) order.  Sliced path (tilt = psi = 0): the rays of an operation run along
  // the axis, so their slices do not decrease — what lets one rank over all of an operation's rays serve every slice.
  // General path: a ray's slice is whatever the geometry says (shuffled).
  std::vector<Row> rows;
  for (int o = 0; o < n_used; ++o) {
    std::vector<int> zs;
    for (int z = 0; z < mz1; ++z) zs.insert(zs.end(), (size_t)cz[(size_t)o * mz1 + z], z);
    if (!sliced) std::shuffle(zs.begin(), zs.end(), g_rng);
    for (size_t i = 0; i < zs.size(); ++i) rows.push_back({o, (int)i, zs[i]});
  }
  std::vector<size_t> by_slice(rows.size());
  for (size_t i = 0; i < rows.size(); ++i) by_slice[i] = i;
  std::stable_sort(by_slice.begin(), by_slice.end(), [&](size_t a, size_t b) { return rows[a].z < rows[b].z; });
  std::vector<size_t> pos_sorted(rows.size());
  for (size_t k = 0; k < by_slice.size(); ++k) pos_sorted[by_slice[k]] = k;
  std::vector<int> srow((size_t)mz1, 0);
  for (const Row& r : rows)
    if (r.z < mz) ++srow[(size_t)r.z + 1];
  for (int z = 0; z < mz; ++z) srow[(size_t)z + 1] += srow[(size_t)z];
  size_t seen = 0;
  for (int lo = 0; lo < n_used; lo += chunk) {   // windows that begin after operation 0, the last one ends past n_used
    std::vector<long long> bref((size_t)chunk, -1), bint((size_t)chunk * mz1, 0);
    pab_row_offsets(cz.data(), n_used, mz, sliced, sliced ? srow.data() : nullptr, lo, chunk, bref.data(), bint.data());
    for (size_t i = 0; i < rows.size(); ++i) {
      const Row& r = rows[i];
      if (r.op < lo || r.op >= lo + chunk) continue;
      ++seen;
      CHECK(bref[(size_t)(r.op - lo)] + r.rank == (long long)i);
      const long long at = bint[(size_t)(r.op - lo) * mz1 + r.z] + r.rank;
      CHECK(at == (long long)(sliced ? pos_sorted[i] : i));
    }
    for (int o = lo; o < lo + chunk; ++o) {
      if (o >= n_used) {   // past the operations in use: left as the caller filled them
        CHECK(bref[(size_t)(o - lo)] == -1);
        for (int z = 0; z < mz1; ++z) CHECK(bint[(size_t)(o - lo) * mz1 + z] == 0);
      } else if (!sliced) {
        for (int z = 0; z < mz1; ++z) CHECK(bint[(size_t)(o - lo) * mz1 + z] == bref[(size_t)(o - lo)]);
      }
    }
  }
  CHECK(seen == rows.size());
}

// ---- slice order = std::stable_sort by slice --------------------------------------------------------------------------------
static void check_slice_order() {
  const int mz = draw(1, 6), rows = draw(0, 40);
  std::vector<short> zz((size_t)rows);
  for (short& z : zz) z = (short)draw(0, mz - 1);
  std::vector<int> srow((size_t)mz + 1, 7), order{1, 2, 3};
  CHECK(pab_slice_order(zz, mz, srow.data(), order));
  std::vector<int> want((size_t)rows);
  for (int r = 0; r < rows; ++r) want[(size_t)r] = r;
  std::stable_sort(want.begin(), want.end(), [&](int a, int b) { return zz[(size_t)a] < zz[(size_t)b]; });
  CHECK(order == want);
  CHECK(srow[0] == 0 && srow[(size_t)mz] == rows);
  for (int z = 0; z < mz; ++z) CHECK(srow[(size_t)z + 1] - srow[(size_t)z] == (int)std::count(zz.begin(), zz.end(), (short)z));
  if (rows > 0) {   // a row without a slice is reported, not indexed (the sanitizers watch srow and order)
    std::vector<short> bad(zz);
    bad[(size_t)draw(0, rows - 1)] = (short)(draw(0, 1) ? -1 - draw(0, 3) : mz + draw(0, 3));
    CHECK(!pab_slice_order(bad, mz, srow.data(), order));
  }
}

// ---- half sets ------------------------------------------------------------------------------------------------------------------
static void check_half_sets(int mode) {
  const int rows = draw(1, 60), span = draw(1, 40);
  std::vector<int32_t> pid((size_t)rows);
  for (int32_t& v : pid) v = 3 * draw(0, span);
  const std::set<int32_t> distinct(pid.begin(), pid.end());
  const std::vector<int32_t> ids(distinct.begin(), distinct.end());
  const size_t nn = ids.size();
  std::vector<int32_t> listed;
  if (mode == 1) {   // the caller's own split; ids that no row has (not multiples of 3, or beyond the span) are harmless
    for (int k = draw(0, 30); k > 0; --k) listed.push_back(draw(-5, 3 * span + 5));
  }
  auto in_first = [&](int32_t id) {
    if (mode == 1) return std::find(listed.begin(), listed.end(), id) != listed.end();
    const size_t at = (size_t)(std::find(ids.begin(), ids.end(), id) - ids.begin());
    if (mode == 2) return at % 2 == 0;
    if (mode == 3) return at < nn / 2;
    return at < nn / 3 || at >= nn * 2 / 3;
  };
  const std::vector<size_t> h1 = pab_half_rows(pid, mode, 1, listed.data(), (int)listed.size());
  const std::vector<size_t> h2 = pab_half_rows(pid, mode, 2, listed.data(), (int)listed.size());
  std::vector<size_t> want1, want2;
  for (size_t r = 0; r < pid.size(); ++r) (in_first(pid[r]) ? want1 : want2).push_back(r);
  CHECK(h1 == want1);   // (the kept rows in their order)
  CHECK(h2 == want2);
  CHECK(h1.size() + h2.size() == pid.size());   // disjoint (want1 / want2 are) and together every row
  if (mode != 1) {      // the split is one of ids: a pixel's rows all go the same way, and the halves' sizes are split_A_b's
    std::set<int32_t> ids1;
    for (size_t r : h1) ids1.insert(pid[r]);
    for (size_t r : h2) CHECK(!ids1.count(pid[r]));
    const size_t n1 = mode == 2 ? (nn + 1) / 2 : mode == 3 ? nn / 2 : nn / 3 + (nn - nn * 2 / 3);
    CHECK(ids1.size() == n1);
  }
}

// ---- band cut -------------------------------------------------------------------------------------------------------------------
static void check_band_cut(bool force) {
  const int d2 = draw(3, 24);
  const double rmax = draw(1, d2) / 2.0, rmin = draw(0, 1) ? 0.0 : draw(0, d2 / 2) / 2.0;
  std::vector<int> rank((size_t)d2 * d2, -1), per_row((size_t)d2, 0);
  int n = 0;
  for (int y = 0; y < d2; ++y)
    for (int x = 0; x < d2; ++x) {
      const double r2 = (double)(y - d2 / 2) * (y - d2 / 2) + (double)(x - d2 / 2) * (x - d2 / 2);
      if (r2 <= rmax * rmax && r2 >= rmin * rmin) { rank[(size_t)y * d2 + x] = n++; ++per_row[(size_t)y]; }
    }
  // bytes of a band of base rows [ya, yb): two planes of doubles and the table rows of the rows [ya, yb + 1) it stages
  auto bytes = [&](int ya, int yb) {
    size_t b = 0;
    for (int y = ya; y < yb + 1 && y < d2; ++y) b += (size_t)16 * per_row[(size_t)y] + (size_t)4 * d2;
    return b;
  };
  size_t row_max = 0;
  for (int y = 0; y < d2; ++y) row_max = std::max(row_max, bytes(y, y + 1));
  const size_t given = force && draw(0, 1) ? (size_t)150 << 10 : (size_t)draw((int)row_max / 2, (int)bytes(0, d2) + 8);
  const size_t budget = force ? std::min(given, std::max(row_max, bytes(0, d2) / 3)) : given;
  const PabBandCut cut = pab_band_cut(rank, d2, force, given);
  CHECK(cut.budget == budget);
  CHECK((int)cut.vrow.size() == d2 + 1 && cut.vrow[0] == 0 && cut.vrow[(size_t)d2] == n);
  for (int y = 0; y < d2; ++y) CHECK(cut.vrow[(size_t)y + 1] - cut.vrow[(size_t)y] == per_row[(size_t)y]);
  CHECK(!cut.band_y.empty() && cut.band_y[0] == 0);
  size_t largest = 0;
  for (size_t t = 0; t + 1 < cut.band_y.size(); ++t) {
    const int ya = cut.band_y[t], yb = cut.band_y[t + 1];
    CHECK(ya < yb && yb <= d2);                          // strictly increasing
    CHECK(bytes(ya, yb) <= budget);                      // every band fits
    if (yb < d2) CHECK(bytes(ya, yb + 1) > budget);      // greedy: it could not take its next row
    CHECK(cut.band_bytes(ya, yb, d2) == bytes(ya, yb));
    largest = std::max(largest, bytes(ya, yb));
  }
  if (cut.row_too_large) {   // the cut stopped at a row that is over the budget on its own
    const int ya = cut.band_y.back();
    CHECK(ya < d2 && bytes(ya, ya + 1) > budget);
    CHECK(!force || given < row_max);
  } else {
    CHECK(cut.band_y.back() == d2);
    CHECK(cut.band_lds == largest);
    // forced: a budget of a third of the whole gives three bands or more (the bands' bytes add up to the whole at least);
    // it is more than a third only where one row with its halo row is
    if (force && row_max <= bytes(0, d2) / 3) CHECK(cut.band_y.size() - 1 >= 3);
  }
}

int main() {
  for (int i = 0; i < 300; ++i) check_row_offsets(i % 2 == 0);
  for (int i = 0; i < 300; ++i) check_slice_order();
  for (int i = 0; i < 400; ++i) check_half_sets(1 + i % 4);
  for (int i = 0; i < 400; ++i) check_band_cut(i % 2 == 0);
  {   // the discs of the tests' boxes, forced: three bands at least
    for (int d2 = 8; d2 <= 64; d2 += 4) {
      std::vector<int> rank((size_t)d2 * d2, -1);
      int n = 0;
      const double rmax = d2 / 2 - 1;
      for (int y = 0; y < d2; ++y)
        for (int x = 0; x < d2; ++x)
          if ((double)(y - d2 / 2) * (y - d2 / 2) + (double)(x - d2 / 2) * (x - d2 / 2) <= rmax * rmax) rank[(size_t)y * d2 + x] = n++;
      const PabBandCut cut = pab_band_cut(rank, d2, true);
      CHECK(!cut.row_too_large && cut.band_y.size() - 1 >= 3 && cut.band_y.back() == d2);
    }
  }
  if (g_failed) {
    std::printf("pab_plan_check: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("pab_plan_check: ok\n");
  return 0;
}
