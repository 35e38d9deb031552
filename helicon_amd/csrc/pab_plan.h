// The host arithmetic of a PathABatch's set-up (path_a_batch.inc) that needs neither the device nor the object: plain
// arguments and std::vector only, so tests/pab_plan_check.cpp can run it on its own under the sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// Half sets (split_A_b, solver:175-203): the rows of one candidate that stay, as indices into its row list, in order.
// pid: the rows' pixel ids.  fsc_mode 1: the ids listed in fsc_ids are the first half (ids no row has are harmless);
// 2: every other of the sorted distinct ids; 3: their first half; 4: their first and last third.  fsc_half 1 keeps the
// first half's rows, 2 the others'.
inline std::vector<size_t> pab_half_rows(const std::vector<int32_t>& pid, int fsc_mode, int fsc_half, const int32_t* fsc_ids,
                                         int n_fsc_ids) {
  std::vector<int32_t> ids(pid);
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  const size_t nn = ids.size();
  std::vector<int32_t> set1;
  if (fsc_mode == 1) { set1.assign(fsc_ids, fsc_ids + n_fsc_ids); std::sort(set1.begin(), set1.end()); }
  else if (fsc_mode == 2) { for (size_t i = 0; i < nn; i += 2) set1.push_back(ids[i]); }
  else if (fsc_mode == 3) { set1.assign(ids.begin(), ids.begin() + nn / 2); }
  else { set1.assign(ids.begin(), ids.begin() + nn / 3); set1.insert(set1.end(), ids.begin() + nn * 2 / 3, ids.end()); }
  std::vector<size_t> keep;
  for (size_t r = 0; r < pid.size(); ++r)
    if (std::binary_search(set1.begin(), set1.end(), pid[r]) == (fsc_half == 1)) keep.push_back(r);
  return keep;
}

// The slice-major order of one candidate's rows: a stable counting sort of the reference's row order by slice.
// zz: the slice of every row; srow[0 .. mz]: first row of every slice (srow[mz] = the number of rows); order[k]: the
// reference-order row that is k-th in slice-major order.  False (nothing to be used): a row's slice is outside [0, mz).
inline bool pab_slice_order(const std::vector<short>& zz, int mz, int* srow, std::vector<int>& order) {
  std::fill(srow, srow + mz + 1, 0);
  for (size_t r = 0; r < zz.size(); ++r) {
    if (zz[r] < 0 || zz[r] >= mz) return false;
    ++srow[zz[r] + 1];
  }
  for (int z = 0; z < mz; ++z) srow[z + 1] += srow[z];
  order.assign(zz.size(), 0);
  std::vector<int> cur(srow, srow + mz);
  for (size_t r = 0; r < zz.size(); ++r) order[(size_t)cur[zz[r]]++] = (int)r;   // counting sort: stable
  return true;
}

// Where the second pass of the device row enumeration writes one candidate's rows of the operations [lo, lo + chunk).
// cz: [n_used][mz + 1] rays per (operation, slice), the last column the rays in two slices (none on the sliced path);
// srow: the candidate's [mz + 1] slice starts (read on the sliced path only).  bref[o - lo]: rows before operation o in
// the reference's order, all of the earlier operations (entries of operations past n_used are left alone).
// bint[(o - lo) * (mz + 1) + z]: in the device order, per slice, the earlier operations' rows of that slice (after the
// slice's first row) minus this operation's rows of the earlier slices — the rank the kernel adds counts all of the
// operation's earlier rays.  General path: device order = reference order.
inline void pab_row_offsets(const int* cz, int n_used, int mz, bool sliced, const int* srow, int lo, int chunk, long long* bref,
                            long long* bint) {
  const int mz1 = mz + 1;
  long long before_ref = 0;
  std::vector<long long> before_z((size_t)mz1, 0);
  for (int o = 0; o < n_used; ++o) {
    long long tot = 0, zoff = 0;
    for (int z = 0; z < mz1; ++z) tot += cz[(size_t)o * mz1 + z];
    if (o >= lo && o < lo + chunk) {
      bref[o - lo] = before_ref;
      for (int z = 0; z < mz1; ++z) {
        long long v = before_ref;
        if (sliced) v = (z < mz ? srow[z] : 0) + before_z[(size_t)z] - zoff;
        bint[(size_t)(o - lo) * mz1 + z] = v;
        zoff += cz[(size_t)o * mz1 + z];
      }
    }
    for (int z = 0; z < mz1; ++z) before_z[(size_t)z] += cz[(size_t)o * mz1 + z];
    before_ref += tot;
  }
}

// The banded form's cut of the disc's d2 rows into bands whose two planes, halo row and table rows fit the budget.
// rank: the voxel ranks of the box, of which plane 0 is read (rank = index inside the plane, negative outside the disc).
// budget: the LDS a band may take; force (HH_PAB_FORCE_BANDED) lowers it so that there are at least three bands.
struct PabBandCut {
  std::vector<int> vrow;     // [d2 + 1] first in-plane index of every row
  std::vector<int> band_y;   // [bands + 1] first row of every band, then d2
  size_t budget = 0;         // bytes a band may take
  size_t band_lds = 0;       // bytes of the largest band
  bool row_too_large = false;   // one row of the disc is over the budget: no cut
  // base rows [ya, yb): rows [ya, yb + 1) staged
  size_t band_bytes(int ya, int yb, int d2) const {
    const int ye = std::min(yb + 1, d2);
    return (size_t)2 * (vrow[(size_t)ye] - vrow[(size_t)ya]) * sizeof(double) + (size_t)(ye - ya) * d2 * sizeof(unsigned);
  }
};
inline PabBandCut pab_band_cut(const std::vector<int>& rank, int d2, bool force, size_t budget = (size_t)150 << 10) {
  PabBandCut cut;
  cut.vrow.assign((size_t)d2 + 1, 0);
  for (int yy = 0; yy < d2; ++yy) {
    int cnt = 0;
    for (int xx = 0; xx < d2; ++xx) cnt += rank[(size_t)yy * d2 + xx] >= 0;
    cut.vrow[(size_t)yy + 1] = cut.vrow[(size_t)yy] + cnt;
  }
  cut.budget = budget;
  if (force) {   // at least three bands, whatever the box
    size_t row_max = 0;
    for (int yy = 0; yy < d2; ++yy) row_max = std::max(row_max, cut.band_bytes(yy, yy + 1, d2));
    cut.budget = std::min(cut.budget, std::max(row_max, cut.band_bytes(0, d2, d2) / 3));
  }
  cut.band_y.assign(1, 0);
  while (cut.band_y.back() < d2) {
    const int ya = cut.band_y.back();
    if (cut.band_bytes(ya, ya + 1, d2) > cut.budget) { cut.row_too_large = true; return cut; }
    int yb = ya + 1;
    while (yb < d2 && cut.band_bytes(ya, yb + 1, d2) <= cut.budget) ++yb;
    cut.band_y.push_back(yb);
  }
  // the kernels lay a band out by its own size (planes, then table rows), so the launch needs the largest band's bytes
  for (size_t t = 0; t + 1 < cut.band_y.size(); ++t) cut.band_lds = std::max(cut.band_lds, cut.band_bytes(cut.band_y[t], cut.band_y[t + 1], d2));
  return cut;
}
