// The host arithmetic of the separable axis passes (axis_pass.inc: k_circ_gemm, k_axis_gemm) that needs neither the device
// nor a context: plain arguments and the standard library only, so tests/axis_plan_check.cpp can run it on its own under
// the sanitizers.  Three things: the geometry of one pass, the operator-block builder and the unit-circle table (with the
// Gaussian filter's circulant column that is built from it).
//
// A pass applies a dense operator A (M x K) along one index of a row-major array; every pass is one of two views:
//     [batch][K][P]   the operator along the MIDDLE index:      Y[b][m][p] = sum_k A[m][k] X[b][k][p]
//     [batch][P][K]   the operator along the CONTIGUOUS index:  Y[b][p][m] = sum_k A[m][k] X[b][p][k]   (operands swapped)
// A (nz, ny, nx) volume's z pass is the first view with P = ny nx, its y pass the first with one z slice per batch, its x
// pass the second with every row folded into P.  The kernels address X at b sb_in + k sk + p sp_in and Y at
// b sb_out + m sk + p sp_out, a workgroup per 64 x 64 tile of (m, p) and per b.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr int AXIS_TILE = 64;   // output tile of a workgroup: 64 rows of the operator x 64 columns P

struct AxisView {
  int64_t batch;
  int K, M;          // in side, out side
  int64_t P;
  bool contiguous;   // the operator runs along the contiguous index
};

struct AxisGeom {
  int K, M;
  int64_t np;               // columns P of the product
  int64_t sk;               // element stride along the operator's index, the same in X (k) and Y (m)
  int64_t sp_in, sp_out;    // element strides along P
  int64_t sb_in, sb_out;    // element strides of one batch
  int64_t gx, gy, gz;       // the grid: tiles along P, tiles along M, batches
  bool tr;                  // the MFMA's operands are swapped: the accumulator's lane index runs along m, where Y is contiguous
};

inline AxisGeom axis_geom(const AxisView& v) {
  AxisGeom g{};
  g.K = v.K; g.M = v.M;
  g.np = v.P;
  g.sk = v.contiguous ? 1 : v.P;
  g.sp_in = v.contiguous ? v.K : 1;
  g.sp_out = v.contiguous ? v.M : 1;
  g.sb_in = (int64_t)v.K * v.P;
  g.sb_out = (int64_t)v.M * v.P;
  g.gx = (v.P + AXIS_TILE - 1) / AXIS_TILE;
  g.gy = (v.M + AXIS_TILE - 1) / AXIS_TILE;
  g.gz = v.batch;
  g.tr = v.contiguous;
  return g;
}

// The pass along `axis` of `maps` leading arrays of shape[3] = (nz, ny, nx), to out side `out` along that axis.
inline AxisGeom axis_geom(const int shape[3], int axis, int out, int64_t maps) {
  const int64_t nz = shape[0], ny = shape[1], nx = shape[2];
  if (axis == 0) return axis_geom(AxisView{maps, shape[0], out, ny * nx, false});
  if (axis == 1) return axis_geom(AxisView{maps * nz, shape[1], out, nx, false});
  return axis_geom(AxisView{1, shape[2], out, maps * nz * ny, true});
}

// Float64 cos / sin (2 pi t / n), t = 0 .. n - 1: what every operator of a pass is read from.
inline void unit_circle(int n, std::vector<double>& c, std::vector<double>& s) {
  c.resize(n);
  s.resize(n);
  for (int t = 0; t < n; ++t) {
    c[t] = std::cos(2.0 * M_PI * t / n);
    s[t] = std::sin(2.0 * M_PI * t / n);
  }
}

// Which entry of a length-n table element [i][j] of an operator reads.
enum class AxisIndex {
  Circulant,   // (i - j) mod n: C[i][j] = c[(i - j) mod n], the operator of a circular convolution
  Dft          // i j mod n:     F[i][j] = e[i j mod n], a discrete Fourier transform
};

// Appends the row-major n x ka operator block [sp p | sq q] (q only when ka = 2 n) to `mats`; returns its offset.
inline size_t append_axis_operator(std::vector<float>& mats, int n, AxisIndex rule, const std::vector<double>& p, double sp,
                                   const std::vector<double>* q, double sq) {
  const size_t off = mats.size();
  const int ka = q ? 2 * n : n;
  mats.resize(off + (size_t)n * ka);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const int t = rule == AxisIndex::Circulant ? ((i - j) % n + n) % n : (int)(((int64_t)i * j) % n);
      mats[off + (size_t)i * ka + j] = (float)(sp * p[t]);
      if (q) mats[off + (size_t)i * ka + n + j] = (float)(sq * (*q)[t]);
    }
  return off;
}

// c = ifft(w) for one axis, w the reference's weight exp(-f2 u^2) on fftshifted float32 coordinates u (float64 sums).
inline void circulant_column(int n, double f2, std::vector<double>& cr, std::vector<double>& ci) {
  std::vector<double> w(n), cs, sn;
  unit_circle(n, cs, sn);
  for (int k = 0; k < n; ++k) {
    const int idx = (k + (n + 1) / 2) % n;
    const float u = (float)(idx - n / 2) / (float)(n / 2);
    w[k] = std::exp(-f2 * (double)(u * u));
  }
  cr.assign(n, 0.0);
  ci.assign(n, 0.0);
  for (int d = 0; d < n; ++d) {
    double sr = 0, si = 0;
    for (int k = 0; k < n; ++k) {
      const int t = (int)(((int64_t)k * d) % n);
      sr += w[k] * cs[t];
      si += w[k] * sn[t];
    }
    cr[d] = sr / n;
    ci[d] = si / n;
  }
}
