// Stand-alone check of helicon_amd/csrc/axis_plan.h on the host: the geometry of the separable axis passes against the
// row-major arrays it has to address and against the seven hand-written set-ups it replaced (written out once below), the
// operator-block builder against a brute-force loop, the unit circle against its expression.  Built with
// -fsanitize=address,undefined and run as a child process by tests/test_axis_plan_host.py.  No GPU, no HIP.
#include "axis_plan.h"

#include <algorithm>
#include <cstdio>
#include <random>

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (g_failed < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

static std::mt19937 g_rng(20261020u);
static int draw(int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(g_rng); }   // inclusive
static double drawf(double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(g_rng); }

// ---- geometry: the offsets a grid produces against the row-major arrays ---------------------------------------------------
// Every in-bounds (block.z, i, p) the grid covers, i < rows along the operator's index (the output's m comes from the grid's
// tiles, the input's k from the kernel's loop over all of K): its offset must be `want(b, i, p)`, the row-major index of that
// element, and the offsets together every index of the array exactly once.
template <class Want>
static void check_side(const AxisGeom& g, int64_t rows, int64_t sp, int64_t sb, int64_t total, Want want) {
  std::vector<unsigned char> seen((size_t)total, 0);
  int64_t hits = 0, wrong = 0, twice = 0;
  const int64_t cols = std::min<int64_t>(g.np, g.gx * AXIS_TILE);
  for (int64_t b = 0; b < g.gz; ++b)
    for (int64_t i = 0; i < rows; ++i)
      for (int64_t p = 0; p < cols; ++p) {
        const int64_t off = b * sb + i * g.sk + p * sp;
        if (off < 0 || off >= total || off != want(b, i, p)) { ++wrong; continue; }
        twice += seen[(size_t)off];
        seen[(size_t)off] = 1;
        ++hits;
      }
  CHECK(wrong == 0);
  CHECK(twice == 0);
  CHECK(hits == total);   // with no offset twice: onto
}

static void check_grid(const AxisGeom& g, int64_t batch) {   // the ceilings, and no smaller
  CHECK(g.gx >= 1 && (g.gx - 1) * AXIS_TILE < g.np && g.np <= g.gx * AXIS_TILE);
  CHECK(g.gy >= 1 && (g.gy - 1) * AXIS_TILE < g.M && g.M <= g.gy * AXIS_TILE);
  CHECK(g.gz == batch);
}

// `maps` arrays of shape (nz, ny, nx), the pass along `axis` to out side M
static void check_shape(const int shape[3], int axis, int M, int maps) {
  const AxisGeom g = axis_geom(shape, axis, M, maps);
  int out[3] = {shape[0], shape[1], shape[2]};
  out[axis] = M;
  const int K = shape[axis];
  CHECK(g.K == K && g.M == M && g.tr == (axis == 2));
  // the row-major index in an array [maps][d0][d1][d2] of (b, i, p) as the pass counts them
  const auto index_in = [&](const int d[3]) {
    return [=](int64_t b, int64_t i, int64_t p) -> int64_t {
      const int64_t d0 = d[0], d1 = d[1], d2 = d[2];
      if (axis == 0) return (b * d0 + i) * d1 * d2 + p;        // b = map, p = y nx + x
      if (axis == 1) return (b * d1 + i) * d2 + p;             // b = map nz + z, p = x
      return p * d2 + i;                                       // p = (map nz + z) ny + y
    };
  };
  const int64_t others = (int64_t)maps * shape[0] * shape[1] * shape[2] / K;
  check_side(g, K, g.sp_in, g.sb_in, others * K, index_in(shape));
  check_side(g, std::min<int64_t>(M, g.gy * AXIS_TILE), g.sp_out, g.sb_out, others * M, index_in(out));
  check_grid(g, axis == 0 ? maps : axis == 1 ? (int64_t)maps * shape[0] : 1);
}

static void check_view(const AxisView& v) {
  const AxisGeom g = axis_geom(v);
  CHECK(g.K == v.K && g.M == v.M && g.tr == v.contiguous && g.np == v.P);
  const auto index_in = [&](int64_t side) {
    return [=](int64_t b, int64_t i, int64_t p) -> int64_t { return v.contiguous ? (b * v.P + p) * side + i : (b * side + i) * v.P + p; };
  };
  check_side(g, v.K, g.sp_in, g.sb_in, v.batch * v.K * v.P, index_in(v.K));
  check_side(g, std::min<int64_t>(v.M, g.gy * AXIS_TILE), g.sp_out, g.sb_out, v.batch * v.M * v.P, index_in(v.M));
  check_grid(g, v.batch);
}

static void check_geometry_all() {
  const int edge[] = {1, 2, 31, 32, 33, 63, 64, 65, 70};
  for (int axis = 0; axis < 3; ++axis)
    for (int K : edge)
      for (int M : {1, 63, 64, 65, K}) {   // the side along the axis crosses the tile, in and out; the other two stay small
        int shape[3] = {draw(1, 5), draw(1, 5), draw(1, 5)};
        shape[axis] = K;
        check_shape(shape, axis, M, draw(1, 3));
      }
  for (int axis = 0; axis < 3; ++axis)   // P crosses the tile: 63 / 64 / 65 columns
    for (int p : {63, 64, 65}) {
      int shape[3] = {3, 3, 3};
      shape[(axis + 1) % 3] = p;
      check_shape(shape, axis, draw(1, 6), draw(1, 3));
    }
  for (int rep = 0; rep < 40; ++rep) {
    const int shape[3] = {draw(1, 70), draw(1, 70), draw(1, 70)};
    for (int axis = 0; axis < 3; ++axis) {
      int M = draw(1, 70);
      if (M == shape[axis]) M = M % 70 + 1;   // in side != out side
      check_shape(shape, axis, M, draw(1, 3));
    }
  }
  for (int rep = 0; rep < 40; ++rep)
    check_view(AxisView{draw(1, 4), draw(1, 70), draw(1, 70), draw(1, 150), rep % 2 == 1});
}

// ---- restatement: the seven set-ups as they were written at their launch sites ----------------------------------------------
struct Old {
  int64_t np, sk, sp_in, sp_out, sb_in, sb_out;
  int64_t gx, gy, gz;
  bool tr;
};
static int64_t tiles(int64_t n) { return (n + 64 - 1) / 64; }

static Old old_map_filter(int nz, int ny, int nx, int axis) {   // hh_low_high_pass_filter_3d
  Old g{};
  const int n = axis == 0 ? nz : axis == 1 ? ny : nx;
  const int64_t mt = tiles(n);
  if (axis == 0) {
    g.np = (int64_t)ny * nx; g.sk = g.np; g.sp_in = 1; g.sb_in = 0;
    g.gx = tiles(g.np); g.gy = mt; g.gz = 1;
  } else if (axis == 1) {
    g.np = nx; g.sk = nx; g.sp_in = 1; g.sb_in = (int64_t)ny * nx;
    g.gx = tiles(g.np); g.gy = mt; g.gz = nz;
  } else {
    g.np = (int64_t)nz * ny; g.sk = 1; g.sp_in = nx; g.sb_in = 0;
    g.gx = tiles(g.np); g.gy = mt; g.gz = 1;
  }
  g.sp_out = g.sp_in; g.sb_out = g.sb_in;
  g.tr = axis == 2;
  return g;
}
static Old old_fc_first(bool cube, int64_t maps, int nz, int ny, int nx) {   // fc_passes, the real input
  Old g{};
  const int n1 = cube ? nz : ny;
  const int64_t per_map = (int64_t)(cube ? nz * ny : ny) * nx;
  g.np = cube ? (int64_t)ny * nx : nx; g.sk = g.np; g.sp_in = g.sp_out = 1; g.sb_in = g.sb_out = per_map;
  g.gx = tiles(g.np); g.gy = tiles(n1); g.gz = maps;
  return g;
}
static Old old_fc_second(int64_t maps, int nz, int ny, int nx) {   // fc_passes, the complex planes along y
  Old g{};
  g.np = nx; g.sk = nx; g.sp_in = g.sp_out = 1; g.sb_in = g.sb_out = (int64_t)ny * nx;
  g.gx = tiles(nx); g.gy = tiles(ny); g.gz = maps * nz;
  return g;
}
static Old old_tf_inverse_z(int n, int ncol) {   // tf_create
  Old g{};
  const int64_t per_spec = (int64_t)n * n * ncol;
  g.np = (int64_t)n * ncol; g.sk = g.np; g.sp_in = g.sp_out = 1; g.sb_in = g.sb_out = per_spec;
  g.gx = tiles(g.np); g.gy = tiles(n); g.gz = 2;
  return g;
}
static Old old_tf_inverse_y(int n, int ncol) {   // tf_create
  Old g{};
  g.np = ncol; g.sk = ncol; g.sp_in = g.sp_out = 1; g.sb_in = g.sb_out = (int64_t)n * ncol;
  g.gx = tiles(ncol); g.gy = tiles(n); g.gz = 2 * n;
  return g;
}
static Old old_filtered_y(int batch, int ony, int onx) {   // filt_y_passes
  Old g{};
  g.np = onx; g.sk = onx; g.sp_in = g.sp_out = 1; g.sb_in = g.sb_out = (int64_t)ony * onx;
  g.gx = tiles(onx); g.gy = tiles(ony); g.gz = batch;
  return g;
}
static Old old_resample(const int in_dims[3], const int out_dims[3], int ax) {   // hh_separable_transform_3d; out_dims: after the pass
  Old g{};
  const int64_t ny_in = in_dims[1], nx_in = in_dims[2], ny_out = out_dims[1], nx_out = out_dims[2];
  const int64_t mt = tiles(out_dims[ax]);
  if (ax == 0) {
    g.np = ny_in * nx_in; g.sk = g.np; g.sp_in = g.sp_out = 1; g.sb_in = g.sb_out = 0;
    g.gx = tiles(g.np); g.gy = mt; g.gz = 1;
  } else if (ax == 1) {
    g.np = nx_in; g.sk = nx_in; g.sp_in = g.sp_out = 1; g.sb_in = ny_in * nx_in; g.sb_out = ny_out * nx_out;
    g.gx = tiles(g.np); g.gy = mt; g.gz = in_dims[0];
  } else {
    g.np = (int64_t)in_dims[0] * ny_in; g.sk = 1; g.sp_in = nx_in; g.sp_out = nx_out; g.sb_in = g.sb_out = 0;
    g.gx = tiles(g.np); g.gy = mt; g.gz = 1;
  }
  g.tr = ax == 2;
  return g;
}

// The same offset b sb + i sk + p sp for every (b, i, p) of the same grid: equal strides, and equal batch offsets for every
// block.z the grid has (a set-up that passed sb = 0 with grid.z = 1 and one that passes the view's sb agree: b is 0).
static void same_offsets(const Old& o, const AxisGeom& g) {
  CHECK(o.np == g.np && o.sk == g.sk && o.sp_in == g.sp_in && o.sp_out == g.sp_out);
  CHECK(o.gx == g.gx && o.gy == g.gy && o.gz == g.gz && o.tr == g.tr);
  for (int64_t b = 0; b < o.gz; ++b) CHECK(b * o.sb_in == b * g.sb_in && b * o.sb_out == b * g.sb_out);
}

static void check_restatement_all() {
  for (int rep = 0; rep < 300; ++rep) {
    const int nz = draw(1, 70), ny = draw(1, 70), nx = draw(1, 70), n = 2 * draw(4, 35), ncol = n / 2 + 1;
    const int side[3] = {nz, ny, nx}, cube[3] = {n, n, n};
    const int64_t nb = draw(1, 5), maps = 2 * nb;
    for (int axis = 0; axis < 3; ++axis) same_offsets(old_map_filter(nz, ny, nx, axis), axis_geom(side, axis, side[axis], 1));
    // the views as fc_passes, tf_create and filt_y_passes write them
    same_offsets(old_fc_first(true, maps, n, n, n), axis_geom(AxisView{maps, n, n, (int64_t)n * n, false}));
    same_offsets(old_fc_first(false, maps, 0, ny, nx), axis_geom(AxisView{maps, ny, ny, nx, false}));
    same_offsets(old_fc_second(maps, n, n, n), axis_geom(AxisView{maps * n, n, n, n, false}));
    same_offsets(old_tf_inverse_z(n, ncol), axis_geom(AxisView{2, n, n, (int64_t)n * ncol, false}));
    same_offsets(old_tf_inverse_y(n, ncol), axis_geom(AxisView{2 * (int64_t)n, n, n, ncol, false}));
    same_offsets(old_filtered_y((int)nb, ny, nx), axis_geom(AxisView{nb, ny, ny, nx, false}));
    // ... and the same passes named by shape and axis
    same_offsets(old_fc_first(true, maps, n, n, n), axis_geom(cube, 0, n, maps));
    same_offsets(old_fc_second(maps, n, n, n), axis_geom(cube, 1, n, maps));
    int in_dims[3] = {nz, ny, nx};
    for (int ax = 0; ax < 3; ++ax) {   // z, y, x in turn, each on the shape the pass before it left
      int out_dims[3] = {in_dims[0], in_dims[1], in_dims[2]};
      out_dims[ax] = draw(1, 70);
      same_offsets(old_resample(in_dims, out_dims, ax), axis_geom(in_dims, ax, out_dims[ax], 1));
      for (int a = 0; a < 3; ++a) in_dims[a] = out_dims[a];
    }
  }
}

// ---- the operator blocks and the unit circle ------------------------------------------------------------------------------
static void check_operator(int n, AxisIndex rule, bool with_q) {
  std::vector<double> p(n), q(n);
  for (int t = 0; t < n; ++t) { p[t] = drawf(-2, 2); q[t] = drawf(-2, 2); }
  const double sp = drawf(-2, 2), sq = drawf(-2, 2);
  std::vector<float> mats = {1.f, 2.f, 3.f};   // what is there stays
  const size_t off = append_axis_operator(mats, n, rule, p, sp, with_q ? &q : nullptr, sq);
  const int ka = with_q ? 2 * n : n;
  CHECK(off == 3 && mats.size() == 3 + (size_t)n * ka && mats[0] == 1.f && mats[1] == 2.f && mats[2] == 3.f);
  if (mats.size() != 3 + (size_t)n * ka) return;
  int wrong = 0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      int t = 0;
      if (rule == AxisIndex::Circulant) {
        t = i - j;
        while (t < 0) t += n;
      } else {
        for (int r = 0; r < j; ++r) t = (t + i) % n;   // i j mod n, by addition
      }
      wrong += mats[off + (size_t)i * ka + j] != (float)(sp * p[t]);
      if (with_q) wrong += mats[off + (size_t)i * ka + n + j] != (float)(sq * q[t]);
    }
  CHECK(wrong == 0);
}

static void check_unit_circle(int n) {
  std::vector<double> c(3, 7.0), s;
  unit_circle(n, c, s);
  CHECK((int)c.size() == n && (int)s.size() == n);
  if ((int)c.size() != n || (int)s.size() != n) return;
  for (int t = 0; t < n; ++t) CHECK(c[t] == std::cos(2.0 * M_PI * t / n) && s[t] == std::sin(2.0 * M_PI * t / n));
}

// c = ifft(w): the transform of c gives the weights back, and an even side's c is real
static void check_circulant_column(int n, double f2) {
  std::vector<double> cr, ci;
  circulant_column(n, f2, cr, ci);
  CHECK((int)cr.size() == n && (int)ci.size() == n);
  if ((int)cr.size() != n || (int)ci.size() != n) return;
  for (int k = 0; k < n; ++k) {
    double wr = 0, wi = 0;
    for (int d = 0; d < n; ++d) {   // (cr + i ci) e^{-2 pi i k d / n}
      const double a = 2.0 * M_PI * (double)(((int64_t)k * d) % n) / n;
      wr += cr[d] * std::cos(a) + ci[d] * std::sin(a);
      wi += ci[d] * std::cos(a) - cr[d] * std::sin(a);
    }
    const int idx = (k + (n + 1) / 2) % n;
    const float u = (float)(idx - n / 2) / (float)(n / 2);
    CHECK(std::fabs(wr - std::exp(-f2 * (double)(u * u))) < 1e-12 && std::fabs(wi) < 1e-12);
  }
  if (n % 2 == 0)
    for (int d = 0; d < n; ++d) CHECK(std::fabs(ci[d]) < 1e-13);
}

int main() {
  check_geometry_all();
  check_restatement_all();
  for (int n : {1, 2, 3, 4, 7, 8, 15, 16, 33, 64, 65})
    for (AxisIndex rule : {AxisIndex::Circulant, AxisIndex::Dft})
      for (bool with_q : {false, true}) check_operator(n, rule, with_q);
  for (int n : {1, 2, 3, 8, 45, 63, 64, 126}) check_unit_circle(n);
  for (int n : {2, 3, 8, 9, 28, 33, 35}) check_circulant_column(n, drawf(0.5, 20.0));
  if (g_failed) std::printf("axis_plan_check: %d check(s) failed\n", g_failed);
  else std::printf("axis_plan_check: ok\n");
  return g_failed ? 1 : 0;
}
