// fourier_correlation.inc — Fourier shell correlation of two cubic maps and Fourier ring correlation of two images
// (lib/analysis.py:116-356: calc_fsc, calc_fsc_per_shell, calc_frc_2d), for a batch of pairs in one call.
//
// For every pair and every shell s the three sums
//     num[s] = sum w Re(F1 conj F2),   den1[s] = sum w |F1|^2,   den2[s] = sum w |F2|^2      over the bins of shell s
// are returned (the ratio and the `denominator > 0` rule stay on the host).  The transforms are per-axis matrix products
// on the exact-f32 MFMA (k_circ_gemm, axis_pass.inc): a DFT along one axis is the product with [cos | -sin] blocks built in
// float64 on the host (axis_plan.h) and rounded to float32, so any side works (odd and prime included) and there is no FFT plan.
//     3-D, F(kz, ky, kx):  z pass on the real input (Re = C x, Im = -S x), y pass on the complex planes
//                          (Re = [C | S][re; im], Im = [-S | C][re; im]), both through k_circ_gemm;
//     2-D, F(ky, kx):      y pass on the real input;
//     last (x) pass:       k_fc_xpass, only the columns that are needed (n / 2 + 1 in 3-D, all nx in 2-D), for both members
//                          of the pair in one workgroup (fc_pair_product), which forms the three products from its
//                          accumulator registers and adds them to the shell sums (fc_add_products, fc_flush).  The spectrum of the last pass is never stored.
// Shell of a 3-D bin: round(sqrt(m)), m = kz^2 + ky^2 + kx^2 in integers, decided without a square root's rounding
// (shell = k iff k (k - 1) < m <= k (k + 1); sqrt(m) is never k + 1/2), clipped to n / 2.  A 2-D bin reads the host's table
// (ties are real there and follow NumPy's float64 expression).  Weight: 1, or — the full spectrum seen from its half —
// 2 off the planes kx = 0 and kx = n / 2 (even n).
// The sums are bit-identical from run to run and do not depend on the batch: every product is formed in float64, scaled
// by a power of two chosen per pair and per sum from max |map| alone (sum w |F|^2 <= (voxels max|x|)^2), rounded to a 64-bit
// integer and added with integer atomics (LDS first, then global), whose result does not depend on the order.  The total
// stays below 2^62; one unit is 2^-61 of that bound or finer.  k_fc_finish converts back to float64.

namespace {

constexpr int FC_T = 64;          // tile of a workgroup: 64 rows of the planes x 64 output columns
constexpr int FC_K = 32;          // slice of the x axis staged through LDS per step
constexpr int FC_MAX_SHELLS = 513;    // LDS shell sums of one workgroup: 3-D n / 2 + 1 <= 257, 2-D min(ny, nx) / 2 + 1 <= 513

struct FcXPass {
  const float* re;         // [2 B][rows][nx] real plane after the earlier passes: maps 0 .. B-1 are the first members
  const float* im;         // the imaginary plane
  const float* cs;         // [nx][ncol] cos(2 pi x k / nx)
  const float* sn;         // [nx][ncol] sin(2 pi x k / nx)
  const int32_t* shell;    // 2-D: [rows][ncol] host table; 3-D: null
  const double* scale;     // [B][3] power-of-two scales of num, den1, den2
  long long* acc;          // [B][nshell][3] fixed-point sums
  int batch, rows, nx, ncol, n, nshell, weighted;
};

// max |x| of every map, as the bit pattern of a non-negative float (ordered like the value; NaN sorts above infinity)
__global__ __launch_bounds__(256) void k_fc_absmax(const float* __restrict__ v, int64_t per_map, unsigned* __restrict__ amax) {
  const float* s = v + (int64_t)blockIdx.y * per_map;
  unsigned m = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_map; i += (int64_t)gridDim.x * 256)
    m = max(m, __float_as_uint(s[i]) & 0x7fffffffu);
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_down((int)m, off, 64));
  if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(amax + blockIdx.y, m);
}

// scale[b][q] = 2^(61 - ilogb(bound)), bound = 2 (voxels)^2 max|a| max|b| >= sum w |products| of the pair; 0 when the
// bound is 0 (every product is 0 then), NaN when a map holds a NaN or an infinity (the sums come back as NaN)
__device__ __forceinline__ void fc_pair_scales(unsigned amax1, unsigned amax2, double voxels, double* scale) {
  const double a1 = (double)__uint_as_float(amax1), a2 = (double)__uint_as_float(amax2);
  const double pr[3] = {a1 * a2, a1 * a1, a2 * a2};
  for (int q = 0; q < 3; ++q) {
    const double bound = 2.0 * voxels * voxels * pr[q];
    double s;
    if (!(bound == bound) || bound > 1.7e308) s = __longlong_as_double(0x7ff8000000000000ll);
    else if (bound == 0.0) s = 0.0;
    else s = ldexp(1.0, 61 - ilogb(bound));
    scale[q] = s;
  }
}

__global__ void k_fc_scales(const unsigned* __restrict__ amax, int batch, double voxels, double* __restrict__ scale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  fc_pair_scales(amax[b], amax[batch + b], voxels, scale + b * 3);
}

__device__ __forceinline__ int fc_shell_3d(int kz, int ky, int kx, int n) {
  const int h = n / 2;
  const int fz = kz <= h ? kz : n - kz, fy = ky <= h ? ky : n - ky, fx = kx <= h ? kx : n - kx;
  const int m = fz * fz + fy * fy + fx * fx;
  int k = (int)sqrtf((float)m);
  while (k * (k + 1) < m) ++k;
  while (k > 0 && k * (k - 1) >= m) --k;
  return k < h ? k : h;
}

// The x pass of one pair's 64 x 64 tile on the shared tile (mfma_tile.inc): the four source planes src = {re1, im1, re2, im2}
// ([rows][nx]) times the tables cs / sn ([nx][ncol]), into four 32 x 32 accumulators per wavefront: Re and Im of both
// members.  A wavefront whose sub-tile lies wholly outside is not `active` and does no product.  Holds the x pass's LDS.
__device__ __forceinline__ void fc_pair_product(const float* const (&src)[4], const float* cs, const float* sn, int rows, int nx, int ncol,
                                                int row0, int col0, bool active, const Tile64& t, f32x16& re1, f32x16& im1, f32x16& re2,
                                                f32x16& im2) {
  __shared__ float as[4][FC_T][FC_K + 1];   // re1, im1, re2, im2
  __shared__ float os[2][FC_K][FC_T + 1];   // cos, sin
  const float* const tab[2] = {cs, sn};
  const int r = t.r, h = t.h, wm = t.wm, wp = t.wp;
  for (int k0 = 0; k0 < nx; k0 += FC_K) {
#pragma unroll
    for (int q = 0; q < 4; ++q) stage_rows(as[q], src[q], nx, row0, rows, k0, nx, t.tid);
    stage_cols(os, tab, ncol, k0, nx, col0, ncol, t.tid);
    __syncthreads();
    if (active) {
      // The slice's products go into accumulators of their own and the slices are then added: a chain of at most 2 FC_K terms
      // plus nx / FC_K slice sums.  One chain over all nx terms loses sqrt(nx) ulp of the LARGEST partial sum at a bin whose
      // terms share a sign: 6.5 ulp at the DC bin of a 126^3 map with an offset (DESIGN.md, "True-FSC side census").
      f32x16 sre1 = {0}, sim1 = {0}, sre2 = {0}, sim2 = {0};
#pragma unroll
      for (int kk = 0; kk < FC_K; kk += 2) {
        const float c = os[0][kk + h][wp + r], s = os[1][kk + h][wp + r];
        const float a1 = as[0][wm + r][kk + h], b1 = as[1][wm + r][kk + h];
        const float a2 = as[2][wm + r][kk + h], b2 = as[3][wm + r][kk + h];
        // (a + i b)(c - i s) = (a c + b s) + i (b c - a s)
        sre1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, c, sre1, 0, 0, 0);
        sre1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, s, sre1, 0, 0, 0);
        sim1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, c, sim1, 0, 0, 0);
        sim1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, -s, sim1, 0, 0, 0);
        sre2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, c, sre2, 0, 0, 0);
        sre2 = __builtin_amdgcn_mfma_f32_32x32x2f32(b2, s, sre2, 0, 0, 0);
        sim2 = __builtin_amdgcn_mfma_f32_32x32x2f32(b2, c, sim2, 0, 0, 0);
        sim2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, -s, sim2, 0, 0, 0);
      }
      re1 += sre1; im1 += sim1; re2 += sre2; im2 += sim2;
    }
    __syncthreads();
  }
}

// The three products of one bin, F1 = x1 + i y1 and F2 = x2 + i y2 with weight w, into a shell's three LDS slots: formed in
// float64, scaled by the pair's powers of two (scale[3]: num, den1, den2), rounded to a 64-bit integer, added with integer
// atomics.  The one place the fixed-point rule is written.
__device__ __forceinline__ void fc_add_products(unsigned long long* slot, double w, double x1, double y1, double x2, double y2,
                                                const double (&scale)[3]) {
  const long long qn = __double2ll_rn(w * (x1 * x2 + y1 * y2) * scale[0]);
  const long long q1 = __double2ll_rn(w * (x1 * x1 + y1 * y1) * scale[1]);
  const long long q2 = __double2ll_rn(w * (x2 * x2 + y2 * y2) * scale[2]);
  if (qn != 0) atomicAdd(slot + 0, (unsigned long long)qn);
  if (q1 != 0) atomicAdd(slot + 1, (unsigned long long)q1);
  if (q2 != 0) atomicAdd(slot + 2, (unsigned long long)q2);
}

// a workgroup's n LDS sums into the global ones
__device__ __forceinline__ void fc_flush(const unsigned long long* sh, int n, long long* acc, int tid) {
  unsigned long long* const G = reinterpret_cast<unsigned long long*>(acc);
  for (int e = tid; e < n; e += TILE_THREADS) {
    const unsigned long long v = sh[e];
    if (v != 0ull) atomicAdd(G + e, v);
  }
}

// One workgroup: 64 rows x 64 columns of F1 and of F2, then the products of the tile into the shell sums.
__global__ __launch_bounds__(256) void k_fc_xpass(FcXPass g) {
  __shared__ unsigned long long sh[FC_MAX_SHELLS * 3];
  const Tile64 t = tile64();
  const int row0 = blockIdx.x * FC_T, col0 = blockIdx.y * FC_T, b = blockIdx.z;
  const int64_t plane = (int64_t)g.rows * g.nx;
  const float* const src[4] = {g.re + (int64_t)b * plane, g.im + (int64_t)b * plane, g.re + (int64_t)(g.batch + b) * plane,
                               g.im + (int64_t)(g.batch + b) * plane};
  for (int e = t.tid; e < g.nshell * 3; e += 256) sh[e] = 0ull;
  const bool active = col0 + t.wp < g.ncol && row0 + t.wm < g.rows;   // wavefront-uniform
  f32x16 re1 = {0}, im1 = {0}, re2 = {0}, im2 = {0};
  fc_pair_product(src, g.cs, g.sn, g.rows, g.nx, g.ncol, row0, col0, active, t, re1, im1, re2, im2);
  const double scale[3] = {g.scale[b * 3 + 0], g.scale[b * 3 + 1], g.scale[b * 3 + 2]};
  if (active) {
    const int col = col0 + t.wp + t.r;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = row0 + t.wm + acc_row(i, t.h);
      if (row >= g.rows || col >= g.ncol) continue;
      int s;
      double w = 1.0;
      if (g.shell) {
        s = g.shell[(int64_t)row * g.ncol + col];
        s = s < 0 ? 0 : (s >= g.nshell ? g.nshell - 1 : s);
      } else {
        s = fc_shell_3d(row / g.n, row % g.n, col, g.n);
        if (g.weighted && col != 0 && 2 * col != g.n) w = 2.0;
      }
      fc_add_products(&sh[s * 3], w, re1[i], im1[i], re2[i], im2[i], scale);
    }
  }
  __syncthreads();
  fc_flush(sh, g.nshell * 3, g.acc + (int64_t)b * g.nshell * 3, t.tid);
}

// sums = acc / scale; `sets` curve sets of nshell x 3 sums share a pair's three scales
__global__ __launch_bounds__(256) void k_fc_finish(const long long* __restrict__ acc, const double* __restrict__ scale, int nshell, int sets,
                                                   int64_t total, double* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / ((int64_t)sets * nshell * 3);
  const double s = scale[b * 3 + i % 3];
  sums[i] = s == 0.0 ? 0.0 : (double)acc[i] / s;   // a NaN scale (a map that is not finite) gives NaN
}

// the x pass's tables: [n][ncol]
size_t fc_xtable(std::vector<float>& mats, int n, int ncol, const std::vector<double>& p) {
  const size_t off = mats.size();
  mats.resize(off + (size_t)n * ncol);
  for (int x = 0; x < n; ++x)
    for (int k = 0; k < ncol; ++k) mats[off + (size_t)x * ncol + k] = (float)p[(int)(((int64_t)x * k) % n)];
  return off;
}

constexpr int64_t FC_SCRATCH_BYTES = (int64_t)8 << 30;   // device planes of one chunk of the batch

// Device scratch of the forward passes and the sums, grow-only, plus a caller's operators / shell table and the two events
// that time a chunk.
struct FcBuffers {
  DevBuf<float> in, p1, p2, mats;   // p1 / p2: [re | im] plane pairs
  DevBuf<int32_t> shell;
  DevBuf<unsigned> amax;            // [pairs][2]: its size says how many pairs the scratch holds
  DevBuf<double> scale, sums;
  DevBuf<long long> acc;
  DevEvents<2> ev;
  int64_t shape_per_map = 0;        // the shape the scratch was sized for
  int shape_nshell = 0;
  void release() {                  // the scratch only: mats and shell are the caller's
    in.reset(); p1.reset(); p2.reset(); amax.reset(); scale.reset(); sums.reset(); acc.reset();
  }
  // Room for `pairs` pairs of maps of per_map voxels: 2 input maps per pair (`with_in`; else the caller's maps are read in
  // place), 4 planes per pair in p1 and (cubes) p2, and at least two curve sets of nshell x 3 sums (the two curves of a
  // one-pair context; a one-pair fc_run carries the second set unused, a few KB).  Only `pairs` may grow between calls:
  // per_map, nshell and cube are those of the holder's one plan.
  int reserve(int64_t pairs, int64_t per_map, int nshell, bool cube, bool with_in) {
    HH_HIP(nullptr, ev.create());
    const int64_t cap = (int64_t)amax.size() / 2;
    if (cap > 0 && (per_map != shape_per_map || nshell != shape_nshell)) return fail(nullptr, HH_ERR_STATE, "FcBuffers::reserve: another shape than the holder's");
    if (pairs <= cap && (!with_in || in)) return HH_OK;
    pairs = std::max(pairs, cap);
    release();   // all of the old scratch goes before any of the new is asked for
    const size_t maps = (size_t)pairs * per_map;
    const size_t n_sums = (size_t)std::max<int64_t>(pairs, 2) * nshell * 3;
    int rc = with_in ? ensure(nullptr, in, 2 * maps) : HH_OK;
    if (!rc) rc = ensure(nullptr, p1, 4 * maps);
    if (!rc && cube) rc = ensure(nullptr, p2, 4 * maps);
    if (!rc) rc = ensure(nullptr, scale, (size_t)pairs * 3);
    if (!rc) rc = ensure(nullptr, acc, n_sums);
    if (!rc) rc = ensure(nullptr, sums, n_sums);
    if (!rc) rc = ensure(nullptr, amax, 2 * (size_t)pairs);   // last: a scratch that counts as holding pairs is whole
    if (rc) {
      release();
      return rc;
    }
    shape_per_map = per_map; shape_nshell = nshell;
    return HH_OK;
  }
};

// The operators of one shape, built in float64 on the host: first pass on the real input, (3-D) second pass on the complex
// planes, the x pass's tables.  nz == 0: images [ny][nx]; else cubes of side nz = ny = nx.
struct FcPlan {
  bool cube = false;
  int nz = 0, ny = 0, nx = 0, ncol = 0, rows = 0, n1 = 0;
  int64_t per_map = 0;
  size_t o_c = 0, o_ms = 0, o_re = 0, o_im = 0, o_xc = 0, o_xs = 0;
  std::vector<float> mats;
};

void fc_plan(FcPlan& p, int nz, int ny, int nx) {
  p.cube = nz > 0;
  p.nz = nz; p.ny = ny; p.nx = nx;
  p.ncol = p.cube ? nx / 2 + 1 : nx;
  p.rows = p.cube ? nz * ny : ny;
  p.per_map = (int64_t)p.rows * nx;
  p.n1 = p.cube ? nz : ny;
  std::vector<double> c, s;
  unit_circle(p.n1, c, s);
  p.o_c = append_axis_operator(p.mats, p.n1, AxisIndex::Dft, c, 1.0, nullptr, 0.0);
  p.o_ms = append_axis_operator(p.mats, p.n1, AxisIndex::Dft, s, -1.0, nullptr, 0.0);
  if (p.cube) {
    unit_circle(ny, c, s);
    p.o_re = append_axis_operator(p.mats, ny, AxisIndex::Dft, c, 1.0, &s, 1.0);
    p.o_im = append_axis_operator(p.mats, ny, AxisIndex::Dft, s, -1.0, &c, 1.0);
  }
  unit_circle(nx, c, s);
  p.o_xc = fc_xtable(p.mats, nx, p.ncol, c);
  p.o_xs = fc_xtable(p.mats, nx, p.ncol, s);
}

// The passes before the last one on device-resident input: `in` holds 2 nb real maps (the first members, then the second
// members), d.p1 / d.p2 are [re | im] plane pairs of 4 nb maps each (p2: cubes only), d.mats the plan's operators on the device.
// Also max |x| of every map and the pairs' scales.  The planes the x pass reads come back in xre / xim.
void fc_passes(const FcPlan& p, const float* in, const FcBuffers& d, int64_t nb, const float** xre, const float** xim) {
  float *const p1 = d.p1, *const p2 = d.p2;
  const float* const mats = d.mats;
  unsigned* const amax = d.amax;
  double* const scale = d.scale;
  const int64_t maps = 2 * nb, per_map = p.per_map;
  const int nx = p.nx, ny = p.ny, nz = p.nz, n1 = p.n1;
  float* const re1 = p1;
  float* const im1 = p1 + maps * per_map;
  hipLaunchKernelGGL(k_fc_absmax, dim3((unsigned)std::min<int64_t>((per_map + 255) / 256, 256), (unsigned)maps), dim3(256), 0, nullptr,
                     in, per_map, amax);
  hipLaunchKernelGGL(k_fc_scales, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, nullptr, amax, (int)nb, (double)per_map, scale);
  // first pass: the real input along z (cubes: P = ny nx, one map per grid.z) or along y (images: P = nx)
  const AxisGeom first = axis_geom(AxisView{maps, n1, n1, p.cube ? (int64_t)ny * nx : nx, false});
  for (int part = 0; part < 2; ++part)
    launch_circ_pass(first, mats + (part == 0 ? p.o_c : p.o_ms), n1, in, nullptr, part == 0 ? re1 : im1, nullptr);
  *xre = re1; *xim = im1;
  if (p.cube) {   // second pass along y: one z slice of one map per grid.z, K = 2 ny over the [re; im] planes
    float* const re2 = p2;
    float* const im2 = p2 + maps * per_map;
    const AxisGeom second = axis_geom(AxisView{maps * nz, ny, ny, nx, false});
    for (int part = 0; part < 2; ++part)
      launch_circ_pass(second, mats + (part == 0 ? p.o_re : p.o_im), 2 * ny, re1, im1, part == 0 ? re2 : im2, nullptr);
    *xre = re2; *xim = im2;
  }
}

// All passes of nb pairs on device-resident input, down to the float64 sums [nb][nshell][3] in d.sums (d.acc: zeroed here)
void fc_device(const FcPlan& p, const float* in, const FcBuffers& d, int64_t nb, int nshell, bool weighted) {
  (void)hipMemsetAsync(d.amax, 0, (size_t)(2 * nb) * sizeof(unsigned), nullptr);
  (void)hipMemsetAsync(d.acc, 0, (size_t)nb * nshell * 3 * sizeof(long long), nullptr);
  const float *xre = nullptr, *xim = nullptr;
  fc_passes(p, in, d, nb, &xre, &xim);
  FcXPass x{};
  x.re = xre; x.im = xim;
  x.cs = d.mats + p.o_xc; x.sn = d.mats + p.o_xs;
  x.shell = p.cube ? nullptr : d.shell;
  x.scale = d.scale; x.acc = d.acc;
  x.batch = (int)nb; x.rows = p.rows; x.nx = p.nx; x.ncol = p.ncol; x.n = p.nx; x.nshell = nshell; x.weighted = weighted ? 1 : 0;
  hipLaunchKernelGGL(k_fc_xpass, dim3((unsigned)((p.rows + FC_T - 1) / FC_T), (unsigned)((p.ncol + FC_T - 1) / FC_T), (unsigned)nb), dim3(256), 0,
                     nullptr, x);
  const int64_t total = nb * nshell * 3;
  hipLaunchKernelGGL(k_fc_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, d.acc, d.scale, nshell, 1, total, d.sums);
}

// chunk of a batch of pairs: input + one or two plane pairs within the scratch cap, and the y pass's grid.z = 2 chunk nz <= 65535
// (both caps pinned by tests/test_launch_cuts_host.py, crossed by tests/test_gpu_launch_cuts.py)
int64_t fc_chunk(const FcPlan& p, int64_t batch) {
  const int64_t bytes_per_pair = (int64_t)(p.cube ? 10 : 6) * p.per_map * (int64_t)sizeof(float);
  int64_t chunk = std::max<int64_t>(1, FC_SCRATCH_BYTES / bytes_per_pair);
  chunk = std::min<int64_t>(chunk, p.cube ? 65535 / (2 * p.nz) : 32767);
  return std::min<int64_t>(chunk, batch);
}

// nz == 0: images [ny][nx] with the host's shell table; else cubes of side nz = ny = nx
int fc_run(const char* name, int device, const float* a, const float* b, int64_t batch, int nz, int ny, int nx, const int32_t* shell,
           int nshell, bool weighted, double* sums, double* kernel_ms) {
  if (int rc = use_device(name, device)) return rc;
  FcPlan p;
  fc_plan(p, nz, ny, nx);
  const bool cube = p.cube;
  const int64_t per_map = p.per_map;
  const int64_t chunk = fc_chunk(p, batch);
  FcBuffers d;
  const size_t map_bytes = (size_t)per_map * sizeof(float);
  if (int rc = d.reserve(chunk, per_map, nshell, cube, true)) return rc;
  if (int rc = ensure(nullptr, d.mats, p.mats.size())) return rc;
  HH_HIP(nullptr, hipMemcpy(d.mats, p.mats.data(), p.mats.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!cube) {
    if (int rc = ensure(nullptr, d.shell, (size_t)per_map)) return rc;
    HH_HIP(nullptr, hipMemcpy(d.shell, shell, (size_t)per_map * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  double ms_total = 0.0;
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = std::min(chunk, batch - b0);
    HH_HIP(nullptr, hipMemcpy(d.in, a + b0 * per_map, (size_t)nb * map_bytes, hipMemcpyHostToDevice));
    HH_HIP(nullptr, hipMemcpy(d.in + nb * per_map, b + b0 * per_map, (size_t)nb * map_bytes, hipMemcpyHostToDevice));
    HH_HIP(nullptr, hipEventRecord(d.ev[0], nullptr));
    fc_device(p, d.in, d, nb, nshell, weighted);
    HH_HIP(nullptr, hipGetLastError());
    HH_HIP(nullptr, hipEventRecord(d.ev[1], nullptr));
    HH_HIP(nullptr, hipMemcpy(sums + b0 * nshell * 3, d.sums, (size_t)nb * nshell * 3 * sizeof(double), hipMemcpyDeviceToHost));
    float ms = 0.f;
    HH_HIP(nullptr, hipEventElapsedTime(&ms, d.ev[0], d.ev[1]));
    ms_total += ms;
  }
  if (kernel_ms) *kernel_ms = ms_total;
  return HH_OK;
}

}  // namespace

extern "C" int hh_fsc_3d(int device, const float* maps1, const float* maps2, int32_t batch, int32_t n, int full_spectrum, double* sums,
                         double* kernel_ms) try {
  if (!maps1 || !maps2 || !sums) return fail(nullptr, HH_ERR_ARG, "hh_fsc_3d: NULL argument");
  if (batch < 1) return fail(nullptr, HH_ERR_ARG, "hh_fsc_3d: batch must be >= 1");
  if (n < 8 || n > 512) return fail(nullptr, HH_ERR_ARG, "hh_fsc_3d: the side of the cubes must lie in [8, 512]");
  return fc_run("hh_fsc_3d", device, maps1, maps2, batch, n, n, n, nullptr, n / 2 + 1, full_spectrum != 0, sums, kernel_ms);
} HH_CATCH_CTX(nullptr, "hh_fsc_3d")

extern "C" int hh_frc_2d(int device, const float* imgs1, const float* imgs2, int32_t batch, int32_t ny, int32_t nx, const int32_t* shell,
                         int32_t n_shells, double* sums, double* kernel_ms) try {
  if (!imgs1 || !imgs2 || !shell || !sums) return fail(nullptr, HH_ERR_ARG, "hh_frc_2d: NULL argument");
  if (batch < 1) return fail(nullptr, HH_ERR_ARG, "hh_frc_2d: batch must be >= 1");
  if (ny < 8 || ny > 1024 || nx < 8 || nx > 1024) return fail(nullptr, HH_ERR_ARG, "hh_frc_2d: both sides of the images must lie in [8, 1024]");
  if (n_shells < 0 || n_shells + 1 > FC_MAX_SHELLS) return fail(nullptr, HH_ERR_ARG, "hh_frc_2d: n_shells must lie in [0, 512]");
  for (int64_t i = 0; i < (int64_t)ny * nx; ++i)
    if (shell[i] < 0 || shell[i] > n_shells) return fail(nullptr, HH_ERR_ARG, "hh_frc_2d: a shell index lies outside [0, n_shells]");
  return fc_run("hh_frc_2d", device, imgs1, imgs2, batch, 0, ny, nx, shell, n_shells + 1, false, sums, kernel_ms);
} HH_CATCH_CTX(nullptr, "hh_frc_2d")
