// map_filter.inc — the 3-D map input of the app (webApps/denovo3D/utils.py:336-383): the Gaussian low / high pass of a
// whole map (lib/filters.py:349-372, 3-D branch) and the map's three axis projections (generate_xyz_projections).
//
// The reference multiplies fftn(x) by fftshift(exp(-f2 (X^2 + Y^2 + Z^2))) and returns Re ifftn(.).  That filter is the
// product w_z(kz) w_y(ky) w_x(kx) of three 1-D weights, so it is three 1-D circulant operators, one along each axis:
//     C = F^-1 diag(w) F,   C[i][j] = c[(i - j) mod n],   c = ifft(w)
// and the high pass folds into the same form: exp(-a R^2) (1 - exp(-b R^2)) = G_a - G_(a+b); high pass alone is x - G_b x.
// Each axis pass is a plain GEMM on the volume as stored (no transposes), on the exact-f32 MFMA (32x32x2):
//     z: (nz x nz) . (nz x ny nx),   y: batched over z, (ny x ny) . (ny x nx),   x: (nz ny x nx) . (nx x nx)^T.
// Any side works (primes included): there is no FFT plan.  The per-axis weights follow gen_pass_filter's rule: unshifted
// index k takes the centred float32 coordinate of (k + ceil(n / 2)) mod n over n // 2 (fftshift, not ifftshift), which for
// an ODD side moves DC off the filter's centre, so c is complex there; for an even side c is real and symmetric.  Complex
// passes therefore run on odd axes only (two real products on a real input, one K = 2n product per output plane on a
// complex one) and the last pass computes the real plane alone.  c is built in float64 on the host and rounded to f32.

namespace {

constexpr int MF_T = 64;   // output tile of a workgroup: 64 rows of the operator x 64 columns of the volume
constexpr int MF_K = 32;   // K slice staged through LDS per step

struct CircPass {
  const float* a;    // [n][ka] row-major operator block (ka = n, or 2n for [Cr | -Ci] / [Ci | Cr] on a complex input)
  const float* b0;   // input plane for k < n
  const float* b1;   // input plane for n <= k < 2n (imaginary part), or null when ka == n
  float* y;          // output plane
  int n, ka;
  int64_t np;        // columns P of the product
  int64_t sk, sp;    // element strides of B / Y along the operator's index and along P
  int64_t sb;        // element stride of one batch (the y pass: one z slice)
};

// Y[b][m][p] = sum_k A[m][k] B[b][k][p] on the shared tile (mfma_tile.inc), one 32 x 32 accumulator per wavefront.  TR swaps
// the MFMA's operands so that the accumulator's lane index runs along m: with the x pass's strides (sk = 1) the stores coalesce.
template <bool TR>
__global__ __launch_bounds__(256) void k_circ_gemm(CircPass g) {
  __shared__ float as[MF_T][MF_K + 1];
  __shared__ float bs[MF_K][MF_T + 1];
  const Tile64 t = tile64();
  const int tid = t.tid, r = t.r, h = t.h, wm = t.wm, wp = t.wp;
  const int m0 = blockIdx.y * MF_T;
  const int64_t p0 = (int64_t)blockIdx.x * MF_T, boff = (int64_t)blockIdx.z * g.sb;
  const float* b0 = g.b0 + boff;
  const float* b1 = g.b1 ? g.b1 + boff : nullptr;
  f32x16 acc = {0};
  for (int k0 = 0; k0 < g.ka; k0 += MF_K) {
    stage_rows(as, g.a, g.ka, m0, g.n, k0, g.ka, tid);
    for (int e = tid; e < MF_T * MF_K; e += 256) {   // its own: the stride along P and the split of K over b0 / b1
      int kk, pp;
      if (g.sp == 1) { kk = e / MF_T; pp = e % MF_T; }   // P contiguous: lanes along P
      else { pp = e / MF_K; kk = e % MF_K; }             // the x pass: lanes along k
      const int k = k0 + kk;
      const int64_t p = p0 + pp;
      float v = 0.f;
      if (k < g.ka && p < g.np) v = k < g.n ? b0[(int64_t)k * g.sk + p * g.sp] : b1[(int64_t)(k - g.n) * g.sk + p * g.sp];
      bs[kk][pp] = v;
    }
    __syncthreads();
    tile_mac<TR>(acc, as, bs, t);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = acc_row(i, h);
    const int m = m0 + wm + (TR ? r : row);
    const int64_t p = p0 + wp + (TR ? row : r);
    if (m < g.n && p < g.np) g.y[boff + (int64_t)m * g.sk + p * g.sp] = acc[i];
  }
}

__global__ __launch_bounds__(256) void k_map_axpy(float* __restrict__ acc, float coef, const float* __restrict__ src, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) acc[i] += coef * src[i];
}

// One z slice per workgroup: its sums along x (out_x[z][y]) and along y (out_y[z][x]); float64 running sums.
__global__ __launch_bounds__(256) void k_map_proj_slices(const float* __restrict__ v, int ny, int nx, float* __restrict__ out_x,
                                                         float* __restrict__ out_y) {
  const int z = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* s = v + (int64_t)z * ny * nx;
  for (int y = wave; y < ny; y += 4) {
    double acc = 0;
    for (int x = lane; x < nx; x += 64) acc += s[(int64_t)y * nx + x];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) out_x[(int64_t)z * ny + y] = (float)acc;
  }
  for (int x = threadIdx.x; x < nx; x += 256) {
    double acc = 0;
    for (int y = 0; y < ny; ++y) acc += s[(int64_t)y * nx + x];
    out_y[(int64_t)z * nx + x] = (float)acc;
  }
}

// One (y, x) column per thread: the sum along z, or along the slab [z_begin, z_end) when z_begin >= 0.
__global__ __launch_bounds__(256) void k_map_proj_columns(const float* __restrict__ v, int nz, int64_t plane, int z_begin, int z_end,
                                                          float* __restrict__ out_z) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= plane) return;
  const int za = z_begin >= 0 ? z_begin : 0, zb = z_begin >= 0 ? z_end : nz;
  double acc = 0;
  for (int z = za; z < zb; ++z) acc += v[(int64_t)z * plane + q];
  out_z[q] = (float)acc;
}

// c = ifft(w) for one axis, w the reference's weight exp(-f2 u^2) on fftshifted float32 coordinates u (float64 sums).
void circulant_column(int n, double f2, std::vector<double>& cr, std::vector<double>& ci) {
  std::vector<double> w(n), cs(n), sn(n);
  for (int k = 0; k < n; ++k) {
    const int idx = (k + (n + 1) / 2) % n;
    const float u = (float)(idx - n / 2) / (float)(n / 2);
    w[k] = std::exp(-f2 * (double)(u * u));
    cs[k] = std::cos(2.0 * M_PI * k / n);
    sn[k] = std::sin(2.0 * M_PI * k / n);
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

// Appends the n x ka operator block [p | q] (q only when ka = 2n), p[i][j] = sp * c_p[(i - j) mod n], to `mats`.
size_t append_operator(std::vector<float>& mats, int n, const std::vector<double>& cp, double sp, const std::vector<double>* cq,
                       double sq) {
  const size_t off = mats.size();
  const int ka = cq ? 2 * n : n;
  mats.resize(off + (size_t)n * ka);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const int d = ((i - j) % n + n) % n;
      mats[off + (size_t)i * ka + j] = (float)(sp * cp[d]);
      if (cq) mats[off + (size_t)i * ka + n + j] = (float)(sq * (*cq)[d]);
    }
  return off;
}

struct CircOp {
  int axis;
  size_t a_off;
  int ka;
  int src0, src1, dst;   // plane ids: 0 = input, 1 / 2 = pair A (re / im), 3 / 4 = pair B, 5 = term result; -1 = none
};

}  // namespace

extern "C" int hh_low_high_pass_filter_3d(int device, const float* data, const int32_t shape[3], double low_pass_fraction,
                                          double high_pass_fraction, float* out) try {
  if (!data || !out || !shape) return fail(nullptr, HH_ERR_ARG, "hh_low_high_pass_filter_3d: NULL argument");
  const int side[3] = {shape[0], shape[1], shape[2]};
  for (int ax = 0; ax < 3; ++ax)
    if (side[ax] < 2 || side[ax] > 1024)
      return fail(nullptr, HH_ERR_ARG, "hh_low_high_pass_filter_3d: every side must lie in [2, 1024] (the reference divides by n // 2)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(nullptr, HH_ERR_HIP, "hh_low_high_pass_filter_3d: no such HIP device (there is no CPU fallback)");
  const int nz = side[0], ny = side[1], nx = side[2];
  const int64_t total = (int64_t)nz * ny * nx;
  // filters.py:363-370: a fraction outside (0, 1) is ignored.  The result is sum_t coef_t G_(f2_t) x, G_0 = identity.
  const bool lp = 0 < low_pass_fraction && low_pass_fraction < 1, hp = 0 < high_pass_fraction && high_pass_fraction < 1;
  const double a = lp ? std::log(2.0) / (low_pass_fraction * low_pass_fraction) : 0.0;
  const double b = hp ? std::log(2.0) / (high_pass_fraction * high_pass_fraction) : 0.0;
  std::vector<std::pair<double, double>> terms;   // (coef, f2)
  if (lp && hp) terms = {{1.0, a}, {-1.0, a + b}};
  else if (lp) terms = {{1.0, a}};
  else if (hp) terms = {{1.0, 0.0}, {-1.0, b}};
  else terms = {{1.0, 0.0}};
  // plan every product: plane 0 is the input, pairs A (1, 2) and B (3, 4) alternate, the last pass writes plane 5
  std::vector<float> mats;
  std::vector<CircOp> ops;
  bool any_odd = false;
  for (const auto& t : terms) {
    if (t.second == 0.0) continue;
    int re = 0, im = -1;   // the current (real, imaginary) planes
    for (int ax = 0; ax < 3; ++ax) {
      const int n = side[ax];
      const bool last = ax == 2, odd = n % 2 == 1;
      const int dre = last ? 5 : (ax == 1 ? 3 : 1), dim = last ? -1 : dre + 1;
      std::vector<double> cr, ci;
      circulant_column(n, t.second, cr, ci);
      if (!odd) {   // C real (and symmetric): each plane on its own
        const size_t off = append_operator(mats, n, cr, 1.0, nullptr, 0.0);
        ops.push_back({ax, off, n, re, -1, dre});
        if (im >= 0 && !last) ops.push_back({ax, off, n, im, -1, dim});
        im = (im >= 0 && !last) ? dim : -1;
      } else if (im < 0) {   // complex C on a real input: Re = Cr x, Im = Ci x
        any_odd = true;
        ops.push_back({ax, append_operator(mats, n, cr, 1.0, nullptr, 0.0), n, re, -1, dre});
        if (!last) ops.push_back({ax, append_operator(mats, n, ci, 1.0, nullptr, 0.0), n, re, -1, dim});
        im = last ? -1 : dim;
      } else {   // complex C on a complex input: Re = [Cr | -Ci] [xr; xi], Im = [Ci | Cr] [xr; xi]
        ops.push_back({ax, append_operator(mats, n, cr, 1.0, &ci, -1.0), 2 * n, re, im, dre});
        if (!last) ops.push_back({ax, append_operator(mats, n, ci, 1.0, &cr, 1.0), 2 * n, re, im, dim});
        im = last ? -1 : dim;
      }
      re = dre;
    }
    ops.push_back({-1, 0, 0, 5, -1, -1});   // marker: accumulate plane 5 with this term's coefficient
  }
  HH_HIP(nullptr, hipSetDevice(device));
  DevArena mem;
  float* planes[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  float* d_mats = nullptr;
  const size_t bytes = (size_t)total * sizeof(float);
  planes[0] = mem.get<float>((size_t)total);
  float* d_acc = mem.get<float>((size_t)total);
  if (!ops.empty()) {
    for (int p : {1, 3, 5}) planes[p] = mem.get<float>((size_t)total);
    if (any_odd)
      for (int p : {2, 4}) planes[p] = mem.get<float>((size_t)total);
    d_mats = mem.get<float>(mats.size());
  }
  if (int rc = arena_ok(nullptr, mem)) return rc;
  hipError_t e = hipSuccess;
  if (d_mats) e = hipMemcpy(d_mats, mats.data(), mats.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(planes[0], data, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemsetAsync(d_acc, 0, bytes, nullptr);
  const unsigned axpy_blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
  size_t next_term = 0;
  for (size_t i = 0; e == hipSuccess && i < terms.size(); ++i) {
    if (terms[i].second == 0.0) {
      hipLaunchKernelGGL(k_map_axpy, dim3(axpy_blocks), dim3(256), 0, nullptr, d_acc, (float)terms[i].first, planes[0], total);
      e = hipGetLastError();
      continue;
    }
    for (; e == hipSuccess && next_term < ops.size(); ++next_term) {
      const CircOp& op = ops[next_term];
      if (op.axis < 0) {
        hipLaunchKernelGGL(k_map_axpy, dim3(axpy_blocks), dim3(256), 0, nullptr, d_acc, (float)terms[i].first, planes[5], total);
        e = hipGetLastError();
        ++next_term;
        break;
      }
      CircPass g{};
      g.a = d_mats + op.a_off;
      g.b0 = planes[op.src0];
      g.b1 = op.src1 >= 0 ? planes[op.src1] : nullptr;
      g.y = planes[op.dst];
      g.n = side[op.axis];
      g.ka = op.ka;
      dim3 grid;
      const unsigned mt = (unsigned)((g.n + MF_T - 1) / MF_T);
      if (op.axis == 0) {        // (nz x nz) . (nz x ny nx)
        g.np = (int64_t)ny * nx; g.sk = g.np; g.sp = 1; g.sb = 0;
        grid = dim3((unsigned)((g.np + MF_T - 1) / MF_T), mt, 1);
      } else if (op.axis == 1) { // per z slice: (ny x ny) . (ny x nx)
        g.np = nx; g.sk = nx; g.sp = 1; g.sb = (int64_t)ny * nx;
        grid = dim3((unsigned)((g.np + MF_T - 1) / MF_T), mt, (unsigned)nz);
      } else {                   // (nz ny x nx) . (nx x nx)^T
        g.np = (int64_t)nz * ny; g.sk = 1; g.sp = nx; g.sb = 0;
        grid = dim3((unsigned)((g.np + MF_T - 1) / MF_T), mt, 1);
      }
      if (op.axis == 2) hipLaunchKernelGGL(k_circ_gemm<true>, grid, dim3(256), 0, nullptr, g);
      else hipLaunchKernelGGL(k_circ_gemm<false>, grid, dim3(256), 0, nullptr, g);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_acc, bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_low_high_pass_filter_3d: ") + hipGetErrorString(e));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_low_high_pass_filter_3d")

extern "C" int hh_map_projections(int device, const float* data, const int32_t shape[3], int32_t slab_begin, int32_t slab_end,
                                  float* out_x, float* out_y, float* out_z) try {
  if (!data || !shape || !out_x || !out_y || !out_z) return fail(nullptr, HH_ERR_ARG, "hh_map_projections: NULL argument");
  const int nz = shape[0], ny = shape[1], nx = shape[2];
  if (nz < 1 || ny < 1 || nx < 1 || nz > 4096 || ny > 4096 || nx > 4096)
    return fail(nullptr, HH_ERR_ARG, "hh_map_projections: sides must lie in [1, 4096]");
  if (slab_begin >= 0 && (slab_end < slab_begin || slab_end > nz))
    return fail(nullptr, HH_ERR_ARG, "hh_map_projections: the slab must satisfy 0 <= begin <= end <= nz");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(nullptr, HH_ERR_HIP, "hh_map_projections: no such HIP device (there is no CPU fallback)");
  HH_HIP(nullptr, hipSetDevice(device));
  const int64_t plane = (int64_t)ny * nx, total = plane * nz;
  DevArena mem;
  float* d_v = mem.get<float>((size_t)total);
  float* d_x = mem.get<float>((size_t)nz * ny);
  float* d_y = mem.get<float>((size_t)nz * nx);
  float* d_z = mem.get<float>((size_t)plane);
  if (int rc = arena_ok(nullptr, mem)) return rc;
  hipError_t e = hipMemcpy(d_v, data, (size_t)total * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_map_proj_slices, dim3((unsigned)nz), dim3(256), 0, nullptr, d_v, ny, nx, d_x, d_y);
    hipLaunchKernelGGL(k_map_proj_columns, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, nullptr, d_v, nz, plane, slab_begin,
                       slab_end, d_z);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out_x, d_x, (size_t)nz * ny * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_y, d_y, (size_t)nz * nx * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_z, d_z, (size_t)plane * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_map_projections: ") + hipGetErrorString(e));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_map_projections")
