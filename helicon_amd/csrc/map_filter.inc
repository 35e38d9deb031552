// map_filter.inc — the 3-D map input of the app (webApps/denovo3D/utils.py:336-383): the Gaussian low / high pass of a
// whole map (lib/filters.py:349-372, 3-D branch) and the map's three axis projections (generate_xyz_projections).
//
// The reference multiplies fftn(x) by fftshift(exp(-f2 (X^2 + Y^2 + Z^2))) and returns Re ifftn(.).  That filter is the
// product w_z(kz) w_y(ky) w_x(kx) of three 1-D weights, so it is three 1-D circulant operators, one along each axis:
//     C = F^-1 diag(w) F,   C[i][j] = c[(i - j) mod n],   c = ifft(w)
// and the high pass folds into the same form: exp(-a R^2) (1 - exp(-b R^2)) = G_a - G_(a+b); high pass alone is x - G_b x.
// Each axis pass is a plain GEMM on the volume as stored (no transposes), on the exact-f32 MFMA (32x32x2): k_circ_gemm
// (axis_pass.inc) in the geometry axis_plan.h gives for the axis,
//     z: (nz x nz) . (nz x ny nx),   y: batched over z, (ny x ny) . (ny x nx),   x: (nz ny x nx) . (nx x nx)^T.
// Any side works (primes included): there is no FFT plan.  The per-axis weights follow gen_pass_filter's rule: unshifted
// index k takes the centred float32 coordinate of (k + ceil(n / 2)) mod n over n // 2 (fftshift, not ifftshift), which for
// an ODD side moves DC off the filter's centre, so c is complex there; for an even side c is real and symmetric.  Complex
// passes therefore run on odd axes only (two real products on a real input, one K = 2n product per output plane on a
// complex one) and the last pass computes the real plane alone.  c is built in float64 on the host and rounded to f32.

namespace {

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
  if (int rc = use_device("hh_low_high_pass_filter_3d", device)) return rc;
  const int64_t total = (int64_t)side[0] * side[1] * side[2];
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
        const size_t off = append_axis_operator(mats, n, AxisIndex::Circulant, cr, 1.0, nullptr, 0.0);
        ops.push_back({ax, off, n, re, -1, dre});
        if (im >= 0 && !last) ops.push_back({ax, off, n, im, -1, dim});
        im = (im >= 0 && !last) ? dim : -1;
      } else if (im < 0) {   // complex C on a real input: Re = Cr x, Im = Ci x
        any_odd = true;
        ops.push_back({ax, append_axis_operator(mats, n, AxisIndex::Circulant, cr, 1.0, nullptr, 0.0), n, re, -1, dre});
        if (!last) ops.push_back({ax, append_axis_operator(mats, n, AxisIndex::Circulant, ci, 1.0, nullptr, 0.0), n, re, -1, dim});
        im = last ? -1 : dim;
      } else {   // complex C on a complex input: Re = [Cr | -Ci] [xr; xi], Im = [Ci | Cr] [xr; xi]
        ops.push_back({ax, append_axis_operator(mats, n, AxisIndex::Circulant, cr, 1.0, &ci, -1.0), 2 * n, re, im, dre});
        if (!last) ops.push_back({ax, append_axis_operator(mats, n, AxisIndex::Circulant, ci, 1.0, &cr, 1.0), 2 * n, re, im, dim});
        im = last ? -1 : dim;
      }
      re = dre;
    }
    ops.push_back({-1, 0, 0, 5, -1, -1});   // marker: accumulate plane 5 with this term's coefficient
  }
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
      launch_circ_pass(axis_geom(side, op.axis, side[op.axis], 1), d_mats + op.a_off, op.ka, planes[op.src0],
                       op.src1 >= 0 ? planes[op.src1] : nullptr, planes[op.dst], nullptr);
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
  if (int rc = use_device("hh_map_projections", device)) return rc;
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
