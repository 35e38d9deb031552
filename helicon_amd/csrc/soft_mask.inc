// soft_mask.inc — the soft mask of the true FSC (commands/trueFSC.py:738-781, _soft_mask) built on the device from a binary
// support that is uploaded once: helicon_amd.true_fsc.soft_mask's definition, quirks included.
//
//   step = max(1, int(w / 4)); the support taken at every step-th voxel: m_a = ceil(n_a / step) samples per axis
//   D2    the exact squared Euclidean distance (integers, decimated voxels) to the nearest decimated inside voxel:
//         k_edt_x    nearest inside voxel along x: one wavefront per line, two ballot scans (from the left, from the right)
//         k_edt_line min_j (g[j] + (i - j)^2) along y, then along z: brute force in int32, lanes along x (every load of
//                    g[j][x ...] coalesces), SM_TILE outputs per lane in registers while j runs.  Exact everywhere: no window.
//         The largest value is 3 * 1023^2 < 2^22; "no inside voxel on this line" is SM_INF = 2^28, and SM_INF + 1023^2 < 2^31.
//   dist  step * sqrt(D2) in float64, interpolated as scipy.ndimage.zoom(order=1, mode="constant") does: per-axis tap tables
//         (sm_taps, host, float64: coordinate i (m - 1) / (n - 1), taps floor and floor + 1, weights 1 - f and f, and a
//         coordinate > m - 1 is OUTSIDE: the whole voxel reads 0), eight taps summed z, y, x (x fastest)
//   soft  1, except on outside voxels: 0 < dist <= w: (cos(dist / w * pi / 2) + 1) / 2;  dist > w: 0          (k_soft_mask)
//
// k_soft_mask stores the mask (float32) and / or multiplies the four resident maps of a true-FSC context by it straight into
// the forward passes' input, what k_tfsc_mask does from an uploaded mask: a trial width costs no upload but its tap tables.
// No atomics anywhere: every output has one writer and a fixed order of operations, so results are bit-identical from run to run.

struct SmTap {     // one full-grid index of one axis
  double w0, w1;   // weights of the taps i0, i1
  int32_t i0, i1;
  int32_t outside; // the coordinate lies beyond the last sample: zoom returns 0 for the voxel
  int32_t pad;
};

struct SmState {
  DevBuf<uint8_t> sup;           // [n_sup][n^3]
  int n_sup = 0;
  DevBuf<int32_t> g0, g1;        // the transform's two grids
  DevBuf<SmTap> taps;
  DevBuf<int32_t> probe;         // D2 of voxel 0 per (width, support): >= SM_INF means an empty decimated support
  DevBuf<float> mask;            // [n^3]: hh_tfsm_soft_mask's staging
};

void sm_release(SmState* s) { delete s; }

namespace {

constexpr int SM_INF = 1 << 28;
constexpr int SM_TILE = 16;
constexpr int SM_MAX_SIDE = 1024;

// One wavefront per decimated line (z, y): out[x] = (distance to the nearest inside voxel of the line)^2, SM_INF without one.
__global__ __launch_bounds__(256) void k_edt_x(const uint8_t* __restrict__ sup, int ny, int nx, int stride, int my, int mx, int64_t lines,
                                               int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (line >= lines) return;   // whole wavefronts leave together
  const int z = (int)(line / my), y = (int)(line % my);
  const uint8_t* const src = sup + ((int64_t)z * stride * ny + (int64_t)y * stride) * nx;
  int32_t* const dst = out + line * mx;
  const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull), from = ~0ull << lane;
  int last = -1;
  for (int x0 = 0; x0 < mx; x0 += 64) {
    const int x = x0 + lane;
    const bool inside = x < mx && src[(int64_t)x * stride] != 0;
    const unsigned long long b = __ballot(inside);
    const unsigned long long mine = b & upto;
    const int left = mine ? x0 + 63 - __clzll((long long)mine) : last;
    if (x < mx) dst[x] = left < 0 ? SM_INF : x - left;
    if (b) last = x0 + 63 - __clzll((long long)b);
  }
  int next = -1;
  for (int x0 = ((mx - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
    const int x = x0 + lane;
    const bool inside = x < mx && src[(int64_t)x * stride] != 0;
    const unsigned long long b = __ballot(inside);
    const unsigned long long mine = b & from;
    const int right = mine ? x0 + __ffsll((long long)mine) - 1 : next;
    if (x < mx) {
      int d = dst[x];   // this lane's own store of the first scan
      if (right >= 0) d = min(d, right - x);
      dst[x] = d >= SM_INF ? SM_INF : d * d;
    }
    if (b) next = x0 + __ffsll((long long)b) - 1;
  }
}

// out[o][i][x] = min(SM_INF, min_j in[o][j][x] + (i - j)^2) over the m samples of a line; element (o, j, x) lies at
// o * so + j * sl + x.  Thread: one (o, x) column and SM_TILE consecutive i.
__global__ __launch_bounds__(256) void k_edt_line(const int32_t* __restrict__ in, int32_t* __restrict__ out, int m, int mx, int64_t columns,
                                                  int64_t so, int64_t sl) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= columns) return;
  const int64_t base = (q / mx) * so + (q % mx);
  const int i0 = blockIdx.y * SM_TILE;
  int acc[SM_TILE];
#pragma unroll
  for (int t = 0; t < SM_TILE; ++t) acc[t] = SM_INF;
  for (int j = 0; j < m; ++j) {
    const int g = in[base + j * sl];
    const int d = i0 - j;
#pragma unroll
    for (int t = 0; t < SM_TILE; ++t) acc[t] = min(acc[t], g + (d + t) * (d + t));
  }
#pragma unroll
  for (int t = 0; t < SM_TILE; ++t)
    if (i0 + t < m) out[base + (i0 + t) * sl] = acc[t];
}

struct SmApply {
  const uint8_t* sup;      // [nz][ny][nx]
  const int32_t* d2;       // [mz][my][mx]
  const SmTap* tz;         // [nz], [ny], [nx]
  const SmTap* ty;
  const SmTap* tx;
  float* mask_out;         // [nz][ny][nx] or null
  const float* maps;       // [4][per_map] or null: map1, map2, map1r, map2r
  float* in1;              // maps != null: map1 m -> in1, map1r m -> in1 + per_map (null: this member is not written)
  float* in2;              // map2 m -> in2, map2r m -> in2 + per_map
  double width, step;
  int64_t per_map;
  int ny, nx, my, mx;
  int plain;               // width <= 0: the mask is the support as 0 / 1
};

__global__ __launch_bounds__(256) void k_soft_mask(SmApply g) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.per_map; i += (int64_t)gridDim.x * 256) {
    float soft = 1.f;
    if (g.sup[i] == 0) {
      if (g.plain) {
        soft = 0.f;
      } else {
        const int x = (int)(i % g.nx), y = (int)((i / g.nx) % g.ny), z = (int)(i / ((int64_t)g.nx * g.ny));
        const SmTap a = g.tz[z], b = g.ty[y], c = g.tx[x];
        double dist = 0.0;
        if (!(a.outside | b.outside | c.outside)) {
          const int iz[2] = {a.i0, a.i1}, iy[2] = {b.i0, b.i1}, ix[2] = {c.i0, c.i1};
          const double wz[2] = {a.w0, a.w1}, wy[2] = {b.w0, b.w1}, wx[2] = {c.w0, c.w1};
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
              for (int r = 0; r < 2; ++r) {
                const double v = g.step * sqrt((double)g.d2[((int64_t)iz[p] * g.my + iy[q]) * g.mx + ix[r]]);
                dist += v * wz[p] * wy[q] * wx[r];
              }
        }
        if (dist > g.width) soft = 0.f;
        else if (dist > 0.0) soft = (float)((cos(dist / g.width * 3.14159265358979323846 / 2.0) + 1.0) / 2.0);
      }
    }
    if (g.mask_out) g.mask_out[i] = soft;
    if (g.maps) {
      if (g.in1) {
        g.in1[i] = g.maps[i] * soft;
        g.in1[g.per_map + i] = g.maps[2 * g.per_map + i] * soft;
      }
      if (g.in2) {
        g.in2[i] = g.maps[g.per_map + i] * soft;
        g.in2[g.per_map + i] = g.maps[3 * g.per_map + i] * soft;
      }
    }
  }
}

// scipy.ndimage.zoom(order=1, mode="constant") along one axis of n outputs over m samples
void sm_taps(int n, int m, SmTap* t) {
  const double ratio = n > 1 ? (double)(m - 1) / (double)(n - 1) : 1.0;
  for (int i = 0; i < n; ++i) {
    const double c = (double)i * ratio;
    const double fl = std::floor(c);
    const double f = c - fl;
    SmTap e{};
    e.outside = c > (double)(m - 1) ? 1 : 0;
    e.i0 = std::min((int)fl, m - 1);
    e.i1 = std::min((int)fl + 1, m - 1);
    e.w0 = 1.0 - f;
    e.w1 = f;
    t[i] = e;
  }
}

int sm_step(double w) { return (int)std::max(1.0, std::min(w / 4.0, 4096.0)); }

bool sm_sides_ok(int nz, int ny, int nx) { return nz >= 1 && ny >= 1 && nx >= 1 && nz <= SM_MAX_SIDE && ny <= SM_MAX_SIDE && nx <= SM_MAX_SIDE; }

// the three passes on the default stream: sup [nz][ny][nx] at every stride-th voxel -> g0 [mz][my][mx] (g1: the second grid)
void sm_edt(const uint8_t* sup, int nz, int ny, int nx, int stride, int32_t* g0, int32_t* g1) {
  const int mz = (nz + stride - 1) / stride, my = (ny + stride - 1) / stride, mx = (nx + stride - 1) / stride;
  const int64_t lines = (int64_t)mz * my;
  hipLaunchKernelGGL(k_edt_x, dim3((unsigned)((lines + 3) / 4)), dim3(256), 0, nullptr, sup, ny, nx, stride, my, mx, lines, g0);
  const int64_t cy = (int64_t)mz * mx, cz = (int64_t)my * mx;   // columns of the y pass (o = z) and of the z pass (o = y)
  hipLaunchKernelGGL(k_edt_line, dim3((unsigned)((cy + 255) / 256), (unsigned)((my + SM_TILE - 1) / SM_TILE)), dim3(256), 0, nullptr, g0, g1, my, mx, cy,
                     (int64_t)my * mx, (int64_t)mx);
  hipLaunchKernelGGL(k_edt_line, dim3((unsigned)((cz + 255) / 256), (unsigned)((mz + SM_TILE - 1) / SM_TILE)), dim3(256), 0, nullptr, g1, g0, mz, mx, cz,
                     (int64_t)mx, (int64_t)my * mx);
}

unsigned sm_grid(int64_t per_map) { return (unsigned)std::min<int64_t>((per_map + 255) / 256, 4096); }

int sm_empty(const char* fn, int step) {
  return fail(nullptr, HH_ERR_ARG, std::string(fn) + ": the support has no inside voxel left when it is taken at every voxel that is a multiple of the step " +
                                       std::to_string(step) + ": there is no distance to take");
}

// the grids, tap tables and probes of a context, grown on demand
int sm_reserve(SmState* s, int64_t cells, int64_t taps, int64_t probes) {
  int rc = ensure(nullptr, s->g0, (size_t)cells);
  if (!rc) rc = ensure(nullptr, s->g1, (size_t)cells);
  if (!rc && taps > 0) rc = ensure(nullptr, s->taps, (size_t)taps);
  if (!rc && probes > 0) rc = ensure(nullptr, s->probe, (size_t)probes);
  return rc;
}

}  // namespace

// i0, i1, w0, w1, outside: [n] each.  Host only: the rule of scipy.ndimage.zoom(order=1) that k_soft_mask reads from tables.
extern "C" int hh_soft_mask_taps(int32_t n, int32_t m, int32_t* i0, int32_t* i1, double* w0, double* w1, int32_t* outside) try {
  if (!i0 || !i1 || !w0 || !w1 || !outside) return fail(nullptr, HH_ERR_ARG, "hh_soft_mask_taps: NULL argument");
  if (n < 1 || m < 1 || n > SM_MAX_SIDE || m > n) return fail(nullptr, HH_ERR_ARG, "hh_soft_mask_taps: 1 <= m <= n <= 1024 is needed");
  std::vector<SmTap> t((size_t)n);
  sm_taps(n, m, t.data());
  for (int i = 0; i < n; ++i) {
    i0[i] = t[(size_t)i].i0; i1[i] = t[(size_t)i].i1; w0[i] = t[(size_t)i].w0; w1[i] = t[(size_t)i].w1; outside[i] = t[(size_t)i].outside;
  }
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_soft_mask_taps")

extern "C" int hh_edt_3d(int device, const uint8_t* support, int32_t nz, int32_t ny, int32_t nx, int32_t stride, int32_t* sqdist_out,
                         double* kernel_ms) try {
  if (!support || !sqdist_out) return fail(nullptr, HH_ERR_ARG, "hh_edt_3d: NULL argument");
  if (!sm_sides_ok(nz, ny, nx)) return fail(nullptr, HH_ERR_ARG, "hh_edt_3d: the sides of the box must lie in [1, 1024]");
  if (stride < 1) return fail(nullptr, HH_ERR_ARG, "hh_edt_3d: stride must be >= 1");
  if (int rc = use_device("hh_edt_3d", device)) return rc;
  const int mz = (nz + stride - 1) / stride, my = (ny + stride - 1) / stride, mx = (nx + stride - 1) / stride;
  const int64_t cells = (int64_t)mz * my * mx, per_map = (int64_t)nz * ny * nx;
  SmState s;
  DevEvents<2> ev;
  if (int rc = ensure(nullptr, s.sup, (size_t)per_map)) return rc;
  if (int rc = sm_reserve(&s, cells, 0, 0)) return rc;
  HH_HIP(nullptr, ev.create());
  HH_HIP(nullptr, hipMemcpy(s.sup, support, (size_t)per_map, hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipEventRecord(ev[0], nullptr));
  sm_edt(s.sup, nz, ny, nx, stride, s.g0, s.g1);
  HH_HIP(nullptr, hipGetLastError());
  HH_HIP(nullptr, hipEventRecord(ev[1], nullptr));
  HH_HIP(nullptr, hipMemcpy(sqdist_out, s.g0, (size_t)cells * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (sqdist_out[0] >= SM_INF) return sm_empty("hh_edt_3d", stride);
  float ms = 0.f;
  HH_HIP(nullptr, hipEventElapsedTime(&ms, ev[0], ev[1]));
  if (kernel_ms) *kernel_ms = ms;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_edt_3d")

namespace {

// one mask from a support on the device (`s`: grids and tap tables reserved by the caller; taps at s->taps: z, y, x)
int sm_one(const char* fn, SmState* s, const uint8_t* d_sup, int nz, int ny, int nx, double w, float* d_mask) {
  const int64_t per_map = (int64_t)nz * ny * nx;
  SmApply g{};
  g.sup = d_sup; g.mask_out = d_mask; g.per_map = per_map; g.ny = ny; g.nx = nx; g.width = w;
  if (!(w > 0)) {
    g.plain = 1;
    hipLaunchKernelGGL(k_soft_mask, dim3(sm_grid(per_map)), dim3(256), 0, nullptr, g);
    HH_HIP(nullptr, hipGetLastError());
    return HH_OK;
  }
  const int step = sm_step(w);
  const int mz = (nz + step - 1) / step, my = (ny + step - 1) / step, mx = (nx + step - 1) / step;
  if (int rc = sm_reserve(s, (int64_t)mz * my * mx, (int64_t)nz + ny + nx, 1)) return rc;
  std::vector<SmTap> t((size_t)(nz + ny + nx));
  sm_taps(nz, mz, t.data());
  sm_taps(ny, my, t.data() + nz);
  sm_taps(nx, mx, t.data() + nz + ny);
  HH_HIP(nullptr, hipMemcpy(s->taps, t.data(), t.size() * sizeof(SmTap), hipMemcpyHostToDevice));
  sm_edt(d_sup, nz, ny, nx, step, s->g0, s->g1);
  HH_HIP(nullptr, hipGetLastError());
  int32_t first = 0;
  HH_HIP(nullptr, hipMemcpy(&first, s->g0, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (first >= SM_INF) return sm_empty(fn, step);
  g.d2 = s->g0; g.tz = s->taps; g.ty = s->taps + nz; g.tx = s->taps + nz + ny;
  g.step = (double)step; g.my = my; g.mx = mx;
  hipLaunchKernelGGL(k_soft_mask, dim3(sm_grid(per_map)), dim3(256), 0, nullptr, g);
  HH_HIP(nullptr, hipGetLastError());
  return HH_OK;
}

}  // namespace

extern "C" int hh_soft_mask_3d(int device, const uint8_t* support, int32_t nz, int32_t ny, int32_t nx, double soft_width, float* mask_out,
                               double* kernel_ms) try {
  if (!support || !mask_out) return fail(nullptr, HH_ERR_ARG, "hh_soft_mask_3d: NULL argument");
  if (!sm_sides_ok(nz, ny, nx)) return fail(nullptr, HH_ERR_ARG, "hh_soft_mask_3d: the sides of the box must lie in [1, 1024]");
  if (!std::isfinite(soft_width)) return fail(nullptr, HH_ERR_ARG, "hh_soft_mask_3d: the width is NaN or infinite");
  const int64_t per_map = (int64_t)nz * ny * nx;
  if (!(soft_width > 0)) {   // the support as 0 / 1, as the host returns it: no device call
    for (int64_t i = 0; i < per_map; ++i) mask_out[i] = support[i] ? 1.f : 0.f;
    if (kernel_ms) *kernel_ms = 0.0;
    return HH_OK;
  }
  if (int rc = use_device("hh_soft_mask_3d", device)) return rc;
  SmState s;
  DevEvents<2> ev;
  if (int rc = ensure(nullptr, s.sup, (size_t)per_map)) return rc;
  if (int rc = ensure(nullptr, s.mask, (size_t)per_map)) return rc;
  HH_HIP(nullptr, ev.create());
  HH_HIP(nullptr, hipMemcpy(s.sup, support, (size_t)per_map, hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipEventRecord(ev[0], nullptr));
  if (int rc = sm_one("hh_soft_mask_3d", &s, s.sup, nz, ny, nx, soft_width, s.mask)) return rc;
  HH_HIP(nullptr, hipEventRecord(ev[1], nullptr));
  HH_HIP(nullptr, hipMemcpy(mask_out, s.mask, (size_t)per_map * sizeof(float), hipMemcpyDeviceToHost));
  float ms = 0.f;
  HH_HIP(nullptr, hipEventElapsedTime(&ms, ev[0], ev[1]));
  if (kernel_ms) *kernel_ms = ms;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_soft_mask_3d")

extern "C" int hh_tfsm_set_support(hh_tfsc* ctx, const uint8_t* support1, const uint8_t* support2) try {
  if (!ctx || !support1) return fail(nullptr, HH_ERR_ARG, "hh_tfsm_set_support: NULL argument");
  hh_tfsc* const c = ctx;
  HH_HIP(nullptr, hipSetDevice(c->device));
  if (!c->soft) c->soft = new SmState;
  SmState* const s = c->soft;
  const int n_sup = support2 ? 2 : 1;
  if (s->n_sup != n_sup) {
    s->sup.reset();
    s->n_sup = 0;
    if (int rc = ensure(nullptr, s->sup, (size_t)n_sup * (size_t)c->per_map)) return rc;
  }
  HH_HIP(nullptr, hipMemcpy(s->sup, support1, (size_t)c->per_map, hipMemcpyHostToDevice));
  if (support2) HH_HIP(nullptr, hipMemcpy(s->sup + c->per_map, support2, (size_t)c->per_map, hipMemcpyHostToDevice));
  s->n_sup = n_sup;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_tfsm_set_support")

extern "C" int hh_tfsm_soft_mask(hh_tfsc* ctx, int which, double soft_width, float* mask_out) try {
  if (!ctx || !mask_out) return fail(nullptr, HH_ERR_ARG, "hh_tfsm_soft_mask: NULL argument");
  if (which < 0 || which > 1) return fail(nullptr, HH_ERR_ARG, "hh_tfsm_soft_mask: which must be 0 or 1");
  if (!std::isfinite(soft_width)) return fail(nullptr, HH_ERR_ARG, "hh_tfsm_soft_mask: the width is NaN or infinite");
  hh_tfsc* const c = ctx;
  SmState* const s = c->soft;
  if (!s || s->n_sup < 1) return fail(nullptr, HH_ERR_STATE, "hh_tfsm_soft_mask: no support is set (hh_tfsm_set_support)");
  HH_HIP(nullptr, hipSetDevice(c->device));
  if (int rc = ensure(nullptr, s->mask, (size_t)c->per_map)) return rc;
  const uint8_t* const sup = s->sup + (s->n_sup == 2 ? which : 0) * c->per_map;
  if (int rc = sm_one("hh_tfsm_soft_mask", s, sup, c->n, c->n, c->n, soft_width, s->mask)) return rc;
  HH_HIP(nullptr, hipMemcpy(mask_out, s->mask, (size_t)c->per_map * sizeof(float), hipMemcpyDeviceToHost));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_tfsm_soft_mask")

extern "C" int hh_tfsm_soft_masked(hh_tfsc* ctx, const double* soft_widths, int32_t batch, int full_spectrum, double* sums,
                                   double* kernel_ms) try {
  if (!ctx || !soft_widths || !sums) return fail(nullptr, HH_ERR_ARG, "hh_tfsm_soft_masked: NULL argument");
  if (batch < 1) return fail(nullptr, HH_ERR_ARG, "hh_tfsm_soft_masked: batch must be >= 1");
  for (int32_t j = 0; j < batch; ++j)
    if (!std::isfinite(soft_widths[j])) return fail(nullptr, HH_ERR_ARG, "hh_tfsm_soft_masked: a width is NaN or infinite");
  hh_tfsc* const c = ctx;
  SmState* const s = c->soft;
  if (!s || s->n_sup < 1) return fail(nullptr, HH_ERR_STATE, "hh_tfsm_soft_masked: no support is set (hh_tfsm_set_support)");
  HH_HIP(nullptr, hipSetDevice(c->device));
  const int64_t per_map = c->per_map;
  const int nshell = c->nshell, n = c->n;
  // widths per chunk: hh_tfsc_masked's rule (two pairs each within fc_run's scratch cap, the y pass's grid.z = 4 chunk n <= 65535)
  int64_t per_launch = std::max<int64_t>(1, FC_SCRATCH_BYTES / (20 * per_map * (int64_t)sizeof(float)));
  per_launch = std::min<int64_t>(per_launch, 65535 / (4 * n));
  per_launch = std::min<int64_t>(per_launch, batch);
  FcBuffers& d = c->fc;
  if (int rc = d.reserve(2 * per_launch, per_map, nshell, true, true)) return rc;
  int64_t cells = 1;   // the largest decimated grid of the list
  for (int32_t j = 0; j < batch; ++j)
    if (soft_widths[j] > 0) {
      const int64_t m = (n + sm_step(soft_widths[j]) - 1) / sm_step(soft_widths[j]);
      cells = std::max(cells, m * m * m);
    }
  const int n_sup = s->n_sup;
  if (int rc = sm_reserve(s, cells, per_launch * 3 * n, per_launch * n_sup)) return rc;
  std::vector<SmTap> taps((size_t)(per_launch * 3 * n));
  std::vector<int32_t> probe((size_t)(per_launch * n_sup));
  double ms_total = 0.0;
  for (int64_t b0 = 0; b0 < batch; b0 += per_launch) {
    const int64_t nb = std::min(per_launch, (int64_t)batch - b0);
    for (int64_t j = 0; j < nb; ++j) {   // one axis table per width: the box is a cube
      const double w = soft_widths[b0 + j];
      const int step = w > 0 ? sm_step(w) : 1;
      sm_taps(n, (n + step - 1) / step, taps.data() + j * 3 * n);
    }
    HH_HIP(nullptr, hipMemcpy(s->taps, taps.data(), (size_t)(nb * 3 * n) * sizeof(SmTap), hipMemcpyHostToDevice));
    HH_HIP(nullptr, hipMemsetAsync(s->probe, 0, (size_t)(nb * n_sup) * sizeof(int32_t), nullptr));
    HH_HIP(nullptr, hipEventRecord(d.ev[0], nullptr));
    const int64_t P = 2 * nb;   // k_tfsc_mask's layout of `in`
    for (int64_t j = 0; j < nb; ++j) {
      const double w = soft_widths[b0 + j];
      const int step = w > 0 ? sm_step(w) : 1;
      const int m = (n + step - 1) / step;
      float* const in1 = d.in + (2 * j) * per_map;
      float* const in2 = d.in + (P + 2 * j) * per_map;
      for (int k = 0; k < n_sup; ++k) {
        SmApply g{};
        g.sup = s->sup + k * per_map;
        g.maps = c->maps; g.per_map = per_map; g.ny = n; g.nx = n; g.width = w;
        g.in1 = (n_sup == 1 || k == 0) ? in1 : nullptr;
        g.in2 = (n_sup == 1 || k == 1) ? in2 : nullptr;
        if (w > 0) {
          sm_edt(g.sup, n, n, n, step, s->g0, s->g1);
          HH_HIP(nullptr, hipMemcpyAsync(s->probe + j * n_sup + k, s->g0, sizeof(int32_t), hipMemcpyDeviceToDevice, nullptr));
          g.d2 = s->g0; g.tz = g.ty = g.tx = s->taps + j * 3 * n;
          g.step = (double)step; g.my = m; g.mx = m;
        } else {
          g.plain = 1;
        }
        hipLaunchKernelGGL(k_soft_mask, dim3(sm_grid(per_map)), dim3(256), 0, nullptr, g);
      }
    }
    HH_HIP(nullptr, hipGetLastError());
    fc_device(c->plan, d.in, d, 2 * nb, nshell, full_spectrum != 0);
    HH_HIP(nullptr, hipGetLastError());
    HH_HIP(nullptr, hipEventRecord(d.ev[1], nullptr));
    HH_HIP(nullptr, hipMemcpy(probe.data(), s->probe, (size_t)(nb * n_sup) * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t e = 0; e < nb * n_sup; ++e)
      if (probe[(size_t)e] >= SM_INF) return sm_empty("hh_tfsm_soft_masked", sm_step(soft_widths[b0 + e / n_sup]));
    HH_HIP(nullptr, hipMemcpy(sums + b0 * 2 * nshell * 3, d.sums, (size_t)(2 * nb) * nshell * 3 * sizeof(double), hipMemcpyDeviceToHost));
    float ms = 0.f;
    HH_HIP(nullptr, hipEventElapsedTime(&ms, d.ev[0], d.ev[1]));
    ms_total += ms;
  }
  if (kernel_ms) *kernel_ms = ms_total;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_tfsm_soft_masked")
