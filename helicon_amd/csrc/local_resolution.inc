// local_resolution.inc — local resolution of two half maps: the Fourier shell correlation of every overlapping window pair
// of side w around a grid of centres, and the resolution at which each window's curve first falls below a threshold.
//
// A window is get_clip3d's (lib/transforms.py:516-555: zeros outside the map) times generate_tapering_filter's cosine edge per
// axis (lib/filters.py:415-466: the 1-D profile comes from the host), its curve calc_fsc_per_shell's (lib/analysis.py:235-290:
// the full spectrum seen from its half, weight 2 off the planes kx = 0 and kx = w / 2), its resolution the linear interpolation
// of commands/trueFSC.py:427-462 between the shells around the first crossing, with shell 0 never searched, w apix when shell 1
// is already below and Nyquist when no shell is.  The context keeps both maps on the device; nothing but the centres and the
// taper goes up and nothing but the results comes back.  Two routes:
//   passes (any even w in [8, 64]):  k_lres_gather writes a chunk's tapered windows into FcBuffers::in (first members, then second
//                                    members), fc_device runs unchanged, k_lres_resolve applies the ratio and the crossing rule
//                                    to its float64 sums.
//   LDS (even w in [8, 24]):         k_lres_lds<W>, one workgroup per window pair; the windows never exist in HBM.  Both tapered
//                                    windows are read into LDS rows of W + 3 floats (W reals, later W / 2 + 1 re | W / 2 + 1 im;
//                                    the odd stride keeps the x pass's one-row-per-lane reads off each other's banks), max |x| gives
//                                    the pair's scales (fc_pair_scales), then x, y and z passes in place: a lane owns a row or a
//                                    column, reads it whole into registers and writes its direct DFT back (fmaf chains over a
//                                    cos / sin table held in registers; every index is a compile-time constant).  After the z pass
//                                    every bin goes through fc_shell_3d and fc_add_products into LDS shell slots, and the first
//                                    lanes apply the ratio and the crossing rule.
// Both routes are bit-identical from run to run and do not depend on the chunking, the budget or the order of the centres: the
// sums are fc_add_products' integer atomics.  The two routes round their transforms differently and need not agree bit for bit.
// k_lres_upsample spreads the grid of results over the full map, trilinear between the centres with unevaluated (NaN) corners dropped.

struct hh_lres {
  int device = 0, nz = 0, ny = 0, nx = 0;
  int64_t scratch_bytes = 0, max_windows = 0;   // hh_lres_set_budget: 0 = the defaults
  DevBuf<float> maps;                           // [2][nz][ny][nx]
  FcPlan plan;                                  // the passes route's operators of side plan_w
  int plan_w = 0;
  FcBuffers fc;
  int tab_w = 0;                                // the LDS route's table [cos | sin] of side tab_w
  DevBuf<float> tab, taper;
  DevBuf<int32_t> centres;
  DevBuf<double> res, curves;
  std::vector<std::pair<const void*, int>> lds_attr;
  ~hh_lres() { (void)hipSetDevice(device); }   // (the buffers go after this body, on the device set here)
};

namespace {

// lanes of a workgroup of k_lres_lds.  From w = 18 on a compute unit holds one or two workgroups, and eight wavefronts keep
// two per SIMD in flight over the LDS round trips: measured at w = 24, 512 lanes take 0.68 of the time of 256.  One lane per
// column of the y and z passes (320 at w = 16, 448 at 20, 640 at 24) was measured too and kept nowhere: slower at 16, 18 and
// 20, 5 % faster at 24 (DESIGN.md, "Local resolution").
constexpr int lr_threads(int w) { return w >= 18 ? 512 : 256; }
constexpr int LR_MIN_W = 8, LR_MAX_W = 64, LR_MAX_LDS_W = 24;
constexpr int64_t LR_LDS_BYTES_MAX = 163840;          // a compute unit's LDS
constexpr int64_t LR_LDS_WINDOWS = (int64_t)1 << 20;  // windows per launch of the LDS route unless the budget says less

// LDS of one workgroup of k_lres_lds: [3 h] shell slots, [h] curve, [3] scales (8 bytes each), then two windows of w w rows of
// w + 3 floats, the cos and sin tables and the two max |x|
constexpr int64_t lr_lds_bytes(int w) {
  const int h = w / 2 + 1;
  return 8 * (int64_t)(3 * h + h + 3) + 4 * ((int64_t)2 * w * w * (w + 3) + 2 * w + 2);
}
static_assert(lr_lds_bytes(LR_MAX_LDS_W) <= LR_LDS_BYTES_MAX, "the largest window pair must fit a compute unit's LDS");
static_assert(4 * lr_lds_bytes(16) <= LR_LDS_BYTES_MAX, "four workgroups per compute unit at w = 16");

// The crossing rule on a curve fsc[0 .. h), h = w / 2 + 1, in float64 (helicon_amd/local_resolution.py: resolution_from_curve
// is the same expression).  Shell 0 is not searched.
__device__ __forceinline__ double lr_resolution(const double* fsc, int w, double apix, double thr) {
  const int h = w / 2 + 1;
  const double box = (double)w * apix;
  for (int k = 1; k < h; ++k)
    if (fsc[k] < thr) {
      if (k == 1) return box;
      const double s0 = (double)(k - 1) / box, s1 = (double)k / box;
      const double x = s0 + (thr - fsc[k - 1]) * (s1 - s0) / (fsc[k] - fsc[k - 1]);
      return 1.0 / x;
    }
  return 1.0 / ((double)(h - 1) / box);
}

__device__ __forceinline__ double lr_ratio(double num, double den1, double den2) {
  const double denom = sqrt(den1 * den2);
  return denom > 0.0 ? num / denom : 1.0;
}

struct LrArgs {
  const float* map1;
  const float* map2;
  const float* taper;       // [w]
  const float* tab;         // [cos w | sin w]  (LDS route)
  const int32_t* centres;   // [windows][3] z, y, x of this launch
  float* in;                // [2 windows][w^3]  (passes route)
  const double* sums;       // [windows][h][3]   (passes route)
  double* res;              // [windows]
  double* curves;           // [windows][h]
  int nz, ny, nx, w, windows;
  double apix, thr;
};

// one tapered voxel pair of the window whose corner is (z0, y0, x0); zeros outside the map
__device__ __forceinline__ void lr_voxel(const LrArgs& g, int z0, int y0, int x0, int z, int y, int x, float& a, float& b) {
  const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
  a = 0.f; b = 0.f;
  if ((unsigned)gz < (unsigned)g.nz && (unsigned)gy < (unsigned)g.ny && (unsigned)gx < (unsigned)g.nx) {
    const int64_t i = ((int64_t)gz * g.ny + gy) * g.nx + gx;
    const float t = g.taper[z] * g.taper[y] * g.taper[x];
    a = g.map1[i] * t;
    b = g.map2[i] * t;
  }
}

// passes route: grid (blocks over w^3, windows)
__global__ __launch_bounds__(256) void k_lres_gather(LrArgs g) {
  const int b = blockIdx.y, w = g.w;
  const int per = w * w * w;
  const int z0 = g.centres[b * 3 + 0] - w / 2, y0 = g.centres[b * 3 + 1] - w / 2, x0 = g.centres[b * 3 + 2] - w / 2;
  float* const o1 = g.in + (int64_t)b * per;
  float* const o2 = g.in + (int64_t)(g.windows + b) * per;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < per; e += gridDim.x * 256) {
    float a1, a2;
    lr_voxel(g, z0, y0, x0, e / (w * w), (e / w) % w, e % w, a1, a2);
    o1[e] = a1;
    o2[e] = a2;
  }
}

// passes route: one lane per window
__global__ __launch_bounds__(256) void k_lres_resolve(LrArgs g) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= g.windows) return;
  const int h = g.w / 2 + 1;
  double* const fsc = g.curves + (int64_t)b * h;
  const double* const s = g.sums + (int64_t)b * h * 3;
  for (int k = 0; k < h; ++k) fsc[k] = lr_ratio(s[k * 3], s[k * 3 + 1], s[k * 3 + 2]);
  g.res[b] = lr_resolution(fsc, g.w, g.apix, g.thr);
}

// The direct DFT of one column of W complex values held at base[t stride] (re) and base[t stride + im_off] (im), in place:
// the column is read whole into registers before its first value is written, and no other lane touches it in this pass.
template <int W>
__device__ __forceinline__ void lr_col_dft(float* base, int stride, int im_off, const float (&c)[W], const float (&s)[W]) {
  float xr[W], xi[W];
#pragma unroll
  for (int t = 0; t < W; ++t) {
    xr[t] = base[t * stride];
    xi[t] = base[t * stride + im_off];
  }
#pragma unroll
  for (int k = 0; k < W; ++k) {
    float re = 0.f, im = 0.f;
#pragma unroll
    for (int t = 0; t < W; ++t) {   // (a + i b)(c - i s) = (a c + b s) + i (b c - a s)
      const int q = (k * t) % W;
      re = fmaf(xr[t], c[q], re);
      re = fmaf(xi[t], s[q], re);
      im = fmaf(xi[t], c[q], im);
      im = fmaf(-xr[t], s[q], im);
    }
    base[k * stride] = re;
    base[k * stride + im_off] = im;
  }
}

// LDS route: one workgroup per window pair
template <int W>
__global__ __launch_bounds__(lr_threads(W)) void k_lres_lds(LrArgs g) {
  constexpr int LR_THREADS = lr_threads(W);
  constexpr int H = W / 2 + 1, RS = W + 3, MEM = W * W * RS;
  extern __shared__ double lr_smem[];
  unsigned long long* const sh = reinterpret_cast<unsigned long long*>(lr_smem);   // [3 H]
  double* const fsc = lr_smem + 3 * H;                                                // [H]
  double* const scale_s = fsc + H;                                                    // [3]
  float* const sp = reinterpret_cast<float*>(scale_s + 3);                            // [2][W][W][RS]
  float* const tc = sp + 2 * MEM;
  float* const ts = tc + W;
  unsigned* const amax = reinterpret_cast<unsigned*>(ts + W);                         // [2]
  const int tid = threadIdx.x, b = blockIdx.x;
  const int z0 = g.centres[b * 3 + 0] - W / 2, y0 = g.centres[b * 3 + 1] - W / 2, x0 = g.centres[b * 3 + 2] - W / 2;
  for (int e = tid; e < 3 * H; e += LR_THREADS) sh[e] = 0ull;
  if (tid < W) {
    tc[tid] = g.tab[tid];
    ts[tid] = g.tab[W + tid];
  }
  if (tid < 2) amax[tid] = 0u;
  __syncthreads();
  unsigned m1 = 0, m2 = 0;
  for (int e = tid; e < W * W * W; e += LR_THREADS) {
    const int z = e / (W * W), y = (e / W) % W, x = e % W;
    float a1, a2;
    lr_voxel(g, z0, y0, x0, z, y, x, a1, a2);
    sp[(z * W + y) * RS + x] = a1;
    sp[MEM + (z * W + y) * RS + x] = a2;
    m1 = max(m1, __float_as_uint(a1) & 0x7fffffffu);
    m2 = max(m2, __float_as_uint(a2) & 0x7fffffffu);
  }
  for (int off = 32; off > 0; off >>= 1) {
    m1 = max(m1, (unsigned)__shfl_down((int)m1, off, 64));
    m2 = max(m2, (unsigned)__shfl_down((int)m2, off, 64));
  }
  if ((tid & 63) == 0) {
    if (m1 != 0) atomicMax(amax + 0, m1);
    if (m2 != 0) atomicMax(amax + 1, m2);
  }
  __syncthreads();
  if (tid == 0) fc_pair_scales(amax[0], amax[1], (double)(W * W * W), scale_s);
  float c[W], s[W];
#pragma unroll
  for (int t = 0; t < W; ++t) {
    c[t] = tc[t];
    s[t] = ts[t];
  }
  // x pass: a row of W reals becomes H re | H im in the same row
  for (int r = tid; r < 2 * W * W; r += LR_THREADS) {
    float* const row = sp + r * RS;
    float x[W];
#pragma unroll
    for (int t = 0; t < W; ++t) x[t] = row[t];
#pragma unroll
    for (int k = 0; k < H; ++k) {
      float re = 0.f, im = 0.f;
#pragma unroll
      for (int t = 0; t < W; ++t) {
        const int q = (k * t) % W;
        re = fmaf(x[t], c[q], re);
        im = fmaf(-x[t], s[q], im);
      }
      row[k] = re;
      row[H + k] = im;
    }
  }
  __syncthreads();
  // y pass: the columns (member, z, kx)
  for (int col = tid; col < 2 * W * H; col += LR_THREADS) lr_col_dft<W>(sp + (col / H) * (W * RS) + col % H, RS, H, c, s);
  __syncthreads();
  // z pass: the columns (member, y, kx)
  for (int col = tid; col < 2 * W * H; col += LR_THREADS) {
    const int my = col / H;
    lr_col_dft<W>(sp + (my / W) * MEM + (my % W) * RS + col % H, W * RS, H, c, s);
  }
  __syncthreads();
  const double scale[3] = {scale_s[0], scale_s[1], scale_s[2]};
  for (int e = tid; e < W * W * H; e += LR_THREADS) {
    const int kx = e % H, ky = (e / H) % W, kz = e / (H * W);
    const float* const p = sp + (kz * W + ky) * RS + kx;
    const double wgt = (kx != 0 && 2 * kx != W) ? 2.0 : 1.0;
    fc_add_products(&sh[fc_shell_3d(kz, ky, kx, W) * 3], wgt, p[0], p[H], p[MEM], p[MEM + H], scale);
  }
  __syncthreads();
  if (tid < H) {
    double v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = scale[q] == 0.0 ? 0.0 : (double)(long long)sh[tid * 3 + q] / scale[q];   // k_fc_finish's rule
    fsc[tid] = lr_ratio(v[0], v[1], v[2]);
  }
  __syncthreads();
  if (tid == 0) g.res[b] = lr_resolution(fsc, W, g.apix, g.thr);
  if (g.curves && tid < H) g.curves[(int64_t)b * H + tid] = fsc[tid];
}

struct LrUp {
  const double* grid;   // [gz][gy][gx]
  float* out;           // [nz][ny][nx]
  int gz, gy, gx, step, nz, ny, nx;
};

// one axis of the trilinear rule: u = clip((p - step / 2) / step, 0, g - 1), i0 = min(floor(u), g - 2); g == 1: corner 0 alone
__device__ __forceinline__ void lr_axis(int p, int step, int g, int& i0, double& f) {
  if (g == 1) {
    i0 = 0; f = 0.0;
    return;
  }
  double u = ((double)p - (double)(step / 2)) / (double)step;
  u = u < 0.0 ? 0.0 : (u > (double)(g - 1) ? (double)(g - 1) : u);
  i0 = min((int)floor(u), g - 2);
  f = u - (double)i0;
}

__global__ __launch_bounds__(256) void k_lres_upsample(LrUp g) {
  const int64_t total = (int64_t)g.nz * g.ny * g.nx;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % g.nx), y = (int)((i / g.nx) % g.ny), z = (int)(i / ((int64_t)g.nx * g.ny));
    int iz, iy, ix;
    double fz, fy, fx;
    lr_axis(z, g.step, g.gz, iz, fz);
    lr_axis(y, g.step, g.gy, iy, fy);
    lr_axis(x, g.step, g.gx, ix, fx);
    double acc = 0.0, wsum = 0.0;
    for (int dz = 0; dz < (g.gz == 1 ? 1 : 2); ++dz)
      for (int dy = 0; dy < (g.gy == 1 ? 1 : 2); ++dy)
        for (int dx = 0; dx < (g.gx == 1 ? 1 : 2); ++dx) {
          const double v = g.grid[((int64_t)(iz + dz) * g.gy + (iy + dy)) * g.gx + (ix + dx)];
          if (v != v) continue;   // an unevaluated corner
          const double wt = (dz ? fz : 1.0 - fz) * (dy ? fy : 1.0 - fy) * (dx ? fx : 1.0 - fx);
          acc += wt * v;
          wsum += wt;
        }
    g.out[i] = wsum > 0.0 ? (float)(acc / wsum) : __uint_as_float(0x7fc00000u);
  }
}

// Host arithmetic of a run: the route that is taken, the LDS route's bytes per workgroup (also when the passes route is
// taken, 0 above its largest window) and the windows of one launch under a budget (0 = the defaults).
struct LrPlan {
  int route = 0;   // 1 = LDS, 2 = passes
  int64_t lds_bytes = 0, windows_per_launch = 0;
};

const char* lr_plan(int w, int route, int64_t scratch_bytes, int64_t max_windows, LrPlan& p) {
  if (w < LR_MIN_W || w > LR_MAX_W || (w & 1)) return "the window must be even and lie in [8, 64]";
  if (route < 0 || route > 2) return "route must be 0 (automatic), 1 (LDS) or 2 (passes)";
  if (route == 1 && w > LR_MAX_LDS_W) return "the LDS route takes windows up to 24";
  if (scratch_bytes < 0 || max_windows < 0) return "a budget must be >= 0";
  p.route = route != 0 ? route : (w <= LR_MAX_LDS_W ? 1 : 2);
  p.lds_bytes = w <= LR_MAX_LDS_W ? lr_lds_bytes(w) : 0;
  if (p.route == 1) {
    p.windows_per_launch = LR_LDS_WINDOWS;
  } else {
    FcPlan q;   // fc_chunk reads the shape only
    q.cube = true;
    q.nz = q.ny = q.nx = w;
    q.per_map = (int64_t)w * w * w;
    p.windows_per_launch = fc_chunk(q, INT64_MAX);
    if (scratch_bytes > 0) p.windows_per_launch = std::min(p.windows_per_launch, std::max<int64_t>(1, scratch_bytes / (10 * q.per_map * (int64_t)sizeof(float))));
  }
  if (max_windows > 0) p.windows_per_launch = std::min(p.windows_per_launch, max_windows);
  return nullptr;
}

template <int W>
int lr_launch_lds(hh_lres* c, const LrArgs& a, int64_t bytes) {
  const void* fn = reinterpret_cast<const void*>(&k_lres_lds<W>);
  bool set = false;
  for (auto& e : c->lds_attr) set = set || e.first == fn;
  if (!set) {
    HH_HIP(nullptr, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    c->lds_attr.emplace_back(fn, (int)bytes);
  }
  hipLaunchKernelGGL(k_lres_lds<W>, dim3((unsigned)a.windows), dim3(lr_threads(W)), (size_t)bytes, nullptr, a);
  return HH_OK;
}

int lr_run(hh_lres* c, int w, const float* taper, const int32_t* centres, int64_t n, double apix, double thr, const LrPlan& p,
           double* res, double* curves, double* kernel_ms) {
  const int h = w / 2 + 1;
  const int64_t per = (int64_t)w * w * w, chunk = std::min(p.windows_per_launch, n);
  const int64_t per_map = (int64_t)c->nz * c->ny * c->nx;
  HH_HIP(nullptr, hipSetDevice(c->device));
  HH_HIP(nullptr, c->fc.ev.create());
  if (int rc = ensure(nullptr, c->taper, (size_t)w)) return rc;
  if (int rc = ensure(nullptr, c->centres, (size_t)n * 3)) return rc;
  if (int rc = ensure(nullptr, c->res, (size_t)chunk)) return rc;
  if (int rc = ensure(nullptr, c->curves, (size_t)chunk * h)) return rc;
  HH_HIP(nullptr, hipMemcpy(c->taper, taper, (size_t)w * sizeof(float), hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipMemcpy(c->centres, centres, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice));
  if (p.route == 1 && c->tab_w != w) {
    std::vector<double> cs, sn;
    unit_circle(w, cs, sn);
    std::vector<float> tab((size_t)2 * w);
    for (int t = 0; t < w; ++t) {
      tab[(size_t)t] = (float)cs[(size_t)t];
      tab[(size_t)(w + t)] = (float)sn[(size_t)t];
    }
    if (int rc = ensure(nullptr, c->tab, tab.size())) return rc;
    HH_HIP(nullptr, hipMemcpy(c->tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    c->tab_w = w;
  }
  if (p.route == 2) {
    if (c->plan_w != w) {   // another window: the scratch and the operators of the old one go first
      c->fc.release();
      c->plan = FcPlan();
      c->plan_w = 0;
      fc_plan(c->plan, w, w, w);
      if (int rc = ensure(nullptr, c->fc.mats, c->plan.mats.size())) return rc;
      HH_HIP(nullptr, hipMemcpy(c->fc.mats, c->plan.mats.data(), c->plan.mats.size() * sizeof(float), hipMemcpyHostToDevice));
      c->plan_w = w;
    }
    if (int rc = c->fc.reserve(chunk, per, h, true, true)) return rc;
  }
  LrArgs a{};
  a.map1 = c->maps; a.map2 = c->maps + per_map;
  a.taper = c->taper; a.tab = c->tab;
  a.res = c->res; a.curves = c->curves;
  a.nz = c->nz; a.ny = c->ny; a.nx = c->nx; a.w = w;
  a.apix = apix; a.thr = thr;
  double ms_total = 0.0;
  for (int64_t b0 = 0; b0 < n; b0 += chunk) {
    const int64_t nb = std::min(chunk, n - b0);
    a.centres = c->centres + b0 * 3;
    a.windows = (int)nb;
    HH_HIP(nullptr, hipEventRecord(c->fc.ev[0], nullptr));
    if (p.route == 1) {
      int rc = HH_OK;
      switch (w) {
        case 8: rc = lr_launch_lds<8>(c, a, p.lds_bytes); break;
        case 10: rc = lr_launch_lds<10>(c, a, p.lds_bytes); break;
        case 12: rc = lr_launch_lds<12>(c, a, p.lds_bytes); break;
        case 14: rc = lr_launch_lds<14>(c, a, p.lds_bytes); break;
        case 16: rc = lr_launch_lds<16>(c, a, p.lds_bytes); break;
        case 18: rc = lr_launch_lds<18>(c, a, p.lds_bytes); break;
        case 20: rc = lr_launch_lds<20>(c, a, p.lds_bytes); break;
        case 22: rc = lr_launch_lds<22>(c, a, p.lds_bytes); break;
        case 24: rc = lr_launch_lds<24>(c, a, p.lds_bytes); break;
        default: return fail(nullptr, HH_ERR_ARG, "hh_lres_run: the LDS route takes even windows in [8, 24]");
      }
      if (rc) return rc;
    } else {
      a.in = c->fc.in;
      a.sums = c->fc.sums;
      hipLaunchKernelGGL(k_lres_gather, dim3((unsigned)std::min<int64_t>((per + 255) / 256, 64), (unsigned)nb), dim3(256), 0, nullptr, a);
      fc_device(c->plan, c->fc.in, c->fc, nb, h, true);
      hipLaunchKernelGGL(k_lres_resolve, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, nullptr, a);
    }
    HH_HIP(nullptr, hipGetLastError());
    HH_HIP(nullptr, hipEventRecord(c->fc.ev[1], nullptr));
    HH_HIP(nullptr, hipMemcpy(res + b0, c->res, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost));
    if (curves) HH_HIP(nullptr, hipMemcpy(curves + b0 * h, c->curves, (size_t)nb * h * sizeof(double), hipMemcpyDeviceToHost));
    float ms = 0.f;
    HH_HIP(nullptr, hipEventElapsedTime(&ms, c->fc.ev[0], c->fc.ev[1]));
    ms_total += ms;
  }
  if (kernel_ms) *kernel_ms = ms_total;
  return HH_OK;
}

}  // namespace

extern "C" int hh_lres_create(hh_lres** out, int device, const float* map1, const float* map2, int32_t nz, int32_t ny, int32_t nx) try {
  if (!out) return fail(nullptr, HH_ERR_ARG, "hh_lres_create: NULL argument");
  *out = nullptr;
  if (!map1 || !map2) return fail(nullptr, HH_ERR_ARG, "hh_lres_create: NULL argument");
  if (nz < 8 || nz > 512 || ny < 8 || ny > 512 || nx < 8 || nx > 512) return fail(nullptr, HH_ERR_ARG, "hh_lres_create: every side of the maps must lie in [8, 512]");
  if (int rc = use_device("hh_lres_create", device)) return rc;
  std::unique_ptr<hh_lres> c(new hh_lres);
  c->device = device; c->nz = nz; c->ny = ny; c->nx = nx;
  const size_t per_map = (size_t)nz * ny * nx;
  if (int rc = ensure(nullptr, c->maps, 2 * per_map)) return rc;
  HH_HIP(nullptr, hipMemcpy(c->maps, map1, per_map * sizeof(float), hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipMemcpy(c->maps + per_map, map2, per_map * sizeof(float), hipMemcpyHostToDevice));
  *out = c.release();
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_lres_create")

extern "C" int hh_lres_destroy(hh_lres* ctx) try {
  delete ctx;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_lres_destroy")

extern "C" int hh_lres_set_budget(hh_lres* ctx, int64_t scratch_bytes, int64_t max_windows_per_launch) try {
  if (!ctx) return fail(nullptr, HH_ERR_ARG, "hh_lres_set_budget: NULL argument");
  if (scratch_bytes < 0 || max_windows_per_launch < 0) return fail(nullptr, HH_ERR_ARG, "hh_lres_set_budget: a budget must be >= 0 (0: the default)");
  ctx->scratch_bytes = scratch_bytes;
  ctx->max_windows = max_windows_per_launch;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_lres_set_budget")

extern "C" int hh_lres_plan(int32_t window, int route, int64_t scratch_bytes, int64_t max_windows_per_launch, int32_t* route_out,
                            int64_t* lds_bytes, int64_t* windows_per_launch) try {
  LrPlan p;
  if (const char* why = lr_plan(window, route, scratch_bytes, max_windows_per_launch, p)) return fail(nullptr, HH_ERR_ARG, std::string("hh_lres_plan: ") + why);
  if (route_out) *route_out = p.route;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  if (windows_per_launch) *windows_per_launch = p.windows_per_launch;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_lres_plan")

extern "C" int hh_lres_run(hh_lres* ctx, int32_t window, const float* taper, const int32_t* centres, int64_t n, double apix, double threshold,
                           int route, double* resolution, double* curves, double* kernel_ms) try {
  if (!ctx || !taper || !centres || !resolution) return fail(nullptr, HH_ERR_ARG, "hh_lres_run: NULL argument");
  LrPlan p;   // what needs no context is checked before the context is read
  if (const char* why = lr_plan(window, route, 0, 0, p)) return fail(nullptr, HH_ERR_ARG, std::string("hh_lres_run: ") + why);
  if (n < 1 || n > INT32_MAX / 3) return fail(nullptr, HH_ERR_ARG, "hh_lres_run: the number of windows must lie in [1, 2^31 / 3)");
  if (!(apix > 0.0) || apix > 1.7e308) return fail(nullptr, HH_ERR_ARG, "hh_lres_run: apix must be positive and finite");
  if (!(threshold > -1.0 && threshold < 1.0)) return fail(nullptr, HH_ERR_ARG, "hh_lres_run: the threshold must lie in (-1, 1)");
  const int32_t side[3] = {ctx->nz, ctx->ny, ctx->nx};
  for (int64_t i = 0; i < n * 3; ++i)
    if (centres[i] < 0 || centres[i] >= side[i % 3]) return fail(nullptr, HH_ERR_ARG, "hh_lres_run: a centre lies outside the map");
  if (const char* why = lr_plan(window, route, ctx->scratch_bytes, ctx->max_windows, p)) return fail(nullptr, HH_ERR_ARG, std::string("hh_lres_run: ") + why);
  return lr_run(ctx, window, taper, centres, n, apix, threshold, p, resolution, curves, kernel_ms);
} HH_CATCH_CTX(nullptr, "hh_lres_run")

extern "C" int hh_lres_upsample(int device, const double* grid, int32_t gz, int32_t gy, int32_t gx, int32_t step, int32_t nz, int32_t ny,
                                int32_t nx, float* out) try {
  if (!grid || !out) return fail(nullptr, HH_ERR_ARG, "hh_lres_upsample: NULL argument");
  if (step < 1) return fail(nullptr, HH_ERR_ARG, "hh_lres_upsample: step must be >= 1");
  if (nz < 1 || nz > 512 || ny < 1 || ny > 512 || nx < 1 || nx > 512) return fail(nullptr, HH_ERR_ARG, "hh_lres_upsample: every side of the map must lie in [1, 512]");
  if (gz < 1 || gz > nz || gy < 1 || gy > ny || gx < 1 || gx > nx) return fail(nullptr, HH_ERR_ARG, "hh_lres_upsample: every side of the grid must lie in [1, the map's]");
  if (int rc = use_device("hh_lres_upsample", device)) return rc;
  const size_t cells = (size_t)gz * gy * gx, voxels = (size_t)nz * ny * nx;
  DevArena arena;
  double* const d_grid = arena.get<double>(cells);
  float* const d_out = arena.get<float>(voxels);
  if (!arena.ok()) return fail(nullptr, HH_ERR_NOMEM, "hh_lres_upsample: " + dev_alloc_failed(arena.failed_bytes()));
  HH_HIP(nullptr, hipMemcpy(d_grid, grid, cells * sizeof(double), hipMemcpyHostToDevice));
  LrUp u{d_grid, d_out, gz, gy, gx, step, nz, ny, nx};
  hipLaunchKernelGGL(k_lres_upsample, dim3((unsigned)std::min<size_t>((voxels + 255) / 256, 65536)), dim3(256), 0, nullptr, u);
  HH_HIP(nullptr, hipGetLastError());
  HH_HIP(nullptr, hipMemcpy(out, d_out, voxels * sizeof(float), hipMemcpyDeviceToHost));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_lres_upsample")
