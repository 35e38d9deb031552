// symmetry_search.inc — real-space helical symmetry search of a 3-D map: for every candidate (twist, rise, Csym) the score
//     Pearson(V[M], S[M]),   S = apply_helical_symmetry(V, apix, twist, rise, csym, fraction, new_size = V.shape, new_apix = apix)
// over a scored region M (a shell of radii about the axis x a slab of central planes), for a whole list of candidates, with
// the map resident on the device (struct hh_hs) and S never stored.  k_apply_helical_symmetry (helicon_hip.hip) is the
// operator for ONE candidate and is pinned bit for bit; this file is held to a score tolerance instead, which frees the
// arithmetic:
//   * one workgroup per (candidate, output plane k of M, tile of at most HS_TILE in-plane voxels of M).  Everything that is uniform
//     over a plane — for repeat hi: k2 = ((k - nz/2) apix + hi rise) / apix + nz/2, the test z0 <= k2 < z1 that decides
//     whether the repeat counts, floor / ceil / weight, and cos / sin of twist hi + 360 ci / csym — is worked out ONCE per
//     workgroup, one (hi, ci) pair per lane, in float64 with the reference's own expressions (contraction off; cos / sin
//     of np.deg2rad's radians), and handed to the voxels through LDS.  Only the window of hi that
//     can pass the z test is visited (about (z1 - z0) apix / rise of the 2 hmax + 1 repeats; the window is widened by one
//     repeat on each side and every entry is tested exactly, so the estimate decides nothing).
//   * per voxel and live pair the in-plane position is the rotation of (j - ny/2, i - nx/2.0) in float32, RELATIVE TO THE
//     AXIS: dj = c jj + s ii, di = c ii - s jj with |dj|, |di| < 1.5 * 1024.  floor and the weights are taken on dj / di
//     before the integer centre is added, so the centre costs no bits, and the bounds test of the reference,
//     floor(j2) in [0, ny - 2], becomes -ny/2 <= floor(dj) <= ny - 2 - ny/2: a comparison of an integer-valued float with
//     integers, exact.  It can therefore differ from the float64 test only where the exact dj lies within the rounding of
//     the float32 dj (3 roundings of values below 1.5 n) of a border.  Those samples are NOT rare on a lattice: a repeat
//     that turns the grid onto itself (twist 30 degrees, every third repeat) puts whole border rows exactly on the
//     border, where the reference's verdict is the sign of its own cos / sin rounding.  So a sample within `edge`
//     (8 ulp of 1.5 n) of a border is decided by hs_border: the reference's float64 expression itself.  Whatever is
//     decided, the four taps jf, jf + 1, if, if + 1 lie inside the plane.  The tap jf + 1 stands for ceil(j2): where they
//     differ the weight of the tap is 0.
//   * the candidate's sum S V, S S, S S^2 over the workgroup's voxels goes to one float64 triple per workgroup
//     (fixed-shape shuffle tree + LDS), k_hs_finalize adds a candidate's triples in index order and writes the score.  No
//     atomics: a score depends on the candidate and the region alone, not on the list around it or on how the list is cut
//     into launches (by a byte budget for the triples, hh_hs_set_budget).
// The map-side sums over M are taken once per region by k_hs_map_moments in the same shape.

struct hh_hs {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int nz = 0, ny = 0, nx = 0;
  double apix = 0, fraction = 1;
  int z0 = 0, z1 = 0;            // source planes the operator reads: [z0, z1) (the 1 % profile rule and `fraction`)
  DevBuf<float> d_map;
  // the scored region
  DevBuf<int32_t> d_vox;         // in-plane voxels of M, (j << 16) | i, row-major order
  int np = 0, kz0 = 0, nplanes = 0, ntiles = 0, nv = 0;
  int64_t region_voxels = 0;
  double sum_v = 0, sum_vv = 0;  // over M
  double rmin = 0, rmax = -1, z_fraction = 0.5;
  // work buffers, grown on demand
  DevBuf<double> d_part;         // the triples of the candidates of one launch
  DevBuf<double> d_params;       // the candidate list and its scores
  DevBuf<float> d_scores;
  int64_t budget = (int64_t)64 << 20;                  // bytes of triples per launch
  double kernel_ms = 0;
  int64_t launches = 0;
  std::string err;
};

namespace {

constexpr int HS_VPT = 8;                 // voxels per lane, at most
constexpr int HS_TILE = 256 * HS_VPT;     // in-plane voxels per workgroup, at most (hs_set_region balances the tiles)
constexpr int HS_MAX_CSYM = 4096;
constexpr double HS_MAX_REPEATS = 1.0e8;  // nz apix / rise above this is refused (hmax stays far inside int32)

int hs_fail(hh_hs* p, int code, const std::string& msg) {
  if (p) p->err = msg; else g_create_error = msg;
  return code;
}
#define HH_CATCH_HS(p, fn) catch (...) { return hh_caught([&](int code, const std::string& m) { return hs_fail(const_cast<hh_hs*>(static_cast<const hh_hs*>(p)), code, m); }, fn); }
#define HS_HIP(p, call)                                                                                \
  do {                                                                                                 \
    hipError_t e__ = (call);                                                                           \
    if (e__ != hipSuccess) return hs_fail(p, HH_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

struct HsArgs {
  const float* map;       // [nz][ny][nx]
  const int32_t* vox;     // [np] (j << 16) | i
  const double* params;   // [candidates of this launch][3] twist (degrees), rise (Angstrom), csym
  double* part;           // [candidate][plane][tile][3] = sum S, sum S^2, sum V S
  int nz, ny, nx, np, kz0, ntiles, z0, z1;
  int nv;                 // voxels per lane in this region: a tile is 256 nv consecutive entries of vox
  double apix;
};

// sum of v over the 256 lanes of the workgroup in a fixed order (shuffle tree per wavefront, then the four wavefronts in
// index order); the result is valid in thread 0.  `slot` is LDS for 4 doubles.
__device__ __forceinline__ double hs_block_sum(double v, double* slot) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

// one (repeat, cyclic copy) of plane k: what the reference computes in float64 before its (j, i) loops (transforms.py:105-
// 116).  Returns false when the repeat's source plane lies outside [z0, z1).
__device__ __forceinline__ bool hs_stage(int k, long long hi, int ci, int csym, double twist, double rise, const HsArgs& a, float4& ent,
                                         int& kf_out, double2& cs64) {
#pragma clang fp contract(off)
  const double k2 = ((double)(k - a.nz / 2) * a.apix + (double)hi * rise) / a.apix + (double)(a.nz / 2);
  if (k2 < (double)a.z0 || k2 >= (double)a.z1) return false;
  const double kf = floor(k2);
  const double wk = k2 - kf;
  // np.deg2rad, then cos / sin of the radians: NOT sincospi of the half turns, whose exact 0 at a quarter turn is not what
  // the reference multiplies by (cos(3 pi / 2) = -1.8e-16 there), and on a border that difference decides (hs_border)
  const double rot = (twist * (double)hi + 360.0 * (double)ci / (double)csym) * (M_PI / 180.0);
  const double c = cos(rot), s = sin(rot);
  cs64 = make_double2(c, s);
  ent = make_float4((float)c, (float)s, (float)wk, 0.f);
  kf_out = 2 * (int)kf + (wk > 0.0 ? 1 : 0);   // ceil(k2) = kf + 1 unless k2 is whole; kf + 1 <= z1 <= nz - 1 then
  return true;
}

// A sample whose float32 position lies within the rounding of that position (HS_EDGE_ULPS) of a border of the admitted
// range: the reference's own float64 expression (transforms.py:117-121, contraction off) decides whether it counts, and
// gives floor and weight when it does.  Whole rows and columns of the border land here when a repeat turns the grid onto
// itself (a twist of 30 degrees does at every third repeat): the exact position is ON the border then, and the
// reference's verdict is the sign of its cos / sin rounding.  Elsewhere this is never called.
__device__ __forceinline__ bool hs_border(double2 cs, float jjf, float iif, int ny, int nx, double apix, float& fj, float& fi, float& wj,
                                          float& wi) {
#pragma clang fp contract(off)
  const double jj = (double)jjf, ii = (double)iif;
  const double j2 = (cs.x * jj + cs.y * ii) * apix / apix + (double)(ny / 2);
  const double i2 = ((-cs.y) * jj + cs.x * ii) * apix / apix + (double)(nx / 2);
  const double j2f = floor(j2), i2f = floor(i2);
  if (j2f < 0.0 || j2f >= (double)(ny - 1) || i2f < 0.0 || i2f >= (double)(nx - 1)) return false;
  fj = (float)(j2f - (double)(ny / 2)); fi = (float)(i2f - (double)(nx / 2));
  wj = (float)(j2 - j2f); wi = (float)(i2 - i2f);
  return true;
}

constexpr float HS_EDGE_ULPS = 8.f;   // the float32 position c jj + s ii carries at most 3 roundings of values below 1.5 n

__global__ __launch_bounds__(256) void k_hs_score(HsArgs a) {
  __shared__ float4 s_ent[256];
  __shared__ double2 s_cs[256];
  __shared__ int s_kf[256];
  __shared__ double s_red[3][4];
  const int tid = threadIdx.x, kp = blockIdx.x, tile = blockIdx.y, g = blockIdx.z;   // planes fastest: neighbours in the
  const int k = a.kz0 + kp;                                                          // dispatch order read shifted source planes
  const double twist = a.params[3 * (size_t)g], rise = a.params[3 * (size_t)g + 1];
  const int csym = (int)a.params[3 * (size_t)g + 2];
  const long long hmax = max(1LL, (long long)((double)a.nz * a.apix / rise));   // transforms.py:88
  // window of repeats whose source plane can lie in [z0, z1): widened by one, every entry tested exactly in hs_stage
  const double kk = (double)(k - a.nz / 2), zc = (double)(a.nz / 2);
  long long hi_a = (long long)floor(((double)a.z0 - zc - kk) * a.apix / rise) - 1;
  long long hi_b = (long long)ceil(((double)a.z1 - zc - kk) * a.apix / rise) + 1;
  hi_a = max(hi_a, -hmax);
  hi_b = min(hi_b, hmax);
  const long long n_ent = hi_b >= hi_a ? (hi_b - hi_a + 1) * (long long)csym : 0;

  const int cy = a.ny / 2, cx = a.nx / 2;
  const float half_nx = (float)a.nx * 0.5f;   // the reference centres columns on nx / 2, rows on ny // 2 (transforms.py:117-121)
  const float jlo = (float)(-cy), jhi = (float)(a.ny - 2 - cy), ilo = (float)(-cx), ihi = (float)(a.nx - 2 - cx);
  const float edge = HS_EDGE_ULPS * 1.1920929e-7f * 1.5f * (float)max(a.ny, a.nx);   // width of the band hs_border decides
  float jj[HS_VPT], ii[HS_VPT], acc[HS_VPT], cnt[HS_VPT];
  int self[HS_VPT];   // offset of the voxel in its plane, -1 past the end of the list
#pragma unroll
  for (int v = 0; v < HS_VPT; ++v) {
    const int p = (tile * a.nv + v) * 256 + tid;
    acc[v] = 0.f; cnt[v] = 0.f; jj[v] = 0.f; ii[v] = 0.f; self[v] = -1;
    if (v < a.nv && p < a.np) {
      const int w = a.vox[p], j = w >> 16, i = w & 0xffff;
      jj[v] = (float)(j - cy);
      ii[v] = (float)i - half_nx;
      self[v] = j * a.nx + i;
    }
  }
  const size_t plane = (size_t)a.ny * a.nx;
  for (long long e0 = 0; e0 < n_ent; e0 += 256) {
    __syncthreads();   // the previous chunk has been read
    {
      const long long e = e0 + tid;
      float4 ent = make_float4(0.f, 0.f, 0.f, 0.f);
      int kf = -1;
      double2 cs64 = make_double2(0.0, 0.0);
      if (e < n_ent && !hs_stage(k, hi_a + e / csym, (int)(e % csym), csym, twist, rise, a, ent, kf, cs64)) kf = -1;
      s_ent[tid] = ent;
      s_cs[tid] = cs64;
      s_kf[tid] = kf;
    }
    __syncthreads();
    const int n = (int)min(256LL, n_ent - e0);
    for (int t = 0; t < n; ++t) {   // the reference's order: repeats ascending, cyclic copies within a repeat
      const int kf2 = s_kf[t];
      if (kf2 < 0) continue;        // uniform over the workgroup
      const float4 ent = s_ent[t];
      const float c = ent.x, s = ent.y, wk = ent.z;
      const float* const d0 = a.map + (size_t)(kf2 >> 1) * plane;
      const float* const d1 = d0 + (size_t)(kf2 & 1) * plane;
#pragma unroll
      for (int v = 0; v < HS_VPT; ++v) {
        if (v >= a.nv) break;   // uniform
        const float dj = c * jj[v] + s * ii[v], di = c * ii[v] - s * jj[v];
        float fj = floorf(dj), fi = floorf(di);
        float wj = dj - fj, wi = di - fi;
        bool ok = fj >= jlo && fj <= jhi && fi >= ilo && fi <= ihi;   // floor(j2) in [0, ny - 2], floor(i2) in [0, nx - 2]
        // distance to the nearest border of [0, ny - 1) x [0, nx - 1), relative to the axis: jlo, jhi + 1, ilo, ihi + 1
        const float near = fminf(fminf(fabsf(dj - jlo), fabsf(dj - (jhi + 1.f))), fminf(fabsf(di - ilo), fabsf(di - (ihi + 1.f))));
        if (near < edge) ok = hs_border(s_cs[t], jj[v], ii[v], a.ny, a.nx, a.apix, fj, fi, wj, wi);
        if (ok) {
          const int off = ((int)fj + cy) * a.nx + ((int)fi + cx);
          const float* const p0 = d0 + off;
          const float* const p1 = d1 + off;
          const float a00 = p0[0], a01 = p0[1], a10 = p0[a.nx], a11 = p0[a.nx + 1];
          const float b00 = p1[0], b01 = p1[1], b10 = p1[a.nx], b11 = p1[a.nx + 1];
          const float a0 = a00 + wi * (a01 - a00), a1 = a10 + wi * (a11 - a10);
          const float b0 = b00 + wi * (b01 - b00), b1 = b10 + wi * (b11 - b10);
          const float va = a0 + wj * (a1 - a0), vb = b0 + wj * (b1 - b0);
          acc[v] += va + wk * (vb - va);
          cnt[v] += 1.f;
        }
      }
    }
  }
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
  for (int v = 0; v < HS_VPT; ++v)
    if (self[v] >= 0) {
      const double sv = cnt[v] > 0.f ? (double)(acc[v] / cnt[v]) : 0.0;   // the average over the operations that contributed
      const double mv = (double)a.map[(size_t)k * plane + self[v]];
      s1 += sv; s2 += sv * sv; s3 += mv * sv;
    }
  __syncthreads();
  s1 = hs_block_sum(s1, s_red[0]);
  s2 = hs_block_sum(s2, s_red[1]);
  s3 = hs_block_sum(s3, s_red[2]);
  if (tid == 0) {
    double* const out = a.part + (((size_t)g * gridDim.x + kp) * a.ntiles + tile) * 3;
    out[0] = s1; out[1] = s2; out[2] = s3;
  }
}

// sum V, sum V^2 over the region: one pair per (plane, tile), added on the host in index order
__global__ __launch_bounds__(256) void k_hs_map_moments(HsArgs a) {
  __shared__ double s_red[2][4];
  const int tid = threadIdx.x, tile = blockIdx.x, kp = blockIdx.y;
  const size_t plane = (size_t)a.ny * a.nx;
  double s1 = 0.0, s2 = 0.0;
  for (int v = 0; v < a.nv; ++v) {
    const int p = (tile * a.nv + v) * 256 + tid;
    if (p < a.np) {
      const int w = a.vox[p];
      const double mv = (double)a.map[(size_t)(a.kz0 + kp) * plane + (size_t)(w >> 16) * a.nx + (w & 0xffff)];
      s1 += mv; s2 += mv * mv;
    }
  }
  s1 = hs_block_sum(s1, s_red[0]);
  s2 = hs_block_sum(s2, s_red[1]);
  if (tid == 0) {
    double* const out = a.part + ((size_t)kp * a.ntiles + tile) * 2;
    out[0] = s1; out[1] = s2;
  }
}

// one workgroup per candidate: its triples in index order (lane t takes t, t + 256, ...; then the fixed tree), then
// Pearson from the five sums in float64.  "No variance" (score 0, as cross_correlation_coefficient's norm == 0) is a
// variance below 1e-12 of the raw second moment: what float64 rounding of the one-pass form leaves of an exact zero.
__global__ __launch_bounds__(256) void k_hs_finalize(const double* __restrict__ part, int64_t n_part, double sum_v, double sum_vv,
                                                     double n_vox, float* __restrict__ scores) {
  __shared__ double s_red[3][4];
  const double* const p = part + (size_t)blockIdx.x * n_part * 3;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int64_t q = threadIdx.x; q < n_part; q += 256) {
    s1 += p[3 * q]; s2 += p[3 * q + 1]; s3 += p[3 * q + 2];
  }
  s1 = hs_block_sum(s1, s_red[0]);
  s2 = hs_block_sum(s2, s_red[1]);
  s3 = hs_block_sum(s3, s_red[2]);
  if (threadIdx.x == 0) {
    const double var_v = sum_vv - sum_v * sum_v / n_vox, var_s = s2 - s1 * s1 / n_vox;
    const double cov = s3 - sum_v * s1 / n_vox;
    float r = 0.f;
    if (var_v > 1e-12 * sum_vv && var_s > 1e-12 * s2) r = (float)(cov / sqrt(var_v * var_s));
    scores[blockIdx.x] = r;
  }
}

void hs_free_region(hh_hs* p) {
  p->d_vox.reset();
  p->d_part.reset();
  p->np = p->nplanes = p->ntiles = p->nv = 0;
  p->region_voxels = 0;
}

HsArgs hs_args(const hh_hs* p) {
  HsArgs a{};
  a.map = p->d_map; a.vox = p->d_vox;
  a.nz = p->nz; a.ny = p->ny; a.nx = p->nx; a.np = p->np; a.kz0 = p->kz0; a.ntiles = p->ntiles; a.z0 = p->z0; a.z1 = p->z1;
  a.nv = p->nv;
  a.apix = p->apix;
  return a;
}

int hs_set_region(hh_hs* p, double rmin, double rmax, double z_fraction) {
  if (!(rmin >= 0) || std::isnan(rmax) || !(z_fraction > 0))
    return hs_fail(p, HH_ERR_ARG, "hh_hs_set_region: rmin must be >= 0, rmax a number (< 0: no outer limit), z_fraction > 0");
  HS_HIP(p, hipSetDevice(p->device));
  HS_HIP(p, hipStreamSynchronize(p->stream));
  hs_free_region(p);
  p->rmin = rmin; p->rmax = rmax; p->z_fraction = z_fraction;
  // M = { rmin^2 <= (j - ny//2)^2 + (i - nx//2)^2 < rmax^2, -h <= k - nz//2 < h }
  std::vector<int32_t> vox;
  const int cy = p->ny / 2, cx = p->nx / 2;
  for (int j = 0; j < p->ny; ++j)
    for (int i = 0; i < p->nx; ++i) {
      const double r2 = (double)((int64_t)(j - cy) * (j - cy) + (int64_t)(i - cx) * (i - cx));
      if (r2 >= rmin * rmin && (rmax < 0 || r2 < rmax * rmax)) vox.push_back((int32_t)((j << 16) | i));
    }
  int k0 = 0, k1 = p->nz;
  if (z_fraction < 1) {
    const int h = std::max(1, (int)((double)p->nz * z_fraction + 0.5) / 2);
    k0 = std::max(0, p->nz / 2 - h);
    k1 = std::min(p->nz, p->nz / 2 + h);
  }
  if (vox.empty() || k1 <= k0) return hs_fail(p, HH_ERR_ARG, "hh_hs_set_region: the region holds no voxel");
  p->np = (int)vox.size(); p->kz0 = k0; p->nplanes = k1 - k0;
  p->ntiles = (p->np + HS_TILE - 1) / HS_TILE;
  p->nv = ((p->np + p->ntiles - 1) / p->ntiles + 255) / 256;   // the fewest tiles, then equal shares: no nearly empty last tile
  p->ntiles = (p->np + 256 * p->nv - 1) / (256 * p->nv);
  p->region_voxels = (int64_t)p->np * p->nplanes;
  const size_t n_part = (size_t)p->nplanes * p->ntiles;
  DevArena mem;
  double* d_mom = mem.get<double>(n_part * 2);
  if (!mem.ok() || !p->d_vox.ensure(vox.size())) {
    hs_free_region(p);
    return hs_fail(p, HH_ERR_NOMEM, "hh_hs_set_region: " + dev_alloc_failed(mem.ok() ? vox.size() * sizeof(int32_t) : mem.failed_bytes()));
  }
  hipError_t e = hipMemcpyAsync(p->d_vox, vox.data(), vox.size() * sizeof(int32_t), hipMemcpyHostToDevice, p->stream);
  std::vector<double> mom(n_part * 2);
  if (e == hipSuccess) {
    HsArgs a = hs_args(p);
    a.part = d_mom;
    hipLaunchKernelGGL(k_hs_map_moments, dim3((unsigned)p->ntiles, (unsigned)p->nplanes), dim3(256), 0, p->stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(mom.data(), d_mom, mom.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
  if (e != hipSuccess) {
    hs_free_region(p);
    return hs_fail(p, HH_ERR_HIP, std::string("hh_hs_set_region: ") + hipGetErrorString(e));
  }
  p->sum_v = p->sum_vv = 0;
  for (size_t q = 0; q < n_part; ++q) { p->sum_v += mom[2 * q]; p->sum_vv += mom[2 * q + 1]; }
  return HH_OK;
}

}  // namespace

extern "C" {

const char* hh_hs_last_error(const hh_hs* p) { return p ? p->err.c_str() : g_create_error.c_str(); }

void hh_hs_destroy(hh_hs* p) try {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->ev0) (void)hipEventDestroy(p->ev0);
  if (p->ev1) (void)hipEventDestroy(p->ev1);
  const hipStream_t stream = p->stream;
  delete p;                                   // frees the device buffers: before their stream goes
  if (stream) (void)hipStreamDestroy(stream);
} catch (...) {
}

int hh_hs_create(hh_hs** out, int device, const float* map, const int32_t shape[3], double apix, double fraction) try {
  if (!out) return hs_fail(nullptr, HH_ERR_ARG, "hh_hs_create: NULL argument");
  *out = nullptr;
  if (!map || !shape) return hs_fail(nullptr, HH_ERR_ARG, "hh_hs_create: NULL argument");
  const int nz = shape[0], ny = shape[1], nx = shape[2];
  if (nz < 2 || ny < 2 || nx < 2 || nz > 1024 || ny > 1024 || nx > 1024)
    return hs_fail(nullptr, HH_ERR_ARG, "hh_hs_create: every side must lie in [2, 1024]");
  if (!(apix > 0) || !std::isfinite(apix) || !(fraction > 0) || !std::isfinite(fraction))
    return hs_fail(nullptr, HH_ERR_ARG, "hh_hs_create: apix and fraction must be positive and finite");
  // z range of the map that carries density (transforms.py:92-99), as hh_apply_helical_symmetry takes it
  const size_t plane = (size_t)ny * nx;
  std::vector<double> prof((size_t)nz, 0.0);
  for (int k = 0; k < nz; ++k) {
    double acc = 0;
    const float* q = map + (size_t)k * plane;
    for (size_t t = 0; t < plane; ++t) acc += q[t];
    prof[(size_t)k] = acc;
  }
  const double thr = 0.01 * *std::max_element(prof.begin(), prof.end());
  int z0 = -1, z1 = -1;
  for (int k = 0; k < nz; ++k)
    if (prof[(size_t)k] > thr) { if (z0 < 0) z0 = k; z1 = k; }
  if (z0 < 0) return hs_fail(nullptr, HH_ERR_ARG, "hh_hs_create: the volume has no density above 1 % of its peak slice");
  const int zmid = (z0 + z1) / 2 + (z0 + z1) % 2;
  const int half = (int)std::min((double)nz * fraction + 0.5, 1.0e9) / 2;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return hs_fail(nullptr, HH_ERR_HIP, "hh_hs_create: no such HIP device (the symmetry search has no CPU fallback)");
  hh_hs* p = new hh_hs;
  p->device = device; p->nz = nz; p->ny = ny; p->nx = nx; p->apix = apix; p->fraction = fraction;
  p->z0 = std::max(z0, zmid - half);
  p->z1 = std::min(z1, zmid + half);
  if (const char* b = std::getenv("HELICON_HS_PARTIAL_BYTES")) {
    const long long v = std::atoll(b);
    if (v > 0) p->budget = v;
  }
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&p->ev0);
  if (e == hipSuccess) e = hipEventCreate(&p->ev1);
  if (e == hipSuccess && !p->d_map.ensure(plane * nz)) {
    hh_hs_destroy(p);
    return hs_fail(nullptr, HH_ERR_NOMEM, "hh_hs_create: " + dev_alloc_failed(plane * nz * sizeof(float)));
  }
  if (e == hipSuccess) e = hipMemcpyAsync(p->d_map, map, plane * nz * sizeof(float), hipMemcpyHostToDevice, p->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
  if (e != hipSuccess) {
    const std::string msg = std::string("hh_hs_create: ") + hipGetErrorString(e);
    hh_hs_destroy(p);
    return hs_fail(nullptr, e == hipErrorOutOfMemory ? HH_ERR_NOMEM : HH_ERR_HIP, msg);
  }
  // the default region; a map too small to have one (rmax = min(ny, nx) // 2 - 1 = 0) stays without until hh_hs_set_region
  const int rc = hs_set_region(p, 0.0, (double)(std::min(ny, nx) / 2 - 1), 0.5);
  if (rc != HH_OK && rc != HH_ERR_ARG) {
    const std::string msg = p->err;
    hh_hs_destroy(p);
    return hs_fail(nullptr, rc, msg);
  }
  p->err.clear();
  *out = p;
  return HH_OK;
} HH_CATCH_HS(nullptr, "hh_hs_create")

int hh_hs_set_region(hh_hs* p, double rmin_px, double rmax_px, double z_fraction) try {
  if (!p) return hs_fail(nullptr, HH_ERR_ARG, "hh_hs_set_region: NULL handle");
  return hs_set_region(p, rmin_px, rmax_px, z_fraction);
} HH_CATCH_HS(p, "hh_hs_set_region")

int hh_hs_set_budget(hh_hs* p, int64_t partial_bytes) try {
  if (!p || partial_bytes < 1) return hs_fail(p, HH_ERR_ARG, "hh_hs_set_budget: needs a handle and a positive byte count");
  p->budget = partial_bytes;
  return HH_OK;
} HH_CATCH_HS(p, "hh_hs_set_budget")

int hh_hs_info(const hh_hs* p, int32_t z_range[2], int64_t* region_voxels, int64_t* launches) try {
  if (!p) return hs_fail(nullptr, HH_ERR_ARG, "hh_hs_info: NULL handle");
  if (z_range) { z_range[0] = p->z0; z_range[1] = p->z1; }
  if (region_voxels) *region_voxels = p->region_voxels;
  if (launches) *launches = p->launches;
  return HH_OK;
} HH_CATCH_HS(p, "hh_hs_info")

int hh_hs_kernel_ms(const hh_hs* p, double* ms) try {
  if (!p || !ms) return hs_fail(const_cast<hh_hs*>(p), HH_ERR_ARG, "hh_hs_kernel_ms: NULL argument");
  *ms = p->kernel_ms;
  return HH_OK;
} HH_CATCH_HS(p, "hh_hs_kernel_ms")

int hh_hs_search(hh_hs* p, const double* params, int64_t g, float* scores) try {
  if (!p) return hs_fail(nullptr, HH_ERR_ARG, "hh_hs_search: NULL handle");
  if (!params || !scores || g < 0) return hs_fail(p, HH_ERR_ARG, "hh_hs_search: bad argument");
  if (p->region_voxels == 0) return hs_fail(p, HH_ERR_ARG, "hh_hs_search: the region holds no voxel (hh_hs_set_region)");
  for (int64_t i = 0; i < g; ++i) {
    const double tw = params[3 * i], rs = params[3 * i + 1], cs = params[3 * i + 2];
    const char* what = nullptr;
    if (!std::isfinite(tw)) what = "twist must be finite";
    else if (!(rs > 0) || !std::isfinite(rs)) what = "rise must be positive and finite";
    else if (!(cs >= 1) || cs > HS_MAX_CSYM || cs != std::floor(cs)) what = "csym must be a whole number in [1, 4096]";
    else if ((double)p->nz * p->apix / rs > HS_MAX_REPEATS) what = "rise is too small for this map (more than 1e8 repeats)";
    if (what) return hs_fail(p, HH_ERR_ARG, "hh_hs_search: candidate " + std::to_string(i) + ": " + what);
  }
  if (g == 0) return HH_OK;
  HS_HIP(p, hipSetDevice(p->device));
  const size_t n_part = (size_t)p->nplanes * p->ntiles;
  const size_t per_cand = n_part * 3 * sizeof(double);
  // 65535: the grid.z limit (pinned by tests/test_launch_cuts_host.py, crossed by tests/test_gpu_launch_cuts.py)
  const size_t per_launch = (size_t)std::max<int64_t>(1, std::min<int64_t>({(int64_t)(p->budget / (int64_t)per_cand), g, 65535}));
  if (!p->d_part.ensure(per_launch * n_part * 3))
    return hs_fail(p, HH_ERR_NOMEM, "hh_hs_search: partial sums: " + dev_alloc_failed(per_launch * per_cand));
  if (!p->d_params.ensure((size_t)g * 3) || !p->d_scores.ensure((size_t)g))
    return hs_fail(p, HH_ERR_NOMEM, "hh_hs_search: candidate list: " + dev_alloc_failed((size_t)g * (p->d_params ? sizeof(float) : 3 * sizeof(double))));
  HS_HIP(p, hipMemcpyAsync(p->d_params, params, (size_t)g * 3 * sizeof(double), hipMemcpyHostToDevice, p->stream));
  HS_HIP(p, hipEventRecord(p->ev0, p->stream));
  HsArgs a = hs_args(p);
  a.part = p->d_part;
  for (int64_t g0 = 0; g0 < g; g0 += (int64_t)per_launch) {
    const unsigned n = (unsigned)std::min<int64_t>((int64_t)per_launch, g - g0);
    a.params = p->d_params + 3 * g0;
    hipLaunchKernelGGL(k_hs_score, dim3((unsigned)p->nplanes, (unsigned)p->ntiles, n), dim3(256), 0, p->stream, a);
    hipLaunchKernelGGL(k_hs_finalize, dim3(n), dim3(256), 0, p->stream, p->d_part, (int64_t)n_part, p->sum_v, p->sum_vv,
                       (double)p->region_voxels, p->d_scores + g0);
    HS_HIP(p, hipGetLastError());
    ++p->launches;
  }
  HS_HIP(p, hipEventRecord(p->ev1, p->stream));
  HS_HIP(p, hipMemcpyAsync(scores, p->d_scores, (size_t)g * sizeof(float), hipMemcpyDeviceToHost, p->stream));
  HS_HIP(p, hipStreamSynchronize(p->stream));
  float ms = 0.f;
  HS_HIP(p, hipEventElapsedTime(&ms, p->ev0, p->ev1));
  p->kernel_ms = ms;
  return HH_OK;
} HH_CATCH_HS(p, "hh_hs_search")

}  // extern "C"
