// true_fsc.inc — the noise-substitution ("true") FSC of two half maps (commands/trueFSC.py, Chen et al. 2013,
// Ultramicroscopy 135:24-35), on a context that keeps one pair of cubic maps of even side n on the device.
//
// create:  z and y forward passes as in fourier_correlation.inc, then k_tfsc_xpass: k_fc_xpass's product (fc_pair_product) with
//          an epilogue that STORES the half spectrum F(kz, ky, kx) of both maps, every bin with
//          m = kz^2 + ky^2 + kx^2 >= m_cut (folded frequencies, integers) replaced by |F| e^{i theta}
//          (lib/filters.py:469-520, randomize_phases_lowpass), and adds the shell sums of two curves in the same pass: the
//          unmasked one and the one of the substituted bins (every bin of the half spectrum once, as calc_fsc counts them).
//          theta: host angles (the reference's uniform draws), or a Philox4x32-10 draw keyed by the seed with the counter
//          (bin, map): the same for any launch shape and any order.
//          Then the inverse transform with irfftn's semantics on a half spectrum that is not Hermitian-consistent: complex
//          inverse passes along z and y (k_circ_gemm with conjugate operators), then k_tfsc_c2r along x with weight 1 on
//          kx = 0 and kx = n / 2 (their imaginary parts meet sin = 0 and drop out) and 2 elsewhere; 1 / n per pass.
// masked:  k_tfsc_mask multiplies the four resident maps by each mask straight into the forward passes' input; the sums of
//          the pairs (map1 m1, map2 m2) and (map1r m1, map2r m2) then come from fc_device unchanged: bit-identical from run to
//          run, independent of the batch and of a mask's place in it.  Only the masks cross the bus.

struct SmState;               // soft_mask.inc: the supports of hh_tfsm_set_support and the distance transform's scratch
void sm_release(SmState* s);

struct hh_tfsc {
  int device = 0, n = 0, ncol = 0, nshell = 0;
  int64_t per_map = 0, per_spec = 0;    // n^3 and n n (n / 2 + 1)
  FcPlan plan;
  size_t o_izr = 0, o_izi = 0, o_iyr = 0, o_iyi = 0, o_xcw = 0, o_xsw = 0;   // inverse operators, after the plan's in fc.mats
  FcBuffers fc;              // the forward passes' scratch, the operators (fc.mats) and the events
  DevBuf<float> maps;        // [4][n^3]: map1, map2, map1r, map2r
  DevBuf<float> spec;        // [re | im][2 maps][n n][ncol]: the substituted half spectra
  DevBuf<double> curves;     // [2][nshell][3]
  DevBuf<float> masks;       // the masks of one chunk of hh_tfsc_masked
  SmState* soft = nullptr;
  ~hh_tfsc() {   // (the buffers and fc go after this body, on the device set here)
    (void)hipSetDevice(device);
    sm_release(soft);
  }
};

namespace {

struct TfXPass {
  const float* re;         // [2][rows][nx] planes after the z and y passes: map1, map2
  const float* im;
  const float* cs;         // [nx][ncol]
  const float* sn;
  const double* scale;     // [3]
  const double* ph1;       // [rows][ncol] host angles of map 1, or null: the generator
  const double* ph2;
  float* sre;              // [2][rows][ncol] the stored spectrum
  float* sim;
  long long* acc;          // [2][nshell][3]: unmasked, randomised-unmasked
  unsigned long long seed;
  long long m_cut;
  int rows, nx, ncol, n, nshell;
};

// Philox4x32-10 (Salmon et al., SC'11): the first of the four output words
__device__ __forceinline__ unsigned tf_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

// One workgroup: 64 rows x 64 columns of F1 and F2 by k_fc_xpass's product (fc_pair_product); the epilogue stores the
// (substituted) bins and adds the products of the original and of the substituted bins to the two curves' shell sums.
__global__ __launch_bounds__(256) void k_tfsc_xpass(TfXPass g) {
  __shared__ unsigned long long sh[2 * 257 * 3];
  const Tile64 t = tile64();
  const int row0 = blockIdx.x * FC_T, col0 = blockIdx.y * FC_T;
  const int64_t plane = (int64_t)g.rows * g.nx;
  const float* const src[4] = {g.re, g.im, g.re + plane, g.im + plane};
  const int nsh = 2 * g.nshell * 3;
  for (int e = t.tid; e < nsh; e += 256) sh[e] = 0ull;
  const bool active = col0 + t.wp < g.ncol && row0 + t.wm < g.rows;
  f32x16 re1 = {0}, im1 = {0}, re2 = {0}, im2 = {0};
  fc_pair_product(src, g.cs, g.sn, g.rows, g.nx, g.ncol, row0, col0, active, t, re1, im1, re2, im2);
  const double scale[3] = {g.scale[0], g.scale[1], g.scale[2]};
  if (active) {
    const int col = col0 + t.wp + t.r;
    const int hn = g.n / 2;
    const int64_t splane = (int64_t)g.rows * g.ncol;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = row0 + t.wm + acc_row(i, t.h);
      if (row >= g.rows || col >= g.ncol) continue;
      const int kz = row / g.n, ky = row % g.n;
      const int s = fc_shell_3d(kz, ky, col, g.n);
      const int fz = kz <= hn ? kz : g.n - kz, fy = ky <= hn ? ky : g.n - ky;
      const long long m = (long long)fz * fz + (long long)fy * fy + (long long)col * col;
      const double x1 = re1[i], y1 = im1[i], x2 = re2[i], y2 = im2[i];
      fc_add_products(&sh[s * 3], 1.0, x1, y1, x2, y2, scale);   // the unmasked curve: calc_fsc's sums
      const int64_t bin = (int64_t)row * g.ncol + col;
      float u1 = re1[i], v1 = im1[i], u2 = re2[i], v2 = im2[i];
      if (m >= g.m_cut) {
        double t1, t2;
        if (g.ph1) {
          t1 = g.ph1[bin];
          t2 = g.ph2[bin];
        } else {
          const unsigned k0 = (unsigned)g.seed, k1 = (unsigned)(g.seed >> 32), b0 = (unsigned)bin, b1 = (unsigned)((unsigned long long)bin >> 32);
          t1 = ((double)tf_philox(b0, b1, 0u, 0u, k0, k1) + 0.5) * (6.283185307179586476925286766559 / 4294967296.0);
          t2 = ((double)tf_philox(b0, b1, 1u, 0u, k0, k1) + 0.5) * (6.283185307179586476925286766559 / 4294967296.0);
        }
        double sn1, cs1, sn2, cs2;
        sincos(t1, &sn1, &cs1);
        sincos(t2, &sn2, &cs2);
        const double a1 = sqrt(x1 * x1 + y1 * y1), a2 = sqrt(x2 * x2 + y2 * y2);
        u1 = (float)(a1 * cs1); v1 = (float)(a1 * sn1);
        u2 = (float)(a2 * cs2); v2 = (float)(a2 * sn2);
      }
      g.sre[bin] = u1; g.sim[bin] = v1;
      g.sre[splane + bin] = u2; g.sim[splane + bin] = v2;
      fc_add_products(&sh[(g.nshell + s) * 3], 1.0, u1, v1, u2, v2, scale);   // the randomised-unmasked curve, from the bins as stored
    }
  }
  __syncthreads();
  fc_flush(sh, nsh, g.acc, t.tid);
}

struct TfC2R {
  const float* re;   // [maps][rows][ncol] planes after the inverse z and y passes
  const float* im;
  const float* cw;   // [ncol][nx]  w_k cos(2 pi k x / n) / n
  const float* sw;   // [ncol][nx] -w_k sin(2 pi k x / n) / n
  float* y;          // [maps][rows][nx]
  int rows, nx, ncol;
};

// The last inverse pass: y[row][x] = sum_k re[row][k] cw[k][x] + im[row][k] sw[k][x] on the shared tile (mfma_tile.inc), one
// 32 x 32 accumulator per wavefront; the accumulator's lane index runs along x: the stores coalesce.
__global__ __launch_bounds__(256) void k_tfsc_c2r(TfC2R g) {
  __shared__ float as[2][FC_T][FC_K + 1];   // re, im
  __shared__ float os[2][FC_K][FC_T + 1];   // cw, sw
  const Tile64 t = tile64();
  const int r = t.r, h = t.h, wm = t.wm, wp = t.wp;
  const int row0 = blockIdx.x * FC_T, col0 = blockIdx.y * FC_T;
  const int64_t splane = (int64_t)g.rows * g.ncol;
  const float* const src[2] = {g.re + (int64_t)blockIdx.z * splane, g.im + (int64_t)blockIdx.z * splane};
  const float* const op[2] = {g.cw, g.sw};
  const bool active = col0 + wp < g.nx && row0 + wm < g.rows;
  f32x16 acc = {0};
  for (int k0 = 0; k0 < g.ncol; k0 += FC_K) {
#pragma unroll
    for (int q = 0; q < 2; ++q) stage_rows(as[q], src[q], g.ncol, row0, g.rows, k0, g.ncol, t.tid);
    stage_cols(os, op, g.nx, k0, g.ncol, col0, g.nx, t.tid);
    __syncthreads();
    if (active) {   // its own step: the Re and Im products alternate within the slice (tile_mac twice would reorder the sum)
#pragma unroll
      for (int kk = 0; kk < FC_K; kk += 2) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[0][wm + r][kk + h], os[0][kk + h][wp + r], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[1][wm + r][kk + h], os[1][kk + h][wp + r], acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!active) return;
  const int col = col0 + wp + r;
  float* const y = g.y + (int64_t)blockIdx.z * g.rows * g.nx;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = row0 + wm + acc_row(i, h);
    if (row < g.rows && col < g.nx) y[(int64_t)row * g.nx + col] = acc[i];
  }
}

// in: [2 P][n^3], P = 2 nb pairs: pair 2 j = (map1 m1_j, map2 m2_j), pair 2 j + 1 = (map1r m1_j, map2r m2_j); the first members
// fill maps 0 .. P - 1, the second members P .. 2 P - 1.  m2 == null: one mask for both members.
__global__ __launch_bounds__(256) void k_tfsc_mask(const float* __restrict__ maps, const float* __restrict__ m1, const float* __restrict__ m2,
                                                   int64_t per_map, int nb, float* __restrict__ in) {
  const int j = blockIdx.y;
  const int64_t P = 2 * (int64_t)nb;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_map; i += (int64_t)gridDim.x * 256) {
    const float a = m1[j * per_map + i], b = m2 ? m2[j * per_map + i] : a;
    in[(2 * j) * per_map + i] = maps[i] * a;
    in[(P + 2 * j) * per_map + i] = maps[per_map + i] * b;
    in[(2 * j + 1) * per_map + i] = maps[2 * per_map + i] * a;
    in[(P + 2 * j + 1) * per_map + i] = maps[3 * per_map + i] * b;
  }
}

// row-major [ncol][n] table of the c2r pass: w_k p[(k x) mod n] scale, w = 1 on k = 0 and k = n / 2, 2 elsewhere; `sine`: those
// two rows are exactly 0 (sin(pi x) is, its float64 value is not)
size_t tf_c2r_table(std::vector<float>& mats, int n, int ncol, const std::vector<double>& p, double scale, bool sine) {
  const size_t off = mats.size();
  mats.resize(off + (size_t)ncol * n);
  for (int k = 0; k < ncol; ++k) {
    const bool edge = k == 0 || 2 * k == n;
    const double w = edge ? (sine ? 0.0 : 1.0) : 2.0;
    for (int x = 0; x < n; ++x) mats[off + (size_t)k * n + x] = (float)(w * scale * p[(int)(((int64_t)k * x) % n)]);
  }
  return off;
}

int tf_create(hh_tfsc* c, const float* map1, const float* map2, int64_t m_cut, const double* phases1, const double* phases2,
              unsigned long long seed) {
  const int n = c->n, ncol = c->ncol, nshell = c->nshell;
  const int64_t per_map = c->per_map, per_spec = c->per_spec;
  HH_HIP(nullptr, hipSetDevice(c->device));
  fc_plan(c->plan, n, n, n);
  std::vector<float> mats = c->plan.mats;
  {   // inverse passes: (c + i s)(a + i b) = (c a - s b) + i (s a + c b), 1 / n each
    std::vector<double> cs, sn;
    unit_circle(n, cs, sn);
    const double q = 1.0 / n;
    c->o_izr = append_axis_operator(mats, n, AxisIndex::Dft, cs, q, &sn, -q);
    c->o_izi = append_axis_operator(mats, n, AxisIndex::Dft, sn, q, &cs, q);
    c->o_iyr = c->o_izr;
    c->o_iyi = c->o_izi;
    c->o_xcw = tf_c2r_table(mats, n, ncol, cs, q, false);
    c->o_xsw = tf_c2r_table(mats, n, ncol, sn, -q, true);
  }
  const size_t map_bytes = (size_t)per_map * sizeof(float);
  FcBuffers& d = c->fc;
  if (int rc = ensure(nullptr, d.mats, mats.size())) return rc;
  HH_HIP(nullptr, hipMemcpy(d.mats, mats.data(), mats.size() * sizeof(float), hipMemcpyHostToDevice));
  if (int rc = ensure(nullptr, c->maps, 4 * (size_t)per_map)) return rc;
  if (int rc = ensure(nullptr, c->spec, 4 * (size_t)per_spec)) return rc;
  if (int rc = ensure(nullptr, c->curves, (size_t)2 * nshell * 3)) return rc;
  if (int rc = d.reserve(1, per_map, nshell, true, false)) return rc;   // create reads the resident maps in place
  HH_HIP(nullptr, hipMemcpy(c->maps, map1, map_bytes, hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipMemcpy(c->maps + per_map, map2, map_bytes, hipMemcpyHostToDevice));
  DevBuf<double> d_ph;      // the host's angles: both maps, freed on the way out
  if (phases1) {
    if (int rc = ensure(nullptr, d_ph, 2 * (size_t)per_spec)) return rc;
    HH_HIP(nullptr, hipMemcpy(d_ph, phases1, (size_t)per_spec * sizeof(double), hipMemcpyHostToDevice));
    HH_HIP(nullptr, hipMemcpy(d_ph + per_spec, phases2, (size_t)per_spec * sizeof(double), hipMemcpyHostToDevice));
  }
  HH_HIP(nullptr, hipMemsetAsync(d.amax, 0, 2 * sizeof(unsigned), nullptr));
  HH_HIP(nullptr, hipMemsetAsync(d.acc, 0, (size_t)2 * nshell * 3 * sizeof(long long), nullptr));
  const float *xre = nullptr, *xim = nullptr;
  fc_passes(c->plan, c->maps, d, 1, &xre, &xim);
  float* const sre = c->spec;
  float* const sim = c->spec + 2 * per_spec;
  TfXPass x{};
  x.re = xre; x.im = xim;
  x.cs = d.mats + c->plan.o_xc; x.sn = d.mats + c->plan.o_xs;
  x.scale = d.scale;
  x.ph1 = d_ph; x.ph2 = d_ph ? d_ph + per_spec : nullptr;
  x.sre = sre; x.sim = sim;
  x.acc = d.acc;
  x.seed = seed; x.m_cut = m_cut;
  x.rows = n * n; x.nx = n; x.ncol = ncol; x.n = n; x.nshell = nshell;
  hipLaunchKernelGGL(k_tfsc_xpass, dim3((unsigned)((n * n + FC_T - 1) / FC_T), (unsigned)((ncol + FC_T - 1) / FC_T), 1), dim3(256), 0, nullptr, x);
  hipLaunchKernelGGL(k_fc_finish, dim3((unsigned)((2 * nshell * 3 + 255) / 256)), dim3(256), 0, nullptr, d.acc, d.scale, nshell, 2,
                     (int64_t)2 * nshell * 3, c->curves);   // the two curves share the one pair's scales
  // inverse: z pass (one map per grid.z, P = n ncol), y pass (one z slice per grid.z, P = ncol), both K = 2 n over [re; im]
  float* const zr = d.p1;
  float* const zi = d.p1 + 2 * per_spec;
  float* const yr = d.p2;
  float* const yi = d.p2 + 2 * per_spec;
  const AxisGeom inv_z = axis_geom(AxisView{2, n, n, (int64_t)n * ncol, false});
  for (int part = 0; part < 2; ++part)
    launch_circ_pass(inv_z, d.mats + (part == 0 ? c->o_izr : c->o_izi), 2 * n, sre, sim, part == 0 ? zr : zi, nullptr);
  const AxisGeom inv_y = axis_geom(AxisView{2 * (int64_t)n, n, n, ncol, false});
  for (int part = 0; part < 2; ++part)
    launch_circ_pass(inv_y, d.mats + (part == 0 ? c->o_iyr : c->o_iyi), 2 * n, zr, zi, part == 0 ? yr : yi, nullptr);
  TfC2R r{};
  r.re = yr; r.im = yi;
  r.cw = d.mats + c->o_xcw; r.sw = d.mats + c->o_xsw;
  r.y = c->maps + 2 * per_map;
  r.rows = n * n; r.nx = n; r.ncol = ncol;
  hipLaunchKernelGGL(k_tfsc_c2r, dim3((unsigned)((n * n + FC_T - 1) / FC_T), (unsigned)((n + FC_T - 1) / FC_T), 2), dim3(256), 0, nullptr, r);
  HH_HIP(nullptr, hipGetLastError());
  HH_HIP(nullptr, hipDeviceSynchronize());
  return HH_OK;
}

}  // namespace

extern "C" int hh_tfsc_create(hh_tfsc** out, int device, const float* map1, const float* map2, int32_t n, int64_t m_cut,
                              const double* phases1, const double* phases2, uint64_t seed) try {
  if (!out) return fail(nullptr, HH_ERR_ARG, "hh_tfsc_create: NULL argument");
  *out = nullptr;
  if (!map1 || !map2) return fail(nullptr, HH_ERR_ARG, "hh_tfsc_create: NULL argument");
  if ((phases1 == nullptr) != (phases2 == nullptr)) return fail(nullptr, HH_ERR_ARG, "hh_tfsc_create: phases1 and phases2 go together (or both NULL)");
  if (n < 8 || n > 512 || (n & 1)) return fail(nullptr, HH_ERR_ARG, "hh_tfsc_create: the side of the cubes must be even and lie in [8, 512]");
  if (m_cut < 0) return fail(nullptr, HH_ERR_ARG, "hh_tfsc_create: m_cut must be >= 0");
  if (int rc = use_device("hh_tfsc_create", device)) return rc;
  std::unique_ptr<hh_tfsc> c(new hh_tfsc);
  c->device = device; c->n = n; c->ncol = n / 2 + 1; c->nshell = n / 2 + 1;
  c->per_map = (int64_t)n * n * n; c->per_spec = (int64_t)n * n * c->ncol;
  if (int rc = tf_create(c.get(), map1, map2, m_cut, phases1, phases2, seed)) return rc;
  *out = c.release();
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_tfsc_create")

extern "C" int hh_tfsc_curves(hh_tfsc* ctx, double* sums) try {
  if (!ctx || !sums) return fail(nullptr, HH_ERR_ARG, "hh_tfsc_curves: NULL argument");
  HH_HIP(nullptr, hipSetDevice(ctx->device));
  HH_HIP(nullptr, hipMemcpy(sums, ctx->curves, (size_t)2 * ctx->nshell * 3 * sizeof(double), hipMemcpyDeviceToHost));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_tfsc_curves")

extern "C" int hh_tfsc_download(hh_tfsc* ctx, int which, float* map_out, float* spec_out) try {
  if (!ctx || (!map_out && !spec_out)) return fail(nullptr, HH_ERR_ARG, "hh_tfsc_download: NULL argument");
  if (which < 0 || which > 1) return fail(nullptr, HH_ERR_ARG, "hh_tfsc_download: which must be 0 or 1");
  HH_HIP(nullptr, hipSetDevice(ctx->device));
  if (map_out)
    HH_HIP(nullptr, hipMemcpy(map_out, ctx->maps + (2 + which) * ctx->per_map, (size_t)ctx->per_map * sizeof(float), hipMemcpyDeviceToHost));
  if (spec_out) {
    const int64_t ps = ctx->per_spec;
    std::vector<float> re((size_t)ps), im((size_t)ps);
    HH_HIP(nullptr, hipMemcpy(re.data(), ctx->spec + which * ps, (size_t)ps * sizeof(float), hipMemcpyDeviceToHost));
    HH_HIP(nullptr, hipMemcpy(im.data(), ctx->spec + (2 + which) * ps, (size_t)ps * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < ps; ++i) {
      spec_out[2 * i] = re[(size_t)i];
      spec_out[2 * i + 1] = im[(size_t)i];
    }
  }
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_tfsc_download")

extern "C" int hh_tfsc_masked(hh_tfsc* ctx, const float* masks1, const float* masks2, int32_t batch, int full_spectrum, double* sums,
                              double* kernel_ms) try {
  if (!ctx || !masks1 || !sums) return fail(nullptr, HH_ERR_ARG, "hh_tfsc_masked: NULL argument");
  if (batch < 1) return fail(nullptr, HH_ERR_ARG, "hh_tfsc_masked: batch must be >= 1");
  hh_tfsc* const c = ctx;
  HH_HIP(nullptr, hipSetDevice(c->device));
  const int64_t per_map = c->per_map;
  const int nshell = c->nshell;
  // masks per chunk: two pairs each within fc_run's scratch cap, and the y pass's grid.z = 4 chunk n <= 65535
  // (pinned by tests/test_launch_cuts_host.py, crossed by tests/test_gpu_launch_cuts.py)
  int64_t chunk = std::max<int64_t>(1, FC_SCRATCH_BYTES / (20 * per_map * (int64_t)sizeof(float)));
  chunk = std::min<int64_t>(chunk, 65535 / (4 * c->n));
  chunk = std::min<int64_t>(chunk, batch);
  FcBuffers& d = c->fc;
  if (int rc = d.reserve(2 * chunk, per_map, nshell, true, true)) return rc;
  const int n_sets = masks2 ? 2 : 1;
  if (int rc = ensure(nullptr, c->masks, (size_t)(n_sets * chunk) * per_map)) return rc;
  double ms_total = 0.0;
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = std::min(chunk, (int64_t)batch - b0);
    float* const d_m1 = c->masks;
    float* const d_m2 = masks2 ? c->masks + nb * per_map : nullptr;
    HH_HIP(nullptr, hipMemcpy(d_m1, masks1 + b0 * per_map, (size_t)nb * per_map * sizeof(float), hipMemcpyHostToDevice));
    if (masks2) HH_HIP(nullptr, hipMemcpy(d_m2, masks2 + b0 * per_map, (size_t)nb * per_map * sizeof(float), hipMemcpyHostToDevice));
    HH_HIP(nullptr, hipEventRecord(d.ev[0], nullptr));
    hipLaunchKernelGGL(k_tfsc_mask, dim3((unsigned)std::min<int64_t>((per_map + 255) / 256, 4096), (unsigned)nb), dim3(256), 0, nullptr, c->maps, d_m1,
                       d_m2, per_map, (int)nb, d.in);
    fc_device(c->plan, d.in, d, 2 * nb, nshell, full_spectrum != 0);
    HH_HIP(nullptr, hipGetLastError());
    HH_HIP(nullptr, hipEventRecord(d.ev[1], nullptr));
    HH_HIP(nullptr, hipMemcpy(sums + b0 * 2 * nshell * 3, d.sums, (size_t)(2 * nb) * nshell * 3 * sizeof(double), hipMemcpyDeviceToHost));
    float ms = 0.f;
    HH_HIP(nullptr, hipEventElapsedTime(&ms, d.ev[0], d.ev[1]));
    ms_total += ms;
  }
  if (kernel_ms) *kernel_ms = ms_total;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_tfsc_masked")

extern "C" int hh_tfsc_destroy(hh_tfsc* ctx) try {
  delete ctx;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_tfsc_destroy")
