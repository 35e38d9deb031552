// structure_factor.inc — the radially binned power |F|^2 of maps and images and the amplitude scaling that brings it onto a
// target profile (lib/filters.py:22-208: calculate_structural_factor, set_structural_factors, match_structural_factors), for a
// batch of maps of one shape on a resident context.  Any sides, odd, prime and unequal included: 3-D (nz, ny, nx), 2-D (ny, nx).
//
// profile: an elementwise prologue (k_sf_prepare: clip(x, t) - t, then * mask, in float64, rounded once), the z and y forward
//          passes as in fourier_correlation.inc (k_circ_gemm), then k_sf_xpass: the nx / 2 + 1 needed columns on the shared
//          tile (slice-wise accumulators as in fc_pair_product); its epilogue forms |F|^2 in float64, weighs it 2 off the
//          planes kx = 0 and kx = nx / 2 (even nx: the full spectrum seen from its half), labels the bin and adds it to fixed-point sums
//          (fc_add_products' scheme: a power of two per map from max |x| alone, 64-bit integer atomics, LDS then global), so
//          the sums are bit-identical from run to run and do not depend on the batch.  It stores the half spectrum when asked.
// bin:     qr = sqrt(qx^2 + qy^2 [+ qz^2]) / apix in float64 from the host's np.fft.fftfreq tables, squares and sums in that
//          order without contraction, correctly rounded square root and division (sf_radius); label = (number of qbins <= qr)
//          - 1 by a search on the host's own np.linspace table (sf_label), the last bin open-ended.  Ties are real (DESIGN.md,
//          "Structure factors") and fall where NumPy's float64 expression puts them.
// match:   k_sf_finish turns the sums and the target (on qbins) into ratio = sqrt(target / sf) (0 where sf == 0) on the device;
//          k_sf_scale multiplies the stored half spectrum (with a mask: that of the RAW data, transformed a second time) by
//          interp1d(qbins, ratio, fill_value = 0)(qr): linear between the edges, ratio[-1] at qr == qbins[-1], 0 above; then
//          the inverse z and y passes (k_circ_gemm, conjugate operators) and k_tfsc_c2r along x: irfftn's semantics.

struct hh_sf {
  int device = 0, ndim = 0, nz = 0, ny = 0, nx = 0, ncol = 0, rows = 0, nbins = 0;
  bool has_target = false;
  double apix = 1.0;
  int64_t per_map = 0, per_spec = 0;   // voxels of a map, bins of its half spectrum
  size_t o_c = 0, o_ms = 0, o_re = 0, o_im = 0, o_xc = 0, o_xs = 0;              // forward operators in mats
  size_t o_izr = 0, o_izi = 0, o_iyr = 0, o_iyi = 0, o_xcw = 0, o_xsw = 0;       // inverse operators
  DevBuf<float> mats;
  DevBuf<double> tab;        // qbins[nbins] | target[nbins] | fftfreq of z (3-D), y, x
  DevBuf<float> in, work, p1, p2, spec, mask;   // scratch of one chunk: p1 / p2 / spec are [re | im] plane pairs
  DevBuf<unsigned> amax;     // [maps]: its size says how many maps the scratch holds
  DevBuf<double> scale, sums, ratio;
  DevBuf<long long> acc;
  DevEvents<5> ev;
  double ms[4] = {0, 0, 0, 0};   // of the last call: profile, second (raw) transform, scaling, inverse
};

namespace {

constexpr int SF_MAX_BINS = 726;   // LDS sums and edges of a workgroup: nbins <= 442 in 3-D (side 512), <= 724 in 2-D (side 1024)
constexpr int64_t SF_SCRATCH_BYTES = (int64_t)4 << 30;   // device planes of one chunk of the batch

// The reference's radius of a bin, bit for bit: squares and sums in its order, nothing contracted, sqrt and / correctly rounded.
__device__ __forceinline__ double sf_radius(double qz, double qy, double qx, bool three, double apix) {
#pragma clang fp contract(off)
  const double xx = qx * qx, yy = qy * qy;
  double s = xx + yy;
  if (three) {
    const double zz = qz * qz;
    s = s + zz;
  }
  return __ddiv_rn(__dsqrt_rn(s), apix);
}

// searchsorted(qb, qr, "right") - 1 on the host's table: a guess from the bin width, then steps on the table itself
__device__ __forceinline__ int sf_label(const double* qb, int nbins, double inv_w, double qr) {
  const double gd = qr * inv_w;
  int g = gd < (double)(nbins - 1) ? (int)gd : nbins - 1;
  g = g < 0 ? 0 : g;
  while (g + 1 < nbins && qb[g + 1] <= qr) ++g;
  while (g > 0 && qb[g] > qr) --g;
  return g;
}

// out = (clip(x, t, None) - t) * mask in float64, rounded to float32 once; a NaN stays a NaN
__global__ __launch_bounds__(256) void k_sf_prepare(const float* __restrict__ in, const float* __restrict__ mask, int has_thresh, double thresh,
                                                    int64_t per_map, float* __restrict__ out) {
  const int64_t base = (int64_t)blockIdx.y * per_map;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_map; i += (int64_t)gridDim.x * 256) {
    double v = (double)in[base + i];
    if (has_thresh) v = (v < thresh ? thresh : v) - thresh;
    if (mask) v *= (double)mask[i];
    out[base + i] = (float)v;
  }
}

// scale[b] = 2^(61 - ilogb(bound)), bound = 2 (voxels max|x|)^2 >= sum w |F|^2 (Parseval); 0 for a zero map, NaN for a map
// that holds a NaN or an infinity (its sums come back as NaN)
__global__ void k_sf_scales(const unsigned* __restrict__ amax, int batch, double voxels, double* __restrict__ scale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const double a = (double)__uint_as_float(amax[b]);
  const double bound = 2.0 * voxels * voxels * a * a;
  double s;
  if (!(bound == bound) || bound > 1.7e308) s = __longlong_as_double(0x7ff8000000000000ll);
  else if (bound == 0.0) s = 0.0;
  else s = ldexp(1.0, 61 - ilogb(bound));
  scale[b] = s;
}

struct SfXPass {
  const float* re;       // [B][rows][nx] planes after the earlier passes
  const float* im;
  const float* cs;       // [nx][ncol] cos(2 pi x k / nx)
  const float* sn;       // [nx][ncol] sin(2 pi x k / nx)
  const double* qbins;   // [nbins]
  const double* fz;      // [nz] fftfreq, null in 2-D
  const double* fy;      // [ny]
  const double* fx;      // [nx]
  const double* scale;   // [B]
  long long* acc;        // [B][nbins] fixed-point sums, or null: no sums (the raw data's transform of a masked match)
  float* sre;            // [B][rows][ncol] the half spectrum, or null
  float* sim;
  double apix;
  int rows, nx, ncol, ny, nbins;
};

// The x pass of one map's 64 x 64 tile on the shared tile (mfma_tile.inc): the planes src = {re, im} ([rows][nx]) times the
// tables cs / sn ([nx][ncol]) into the Re and Im accumulators of each wavefront; every staged slice sums into accumulators
// of its own first (fc_pair_product: a chain of 2 FC_K terms plus nx / FC_K slice sums).  Holds the x pass's LDS.
__device__ __forceinline__ void sf_product(const float* const (&src)[2], const float* cs, const float* sn, int rows, int nx, int ncol,
                                           int row0, int col0, bool active, const Tile64& t, f32x16& re, f32x16& im) {
  __shared__ float as[2][FC_T][FC_K + 1];   // re, im
  __shared__ float os[2][FC_K][FC_T + 1];   // cos, sin
  const float* const tab[2] = {cs, sn};
  const int r = t.r, h = t.h, wm = t.wm, wp = t.wp;
  for (int k0 = 0; k0 < nx; k0 += FC_K) {
#pragma unroll
    for (int q = 0; q < 2; ++q) stage_rows(as[q], src[q], nx, row0, rows, k0, nx, t.tid);
    stage_cols(os, tab, ncol, k0, nx, col0, ncol, t.tid);
    __syncthreads();
    if (active) {
      f32x16 sre = {0}, sim = {0};
#pragma unroll
      for (int kk = 0; kk < FC_K; kk += 2) {
        const float c = os[0][kk + h][wp + r], s = os[1][kk + h][wp + r];
        const float a = as[0][wm + r][kk + h], b = as[1][wm + r][kk + h];
        // (a + i b)(c - i s) = (a c + b s) + i (b c - a s)
        sre = __builtin_amdgcn_mfma_f32_32x32x2f32(a, c, sre, 0, 0, 0);
        sre = __builtin_amdgcn_mfma_f32_32x32x2f32(b, s, sre, 0, 0, 0);
        sim = __builtin_amdgcn_mfma_f32_32x32x2f32(b, c, sim, 0, 0, 0);
        sim = __builtin_amdgcn_mfma_f32_32x32x2f32(a, -s, sim, 0, 0, 0);
      }
      re += sre; im += sim;
    }
    __syncthreads();
  }
}

// One workgroup: 64 rows x 64 columns of one map's half spectrum; the epilogue stores the bins and adds w |F|^2 to the bins' sums.
__global__ __launch_bounds__(256) void k_sf_xpass(SfXPass g) {
  __shared__ unsigned long long sh[SF_MAX_BINS];
  __shared__ double qb[SF_MAX_BINS];
  const Tile64 t = tile64();
  const int row0 = blockIdx.x * FC_T, col0 = blockIdx.y * FC_T, b = blockIdx.z;
  const int64_t plane = (int64_t)g.rows * g.nx;
  const float* const src[2] = {g.re + (int64_t)b * plane, g.im + (int64_t)b * plane};
  for (int e = t.tid; e < g.nbins; e += 256) {
    sh[e] = 0ull;
    qb[e] = g.qbins[e];
  }
  const bool active = col0 + t.wp < g.ncol && row0 + t.wm < g.rows;   // wavefront-uniform
  f32x16 re = {0}, im = {0};
  sf_product(src, g.cs, g.sn, g.rows, g.nx, g.ncol, row0, col0, active, t, re, im);   // (its barriers order the fill above)
  if (active) {
    const int col = col0 + t.wp + t.r;
    const bool in_col = col < g.ncol;
    const double qx = in_col ? g.fx[col] : 0.0;
    const double w = (col != 0 && 2 * col != g.nx) ? 2.0 : 1.0;
    const double scale = g.acc ? g.scale[b] : 0.0;
    const double inv_w = 1.0 / qb[1];
    const int64_t sbase = (int64_t)b * g.rows * g.ncol;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = row0 + t.wm + acc_row(i, t.h);
      if (row >= g.rows || !in_col) continue;
      if (g.sre) {
        const int64_t bin = sbase + (int64_t)row * g.ncol + col;
        g.sre[bin] = re[i];
        g.sim[bin] = im[i];
      }
      if (g.acc) {
        const double qr = g.fz ? sf_radius(g.fz[row / g.ny], g.fy[row % g.ny], qx, true, g.apix) : sf_radius(0.0, g.fy[row], qx, false, g.apix);
        const int s = sf_label(qb, g.nbins, inv_w, qr);
        const double x = re[i], y = im[i];
        const long long q = __double2ll_rn(w * (x * x + y * y) * scale);
        if (q != 0) atomicAdd(&sh[s], (unsigned long long)q);
      }
    }
  }
  __syncthreads();
  if (g.acc) fc_flush(sh, g.nbins, g.acc + (int64_t)b * g.nbins, t.tid);
}

// sums = acc / scale and, with a target, ratio = sqrt(target / sums) where sums != 0, else 0 (a NaN sum gives a NaN ratio)
__global__ __launch_bounds__(256) void k_sf_finish(const long long* __restrict__ acc, const double* __restrict__ scale,
                                                   const double* __restrict__ target, int nbins, int64_t total, double* __restrict__ sums,
                                                   double* __restrict__ ratio) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const double s = scale[i / nbins];
  const double v = s == 0.0 ? 0.0 : (double)acc[i] / s;
  sums[i] = v;
  if (target) ratio[i] = v != 0.0 ? sqrt(target[i % nbins] / v) : 0.0;
}

struct SfScale {
  float* re;             // [B][rows][ncol] the half spectrum, scaled in place
  float* im;
  const double* qbins;
  const double* ratio;   // [B][nbins]
  const double* fz;
  const double* fy;
  const double* fx;
  double apix;
  int64_t per_spec;
  int ncol, ny, nbins;
};

// F *= interp1d(qbins, ratio, bounds_error = False, fill_value = 0)(qr): the bin's radius and its place among the edges as
// k_sf_xpass decides them; linear between two edges, ratio[nbins - 1] on the last edge, 0 beyond it.
__global__ __launch_bounds__(256) void k_sf_scale(SfScale g) {
  __shared__ double qb[SF_MAX_BINS];
  __shared__ double rt[SF_MAX_BINS];
  const int b = blockIdx.y;
  for (int e = threadIdx.x; e < g.nbins; e += 256) {
    qb[e] = g.qbins[e];
    rt[e] = g.ratio[(int64_t)b * g.nbins + e];
  }
  __syncthreads();
  const double inv_w = 1.0 / qb[1];
  float* const re = g.re + (int64_t)b * g.per_spec;
  float* const im = g.im + (int64_t)b * g.per_spec;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.per_spec; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / g.ncol;
    const int col = (int)(i - row * g.ncol);
    const double qr = g.fz ? sf_radius(g.fz[row / g.ny], g.fy[row % g.ny], g.fx[col], true, g.apix)
                           : sf_radius(0.0, g.fy[row], g.fx[col], false, g.apix);
    const int s = sf_label(qb, g.nbins, inv_w, qr);
    double v;
    if (s == g.nbins - 1) v = qr == qb[s] ? rt[s] : 0.0;
    else v = rt[s] + (rt[s + 1] - rt[s]) / (qb[s + 1] - qb[s]) * (qr - qb[s]);
    re[i] = (float)((double)re[i] * v);
    im[i] = (float)((double)im[i] * v);
  }
}

// chunk of a batch of maps: input, prepared input, one or two plane pairs and the half spectrum within the scratch cap, and the
// y pass's grid.z = chunk nz <= 65535 (both pinned by tests/test_structure_factor_host.py, crossed by tests/test_gpu_structure_factor.py)
int64_t sf_chunk(const hh_sf* c, int64_t batch) {
  const int64_t bytes_per_map = (int64_t)(c->nz ? 8 : 6) * c->per_map * (int64_t)sizeof(float);
  int64_t chunk = std::max<int64_t>(1, SF_SCRATCH_BYTES / bytes_per_map);
  chunk = std::min<int64_t>(chunk, c->nz ? 65535 / c->nz : 65535);
  return std::min<int64_t>(chunk, batch);
}

int sf_reserve(hh_sf* c, int64_t maps) {
  HH_HIP(nullptr, c->ev.create());
  if ((int64_t)c->amax.size() >= maps) return HH_OK;
  c->amax.reset();   // a scratch that counts as holding maps is whole
  const size_t m = (size_t)maps;
  int rc = ensure(nullptr, c->in, m * c->per_map);
  if (!rc) rc = ensure(nullptr, c->work, m * c->per_map);
  if (!rc) rc = ensure(nullptr, c->p1, 2 * m * c->per_map);
  if (!rc && c->nz) rc = ensure(nullptr, c->p2, 2 * m * c->per_map);
  if (!rc) rc = ensure(nullptr, c->spec, 2 * m * c->per_spec);
  if (!rc) rc = ensure(nullptr, c->mask, (size_t)c->per_map);
  if (!rc) rc = ensure(nullptr, c->scale, m);
  if (!rc) rc = ensure(nullptr, c->acc, m * c->nbins);
  if (!rc) rc = ensure(nullptr, c->sums, m * c->nbins);
  if (!rc) rc = ensure(nullptr, c->ratio, m * c->nbins);
  if (!rc) rc = ensure(nullptr, c->amax, m);
  return rc;
}

// The forward transform of nb device-resident maps: z and y passes (3-D) or the y pass (2-D) through k_circ_gemm, then
// k_sf_xpass with the sums (`sum`) and / or the stored half spectrum (`store`).
void sf_forward(const hh_sf* c, const float* in, int64_t nb, bool sum, bool store) {
  const float* const mats = c->mats;
  const int64_t per_map = c->per_map;
  float* const re1 = c->p1;
  float* const im1 = c->p1 + nb * per_map;
  const int n1 = c->nz ? c->nz : c->ny;
  const AxisGeom first = axis_geom(AxisView{nb, n1, n1, c->nz ? (int64_t)c->ny * c->nx : c->nx, false});
  for (int part = 0; part < 2; ++part) launch_circ_pass(first, mats + (part == 0 ? c->o_c : c->o_ms), n1, in, nullptr, part == 0 ? re1 : im1, nullptr);
  const float *xre = re1, *xim = im1;
  if (c->nz) {
    float* const re2 = c->p2;
    float* const im2 = c->p2 + nb * per_map;
    const AxisGeom second = axis_geom(AxisView{nb * c->nz, c->ny, c->ny, c->nx, false});
    for (int part = 0; part < 2; ++part)
      launch_circ_pass(second, mats + (part == 0 ? c->o_re : c->o_im), 2 * c->ny, re1, im1, part == 0 ? re2 : im2, nullptr);
    xre = re2; xim = im2;
  }
  const double* const tab = c->tab;
  SfXPass x{};
  x.re = xre; x.im = xim;
  x.cs = mats + c->o_xc; x.sn = mats + c->o_xs;
  x.qbins = tab;
  x.fz = c->nz ? tab + 2 * c->nbins : nullptr;
  x.fy = tab + 2 * c->nbins + c->nz;
  x.fx = x.fy + c->ny;
  x.scale = c->scale;
  x.acc = sum ? c->acc.get() : nullptr;
  x.sre = store ? c->spec.get() : nullptr;
  x.sim = store ? c->spec + nb * c->per_spec : nullptr;
  x.apix = c->apix;
  x.rows = c->rows; x.nx = c->nx; x.ncol = c->ncol; x.ny = c->ny; x.nbins = c->nbins;
  hipLaunchKernelGGL(k_sf_xpass, dim3((unsigned)((c->rows + FC_T - 1) / FC_T), (unsigned)((c->ncol + FC_T - 1) / FC_T), (unsigned)nb), dim3(256), 0,
                     nullptr, x);
}

// The stored half spectra of nb maps times the interpolated ratio, then back: inverse z and y passes (3-D) or the y pass
// (2-D) with 1 / n each, and the c2r pass along x (k_tfsc_c2r) into `out` [nb][rows][nx].
void sf_scale_inverse(hh_sf* c, int64_t nb, float* out) {
  const float* const mats = c->mats;
  const double* const tab = c->tab;
  const int64_t per_spec = c->per_spec;
  float* const sre = c->spec;
  float* const sim = c->spec + nb * per_spec;
  SfScale s{};
  s.re = sre; s.im = sim;
  s.qbins = tab; s.ratio = c->ratio;
  s.fz = c->nz ? tab + 2 * c->nbins : nullptr;
  s.fy = tab + 2 * c->nbins + c->nz;
  s.fx = s.fy + c->ny;
  s.apix = c->apix; s.per_spec = per_spec; s.ncol = c->ncol; s.ny = c->ny; s.nbins = c->nbins;
  hipLaunchKernelGGL(k_sf_scale, dim3((unsigned)std::min<int64_t>((per_spec + 255) / 256, 4096), (unsigned)nb), dim3(256), 0, nullptr, s);
  (void)hipEventRecord(c->ev[3], nullptr);
  const float *yr = sre, *yi = sim;
  if (c->nz) {   // z: one map per grid.z, P = ny ncol, K = 2 nz over [re; im]
    float* const zr = c->p1;
    float* const zi = c->p1 + nb * per_spec;
    const AxisGeom inv_z = axis_geom(AxisView{nb, c->nz, c->nz, (int64_t)c->ny * c->ncol, false});
    for (int part = 0; part < 2; ++part)
      launch_circ_pass(inv_z, mats + (part == 0 ? c->o_izr : c->o_izi), 2 * c->nz, sre, sim, part == 0 ? zr : zi, nullptr);
    float* const y2r = c->p2;
    float* const y2i = c->p2 + nb * per_spec;
    const AxisGeom inv_y = axis_geom(AxisView{nb * c->nz, c->ny, c->ny, c->ncol, false});
    for (int part = 0; part < 2; ++part)
      launch_circ_pass(inv_y, mats + (part == 0 ? c->o_iyr : c->o_iyi), 2 * c->ny, zr, zi, part == 0 ? y2r : y2i, nullptr);
    yr = y2r; yi = y2i;
  } else {       // y: one image per grid.z, P = ncol
    float* const y1r = c->p1;
    float* const y1i = c->p1 + nb * per_spec;
    const AxisGeom inv_y = axis_geom(AxisView{nb, c->ny, c->ny, c->ncol, false});
    for (int part = 0; part < 2; ++part)
      launch_circ_pass(inv_y, mats + (part == 0 ? c->o_iyr : c->o_iyi), 2 * c->ny, sre, sim, part == 0 ? y1r : y1i, nullptr);
    yr = y1r; yi = y1i;
  }
  TfC2R r{};
  r.re = yr; r.im = yi;
  r.cw = mats + c->o_xcw; r.sw = mats + c->o_xsw;
  r.y = out;
  r.rows = c->rows; r.nx = c->nx; r.ncol = c->ncol;
  hipLaunchKernelGGL(k_tfsc_c2r, dim3((unsigned)((c->rows + FC_T - 1) / FC_T), (unsigned)((c->nx + FC_T - 1) / FC_T), (unsigned)nb), dim3(256), 0,
                     nullptr, r);
}

// profile (sums_out / spec_out) or match (maps_out) of `batch` host maps, chunk by chunk
int sf_run(hh_sf* c, const float* maps, int64_t batch, const float* mask, bool has_thresh, double thresh, double* sums_out, float* spec_out,
           float* maps_out) {
  HH_HIP(nullptr, hipSetDevice(c->device));
  const int64_t per_map = c->per_map, per_spec = c->per_spec;
  const int nbins = c->nbins;
  const int64_t chunk = sf_chunk(c, batch);
  if (int rc = sf_reserve(c, chunk)) return rc;
  const size_t map_bytes = (size_t)per_map * sizeof(float);
  if (mask) HH_HIP(nullptr, hipMemcpy(c->mask, mask, map_bytes, hipMemcpyHostToDevice));
  const bool prepare = mask || has_thresh;
  const bool second = maps_out && mask;   // the spectrum that is scaled is the raw data's
  std::vector<float> re, im;
  for (int q = 0; q < 4; ++q) c->ms[q] = 0.0;
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = std::min(chunk, batch - b0);
    HH_HIP(nullptr, hipMemcpy(c->in, maps + b0 * per_map, (size_t)nb * map_bytes, hipMemcpyHostToDevice));
    HH_HIP(nullptr, hipEventRecord(c->ev[0], nullptr));
    const float* data = c->in;
    if (prepare) {
      hipLaunchKernelGGL(k_sf_prepare, dim3((unsigned)std::min<int64_t>((per_map + 255) / 256, 4096), (unsigned)nb), dim3(256), 0, nullptr, c->in,
                         mask ? c->mask.get() : nullptr, has_thresh ? 1 : 0, thresh, per_map, c->work);
      data = c->work;
    }
    HH_HIP(nullptr, hipMemsetAsync(c->amax, 0, (size_t)nb * sizeof(unsigned), nullptr));
    HH_HIP(nullptr, hipMemsetAsync(c->acc, 0, (size_t)nb * nbins * sizeof(long long), nullptr));
    hipLaunchKernelGGL(k_fc_absmax, dim3((unsigned)std::min<int64_t>((per_map + 255) / 256, 256), (unsigned)nb), dim3(256), 0, nullptr, data, per_map,
                       c->amax);
    hipLaunchKernelGGL(k_sf_scales, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, nullptr, c->amax, (int)nb, (double)per_map, c->scale);
    sf_forward(c, data, nb, true, spec_out || (maps_out && !second));
    const int64_t total = nb * nbins;
    hipLaunchKernelGGL(k_sf_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, c->acc, c->scale,
                       c->has_target ? c->tab + nbins : nullptr, nbins, total, c->sums, c->ratio);
    HH_HIP(nullptr, hipEventRecord(c->ev[1], nullptr));
    if (maps_out) {
      if (second) sf_forward(c, c->in, nb, false, true);
      HH_HIP(nullptr, hipEventRecord(c->ev[2], nullptr));
      sf_scale_inverse(c, nb, c->work);   // (records ev[3] after the scaling)
      HH_HIP(nullptr, hipEventRecord(c->ev[4], nullptr));
    }
    HH_HIP(nullptr, hipGetLastError());
    if (sums_out) HH_HIP(nullptr, hipMemcpy(sums_out + b0 * nbins, c->sums, (size_t)total * sizeof(double), hipMemcpyDeviceToHost));
    if (maps_out) HH_HIP(nullptr, hipMemcpy(maps_out + b0 * per_map, c->work, (size_t)nb * map_bytes, hipMemcpyDeviceToHost));
    if (spec_out) {   // interleaved complex64
      const size_t ps = (size_t)(nb * per_spec);
      re.resize(ps); im.resize(ps);
      HH_HIP(nullptr, hipMemcpy(re.data(), c->spec, ps * sizeof(float), hipMemcpyDeviceToHost));
      HH_HIP(nullptr, hipMemcpy(im.data(), c->spec + nb * per_spec, ps * sizeof(float), hipMemcpyDeviceToHost));
      float* const o = spec_out + 2 * b0 * per_spec;
      for (size_t i = 0; i < ps; ++i) {
        o[2 * i] = re[i];
        o[2 * i + 1] = im[i];
      }
    }
    HH_HIP(nullptr, hipDeviceSynchronize());
    const int n_ev = maps_out ? 4 : 1;
    for (int q = 0; q < n_ev; ++q) {
      float ms = 0.f;
      HH_HIP(nullptr, hipEventElapsedTime(&ms, c->ev[q], c->ev[q + 1]));
      c->ms[q] += ms;
    }
  }
  return HH_OK;
}

int sf_create(hh_sf* c, const double* qbins, const double* target, const double* freq) {
  const int nz = c->nz, ny = c->ny, nx = c->nx, ncol = c->ncol, nbins = c->nbins;
  std::vector<float> mats;
  std::vector<double> cs, sn;
  const int n1 = nz ? nz : ny;
  unit_circle(n1, cs, sn);
  c->o_c = append_axis_operator(mats, n1, AxisIndex::Dft, cs, 1.0, nullptr, 0.0);
  c->o_ms = append_axis_operator(mats, n1, AxisIndex::Dft, sn, -1.0, nullptr, 0.0);
  // inverse passes: (c + i s)(a + i b) = (c a - s b) + i (s a + c b), 1 / n each
  if (nz) {
    c->o_izr = append_axis_operator(mats, nz, AxisIndex::Dft, cs, 1.0 / nz, &sn, -1.0 / nz);
    c->o_izi = append_axis_operator(mats, nz, AxisIndex::Dft, sn, 1.0 / nz, &cs, 1.0 / nz);
    unit_circle(ny, cs, sn);
    c->o_re = append_axis_operator(mats, ny, AxisIndex::Dft, cs, 1.0, &sn, 1.0);
    c->o_im = append_axis_operator(mats, ny, AxisIndex::Dft, sn, -1.0, &cs, 1.0);
  }
  c->o_iyr = append_axis_operator(mats, ny, AxisIndex::Dft, cs, 1.0 / ny, &sn, -1.0 / ny);
  c->o_iyi = append_axis_operator(mats, ny, AxisIndex::Dft, sn, 1.0 / ny, &cs, 1.0 / ny);
  unit_circle(nx, cs, sn);
  c->o_xc = fc_xtable(mats, nx, ncol, cs);
  c->o_xs = fc_xtable(mats, nx, ncol, sn);
  c->o_xcw = tf_c2r_table(mats, nx, ncol, cs, 1.0 / nx, false);
  c->o_xsw = tf_c2r_table(mats, nx, ncol, sn, -1.0 / nx, true);
  if (int rc = ensure(nullptr, c->mats, mats.size())) return rc;
  HH_HIP(nullptr, hipMemcpy(c->mats, mats.data(), mats.size() * sizeof(float), hipMemcpyHostToDevice));
  std::vector<double> tab((size_t)2 * nbins + nz + ny + nx, 0.0);
  std::copy(qbins, qbins + nbins, tab.begin());
  if (target) std::copy(target, target + nbins, tab.begin() + nbins);
  std::copy(freq, freq + nz + ny + nx, tab.begin() + 2 * nbins);
  if (int rc = ensure(nullptr, c->tab, tab.size())) return rc;
  HH_HIP(nullptr, hipMemcpy(c->tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  return HH_OK;
}

}  // namespace

extern "C" int hh_sf_create(hh_sf** out, int device, int32_t ndim, const int32_t* shape, double apix, int32_t nbins, const double* qbins,
                            const double* target, const double* freq) try {
  if (!out) return fail(nullptr, HH_ERR_ARG, "hh_sf_create: NULL argument");
  *out = nullptr;
  if (!shape || !qbins || !freq) return fail(nullptr, HH_ERR_ARG, "hh_sf_create: NULL argument");
  if (ndim != 2 && ndim != 3) return fail(nullptr, HH_ERR_ARG, "hh_sf_create: ndim must be 2 or 3");
  const int top = ndim == 3 ? 512 : 1024;
  for (int a = 0; a < ndim; ++a)
    if (shape[a] < 2 || shape[a] > top)
      return fail(nullptr, HH_ERR_ARG, "hh_sf_create: the sides must lie in [2, 512] (3-D) or [2, 1024] (2-D)");
  if (!(apix > 0.0) || !(apix < 1.7e308)) return fail(nullptr, HH_ERR_ARG, "hh_sf_create: apix must be positive and finite");
  if (nbins < 2 || nbins > SF_MAX_BINS) return fail(nullptr, HH_ERR_ARG, "hh_sf_create: nbins must lie in [2, 726]");
  if (qbins[0] != 0.0) return fail(nullptr, HH_ERR_ARG, "hh_sf_create: qbins must start at 0");
  for (int i = 1; i < nbins; ++i)
    if (!(qbins[i] > qbins[i - 1]) || !(qbins[i] < 1.7e308)) return fail(nullptr, HH_ERR_ARG, "hh_sf_create: qbins must be finite and increasing");
  int sides = 0;
  for (int a = 0; a < ndim; ++a) sides += shape[a];
  for (int i = 0; i < sides; ++i)
    if (!(std::fabs(freq[i]) <= 1.0)) return fail(nullptr, HH_ERR_ARG, "hh_sf_create: a frequency lies outside [-1, 1]");
  if (int rc = use_device("hh_sf_create", device)) return rc;
  std::unique_ptr<hh_sf> c(new hh_sf);
  c->device = device; c->ndim = ndim;
  c->nz = ndim == 3 ? shape[0] : 0; c->ny = shape[ndim - 2]; c->nx = shape[ndim - 1];
  c->ncol = c->nx / 2 + 1;
  c->rows = (c->nz ? c->nz : 1) * c->ny;
  c->per_map = (int64_t)c->rows * c->nx; c->per_spec = (int64_t)c->rows * c->ncol;
  c->nbins = nbins; c->apix = apix; c->has_target = target != nullptr;
  if (int rc = sf_create(c.get(), qbins, target, freq)) return rc;
  *out = c.release();
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_sf_create")

extern "C" int hh_sf_profile(hh_sf* ctx, const float* maps, int32_t batch, const float* mask, int has_thresh, double thresh, double* sums,
                             float* spec_out) try {
  if (!ctx || !maps || !sums) return fail(nullptr, HH_ERR_ARG, "hh_sf_profile: NULL argument");
  if (batch < 1) return fail(nullptr, HH_ERR_ARG, "hh_sf_profile: batch must be >= 1");
  if (has_thresh && !(thresh == thresh)) return fail(nullptr, HH_ERR_ARG, "hh_sf_profile: thresh is NaN");
  return sf_run(ctx, maps, batch, mask, has_thresh != 0, thresh, sums, spec_out, nullptr);
} HH_CATCH_CTX(nullptr, "hh_sf_profile")

extern "C" int hh_sf_match(hh_sf* ctx, const float* maps, int32_t batch, const float* mask, int has_thresh, double thresh, float* maps_out,
                           double* sums) try {
  if (!ctx || !maps || !maps_out) return fail(nullptr, HH_ERR_ARG, "hh_sf_match: NULL argument");
  if (batch < 1) return fail(nullptr, HH_ERR_ARG, "hh_sf_match: batch must be >= 1");
  if (!ctx->has_target) return fail(nullptr, HH_ERR_STATE, "hh_sf_match: the context was created without a target");
  if (has_thresh && !(thresh == thresh)) return fail(nullptr, HH_ERR_ARG, "hh_sf_match: thresh is NaN");
  return sf_run(ctx, maps, batch, mask, has_thresh != 0, thresh, sums, nullptr, maps_out);
} HH_CATCH_CTX(nullptr, "hh_sf_match")

extern "C" int hh_sf_kernel_ms(hh_sf* ctx, double* ms) try {
  if (!ctx || !ms) return fail(nullptr, HH_ERR_ARG, "hh_sf_kernel_ms: NULL argument");
  for (int q = 0; q < 4; ++q) ms[q] = ctx->ms[q];
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_sf_kernel_ms")

extern "C" int hh_sf_destroy(hh_sf* ctx) try {
  if (ctx) (void)hipSetDevice(ctx->device);
  delete ctx;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_sf_destroy")
