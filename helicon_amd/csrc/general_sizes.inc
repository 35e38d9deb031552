// general_sizes.inc — the sweep for images that are not square powers of two (included by helicon_hip.hip).
//
// The reference takes any (ny, nx) (utils.py:31-47, 91-106; transforms.py:687-704): class-average boxes of
// 200-400 pixels, rectangular crops.  The tuned kernels above are instantiated for square sides 32...1024 with eight
// points per lane; this file is the same algorithm for any size with plain, runtime-sized kernels:
//   * k_gen_run_table        column transforms G_c[ky] of every table row, a direct sum over the footprint's rows with
//                            the ny-point phase table (any ny; rows ky = 0 ... ny/2, no packed row);
//   * k_gen_column_factors   column_factors_of for nx columns (padded to a multiple of 4);
//   * k_gen_fused            one ky block (8 rows, one wavefront each) x the candidates of one run per workgroup:
//                            build the row from the table slice and the candidate's factors, nx-point Stockham
//                            transform of radices {2, 3, 4, 5, any prime <= 31} between two LDS buffers, log1p|F|, three
//                            masked moments;  k_finalize turns them into Pearson scores as everywhere else;
//   * k_gen_dft_rows/cols    the experimental image's half-plane spectrum by direct DFT in float64 (once per sweep);
//   * k_gen_centres/raster   simulate_helical_projection for one candidate.
// Same window tests, same float32 roundings of the lattice coordinates and the same Hermitian weights as the tuned
// path; candidate lists are swept run by run (a list without shared-twist runs is a list of runs of length one).
// Not provided for general sizes: tilt / psi (the table identity needs them zero; the tuned path's raster pipeline
// covers them for power-of-two squares), Fourier filtering of the image.

namespace {

struct GenDims {
  int ny, nx;
  int nky;   // ny / 2 + 1 rows of the half plane
  int nxp;   // nx rounded up to a multiple of 4
};

constexpr int GEN_MAX_STAGES = 12;
constexpr size_t GEN_SEG_NK = 512;   // several segments: bins per k_segment_corr workgroup row (the flat bin axis is padded to a multiple)
struct GenPlan {
  int n_stages;
  int radix[GEN_MAX_STAGES];
  unsigned magic[GEN_MAX_STAGES];  // ceil(2^32 / NS) of the stage: j / NS = umulhi(j, magic) for j < 2^16
};

// ---- simulate ---------------------------------------------------------------------------------------------------
__global__ void k_gen_centres(const double* __restrict__ params, const double* __restrict__ units, DevGeom g, int m,
                              float2* __restrict__ out) {
  const Cand c = decode_candidate(params, g);
  const int ci = blockIdx.x * blockDim.x + threadIdx.x;
  if (ci < m && ci < c.M) out[ci] = centre_position(c, g, units, ci);
}

// one thread per pixel; the centres are visited in lattice order (fixed summation order), truncated footprints with
// the raster kernel's own tests
__global__ void k_gen_raster(const float2* __restrict__ cent, int m, DevGeom g, GenDims d, float* __restrict__ img) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= d.nx) return;
  const float rp = (float)g.rpx;
  const float k2 = g.inv_sigma2 * 1.44269504088896341f;
  const float qx = (float)(x - d.nx / 2) * g.apix, qy = (float)(y - d.ny / 2) * g.apix;
  float acc = 0.f;
  for (int ci = 0; ci < m; ++ci) {
    const float2 p = cent[ci];
    const float cx = p.y * g.inv_apix + (float)(d.nx / 2);
    const float cy = p.x * g.inv_apix + (float)(d.ny / 2);
    if (!(fabsf((float)x - cx) <= rp)) continue;
    if (y < (int)ceilf(cy - rp) || y > (int)floorf(cy + rp)) continue;
    const float dx = qx - p.y, dy = qy - p.x;
    acc += __builtin_amdgcn_exp2f(fmaf(dy * dy, -k2, -(dx * dx * k2)));
  }
  img[(size_t)y * d.nx + x] = acc;
}

// ---- reference spectrum: direct DFT, float64 ----------------------------------------------------------------------
// R[s][y][kx] = sum_x img[s][y][x] W_nx^(kx x)
__global__ void k_gen_dft_rows(const float* __restrict__ img, GenDims d, double2* __restrict__ r) {
  const int kx = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, s = blockIdx.z;
  if (kx >= d.nx) return;
  const float* const row = img + ((size_t)s * d.ny + y) * d.nx;
  double re = 0, im = 0;
  int idx = 0;  // (kx * x) mod nx
  for (int x = 0; x < d.nx; ++x) {
    double sn, cs;
    sincospi(-2.0 * (double)idx / (double)d.nx, &sn, &cs);
    re += (double)row[x] * cs;
    im += (double)row[x] * sn;
    idx += kx;
    if (idx >= d.nx) idx -= d.nx;
  }
  r[((size_t)s * d.ny + y) * d.nx + kx] = make_double2(re, im);
}

// F[s][ky][kx] = sum_y R[s][y][kx] W_ny^(ky y), ky <= ny / 2
__global__ void k_gen_dft_cols(const double2* __restrict__ r, GenDims d, double2* __restrict__ f) {
  const int kx = blockIdx.x * blockDim.x + threadIdx.x, ky = blockIdx.y, s = blockIdx.z;
  if (kx >= d.nx) return;
  double re = 0, im = 0;
  int idx = 0;
  for (int y = 0; y < d.ny; ++y) {
    double sn, cs;
    sincospi(-2.0 * (double)idx / (double)d.ny, &sn, &cs);
    const double2 v = r[((size_t)s * d.ny + y) * d.nx + kx];
    re += v.x * cs - v.y * sn;
    im += v.x * sn + v.y * cs;
    idx += ky;
    if (idx >= d.ny) idx -= d.ny;
  }
  f[((size_t)s * d.nky + ky) * d.nx + kx] = make_double2(re, im);
}

// ---- candidates with tilt / psi on a general image size: scored from the candidate's own float64 spectrum ----------------------
// One workgroup per candidate: q = log1p|F| (or |F|) over the half plane, the segment-independent moments once, the
// covariance numerator per segment; sums in float64 in a fixed order (thread-strided, then a tree), Pearson as
// pearson_from_moments.  f: [B][nh] (k_gen_dft_cols), w2: [S][nh] {w, w (E - Ebar)}.
__global__ __launch_bounds__(256) void k_gen_direct_scores(const double2* __restrict__ f, size_t nh, int log_flag,
                                                           const float2* __restrict__ w2, int n_seg, const RefConsts* __restrict__ rc,
                                                           float* __restrict__ scores, int64_t ld, int64_t g0) {
  __shared__ double red[3][256];
  const int b = blockIdx.x;
  const double2* const fb = f + (size_t)b * nh;
  auto block_sum3 = [&](double& a, double& bb, double& cc) {
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = bb; red[2][threadIdx.x] = cc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off)
        for (int e = 0; e < 3; ++e) red[e][threadIdx.x] += red[e][threadIdx.x + off];
      __syncthreads();
    }
    a = red[0][0]; bb = red[1][0]; cc = red[2][0];
    __syncthreads();
  };
  double s1 = 0, s2 = 0, dummy = 0;
  for (size_t i = threadIdx.x; i < nh; i += 256) {
    const double amp = hypot(fb[i].x, fb[i].y);
    const double q = log_flag ? log1p(amp) : amp;
    const double w = (double)w2[i].x;
    s1 += w * q;
    s2 += w * q * q;
  }
  block_sum3(s1, s2, dummy);
  for (int s = 0; s < n_seg; ++s) {
    double s3 = 0, z0 = 0, z1 = 0;
    const float2* const ws = w2 + (size_t)s * nh;
    for (size_t i = threadIdx.x; i < nh; i += 256) {
      const double amp = hypot(fb[i].x, fb[i].y);
      s3 += (double)ws[i].y * (log_flag ? log1p(amp) : amp);
    }
    block_sum3(s3, z0, z1);
    if (threadIdx.x == 0) scores[(size_t)s * ld + g0 + b] = pearson_from_moments(s1, s2, s3, rc[s]);
  }
}

// ---- Gaussian low / high pass of one image, any (ny, nx) (helicon.low_high_pass_filter, lib/filters.py:314-372) ------
// The reference multiplies fft2(data) by np.fft.fftshift(filter), the filter laid out on the CENTRED float32 grid
// (i - n // 2) / (n // 2): unshifted index k therefore takes the filter value of centred index (k + ceil(n / 2)) mod n
// (for an odd side that is NOT the frequency's own position — fftshift, not ifftshift — and the quirk is kept), and
// np.real(ifftn(.)) is returned.  Direct float64 transforms: this is a once-per-image step.
__device__ __forceinline__ double gen_pass_filter(int ky, int kx, const GenDims& d, double f2_lp, double f2_hp) {
  const int iy = (ky + (d.ny + 1) / 2) % d.ny, ix = (kx + (d.nx + 1) / 2) % d.nx;
  const float y = (float)(iy - d.ny / 2) / (float)(d.ny / 2), x = (float)(ix - d.nx / 2) / (float)(d.nx / 2);
  const float r2 = x * x + y * y;
  double f = 1.0;
  if (f2_lp > 0) f *= exp(-f2_lp * (double)r2);
  if (f2_hp > 0) f *= 1.0 - exp(-f2_hp * (double)r2);
  return f;
}

// G[ky][kx] = F_full[ky][kx] filter(ky, kx) for every ky (the half plane's Hermitian extension)
__global__ void k_gen_filter_full(const double2* __restrict__ f, GenDims d, double f2_lp, double f2_hp, double2* __restrict__ g) {
  const int kx = blockIdx.x * blockDim.x + threadIdx.x, ky = blockIdx.y;
  if (kx >= d.nx) return;
  double2 v;
  if (ky < d.nky) {
    v = f[(size_t)ky * d.nx + kx];
  } else {
    v = f[(size_t)(d.ny - ky) * d.nx + (d.nx - kx) % d.nx];
    v.y = -v.y;
  }
  const double w = gen_pass_filter(ky, kx, d, f2_lp, f2_hp);
  g[(size_t)ky * d.nx + kx] = make_double2(v.x * w, v.y * w);
}

// R[y][kx] = sum_ky G[ky][kx] W_ny^(-ky y)
__global__ void k_gen_idft_cols(const double2* __restrict__ g, GenDims d, double2* __restrict__ r) {
  const int kx = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (kx >= d.nx) return;
  double re = 0, im = 0;
  int idx = 0;
  for (int ky = 0; ky < d.ny; ++ky) {
    double sn, cs;
    sincospi(2.0 * (double)idx / (double)d.ny, &sn, &cs);
    const double2 v = g[(size_t)ky * d.nx + kx];
    re += v.x * cs - v.y * sn;
    im += v.x * sn + v.y * cs;
    idx += y;
    if (idx >= d.ny) idx -= d.ny;
  }
  r[(size_t)y * d.nx + kx] = make_double2(re, im);
}

// out[y][x] = Re sum_kx R[y][kx] W_nx^(-kx x) / (ny nx)
__global__ void k_gen_idft_rows(const double2* __restrict__ r, GenDims d, float* __restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= d.nx) return;
  double re = 0;
  int idx = 0;
  for (int kx = 0; kx < d.nx; ++kx) {
    double sn, cs;
    sincospi(2.0 * (double)idx / (double)d.nx, &sn, &cs);
    const double2 v = r[(size_t)y * d.nx + kx];
    re += v.x * cs - v.y * sn;
    idx += x;
    if (idx >= d.nx) idx -= d.nx;
  }
  out[(size_t)y * d.nx + x] = (float)(re / ((double)d.ny * (double)d.nx));
}

// full fftshifted plane from the half plane (hh_power_spectrum): pwr = log1p|F| or |F|, phase, min / max
__global__ void k_gen_expand(const double2* __restrict__ f, GenDims d, int log_flag, float* __restrict__ pwr,
                             float* __restrict__ phase, unsigned* __restrict__ minmax) {
  const int iy = blockIdx.x;
  const int uy = (iy - d.ny / 2 + d.ny) % d.ny;  // fftshift: index u moves to (u + n/2) mod n
  float lmin = INFINITY, lmax = 0.f;
  for (int ix = threadIdx.x; ix < d.nx; ix += blockDim.x) {
    const int ux = (ix - d.nx / 2 + d.nx) % d.nx;
    double2 v;
    if (uy < d.nky) {
      v = f[(size_t)uy * d.nx + ux];
    } else {
      v = f[(size_t)(d.ny - uy) * d.nx + (d.nx - ux) % d.nx];
      v.y = -v.y;
    }
    const double a = sqrt(v.x * v.x + v.y * v.y);
    const float q = (float)(log_flag ? log1p(a) : a);
    pwr[(size_t)iy * d.nx + ix] = q;
    if (phase) phase[(size_t)iy * d.nx + ix] = (float)atan2(v.y, v.x);
    lmin = fminf(lmin, q);
    lmax = fmaxf(lmax, q);
  }
  atomicMin(&minmax[0], __float_as_uint(lmin));
  atomicMax(&minmax[1], __float_as_uint(lmax));
}

// 1 into *differ when two lists of n 64-bit words are not bit-identical
__global__ void k_gen_same_list(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ b, int64_t n,
                                int* __restrict__ differ) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) bad |= a[i] != b[i];
  if (bad) *differ = 1;
}

// ---- run tables ---------------------------------------------------------------------------------------------------
struct GenTableArgs {
  const double* params;   // first candidate of run r at params + 4 * run_first[r]
  const int* run_first;   // [runs] candidate index (inside the batch) of each run's first candidate
  const int* run_imax;    // [runs]
  const double* units;
  const float2* tw_ny;    // [ny] exp(-2 pi i k / ny)
  float2* table;          // [runs][cap][nky]
  int cap;
  DevGeom g;
  GenDims d;
};

// row (i, u) of a run's table: sum over the csym copies s of G_(i,s,u)[ky], ky = 0 ... ny/2 (k_run_table's sums with
// an ny-point phase table; one workgroup = 4 table rows, thread = ky strided)
__global__ __launch_bounds__(256) void k_gen_run_table(GenTableArgs a) {
  constexpr int SUB = 4;
  const int run = blockIdx.y;
  const DevGeom& g = a.g;
  Cand c = decode_candidate(a.params + 4 * (size_t)a.run_first[run], g);
  c.imax = a.run_imax[run];
  const int rows = (2 * c.imax + 1) * g.n_units;
  float2* const tab = a.table + (size_t)run * a.cap * a.d.nky;
  const float rp = (float)g.rpx;
  const float k2 = g.inv_sigma2 * 1.44269504088896341f;
  const int ny = a.d.ny;
  for (int sub = 0; sub < SUB; ++sub) {
    const int row = blockIdx.x * SUB + sub;
    if (row >= rows) return;
    const int ir = row / g.n_units, u = row % g.n_units;
    for (int ky = threadIdx.x; ky < a.d.nky; ky += 256) {
      float2 acc = make_float2(0.f, 0.f);
      for (int sc = 0; sc < c.csym; ++sc) {
        const float yc = centre_position(c, g, a.units, (ir * c.csym + sc) * g.n_units + u).x;
        const float cy = yc * g.inv_apix + (float)(ny / 2);
        if (!(cy >= -rp - 1.f && cy <= (float)ny + rp)) continue;
        const int y0 = max(0, (int)ceilf(cy - rp)), y1 = min(ny - 1, (int)floorf(cy + rp));
        int idx = (int)(((long long)ky * y0) % ny);
        for (int y = y0; y <= y1; ++y) {
          const float dyv = (float)(y - ny / 2) * g.apix - yc;
          const float e = __builtin_amdgcn_exp2f(-dyv * dyv * k2);
          const float2 w = a.tw_ny[idx];
          acc.x = fmaf(e, w.x, acc.x);
          acc.y = fmaf(e, w.y, acc.y);
          idx += ky;
          if (idx >= ny) idx -= ny;
        }
      }
      tab[(size_t)row * a.d.nky + ky] = acc;
    }
  }
}

// ---- column factors -----------------------------------------------------------------------------------------------
struct GenFactorArgs {
  const double* params;   // [B][4]
  const double* units;
  const int* run_of;      // [B] run of every candidate of the batch
  const int* run_imax;    // [runs]
  float* eg;              // [B][kg][nxp]
  int* cgs;               // [B][nxp/4 + 4]
  int kg, rows_lds;
  DevGeom g;
  GenDims d;
};

// column_factors_of for nx columns: one workgroup (256 threads) per candidate, threads stride over the columns
__global__ __launch_bounds__(256) void k_gen_column_factors(GenFactorArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_g[];
  float* const xc_tab = reinterpret_cast<float*>(smem_g);       // [rows_lds]
  int* const kc_s = reinterpret_cast<int*>(xc_tab + a.rows_lds);
  const int b = blockIdx.x, tid = threadIdx.x;
  const DevGeom& g = a.g;
  const GenDims& d = a.d;
  const Cand c = decode_candidate(a.params + 4 * (size_t)b, g);
  const int imax_t = a.run_imax[a.run_of[b]];
  const int rows = (2 * imax_t + 1) * g.n_units;
  const float rp = (float)g.rpx;
  const float k2 = g.inv_sigma2 * 1.44269504088896341f;
  if (tid == 0) *kc_s = 0;
  for (int r = tid; r < a.rows_lds; r += 256) {
    int i = r - imax_t, u = 0;
    if (g.n_units > 1) {
      i = r / g.n_units - imax_t;
      u = r % g.n_units;
    }
    const bool ok = r < rows && i >= -c.imax && i <= c.imax;
    xc_tab[r] = ok ? (float)a.units[3 * u + 2] + (float)((double)i * c.rise) : __builtin_nanf("");
  }
  __syncthreads();
  const int stride = d.nxp / 4 + 4;
  int* const cgo = a.cgs + (size_t)b * stride;
  for (int x = tid; x < d.nxp; x += 256) {  // nxp is a multiple of 4: the four threads of a column group stay together
    const int x0 = x & ~3;
    int cg = 0;
    if (c.M > 0) {
      const float lo = ((float)(x0 - d.nx / 2) * g.apix - rp * g.apix - g.slack) / (float)c.rise;
      const int i0 = max(-c.imax, (int)ceilf(fmaxf(lo, -2.0e9f)));
      cg = (min(i0, c.imax) + imax_t) * g.n_units;
    }
    cg = max(0, min(cg, a.rows_lds - a.kg));
    unsigned hit = 0;
    if (x < d.nx)
      for (int k = 0; k < a.kg; ++k) {
        const float cx = xc_tab[cg + k] * g.inv_apix + (float)(d.nx / 2);
        hit |= fabsf((float)x - cx) <= rp ? (1u << k) : 0u;
      }
    hit |= __shfl_xor((int)hit, 1, 64);
    hit |= __shfl_xor((int)hit, 2, 64);
    const int first = hit ? __ffs((int)hit) - 1 : 0;
    const int count = hit ? (32 - __clz((int)hit)) - first : 0;
    cg += first;
    if ((x & 3) == 0 && count > 0) atomicMax(kc_s, count);
    for (int k = 0; k < a.kg; ++k) {
      float wgt = 0.f;
      if (k < count && x < d.nx) {
        const float xc = xc_tab[cg + k];
        const float cx = xc * g.inv_apix + (float)(d.nx / 2);
        const float dx = (float)(x - d.nx / 2) * g.apix - xc;
        if (fabsf((float)x - cx) <= rp) wgt = __builtin_amdgcn_exp2f(-dx * dx * k2);
      }
      a.eg[((size_t)b * a.kg + k) * d.nxp + x] = wgt;
    }
    if ((x & 3) == 0) cgo[x >> 2] = cg;
  }
  __syncthreads();
  if (tid < 4) cgo[d.nxp / 4 + tid] = *kc_s;
}

// ---- the fused pass ------------------------------------------------------------------------------------------------
struct GenFusedArgs {
  const float2* table;    // [runs][cap][nky]
  const int* run_imax;    // [runs]
  const int* layer_run;   // [layers] grid layer -> run (a run is cut into one or more layers of candidates: gen_sweep)
  const int* layer_first; // [layers] first candidate of the layer inside the batch
  const int* layer_count; // [layers] candidates of the layer
  const float* eg;        // [B][kg][nxp]
  const int* cgs;         // [B][nxp/4 + 4]
  const float2* w2;       // [nky][nx] {w, w (E - Ebar)} natural order
  const float2* tw_nx;    // [nx]
  double* partials;       // [B][nky][3]
  float* q_out;           // several segments: [B][q_stride] masked q, bin (ky, kx) at ky nx + kx (NULL: one segment)
  int64_t q_stride;
  int cap, rows_lds, kg, n_units, log_flag;
  GenPlan plan;
  GenDims d;
};

template <int R>
__device__ __forceinline__ void gen_bfly(float2 (&a)[R], const float2* tw, int step);  // step = nx / R

template <>
__device__ __forceinline__ void gen_bfly<2>(float2 (&a)[2], const float2*, int) { bfly<2>(a); }
template <>
__device__ __forceinline__ void gen_bfly<4>(float2 (&a)[4], const float2*, int) { bfly<4>(a); }
template <>
__device__ __forceinline__ void gen_bfly<8>(float2 (&a)[8], const float2*, int) { bfly<8>(a); }

template <>
__device__ __forceinline__ void gen_bfly<3>(float2 (&a)[3], const float2*, int) {
  constexpr float s = 0.86602540378443864676f;  // sin(2 pi / 3)
  const float2 t1 = cadd(a[1], a[2]), t2 = csub(a[1], a[2]);
  const float2 m = make_float2(a[0].x - 0.5f * t1.x, a[0].y - 0.5f * t1.y);
  const float2 r = make_float2(s * t2.y, -s * t2.x);  // -i s t2
  a[0] = cadd(a[0], t1);
  a[1] = cadd(m, r);
  a[2] = csub(m, r);
}

template <>
__device__ __forceinline__ void gen_bfly<5>(float2 (&a)[5], const float2*, int) {
  constexpr float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;   // cos(2 pi/5), cos(4 pi/5)
  constexpr float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;    // sin(2 pi/5), sin(4 pi/5)
  const float2 p1 = cadd(a[1], a[4]), m1 = csub(a[1], a[4]), p2 = cadd(a[2], a[3]), m2 = csub(a[2], a[3]);
  const float2 x0 = a[0];
  const float2 u1 = make_float2(x0.x + c1 * p1.x + c2 * p2.x, x0.y + c1 * p1.y + c2 * p2.y);
  const float2 u2 = make_float2(x0.x + c2 * p1.x + c1 * p2.x, x0.y + c2 * p1.y + c1 * p2.y);
  // -i (s1 m1 + s2 m2) and -i (s2 m1 - s1 m2)
  const float2 v1 = make_float2(s1 * m1.y + s2 * m2.y, -(s1 * m1.x + s2 * m2.x));
  const float2 v2 = make_float2(s2 * m1.y - s1 * m2.y, -(s2 * m1.x - s1 * m2.x));
  a[0] = make_float2(x0.x + p1.x + p2.x, x0.y + p1.y + p2.y);
  a[1] = cadd(u1, v1);
  a[4] = csub(u1, v1);
  a[2] = cadd(u2, v2);
  a[3] = csub(u2, v2);
}

// one Stockham stage of radix R (NS = product of the earlier radices) from src to dst, by one wavefront
template <int R>
__device__ __forceinline__ void gen_stage(const float2* src, float2* dst, const float2* tw, int nx, int ns, unsigned magic,
                                          int lane) {
  const int nb = nx / R, step = nb / ns;  // step = nx / (NS R): twiddle index of (r, k) is r k step < nx
  for (int j = lane; j < nb; j += 64) {
    const int q = ns == 1 ? j : (int)__umulhi((unsigned)j, magic);  // j / NS
    const int k = j - q * ns;
    float2 a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = src[j + r * nb];
    if (ns > 1) {
#pragma unroll
      for (int r = 1; r < R; ++r) a[r] = cmul(a[r], tw[r * k * step]);
    }
    gen_bfly<R>(a, tw, nb);
    float2* const o = dst + q * ns * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r) o[r * ns] = a[r];
  }
}

// any other (prime) radix p <= 31: p^2 terms per butterfly straight from LDS, no register array
__device__ __forceinline__ void gen_stage_prime(const float2* src, float2* dst, const float2* tw, int nx, int p, int ns,
                                                unsigned magic, int lane) {
  const int nb = nx / p, step = nb / ns;
  for (int j = lane; j < nb; j += 64) {
    const int q = ns == 1 ? j : (int)__umulhi((unsigned)j, magic);
    const int k = j - q * ns;
    float2* const o = dst + q * ns * p + k;
    for (int m = 0; m < p; ++m) {  // output m of the p-point DFT of the twiddled inputs
      float2 acc = make_float2(0.f, 0.f);
      int idx = 0;  // (r m) mod p
      for (int r = 0; r < p; ++r) {
        float2 v = src[j + r * nb];
        if (ns > 1 && r > 0) v = cmul(v, tw[r * k * step]);
        const float2 w = tw[idx * nb];  // W_p^(r m) = W_nx^(nb (r m mod p))
        acc.x += v.x * w.x - v.y * w.y;
        acc.y += v.x * w.y + v.y * w.x;
        idx += m;
        if (idx >= p) idx -= p;
      }
      o[m * ns] = acc;
    }
  }
}

constexpr int GEN_THREADS = 512;  // 8 wavefronts = the 8 rows of a ky block

// GEN_WMAX: weight registers per lane (bins kx = lane + 64 m, m < GEN_WMAX): 4 for nx <= 256, 8 for nx <= 512, 16 above
template <int GEN_WMAX>
__global__ __launch_bounds__(GEN_THREADS) void k_gen_fused(GenFusedArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_g[];
  const GenDims& d = a.d;
  const int tid = threadIdx.x, gi = tid >> 6, lane = tid & 63;
  const int stride_cg = d.nxp / 4 + 4;
  float2* const bufs = reinterpret_cast<float2*>(smem_g);                       // [8][2][nxp]
  float2* const gs = bufs + (size_t)16 * d.nxp;                                 // [8][rows_lds]
  float2* const twl = gs + (size_t)8 * a.rows_lds;                              // [nx]
  float* const eg = reinterpret_cast<float*>(twl + ((d.nx + 1) & ~1));          // [kg][nxp] (16-byte aligned)
  int* const cgs = reinterpret_cast<int*>(eg + (size_t)a.kg * d.nxp);           // [nxp/4 + 4]
  float2* const b0 = bufs + (size_t)gi * 2 * d.nxp;
  float2* const b1 = b0 + d.nxp;
  const int kb = blockIdx.x, run = a.layer_run[blockIdx.y];
  const int row = kb * 8 + gi;
  const bool active = row < d.nky;
  const int cfirst = a.layer_first[blockIdx.y], nc = a.layer_count[blockIdx.y];

  for (int i = tid; i < d.nx; i += GEN_THREADS) twl[i] = a.tw_nx[i];
  {
    const int rows = (2 * a.run_imax[run] + 1) * a.n_units;
    const float2* const tab = a.table + (size_t)run * a.cap * d.nky;
    for (int e = tid; e < a.rows_lds * 8; e += GEN_THREADS) {
      const int cr = e >> 3, r8 = e & 7;
      const int ky = kb * 8 + r8;
      gs[r8 * a.rows_lds + cr] = (cr < rows && ky < d.nky) ? tab[(size_t)cr * d.nky + ky] : make_float2(0.f, 0.f);
    }
  }
  // the row's weights {w, w (E - Ebar)} of the lane's bins kx = lane + 64 m, kept in registers for all candidates
  float2 wreg[GEN_WMAX];
  {
    const float2* const wrow = a.w2 + (size_t)(active ? row : 0) * d.nx;
#pragma unroll
    for (int m = 0; m < GEN_WMAX; ++m) {
      const int kx = lane + 64 * m;
      wreg[m] = kx < d.nx ? wrow[kx] : make_float2(0.f, 0.f);
    }
  }
  const int n_e4 = a.kg * (d.nxp / 4);

#pragma unroll 1
  for (int cc = 0; cc < nc; ++cc) {
    const size_t b = (size_t)(cfirst + cc);
    __syncthreads();  // the previous candidate's factors have been consumed (and the staging above is complete)
    {
      const float4* const src = reinterpret_cast<const float4*>(a.eg + b * a.kg * d.nxp);
      for (int e = tid; e < n_e4; e += GEN_THREADS) reinterpret_cast<float4*>(eg)[e] = src[e];
      for (int e = tid; e < stride_cg; e += GEN_THREADS) cgs[e] = a.cgs[b * stride_cg + e];
    }
    __syncthreads();
    if (!active) continue;  // (a row past ny/2 in the last block: only the barriers)
    const int kc = max(0, min(a.kg, cgs[d.nxp / 4]));
    // ---- the row of H: four columns per lane and step
    for (int xg = lane; xg < d.nxp / 4; xg += 64) {
      const float2* const grow = gs + gi * a.rows_lds + cgs[xg];
      const float* const erow = eg + 4 * xg;
      float2 p0 = make_float2(0.f, 0.f), p1 = p0, p2 = p0, p3 = p0;
      for (int k = 0; k < kc; ++k) {
        const float2 gk = grow[k];
        const float4 e4 = *reinterpret_cast<const float4*>(erow + (size_t)k * d.nxp);
        p0.x = fmaf(e4.x, gk.x, p0.x); p0.y = fmaf(e4.x, gk.y, p0.y);
        p1.x = fmaf(e4.y, gk.x, p1.x); p1.y = fmaf(e4.y, gk.y, p1.y);
        p2.x = fmaf(e4.z, gk.x, p2.x); p2.y = fmaf(e4.z, gk.y, p2.y);
        p3.x = fmaf(e4.w, gk.x, p3.x); p3.y = fmaf(e4.w, gk.y, p3.y);
      }
      float4* const dst = reinterpret_cast<float4*>(b0 + 4 * xg);
      dst[0] = make_float4(p0.x, p0.y, p1.x, p1.y);
      dst[1] = make_float4(p2.x, p2.y, p3.x, p3.y);
    }
    group_sync<64>();
    // ---- nx-point transform along x, ping-pong between the row's two buffers
    float2* src = b0;
    float2* dst = b1;
    int ns = 1;
    for (int s = 0; s < a.plan.n_stages; ++s) {
      const int r = a.plan.radix[s];
      const unsigned mg = a.plan.magic[s];
      switch (r) {
        case 2: gen_stage<2>(src, dst, twl, d.nx, ns, mg, lane); break;
        case 3: gen_stage<3>(src, dst, twl, d.nx, ns, mg, lane); break;
        case 4: gen_stage<4>(src, dst, twl, d.nx, ns, mg, lane); break;
        case 5: gen_stage<5>(src, dst, twl, d.nx, ns, mg, lane); break;
        case 8: gen_stage<8>(src, dst, twl, d.nx, ns, mg, lane); break;
        default: gen_stage_prime(src, dst, twl, d.nx, r, ns, mg, lane); break;
      }
      group_sync<64>();
      float2* const t = src; src = dst; dst = t;
      ns *= r;
    }
    // ---- amplitudes and the three masked moments of the row
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int m = 0; m < GEN_WMAX; ++m) {
      const int kx = lane + 64 * m;
      if (64 * m < d.nx) {   // (wave-uniform; lanes past the row's end carry zero weights and read a valid slot)
        const float2 w = wreg[m];
        const float2 f = src[min(kx, d.nx - 1)];
        const float av = __builtin_amdgcn_sqrtf(f.x * f.x + f.y * f.y);
        const float q = a.log_flag ? __log2f(1.0f + av) : av;
        s1 += w.x * q;
        s2 += w.x * q * q;
        s3 += w.y * q;
        if (a.q_out && kx < d.nx) a.q_out[b * a.q_stride + (size_t)row * d.nx + kx] = w.x > 0.f ? q : 0.f;
      }
    }
    s1 = group_sum<64>(s1);
    s2 = group_sum<64>(s2);
    s3 = group_sum<64>(s3);
    if (lane == group_sum_lane<64>()) {
      double* const o = a.partials + (b * d.nky + row) * 3;
      o[0] = s1;
      o[1] = s2;
      o[2] = s3;
    }
    group_sync<64>();  // the moments' reads of src are done before the next candidate's build writes b0
  }
}

}  // namespace

// one batch of a sweep as gen_sweep launches it
struct GenBatchPlan {
  int nb, runs, rows, kg, rows_lds, n_kb, layers;
  size_t lds;
  bool two_step;
  GenRowsPlan rp;
};

// state of a general-size context (owned by hh_ctx)
struct hh_gen {
  GenDims d{};
  GenPlan plan{};
  DevBuf<float2> d_tw_nx;
  DevBuf<float2> d_tw_ny;
  DevBuf<float2> d_w2;             // [S][nky][nx]
  DevBuf<float2> d_table;
  DevBuf<float> d_eg;
  DevBuf<int> d_cgs;
  DevBuf<int> d_runs;              // [4][cap_runs]: run_first, run_count, run_imax, (run_of: [cap_cand])
  DevBuf<int> d_run_of;
  DevBuf<int> d_layers;            // [3][layers]: layer_run, layer_first, layer_count
  int slots = 0;                   // resident k_gen_fused workgroups (for the LDS size slots_lds)
  size_t slots_lds = 0;
  bool slots_two_step = false;      // ... counted for k_gen_rows (gen_rows.hip) rather than k_gen_fused
  DevBuf<double> d_partials;
  DevBuf<double2> d_r;             // DFT scratch
  DevBuf<double2> d_f;
  DevBuf<float2> d_cent;
  std::vector<double> h_params;    // host copy of a device-only candidate list
  // the last single-batch sweep: its list (host and device copies), geometry and launch plan; d_runs / d_run_of /
  // d_layers still hold its arrays
  bool plan_valid = false, plan_stockham = false;
  int64_t plan_n = 0, plan_batch_cap = 0;
  DevGeom plan_geom{};
  GenBatchPlan last{};
  std::vector<double> plan_params;
  DevBuf<double> d_plan_params;
  DevBuf<int> d_differ;
  // several segments through the two-step row kernel: q of a batch [b_pad][kp] (kp = nky nx rounded up to GEN_SEG_NK),
  // all segments' centred spectra [s_pad][kp], covariance numerators [kp / GEN_SEG_NK][b_pad][s_pad], summed moments
  DevBuf<float> d_q;
  DevBuf<float> d_wec;
  DevBuf<float> d_cpart;
  DevBuf<double> d_psum;
  DevBuf<RefConsts> d_ref;
  int32_t last_row_kernel[3] = {0, 0, 0};   // the last sweep's row kernel: {R1, R2, LDS bytes}, {0, 0, LDS} Stockham, all zero direct
  bool direct_only = false;       // nx without a row-transform plan (a prime factor above 31): every sweep is gen_sweep_direct
  int s_pad = 0, b_pad = 0;
  size_t kp = 0;
  DevBuf<int> d_seg_slices;        // [n_seg_slices] 512-bin slices of the flat bin axis with any weight
  int n_seg_slices = 0;
};

