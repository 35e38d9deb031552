// zoom_sweep.inc — the sweep on Fourier-zoomed spectra: compute_power_spectra(sim, apix, cutoff_res, output_size) of every
// candidate against the same view of the experimental image (lib/transforms.py:663-713, 771-820), in one batched call.
//
// The zoomed transform is the image's Fourier sum at ony x onx frequencies that are no FFT grid (fourier_zoom.inc).  A
// simulated projection is a sum of truncated Gaussian footprints and every footprint is a product ex_c(x) ey_c(y), so
//     F[u][v] = sum_c Gy_c[u] Gx_c[v],   Gy_c[u] = sum_y ey_c(y) e^{-2 pi i f_y[u] (y - ny/2)},   Gx_c[v] likewise along x
// over the lattice centres c whose footprint meets the image: one complex [ony x C] . [C x onx] product per candidate.
// k_zoom_sweep does all of it for one output tile of one candidate: lattice centres with the sweep's own device code
// (decode_candidate / centre_position), the raster's window tests, the factors by Horner's rule over a footprint's taps,
// the product on the exact-f32 MFMA (32x32x2, K staged through LDS in mfma_tile.inc's layout, four real products for
// the complex one), and the epilogue |F| -> log1p -> masked moments fused, so F never leaves the registers.  The
// reference side is k_zoom_rows / k_zoom_cols on the device plus k_zoom_weights ({w, w (E - Ebar)} per segment).
// With a spectrum filter set (hh_set_spectrum_filter, at the end of this file) the kernel's other epilogue stores q instead
// and filtered_sweep.inc takes it from there; without a zoom that runs at the identity zoom (the image's shape and Nyquist).
//
// The whole plane is computed: the zoomed grid is not closed under negation (row ony/2 and column onx/2 of an even side
// have no Friedel partner on the grid), so there is no half-plane fold here; tiles without a masked bin are skipped.

struct hh_zoom {
  bool on = false;
  int ony = 0, onx = 0;
  double cutoff_y = 0, cutoff_x = 0;
  double apix_ref = 0;            // pixel size the reference was prepared with (the frequencies depend on it)
  int tiles_v = 0, n_tiles = 0;   // active output tiles (any masked bin)
  DevBuf<float> d_img;            // [S][ny][nx]
  DevBuf<double2> d_r;            // [ny][onx] row pass of one image
  DevBuf<float> d_pwr;            // [ony][onx] fftshifted spectrum of one image
  DevBuf<unsigned> d_mm;          // k_zoom_cols' min / max slots (unused here: Pearson drops the normalisation)
  DevBuf<uint8_t> d_mask;         // [ony][onx] fftshifted
  DevBuf<float> d_w;              // [ony][onx] unshifted mask weight
  DevBuf<float> d_wec;            // [S][ony][onx] unshifted w (E_s - Ebar_s)
  DevBuf<RefConsts> d_ref;        // [S]
  DevBuf<int> d_tiles;
  DevBuf<double> d_partials;      // [S][batch][n_tiles][3]
  std::vector<RefConsts> ref;
  // the view the reference was prepared on: the zoom's, or the identity zoom (the image's own shape and Nyquist) when only
  // a spectrum filter is set
  int r_ony = 0, r_onx = 0;
  double r_cy = 0, r_cx = 0;
  // the spectrum filter (hh_set_spectrum_filter; kernels and host side in filtered_sweep.inc)
  bool f_on = false;
  double f_lp = 0, f_hp = 0;      // fractions inside (0, 1), or 0 = that pass is off
  bool f_ref = false;             // the reference was prepared with the filter
  int f_terms = 0;                // separable terms J of the operator: L q = c0 q + sum_j Ay_j q Ax_j^T
  float f_c0 = 0.f;
  int f_tiles_v = 0, f_n_tiles = 0;
  DevBuf<float> d_ay;             // [J][ony][ony]
  DevBuf<float> d_ax;             // [J][onx][onx], the term's sign folded in
  DevBuf<float> d_fq;             // [B][ony][onx] q of one batch (also: the filtered spectrum of a reference image)
  DevBuf<float> d_ft;             // [J][B][ony][onx] y pass of one batch
  DevBuf<int> d_tiles_all;        // every tile of k_zoom_sweep (the filter needs the whole plane)
  DevBuf<int> d_ftiles;           // x-pass tiles with a masked bin; behind them, at f_all_off, every x-pass tile
  int f_all_off = 0, f_all_tiles = 0;
  DevBuf<double> d_fpart;         // [S][B][f_n_tiles][3]
};

namespace {

constexpr int ZS_TU = 128;     // output tile of a workgroup: 128 rows (u) x 128 columns (v); a wavefront owns 32 x 64
constexpr int ZS_TV = 128;
constexpr int ZS_THREADS = 512;
constexpr int ZS_WAVES = ZS_THREADS / 64;
constexpr int ZS_K = 32;       // lattice centres per K slice
constexpr int ZS_CHUNK = ZS_THREADS;  // lattice centres tested per step (one per lane of the workgroup)
constexpr int ZS_TAPS = 64;    // footprints up to this many pixels keep their profiles in LDS
constexpr int ZS_LIST = ZS_CHUNK + ZS_K;
constexpr int64_t ZS_BATCH = 8192;   // pinned by tests/test_launch_cuts_host.py, crossed by tests/test_gpu_launch_cuts.py

struct ZoomLds {   // dynamic LDS of k_zoom_sweep
  float as_re[ZS_TU][ZS_K + 1], as_im[ZS_TU][ZS_K + 1];
  float bs_re[ZS_K][ZS_TV + 1], bs_im[ZS_K][ZS_TV + 1];
  float prof_y[ZS_K][ZS_TAPS], prof_x[ZS_K][ZS_TAPS];
  float yc[ZS_LIST], xc[ZS_LIST];
  int y0[ZS_LIST], ly[ZS_LIST], x0[ZS_LIST], lx[ZS_LIST];
  double red[ZS_WAVES][3];
  int wave_cnt[ZS_WAVES];
};
static_assert(offsetof(ZoomLds, prof_y) % 16 == 0 && offsetof(ZoomLds, prof_x) % 16 == 0 && ZS_TAPS % 4 == 0,
              "the profiles are read four taps at a time");

struct ZoomSweepArgs {
  const double* params;   // [batch][4]
  const double* units;
  const float* w;         // [ony][onx]
  const float* wec;       // [S][ony][onx]
  const int* tiles;       // [n_tiles]: tu * tiles_v + tv
  double* partials;       // [S][batch][n_tiles][3]
  DevGeom g;
  ZoomDims d;
  double apix, cutoff_y, cutoff_x;
  int tiles_v, n_seg;
  float* q_out;           // [batch][ony][onx]: the q-storing epilogue's plane (the filtered sweep), else unused
};

// One tap of a footprint's profile along one axis: 2^(-k2 ((p - half) apix - centre)^2), the raster's arithmetic.
__device__ __forceinline__ float zoom_tap(int p, int half, float apix, float centre, float k2) {
  const float dq = (float)(p - half) * apix - centre;
  return __builtin_amdgcn_exp2f(-(dq * dq * k2));
}

// sum_j e_j e^{-2 pi i f (p0 + j - half)} over the len taps from pixel p0: Horner's rule in w = e^{-2 pi i f} from the
// last tap, then the phase of the first one (its argument reduced in float64).  An LDS profile is zero past its last tap
// and is read four taps at a time (the extra steps leave the zero sum as it is: same result as tap by tap).
template <bool LDSP>
__device__ __forceinline__ float2 zoom_factor(double f, float2 w, int p0, int len, int half, float centre, float apix, float k2,
                                              const float* prof) {
  float sr = 0.f, si = 0.f;
  auto step = [&](float e) __attribute__((always_inline)) {
    const float nr = fmaf(sr, w.x, fmaf(-si, w.y, e));
    si = fmaf(sr, w.y, si * w.x);
    sr = nr;
  };
  if constexpr (LDSP) {
    const float4* const p4 = reinterpret_cast<const float4*>(prof);
    for (int q = ((len + 3) >> 2) - 1; q >= 0; --q) {
      const float4 e = p4[q];
      step(e.w);
      step(e.z);
      step(e.y);
      step(e.x);
    }
  } else {
    for (int j = len - 1; j >= 0; --j) step(zoom_tap(p0 + j, half, apix, centre, k2));
  }
  double t = f * (double)(p0 - half);
  t -= rint(t);
  float sn, cs;
  sincospif(-2.0f * (float)t, &sn, &cs);
  return make_float2(sr * cs - si * sn, sr * sn + si * cs);
}

// A lane's place in k_zoom_sweep's tile: 4 x 2 wavefronts of 32 x 64 (two 32 x 32 accumulator columns t = 0, 1), r and h as
// in mfma_tile.inc, the tile's origin (u0, v0) on the plane.
struct ZoomTile {
  int tid, lane, wave, r, h, wu, wv, u0, v0;
};
__device__ __forceinline__ ZoomTile zoom_tile(const ZoomSweepArgs& a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = a.tiles[blockIdx.x];
  return {tid, lane, wave, lane & 31, lane >> 5, wave & 3, wave >> 2, (tile / a.tiles_v) * ZS_TU, (tile % a.tiles_v) * ZS_TV};
}
// row u and column v of accumulator register i of column block t
__device__ __forceinline__ int zoom_u(const ZoomTile& z, int i) { return z.u0 + z.wu * 32 + acc_row(i, z.h); }
__device__ __forceinline__ int zoom_v(const ZoomTile& z, int t) { return z.v0 + z.wv * 64 + t * 32 + z.r; }

// The product of one output tile of candidate blockIdx.y, up to the accumulators: the lane's two frequencies, the walk of
// the lattice and, per K slice of centres, profiles, Horner factors, staging and the MFMA steps, into the caller's N
// accumulators per column block, out[n][t].  step(acc, ar, ai, br, bi, t) accumulates one step of column block t from the
// operands (ar + i ai) = Gy, (br + i bi) = Gx: the caller decides which real products it keeps apart.  The walk runs on
// accumulators of its own, zeroed after the set-up and handed over at the end, so that none is live across the set-up.
template <bool LDSP, int N, class Step>
__device__ __forceinline__ void zoom_product(const ZoomSweepArgs& a, ZoomLds& L, const ZoomTile& z, f32x16 (&out)[N][2], Step step) {
  const int tid = z.tid, lane = z.lane, wave = z.wave, r = z.r, h = z.h, wu = z.wu, wv = z.wv, u0 = z.u0, v0 = z.v0;
  const DevGeom& g = a.g;
  const int ny = a.d.ny, nx = a.d.nx, ony = a.d.ony, onx = a.d.onx;
  const float rp = (float)g.rpx;
  const float k2 = g.inv_sigma2 * 1.44269504088896341f;
  const Cand c = decode_candidate(a.params + 4 * (size_t)blockIdx.y, g);

  // the two frequencies this lane builds factors for, and their unit steps w = e^{-2 pi i f}
  const int ul = tid & (ZS_TU - 1), vl = tid & (ZS_TV - 1);
  const bool u_ok = u0 + ul < ony, v_ok = v0 + vl < onx;
  const double fy = u_ok ? zoom_freq(u0 + ul, ony, a.d.sy, a.apix, a.cutoff_y) : 0.0;
  const double fx = v_ok ? zoom_freq(v0 + vl, onx, a.d.sx, a.apix, a.cutoff_x) : 0.0;
  float2 wy, wx;
  {
    double sn, cs;
    sincospi(-2.0 * fy, &sn, &cs);
    wy = make_float2((float)cs, (float)sn);
    sincospi(-2.0 * fx, &sn, &cs);
    wx = make_float2((float)cs, (float)sn);
  }

  f32x16 acc[N][2];
#pragma unroll
  for (int n = 0; n < N; ++n) acc[n][0] = acc[n][1] = f32x16{0};

  // one K slice: list entries [s0, s0 + cnt), cnt <= ZS_K (the rest of the slice is zero)
  auto slice = [&](int s0, int cnt) __attribute__((always_inline)) {
    if constexpr (LDSP) {
      for (int e = tid; e < ZS_K * ZS_TAPS; e += ZS_THREADS) {
        const int k = e / ZS_TAPS, j = e % ZS_TAPS;
        if (k < cnt) {
          L.prof_y[k][j] = j < L.ly[s0 + k] ? zoom_tap(L.y0[s0 + k] + j, ny / 2, g.apix, L.yc[s0 + k], k2) : 0.f;
          L.prof_x[k][j] = j < L.lx[s0 + k] ? zoom_tap(L.x0[s0 + k] + j, nx / 2, g.apix, L.xc[s0 + k], k2) : 0.f;
        }
      }
      __syncthreads();
    }
    for (int k = tid / ZS_TU; k < ZS_K; k += ZS_THREADS / ZS_TU) {
      float2 v = make_float2(0.f, 0.f);
      if (k < cnt && u_ok)
        v = zoom_factor<LDSP>(fy, wy, L.y0[s0 + k], L.ly[s0 + k], ny / 2, L.yc[s0 + k], g.apix, k2, L.prof_y[k]);
      L.as_re[ul][k] = v.x;
      L.as_im[ul][k] = v.y;
    }
    for (int k = tid / ZS_TV; k < ZS_K; k += ZS_THREADS / ZS_TV) {
      float2 v = make_float2(0.f, 0.f);
      if (k < cnt && v_ok)
        v = zoom_factor<LDSP>(fx, wx, L.x0[s0 + k], L.lx[s0 + k], nx / 2, L.xc[s0 + k], g.apix, k2, L.prof_x[k]);
      L.bs_re[k][vl] = v.x;
      L.bs_im[k][vl] = v.y;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < ZS_K; kk += 2) {
      const float ar = L.as_re[wu * 32 + r][kk + h], ai = L.as_im[wu * 32 + r][kk + h];
#pragma unroll
      for (int t = 0; t < 2; ++t) step(acc, ar, ai, L.bs_re[kk + h][wv * 64 + t * 32 + r], L.bs_im[kk + h][wv * 64 + t * 32 + r], t);
    }
    __syncthreads();
  };

  // Walk the lattice in chunks of one centre per lane; the centres whose footprint meets the image are appended to the
  // list in lattice order (ballot + prefix), full K slices are consumed, the remainder waits for the next chunk.
  int pending = 0;
  for (int base = 0; base < c.M; base += ZS_CHUNK) {
    const int ci = base + tid;
    bool hit = false;
    float2 p = make_float2(0.f, 0.f);
    int y0 = 0, y1 = -1, x0 = 0, x1 = -1;
    if (ci < c.M) {
      p = centre_position(c, g, a.units, ci);
      const float cy = p.x * g.inv_apix + (float)(ny / 2), cx = p.y * g.inv_apix + (float)(nx / 2);
      if (cy >= -rp - 1.f && cy <= (float)ny + rp && cx >= -rp - 1.f && cx <= (float)nx + rp) {
        y0 = max(0, (int)ceilf(cy - rp));
        y1 = min(ny - 1, (int)floorf(cy + rp));
        x0 = max(0, (int)ceilf(cx - rp));
        x1 = min(nx - 1, (int)floorf(cx + rp));
        hit = y0 <= y1 && x0 <= x1;
      }
    }
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) L.wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    int off = pending, total = pending;
    for (int w = 0; w < ZS_WAVES; ++w) {
      if (w < wave) off += L.wave_cnt[w];
      total += L.wave_cnt[w];
    }
    if (hit) {
      const int at = off + __popcll(bal & ((1ull << lane) - 1ull));
      L.yc[at] = p.x;
      L.xc[at] = p.y;
      L.y0[at] = y0;
      L.ly[at] = y1 - y0 + 1;
      L.x0[at] = x0;
      L.lx[at] = x1 - x0 + 1;
    }
    __syncthreads();
    const bool last = base + ZS_CHUNK >= c.M;   // the last chunk also consumes the partial slice
    int s0 = 0;
    for (; total - s0 >= ZS_K || (last && s0 < total); s0 += ZS_K) slice(s0, min(ZS_K, total - s0));
    pending = max(0, total - s0);
    if (s0 > 0 && pending > 0) {   // move the remainder (< ZS_K entries) to the front
      float ryc = 0.f, rxc = 0.f;
      int ry0 = 0, rly = 0, rx0 = 0, rlx = 0;
      if (tid < pending) {
        ryc = L.yc[s0 + tid]; rxc = L.xc[s0 + tid];
        ry0 = L.y0[s0 + tid]; rly = L.ly[s0 + tid]; rx0 = L.x0[s0 + tid]; rlx = L.lx[s0 + tid];
      }
      __syncthreads();
      if (tid < pending) {
        L.yc[tid] = ryc; L.xc[tid] = rxc;
        L.y0[tid] = ry0; L.ly[tid] = rly; L.x0[tid] = rx0; L.lx[tid] = rlx;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int n = 0; n < N; ++n) {
    out[n][0] = acc[n][0];
    out[n][1] = acc[n][1];
  }
}

template <int LOG, bool LDSP, bool QS>
__global__ __launch_bounds__(ZS_THREADS) void k_zoom_sweep(ZoomSweepArgs a) {
  extern __shared__ __align__(16) unsigned char zoom_lds_raw[];
  ZoomLds& L = *reinterpret_cast<ZoomLds*>(zoom_lds_raw);
  const ZoomTile z = zoom_tile(a);
  const int b = blockIdx.y, n_tiles = gridDim.x, batch = gridDim.y;
  const int ony = a.d.ony, onx = a.d.onx;

  // F = sum_c Gy_c Gx_c: Re and Im, two accumulators per column block (the -ai operand folds the subtraction in)
  f32x16 acc[2][2];
  zoom_product<LDSP>(a, L, z, acc, [](f32x16 (&p)[2][2], float ar, float ai, float br, float bi, int t) __attribute__((always_inline)) {
    p[0][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, br, p[0][t], 0, 0, 0);
    p[0][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(-ai, bi, p[0][t], 0, 0, 0);
    p[1][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bi, p[1][t], 0, 0, 0);
    p[1][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br, p[1][t], 0, 0, 0);
  });
  const auto &acc_re = acc[0], &acc_im = acc[1];

  const size_t plane = (size_t)ony * onx;
  if constexpr (QS) {   // the q-storing epilogue: the tile of q itself, for the filter passes (filtered_sweep.inc)
    float* const qb = a.q_out + (size_t)b * plane;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int u = zoom_u(z, i), v = zoom_v(z, t);
        if (u < ony && v < onx) qb[(size_t)u * onx + v] = amp_to_q<LOG>(make_float2(acc_re[t][i], acc_im[t][i]));
      }
    return;
  }
  // epilogue: q = log1p|F| (or |F|) and the three masked moments of this tile, per segment
  for (int s = 0; s < a.n_seg; ++s) {
    const float* const wec = a.wec + (size_t)s * plane;
    float f1 = 0.f, f2 = 0.f, f3 = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int u = zoom_u(z, i), v = zoom_v(z, t);
        if (u < ony && v < onx) {
          const size_t at = (size_t)u * onx + v;
          const float wt = a.w[at];
          if (wt != 0.f) {
            const float q = amp_to_q<LOG>(make_float2(acc_re[t][i], acc_im[t][i]));
            f1 = fmaf(wt, q, f1);
            f2 = fmaf(wt * q, q, f2);
            f3 = fmaf(wec[at], q, f3);
          }
        }
      }
    double sum[3] = {f1, f2, f3};
    block_sums(sum, L.red, z.tid, a.partials + (((size_t)s * batch + b) * n_tiles + blockIdx.x) * 3);
  }
}

// {w, w (E - Ebar)} of one segment from its fftshifted spectrum and the fftshifted mask, on the unshifted plane the
// sweep kernel indexes; the reference's three constants.  One workgroup: a once-per-reference step.
__global__ __launch_bounds__(1024) void k_zoom_weights(const float* __restrict__ pwr, const uint8_t* __restrict__ mask, int ony,
                                                       int onx, float* __restrict__ w, float* __restrict__ wec,
                                                       RefConsts* __restrict__ ref) {
  __shared__ double red[16][2];
  __shared__ double tot[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = ony * onx;
  auto block_sum2 = [&](double x, double y) {
    for (int o = 32; o > 0; o >>= 1) {
      x += __shfl_down(x, o, 64);
      y += __shfl_down(y, o, 64);
    }
    if (lane == 0) { red[wave][0] = x; red[wave][1] = y; }
    __syncthreads();
    if (tid == 0) {
      double sx = 0, sy = 0;
      for (int k = 0; k < 16; ++k) { sx += red[k][0]; sy += red[k][1]; }
      tot[0] = sx; tot[1] = sy;
    }
    __syncthreads();
  };
  double sw = 0, se = 0;
  for (int i = tid; i < n; i += 1024)
    if (mask[i]) { sw += 1.0; se += (double)pwr[i]; }
  block_sum2(sw, se);
  sw = tot[0];
  const double ebar = sw > 0 ? tot[1] / sw : 0.0;
  __syncthreads();
  double swec = 0, var_e = 0;
  for (int i = tid; i < n; i += 1024) {
    const int su = i / onx, sv = i % onx;
    const int u = (su + ony - ony / 2) % ony, v = (sv + onx - onx / 2) % onx;   // np.fft.fftshift moved u to (u + n/2) mod n
    const double m = mask[i] ? 1.0 : 0.0, dc = (double)pwr[i] - ebar;
    const float x = (float)(m * dc);
    w[(size_t)u * onx + v] = (float)m;
    wec[(size_t)u * onx + v] = x;
    swec += (double)x;
    var_e += m * dc * dc;
  }
  block_sum2(swec, var_e);
  if (tid == 0) *ref = RefConsts{sw, tot[0], tot[1]};
}

void zoom_free(hh_ctx* c) {
  delete c->zoom;   // its buffers free themselves
  c->zoom = nullptr;
}

// true when the sweep scores through the product kernel: a zoom, or a spectrum filter (then at the identity zoom)
bool zoom_on(const hh_ctx* c) { return c->zoom && (c->zoom->on || c->zoom->f_on); }

int64_t zoom_filter_bytes(const hh_ctx* c) {
  const hh_zoom* z = c->zoom;
  if (!z) return 0;
  int64_t total = 0;
  for (const void* p : {(const void*)z->d_ay, (const void*)z->d_ax, (const void*)z->d_fq, (const void*)z->d_ft, (const void*)z->d_tiles_all,
                        (const void*)z->d_ftiles, (const void*)z->d_fpart}) {
    size_t n = 0;
    if (p && hipMemPtrGetInfo(const_cast<void*>(p), &n) == hipSuccess) total += (int64_t)n;
  }
  return total;
}

// filtered_sweep.inc
int filt_prepare(hh_ctx* c, const uint8_t* mask);
int filt_reference_plane(hh_ctx* c, const float** pwr);
int filt_sweep(hh_ctx* c, const double* d_params, int64_t n_cand, float* d_scores, int64_t ld);

// phase_sweep.inc: the reference side of the phase score (w M_exp per segment and its norm), prepared with the spectra
int phase_prepare(hh_ctx* c, int n_segments, size_t plane);
int phase_reference_plane(hh_ctx* c, int s, const ZoomDims& d, double cutoff_y, int log_flag);

// hh_set_reference with a zoom set: images [S][ny][nx] (host), mask [ony][onx] bytes on the fftshifted zoomed plane.
int zoom_set_reference(hh_ctx* c, const float* images, int n_segments, const uint8_t* mask, int log_flag) {
  hh_zoom* z = c->zoom;
  if (!c->have_geom) return fail(c, HH_ERR_STATE, "hh_set_reference: a spectrum zoom needs the pixel size; call hh_set_geometry first");
  const double apix = c->apix;
  const int ny = c->ny, nx = c->nx, ony = z->on ? z->ony : ny, onx = z->on ? z->onx : nx;
  const double cutoff_y = z->on ? z->cutoff_y : 2 * apix, cutoff_x = z->on ? z->cutoff_x : 2 * apix;
  const size_t plane = (size_t)ony * onx, npix = (size_t)ny * nx;
  // active tiles, from the mask alone (unshifted index u sits at fftshifted row (u + ony/2) mod ony)
  const int tiles_u = (ony + ZS_TU - 1) / ZS_TU, tiles_v = (onx + ZS_TV - 1) / ZS_TV;
  std::vector<int> tiles;
  for (int tu = 0; tu < tiles_u; ++tu)
    for (int tv = 0; tv < tiles_v; ++tv) {
      bool any = false;
      for (int u = tu * ZS_TU; u < std::min(ony, (tu + 1) * ZS_TU) && !any; ++u)
        for (int v = tv * ZS_TV; v < std::min(onx, (tv + 1) * ZS_TV) && !any; ++v)
          any = mask[(size_t)((u + ony / 2) % ony) * onx + (v + onx / 2) % onx] != 0;
      if (any) tiles.push_back(tu * tiles_v + tv);
    }
  if (tiles.empty()) return fail(c, HH_ERR_ARG, "hh_set_reference: the mask selects no Fourier bin");
  c->n_segments = 0;   // from here on the old reference is gone
  int rc;
  if ((rc = ensure(c, z->d_img, (size_t)n_segments * npix))) return rc;
  if ((rc = ensure(c, z->d_r, (size_t)ny * onx))) return rc;
  if ((rc = ensure(c, z->d_pwr, plane))) return rc;
  if ((rc = ensure(c, z->d_mm, 2))) return rc;
  if ((rc = ensure(c, z->d_mask, plane))) return rc;
  if ((rc = ensure(c, z->d_w, plane))) return rc;
  if ((rc = ensure(c, z->d_wec, (size_t)n_segments * plane))) return rc;
  if ((rc = ensure(c, z->d_ref, (size_t)n_segments))) return rc;
  if ((rc = ensure(c, z->d_tiles, (size_t)tiles_u * tiles_v))) return rc;
  z->r_ony = ony;
  z->r_onx = onx;
  z->r_cy = cutoff_y;
  z->r_cx = cutoff_x;
  z->f_ref = false;
  if (z->f_on && (rc = filt_prepare(c, mask))) return rc;
  if (phase_on(c) && (rc = phase_prepare(c, n_segments, plane))) return rc;
  const unsigned init[2] = {0x7f800000u, 0u};
  HH_HIP(c, hipMemcpyAsync(z->d_img, images, (size_t)n_segments * npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HH_HIP(c, hipMemcpyAsync(z->d_mask, mask, plane, hipMemcpyHostToDevice, c->stream));
  HH_HIP(c, hipMemcpyAsync(z->d_mm, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
  HH_HIP(c, hipMemcpyAsync(z->d_tiles, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  const ZoomDims d{ny, nx, ony, onx, 2 * apix / cutoff_y, 2 * apix / cutoff_x};
  for (int s = 0; s < n_segments; ++s) {
    hipLaunchKernelGGL(k_zoom_rows, dim3((onx + 127) / 128, ny), dim3(128), 0, c->stream, z->d_img + (size_t)s * npix, d, apix,
                       cutoff_x, z->d_r);
    hipLaunchKernelGGL(k_zoom_cols, dim3((onx + 127) / 128, ony), dim3(128), 0, c->stream, z->d_r, d, apix, cutoff_y,
                       log_flag ? 1 : 0, z->d_pwr, (float*)nullptr, z->d_mm);
    if (phase_on(c) && (rc = phase_reference_plane(c, s, d, cutoff_y, log_flag))) return rc;
    const float* pwr = z->d_pwr;
    if (z->f_on && (rc = filt_reference_plane(c, &pwr))) return rc;   // the same filter as every candidate's spectrum
    hipLaunchKernelGGL(k_zoom_weights, dim3(1), dim3(1024), 0, c->stream, pwr, z->d_mask, ony, onx, z->d_w,
                       z->d_wec + (size_t)s * plane, z->d_ref + s);
    HH_HIP(c, hipGetLastError());
  }
  z->ref.assign(n_segments, RefConsts{});
  HH_HIP(c, hipMemcpyAsync(z->ref.data(), z->d_ref, (size_t)n_segments * sizeof(RefConsts), hipMemcpyDeviceToHost, c->stream));
  HH_HIP(c, hipStreamSynchronize(c->stream));   // (images, mask, init and tiles are the caller's / locals)
  z->tiles_v = tiles_v;
  z->n_tiles = (int)tiles.size();
  z->apix_ref = apix;
  z->f_ref = z->f_on;
  c->n_segments = n_segments;
  c->log_flag = log_flag ? 1 : 0;
  return HH_OK;
}

template <int LOG, bool LDSP, bool QS>
int launch_zoom(hh_ctx* c, const ZoomSweepArgs& a, int n_tiles, int batch) {
  if (int rc = ensure_lds_attr(c, reinterpret_cast<const void*>(&k_zoom_sweep<LOG, LDSP, QS>), (int)sizeof(ZoomLds))) return rc;
  hipLaunchKernelGGL((k_zoom_sweep<LOG, LDSP, QS>), dim3(n_tiles, batch), dim3(ZS_THREADS), sizeof(ZoomLds), c->stream, a);
  HH_HIP(c, hipGetLastError());
  return HH_OK;
}

template <bool QS>
int launch_zoom_any(hh_ctx* c, const ZoomSweepArgs& a, int n_tiles, int batch) {
  const bool ldsp = 2 * c->geom.rpx + 1 <= ZS_TAPS;
  if (c->log_flag) return ldsp ? launch_zoom<1, true, QS>(c, a, n_tiles, batch) : launch_zoom<1, false, QS>(c, a, n_tiles, batch);
  return ldsp ? launch_zoom<0, true, QS>(c, a, n_tiles, batch) : launch_zoom<0, false, QS>(c, a, n_tiles, batch);
}

// the arguments every launch of k_zoom_sweep shares (params, tiles, partials / q_out: the caller's)
ZoomSweepArgs zoom_args(const hh_ctx* c) {
  const hh_zoom* z = c->zoom;
  ZoomSweepArgs a{};
  a.units = c->d_units;
  a.w = z->d_w;
  a.wec = z->d_wec;
  a.g = c->geom;
  a.d = ZoomDims{c->ny, c->nx, z->r_ony, z->r_onx, 2 * z->apix_ref / z->r_cy, 2 * z->apix_ref / z->r_cx};
  a.apix = z->apix_ref;
  a.cutoff_y = z->r_cy;
  a.cutoff_x = z->r_cx;
  a.tiles_v = z->tiles_v;
  a.n_seg = c->n_segments;
  return a;
}

// Every hh_sweep* entry point with a zoom set.  ld: row stride of d_scores (0: n_cand).
int zoom_sweep(hh_ctx* c, const double* d_params, int64_t n_cand, float* d_scores, int64_t ld) {
  hh_zoom* z = c->zoom;
  if (z->f_ref) return filt_sweep(c, d_params, n_cand, d_scores, ld);
  const int64_t stride = ld > 0 ? ld : n_cand;
  const int S = c->n_segments, npart = z->n_tiles;
  const int64_t cap = std::min<int64_t>(n_cand, ZS_BATCH);
  if (int rc = ensure(c, z->d_partials, (size_t)S * cap * npart * 3)) return rc;
  c->last_first_pass = 3;
  for (int64_t b0 = 0; b0 < n_cand; b0 += cap) {
    const int nb = (int)std::min<int64_t>(cap, n_cand - b0);
    ZoomSweepArgs a = zoom_args(c);
    a.params = d_params + 4 * b0;
    a.tiles = z->d_tiles;
    a.partials = z->d_partials;
    if (int rc = launch_zoom_any<false>(c, a, npart, nb)) return rc;
    for (int s = 0; s < S; ++s) {
      hipLaunchKernelGGL(k_finalize, dim3(std::min(1024, (nb + 3) / 4)), dim3(256), 0, c->stream,
                         z->d_partials + (size_t)s * nb * npart * 3, npart, (int64_t)nb, z->ref[s], d_scores + (size_t)s * stride + b0);
      HH_HIP(c, hipGetLastError());
    }
  }
  return HH_OK;
}

}  // namespace

extern "C" int hh_set_spectrum_zoom(hh_ctx* c, int ony, int onx, double cutoff_y, double cutoff_x) try {
  if (!c) return HH_ERR_ARG;
  if (ony == 0 && onx == 0 && cutoff_y == 0.0 && cutoff_x == 0.0) {   // back to the default sampling
    if (c->zoom && c->zoom->on) {
      c->zoom->on = false;
      c->n_segments = 0;   // the reference was prepared for the zoomed plane: hh_set_reference comes next
    }
    return HH_OK;
  }
  if (ony < 8 || onx < 8 || ony > 1024 || onx > 1024)
    return fail(c, HH_ERR_ARG, "hh_set_spectrum_zoom: the spectrum's sides must lie in [8, 1024]");
  if (!(cutoff_y > 0) || !(cutoff_x > 0) || !std::isfinite(cutoff_y) || !std::isfinite(cutoff_x))
    return fail(c, HH_ERR_ARG, "hh_set_spectrum_zoom: the cutoff resolutions must be positive and finite");
  if (!c->zoom) c->zoom = new hh_zoom();
  hh_zoom* z = c->zoom;
  z->on = true;
  z->ony = ony;
  z->onx = onx;
  z->cutoff_y = cutoff_y;
  z->cutoff_x = cutoff_x;
  c->n_segments = 0;   // any earlier reference belongs to another sampling
  return HH_OK;
} HH_CATCH_CTX(c, "hh_set_spectrum_zoom")

extern "C" int hh_set_spectrum_filter(hh_ctx* c, double low_pass_fraction, double high_pass_fraction) try {
  if (!c) return HH_ERR_ARG;
  if (std::isnan(low_pass_fraction) || std::isnan(high_pass_fraction))
    return fail(c, HH_ERR_ARG, "hh_set_spectrum_filter: a fraction is NaN");
  // filters.py:363-370: a fraction outside (0, 1) is ignored
  const double lp = low_pass_fraction > 0 && low_pass_fraction < 1 ? low_pass_fraction : 0.0;
  const double hp = high_pass_fraction > 0 && high_pass_fraction < 1 ? high_pass_fraction : 0.0;
  if (!c->zoom) {
    if (lp == 0.0 && hp == 0.0) return HH_OK;
    c->zoom = new hh_zoom();
  }
  hh_zoom* z = c->zoom;
  if (lp == z->f_lp && hp == z->f_hp) return HH_OK;
  if ((lp != 0.0 || hp != 0.0) && phase_on(c))
    return fail(c, HH_ERR_ARG, "hh_set_spectrum_filter: the phase score (hh_set_spectrum_phase) reads the unfiltered transform; clear it first");
  z->f_lp = lp;
  z->f_hp = hp;
  z->f_on = lp != 0.0 || hp != 0.0;
  c->n_segments = 0;   // the reference was prepared for another filter: hh_set_reference comes next
  return HH_OK;
} HH_CATCH_CTX(c, "hh_set_spectrum_filter")
