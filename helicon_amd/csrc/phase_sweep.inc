// phase_sweep.inc — the sweep's phase score: the phase difference across the meridian (lib/transforms.py:823-842,
// compute_phase_difference_across_meridian: "0 -> even order, 180 -> odd order") of every candidate against the same
// view of the experimental image, mixed with the amplitude score.
//
// On the scored plane (the zoom's, or the image's own shape and Nyquist without one) and with centre-origin transforms,
//     F (u, v) = sum_{y,x} img[y, x] e^{-2 pi i (f_y[u] (y - ny/2) + f_x[v] (x - nx/2))}
//     F~(u, v) = the same sum at (-f_y[u], f_x[v])             across the meridian (the helix lies along x)
//     c = Re(F conj F~) / (|F| |F~|)  (0 where that is 0 / 0),   q = log1p|F| or |F|,   M = q c
//     phase score = cosine_similarity(M_exp[mask], M_cand[mask])  (analysis.py:802-821)
//     score       = (1 - weight) * amplitude Pearson + weight * phase score
// k_zoom_sweep forms a candidate's F = sum_c Gy_c[u] Gx_c[v] as four real products on the f32 MFMA.  The footprints are
// real, so Gy_c at -f_y is the conjugate of Gy_c at f_y: with P1 = sum ar br, P2 = sum ai bi, P3 = sum ar bi,
// P4 = sum ai br (a = Gy, b = Gx)
//     F = (P1 - P2) + i (P3 + P4),     F~ = (P1 + P2) + i (P3 - P4)
// and k_phase_sweep runs k_zoom_sweep's product body (zoom_product, zoom_sweep.inc) with the four products kept in
// accumulators of their own: the same MFMA count, an epilogue with two more sums (sum w M^2, sum (w M_exp) M).  F~ needs no partner
// row on the grid, so the unpaired row u = ony/2 of a zoomed plane is scored like any other.  Both q and M enter their
// scores up to a constant factor, so the logarithm is taken in base 2 as everywhere in the sweep.
// The reference side is k_zoom_rows plus k_phase_cols (F and F~ of the experimental image in float64) and
// k_phase_weights (w M_exp per segment, sum w M_exp^2); k_phase_finalize writes the three scores.

struct hh_phase {
  bool on = false;
  double weight = 0;
  DevBuf<float> d_pm;             // [ony][onx] fftshifted M of one image
  DevBuf<float> d_pc;             // [ony][onx] fftshifted c of one image (hh_phase_map)
  DevBuf<float> d_wm;             // [S][ony][onx] unshifted w M_exp
  DevBuf<double> d_see;           // [S] sum of the float32-rounded (w M_exp)^2
  DevBuf<double> d_partials;      // [S][batch][n_tiles][5]
  DevBuf<double> d_params;        // hh_sweep_parts' staging
  DevBuf<float> d_out;            // hh_sweep_parts' staging: [3][S][g]
  DevBuf<float> d_img;            // hh_phase_map's image and row pass
  DevBuf<double2> d_r;
  std::vector<double> see;
};

namespace {

struct PhaseLds {   // dynamic LDS of k_phase_sweep
  ZoomLds z;
  double red[ZS_WAVES][5];
};

struct PhaseSweepArgs {
  ZoomSweepArgs z;    // partials: [S][batch][n_tiles][5] here
  const float* wm;    // [S][ony][onx]
};

template <int LOG, bool LDSP>
__global__ __launch_bounds__(ZS_THREADS) void k_phase_sweep(PhaseSweepArgs pa) {
  extern __shared__ __align__(16) unsigned char phase_lds_raw[];
  PhaseLds& PL = *reinterpret_cast<PhaseLds*>(phase_lds_raw);
  const ZoomSweepArgs& a = pa.z;
  const ZoomTile z = zoom_tile(a);
  const int b = blockIdx.y, n_tiles = gridDim.x, batch = gridDim.y;
  const int ony = a.d.ony, onx = a.d.onx;

  // P1 = sum ar br, P2 = sum ai bi, P3 = sum ar bi, P4 = sum ai br
  f32x16 acc[4][2];
  zoom_product<LDSP>(a, PL.z, z, acc, [](f32x16 (&p)[4][2], float ar, float ai, float br, float bi, int t) __attribute__((always_inline)) {
    p[0][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, br, p[0][t], 0, 0, 0);
    p[1][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, bi, p[1][t], 0, 0, 0);
    p[2][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bi, p[2][t], 0, 0, 0);
    p[3][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br, p[3][t], 0, 0, 0);
  });
  const auto &p1 = acc[0], &p2 = acc[1], &p3 = acc[2], &p4 = acc[3];

  // epilogue: per masked bin q, c and M = q c; per segment the three amplitude moments, sum w M^2 and sum (w M_exp) M
  const size_t plane = (size_t)ony * onx;
  for (int s = 0; s < a.n_seg; ++s) {
    const float* const wec = a.wec + (size_t)s * plane;
    const float* const wm = pa.wm + (size_t)s * plane;
    float f1 = 0.f, f2 = 0.f, f3 = 0.f, f4 = 0.f, f5 = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int u = zoom_u(z, i), v = zoom_v(z, t);
        if (u < ony && v < onx) {
          const size_t at = (size_t)u * onx + v;
          const float wt = a.w[at];
          if (wt != 0.f) {
            const float fr = p1[t][i] - p2[t][i], fi = p3[t][i] + p4[t][i];   // F
            const float gr = p1[t][i] + p2[t][i], gi = p3[t][i] - p4[t][i];   // F~
            const float af = __builtin_amdgcn_sqrtf(fr * fr + fi * fi), ag = __builtin_amdgcn_sqrtf(gr * gr + gi * gi);
            float q = af;
            if constexpr (LOG) q = __log2f(1.0f + af);
            const float den = af * ag;
            const float m = den > 0.f ? q * __fdividef(fr * gr + fi * gi, den) : 0.f;   // Re(F conj F~) = P1^2 - P2^2 + P3^2 - P4^2
            f1 = fmaf(wt, q, f1);
            f2 = fmaf(wt * q, q, f2);
            f3 = fmaf(wec[at], q, f3);
            f4 = fmaf(wt * m, m, f4);
            f5 = fmaf(wm[at], m, f5);
          }
        }
      }
    double sum[5] = {f1, f2, f3, f4, f5};
    block_sums(sum, PL.red, z.tid, a.partials + (((size_t)s * batch + b) * n_tiles + blockIdx.x) * 5);
  }
}

// F and F~ of one image from its row pass (k_zoom_rows), in float64: the column sum at f_y[u] and at -f_y[u]; M = q c and
// c on the fftshifted plane.  (k_zoom_cols' sign (-1)^(u + v) multiplies F and F~ alike and leaves c as it is.)
__global__ __launch_bounds__(128) void k_phase_cols(const double2* __restrict__ r, ZoomDims d, double apix, double cutoff_y, int log_flag,
                                                    float* __restrict__ m_out, float* __restrict__ c_out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x, u = blockIdx.y;
  if (v >= d.onx) return;
  const double f = zoom_freq(u, d.ony, d.sy, apix, cutoff_y);
  double fr = 0, fi = 0, gr = 0, gi = 0;
  for (int a = 0; a < d.ny; ++a) {
    double sn, cs;
    sincospi(-2.0 * f * (double)(a - d.ny / 2), &sn, &cs);
    const double2 w = r[(size_t)a * d.onx + v];
    fr += w.x * cs - w.y * sn;
    fi += w.x * sn + w.y * cs;
    gr += w.x * cs + w.y * sn;
    gi += w.y * cs - w.x * sn;
  }
  const double af = sqrt(fr * fr + fi * fi), ag = sqrt(gr * gr + gi * gi);
  const double den = af * ag;
  const double cc = den > 0 ? (fr * gr + fi * gi) / den : 0.0;
  const double q = log_flag ? log1p(af) : af;
  const int su = (u + d.ony / 2) % d.ony, sv = (v + d.onx / 2) % d.onx;   // np.fft.fftshift
  m_out[(size_t)su * d.onx + sv] = (float)(q * cc);
  if (c_out) c_out[(size_t)su * d.onx + sv] = (float)cc;
}

// w M_exp of one segment on the unshifted plane the sweep kernel indexes, and sum (w M_exp)^2 of the float32 values the
// kernel multiplies by.  One workgroup, fixed order: a once-per-reference step.
__global__ __launch_bounds__(1024) void k_phase_weights(const float* __restrict__ pm, const uint8_t* __restrict__ mask, int ony, int onx,
                                                        float* __restrict__ wm, double* __restrict__ see) {
  __shared__ double red[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = ony * onx;
  double acc = 0;
  for (int i = tid; i < n; i += 1024) {
    const int su = i / onx, sv = i % onx;
    const int u = (su + ony - ony / 2) % ony, v = (sv + onx - onx / 2) % onx;
    const float x = mask[i] ? pm[i] : 0.f;
    wm[(size_t)u * onx + v] = x;
    acc += (double)x * (double)x;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    double tot = 0;
    for (int k = 0; k < 16; ++k) tot += red[k];
    *see = tot;
  }
}

// The three scores of every candidate from its tiles' five sums: a 64-lane team per candidate strides over the tiles, the
// sums are reduced in float64 by shuffles (a fixed order), lane 0 writes.  amp / phase may be NULL.
__global__ void k_phase_finalize(const double* __restrict__ partials, int npart, int n, RefConsts rc, double see, float weight,
                                 float* __restrict__ scores, float* __restrict__ amp, float* __restrict__ phase) {
  const int lane = threadIdx.x & 63, per_block = blockDim.x / 64;
  for (int i = blockIdx.x * per_block + threadIdx.x / 64; i < n; i += gridDim.x * per_block) {
    double s[5] = {0, 0, 0, 0, 0};
    const double* const base = partials + (size_t)i * npart * 5;
    for (int k = lane; k < npart; k += 64)
#pragma unroll
      for (int e = 0; e < 5; ++e) s[e] += base[(size_t)k * 5 + e];
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int e = 0; e < 5; ++e) s[e] += __shfl_down(s[e], o, 64);
    if (lane == 0) {
      const float am = pearson_from_moments(s[0], s[1], s[2], rc);
      const double den = s[3] * see;
      const float ph = den > 0 ? (float)(s[4] / sqrt(den)) : 0.f;   // analysis.py:817-818: a zero norm -> 0
      scores[i] = (1.0f - weight) * am + weight * ph;
      if (amp) amp[i] = am;
      if (phase) phase[i] = ph;
    }
  }
}

bool phase_on(const hh_ctx* c) { return c->phase && c->phase->on; }

void phase_free(hh_ctx* c) {
  delete c->phase;   // its buffers free themselves
  c->phase = nullptr;
}

// hh_set_reference with the phase score on, before the images are transformed: the buffers the reference side needs
int phase_prepare(hh_ctx* c, int n_segments, size_t plane) {
  hh_phase* p = c->phase;
  int rc;
  if ((rc = ensure(c, p->d_pm, plane))) return rc;
  if ((rc = ensure(c, p->d_wm, (size_t)n_segments * plane))) return rc;
  if ((rc = ensure(c, p->d_see, (size_t)n_segments))) return rc;
  p->see.assign(n_segments, 0.0);
  return HH_OK;
}

// Segment s, whose row pass sits in the zoom's d_r: M_exp, then w M_exp and its norm (fetched with the caller's
// synchronisation at the end of hh_set_reference)
int phase_reference_plane(hh_ctx* c, int s, const ZoomDims& d, double cutoff_y, int log_flag) {
  hh_phase* p = c->phase;
  const hh_zoom* z = c->zoom;
  const size_t plane = (size_t)d.ony * d.onx;
  hipLaunchKernelGGL(k_phase_cols, dim3((d.onx + 127) / 128, d.ony), dim3(128), 0, c->stream, z->d_r, d, c->apix, cutoff_y,
                     log_flag ? 1 : 0, p->d_pm, (float*)nullptr);
  hipLaunchKernelGGL(k_phase_weights, dim3(1), dim3(1024), 0, c->stream, p->d_pm, z->d_mask, d.ony, d.onx, p->d_wm + (size_t)s * plane,
                     p->d_see + s);
  HH_HIP(c, hipGetLastError());
  HH_HIP(c, hipMemcpyAsync(&p->see[s], p->d_see + s, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return HH_OK;
}

template <int LOG, bool LDSP>
int launch_phase(hh_ctx* c, const PhaseSweepArgs& a, int n_tiles, int batch) {
  if (int rc = ensure_lds_attr(c, reinterpret_cast<const void*>(&k_phase_sweep<LOG, LDSP>), (int)sizeof(PhaseLds))) return rc;
  hipLaunchKernelGGL((k_phase_sweep<LOG, LDSP>), dim3(n_tiles, batch), dim3(ZS_THREADS), sizeof(PhaseLds), c->stream, a);
  HH_HIP(c, hipGetLastError());
  return HH_OK;
}

// Every hh_sweep* entry point with the phase score on.  ld: row stride of d_scores, d_amp and d_phase (0: n_cand); the
// last two may be NULL.
int phase_sweep(hh_ctx* c, const double* d_params, int64_t n_cand, float* d_scores, int64_t ld, float* d_amp, float* d_phase) {
  hh_phase* p = c->phase;
  hh_zoom* z = c->zoom;
  const int64_t stride = ld > 0 ? ld : n_cand;
  const int S = c->n_segments, npart = z->n_tiles;
  const int64_t cap = std::min<int64_t>(n_cand, ZS_BATCH);
  if (int rc = ensure(c, p->d_partials, (size_t)S * cap * npart * 5)) return rc;
  c->last_first_pass = 5;
  const bool ldsp = 2 * c->geom.rpx + 1 <= ZS_TAPS;
  for (int64_t b0 = 0; b0 < n_cand; b0 += cap) {
    const int nb = (int)std::min<int64_t>(cap, n_cand - b0);
    PhaseSweepArgs a{zoom_args(c), p->d_wm};
    a.z.params = d_params + 4 * b0;
    a.z.tiles = z->d_tiles;
    a.z.partials = p->d_partials;
    int rc;
    if (c->log_flag) rc = ldsp ? launch_phase<1, true>(c, a, npart, nb) : launch_phase<1, false>(c, a, npart, nb);
    else rc = ldsp ? launch_phase<0, true>(c, a, npart, nb) : launch_phase<0, false>(c, a, npart, nb);
    if (rc) return rc;
    for (int s = 0; s < S; ++s) {
      const size_t at = (size_t)s * stride + b0;
      hipLaunchKernelGGL(k_phase_finalize, dim3(std::min(1024, (nb + 3) / 4)), dim3(256), 0, c->stream,
                         p->d_partials + (size_t)s * nb * npart * 5, npart, nb, z->ref[s], p->see[s], (float)p->weight, d_scores + at,
                         d_amp ? d_amp + at : nullptr, d_phase ? d_phase + at : nullptr);
      HH_HIP(c, hipGetLastError());
    }
  }
  return HH_OK;
}

}  // namespace

extern "C" int hh_set_spectrum_phase(hh_ctx* c, double weight) try {
  if (!c) return HH_ERR_ARG;
  if (!(weight >= 0.0 && weight <= 1.0)) return fail(c, HH_ERR_ARG, "hh_set_spectrum_phase: the weight must lie in [0, 1]");
  if (weight == 0.0) {   // back to the amplitude score alone
    if (phase_on(c)) {
      c->phase->on = false;
      c->phase->weight = 0;
      c->n_segments = 0;   // the reference was prepared with the phase tables: hh_set_reference comes next
    }
    return HH_OK;
  }
  if (c->zoom && c->zoom->f_on)
    return fail(c, HH_ERR_ARG, "hh_set_spectrum_phase: a spectrum filter (hh_set_spectrum_filter) is set; the phase score reads the unfiltered transform");
  if (!c->zoom) c->zoom = new hh_zoom();   // the phase score runs on the zoom's reference side (the identity zoom without one)
  if (!c->phase) c->phase = new hh_phase();
  if (!c->phase->on) {
    c->phase->on = true;
    c->n_segments = 0;   // the reference lacks the phase tables: hh_set_reference comes next
  }
  c->phase->weight = weight;
  return HH_OK;
} HH_CATCH_CTX(c, "hh_set_spectrum_phase")

extern "C" int hh_sweep_parts(hh_ctx* c, const double* params, int64_t g, float* scores, float* amplitude, float* phase) try {
  int rc = check_ready(c, true);
  if (rc) return rc;
  if (!phase_on(c)) return fail(c, HH_ERR_STATE, "hh_sweep_parts: the phase score is off (hh_set_spectrum_phase)");
  if (!params || g < 0) return fail(c, HH_ERR_ARG, "hh_sweep_parts: bad argument");
  if (g == 0) return HH_OK;
  HH_HIP(c, hipSetDevice(c->device));
  hh_phase* p = c->phase;
  const size_t n = (size_t)g * c->n_segments;
  if ((rc = ensure(c, p->d_params, (size_t)g * 4))) return rc;
  if ((rc = ensure(c, p->d_out, 3 * n))) return rc;
  HH_HIP(c, hipMemcpyAsync(p->d_params, params, (size_t)g * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = phase_sweep(c, p->d_params, g, p->d_out, 0, p->d_out + n, p->d_out + 2 * n))) return rc;
  float* const host[3] = {scores, amplitude, phase};
  for (int k = 0; k < 3; ++k)
    if (host[k]) HH_HIP(c, hipMemcpyAsync(host[k], p->d_out + k * n, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HH_HIP(c, hipStreamSynchronize(c->stream));
  return HH_OK;
} HH_CATCH_CTX(c, "hh_sweep_parts")

extern "C" int hh_phase_map(hh_ctx* c, const float* image, int log_flag, float* map_out, float* cos_out) try {
  if (!c) return HH_ERR_ARG;
  if (!image || (!map_out && !cos_out)) return fail(c, HH_ERR_ARG, "hh_phase_map: bad argument");
  if (!c->have_geom) return fail(c, HH_ERR_STATE, "hh_phase_map: the frequencies need the pixel size; call hh_set_geometry first");
  HH_HIP(c, hipSetDevice(c->device));
  if (!c->phase) c->phase = new hh_phase();
  hh_phase* p = c->phase;
  const hh_zoom* z = c->zoom;
  const bool zoomed = z && z->on;
  const double apix = c->apix;
  const int ny = c->ny, nx = c->nx, ony = zoomed ? z->ony : ny, onx = zoomed ? z->onx : nx;
  const double cutoff_y = zoomed ? z->cutoff_y : 2 * apix, cutoff_x = zoomed ? z->cutoff_x : 2 * apix;
  const size_t plane = (size_t)ony * onx, npix = (size_t)ny * nx;
  int rc;
  if ((rc = ensure(c, p->d_img, npix))) return rc;
  if ((rc = ensure(c, p->d_r, (size_t)ny * onx))) return rc;
  if ((rc = ensure(c, p->d_pm, plane))) return rc;
  if ((rc = ensure(c, p->d_pc, plane))) return rc;
  const ZoomDims d{ny, nx, ony, onx, 2 * apix / cutoff_y, 2 * apix / cutoff_x};
  HH_HIP(c, hipMemcpyAsync(p->d_img, image, npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_zoom_rows, dim3((onx + 127) / 128, ny), dim3(128), 0, c->stream, p->d_img, d, apix, cutoff_x, p->d_r);
  hipLaunchKernelGGL(k_phase_cols, dim3((onx + 127) / 128, ony), dim3(128), 0, c->stream, p->d_r, d, apix, cutoff_y, log_flag ? 1 : 0,
                     p->d_pm, p->d_pc);
  HH_HIP(c, hipGetLastError());
  if (map_out) HH_HIP(c, hipMemcpyAsync(map_out, p->d_pm, plane * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (cos_out) HH_HIP(c, hipMemcpyAsync(cos_out, p->d_pc, plane * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HH_HIP(c, hipStreamSynchronize(c->stream));
  return HH_OK;
} HH_CATCH_CTX(c, "hh_phase_map")
