// filtered_sweep.inc — the sweep on low / high-pass filtered spectra: compute_power_spectra(sim, apix, cutoff_res, output_size,
// log, low_pass_fraction, high_pass_fraction) of every candidate against the same view of the experimental image
// (lib/transforms.py:771-820, lines 811-816: the filter acts on the spectrum IMAGE log1p|F|), in one batched call.
//
// low_high_pass_filter (lib/filters.py:314-372) is Re ifft2(fft2(q) . w) with Gaussian weights: a linear circulant operator
// L on the plane that commutes with fftshift, so it acts on the unshifted plane k_zoom_sweep works on.  Each Gaussian is
// separable, G q = Re(Cy q Cx^T) with the circulant operators of axis_plan.h (c = ifft(w); real on an even side, complex
// on an odd one, where fftshift is not ifftshift):
//     low pass alone  G_a q        high pass alone  q - G_b q        both  G_a q - G_(a+b) q
//     Re(Cy q Cx^T) = Cyr q Cxr^T - Cyi q Cxi^T   (the second product only when both sides are odd)
// so L q = c0 q + sum_j Ay_j q Ax_j^T with J <= 4 terms, the signs folded into Ax_j.  Per batch of B candidates:
//   1. k_zoom_sweep<QS>: the product kernel with the q-storing epilogue, every tile, q -> [B][ony][onx];
//   2. k_circ_gemm (axis_pass.inc) per term: T_j = Ay_j q, batched over the candidates' planes;
//   3. k_filter_xpass: sum_j T_j Ax_j^T as ONE product with K = J onx on the exact-f32 MFMA, then in the accumulator
//      registers + c0 q and the masked moments against {w, w (E - Ebar)} of every segment, reduced in float64 in a fixed
//      order to one triple per (segment, candidate, tile): L q is never stored.  Tiles without a masked bin are not computed;
//   4. k_finalize: Pearson from the moments (the min-max normalisation is affine and cancels).
// The reference side runs the experimental image's spectrum through passes 2 and 3 (storing epilogue) before k_zoom_weights.

namespace {

constexpr int FS_T = 64;    // x-pass output tile of a workgroup: 64 rows (u) x 64 columns (v), four wavefronts of 32 x 32
constexpr int FS_K = 32;    // K slice staged through LDS
constexpr int64_t FS_BYTES = (int64_t)128 << 20;   // q and T of one batch stay below this
constexpr int64_t FS_BATCH = 1024;   // both pinned by tests/test_launch_cuts_host.py, crossed by tests/test_gpu_launch_cuts.py

struct FiltArgs {
  const float* t;       // [J][batch][ony][onx] y passes
  const float* ax;      // [J][onx][onx]: row v of sign_j Cx_j
  const float* q;       // [batch][ony][onx]: the identity term's plane (read when c0 != 0)
  const float* w;       // [ony][onx]
  const float* wec;     // [S][ony][onx]
  const int* tiles;     // tu * tiles_v + tv
  double* partials;     // [S][batch][n_tiles][3]
  float* out;           // STORE: [batch][ony][onx]
  float c0;
  int ony, onx, n_terms, tiles_v, n_seg;
};

// One output tile of one candidate: acc[u][v] = sum_j sum_k T_j[u][k] Ax_j[v][k] (both operands are read along k: whole
// 128-byte lines), then the epilogue.  STORE writes L q (the reference image's plane); otherwise the moments.
template <bool STORE>
__global__ __launch_bounds__(256) void k_filter_xpass(FiltArgs a) {
  __shared__ float as[FS_T][FS_K + 1];
  __shared__ float bs[FS_K][FS_T + 1];
  __shared__ double red[4][3];
  const Tile64 t = tile64();
  const int tid = t.tid;
  const int b = blockIdx.y, batch = gridDim.y, n_tiles = gridDim.x;
  const int tile = a.tiles[blockIdx.x];
  const int u0 = (tile / a.tiles_v) * FS_T, v0 = (tile % a.tiles_v) * FS_T;
  const int ony = a.ony, onx = a.onx;
  const size_t plane = (size_t)ony * onx;
  f32x16 acc = {0};
  for (int j = 0; j < a.n_terms; ++j) {
    const float* const tj = a.t + ((size_t)j * batch + b) * plane;
    const float* const axj = a.ax + (size_t)j * onx * onx;
    for (int k0 = 0; k0 < onx; k0 += FS_K) {
      for (int e = tid; e < FS_T * FS_K; e += 256) {   // its own: both operands lie along k and fill from one index
        const int mm = e / FS_K, kk = e % FS_K, k = k0 + kk;
        const int u = u0 + mm, v = v0 + mm;
        as[mm][kk] = (u < ony && k < onx) ? tj[(size_t)u * onx + k] : 0.f;
        bs[kk][mm] = (v < onx && k < onx) ? axj[(size_t)v * onx + k] : 0.f;
      }
      __syncthreads();
      tile_mac<false>(acc, as, bs, t);
      __syncthreads();
    }
  }
  // L q of this lane's 16 bins
  float val[16];
  int at[16];
  bool ok[16];
  const int v = v0 + t.wp + t.r;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int u = u0 + t.wm + acc_row(i, t.h);
    ok[i] = u < ony && v < onx;
    at[i] = u * onx + v;
    val[i] = acc[i];
    if (ok[i] && a.c0 != 0.f) val[i] = fmaf(a.c0, a.q[(size_t)b * plane + at[i]], val[i]);
  }
  if constexpr (STORE) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (ok[i]) a.out[(size_t)b * plane + at[i]] = val[i];
  } else {
    for (int s = 0; s < a.n_seg; ++s) {
      const float* const wec = a.wec + (size_t)s * plane;
      float f1 = 0.f, f2 = 0.f, f3 = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (ok[i]) {
          const float wt = a.w[at[i]];
          if (wt != 0.f) {
            f1 = fmaf(wt, val[i], f1);
            f2 = fmaf(wt * val[i], val[i], f2);
            f3 = fmaf(wec[at[i]], val[i], f3);
          }
        }
      double sum[3] = {f1, f2, f3};
      block_sums(sum, red, tid, a.partials + (((size_t)s * batch + b) * n_tiles + blockIdx.x) * 3);
    }
  }
}

// T_j = Ay_j . src for every term, src = [batch][ony][onx] planes, into z->d_ft ([J][batch][ony][onx]).
int filt_y_passes(hh_ctx* c, const float* src, int batch) {
  hh_zoom* z = c->zoom;
  const int ony = z->r_ony, onx = z->r_onx;
  const size_t plane = (size_t)ony * onx;
  const AxisGeom pass = axis_geom(AxisView{batch, ony, ony, onx, false});
  for (int j = 0; j < z->f_terms; ++j) {
    launch_circ_pass(pass, z->d_ay + (size_t)j * ony * ony, ony, src, nullptr, z->d_ft + (size_t)j * batch * plane, c->stream);
    HH_HIP(c, hipGetLastError());
  }
  return HH_OK;
}

FiltArgs filt_args(const hh_ctx* c, const float* q) {
  const hh_zoom* z = c->zoom;
  FiltArgs a{};
  a.t = z->d_ft;
  a.ax = z->d_ax;
  a.q = q;
  a.w = z->d_w;
  a.wec = z->d_wec;
  a.c0 = z->f_c0;
  a.ony = z->r_ony;
  a.onx = z->r_onx;
  a.n_terms = z->f_terms;
  a.tiles_v = z->f_tiles_v;
  a.n_seg = c->n_segments;
  return a;
}

// hh_set_reference with a filter set, before the images are transformed: the operators of the view (r_ony x r_onx), the tile
// lists and the buffers one plane needs.  mask: [ony][onx] bytes on the fftshifted plane.
int filt_prepare(hh_ctx* c, const uint8_t* mask) {
  hh_zoom* z = c->zoom;
  const int ony = z->r_ony, onx = z->r_onx;
  const size_t plane = (size_t)ony * onx;
  // L = sum_t coef_t G_(f2_t), G_0 = identity (map_filter.inc states the same expansion for the 3-D filter)
  const bool lp = z->f_lp > 0, hp = z->f_hp > 0;
  const double fa = lp ? std::log(2.0) / (z->f_lp * z->f_lp) : 0.0, fb = hp ? std::log(2.0) / (z->f_hp * z->f_hp) : 0.0;
  std::vector<std::pair<double, double>> gauss;   // (coef, f2)
  if (lp && hp) gauss = {{1.0, fa}, {-1.0, fa + fb}};
  else if (lp) gauss = {{1.0, fa}};
  else gauss = {{-1.0, fb}};
  z->f_c0 = (hp && !lp) ? 1.f : 0.f;
  std::vector<float> ay, ax;
  int terms = 0;
  for (const auto& gs : gauss) {
    std::vector<double> yr, yi, xr, xi;
    circulant_column(ony, gs.second, yr, yi);
    circulant_column(onx, gs.second, xr, xi);
    append_axis_operator(ay, ony, AxisIndex::Circulant, yr, 1.0, nullptr, 0.0);
    append_axis_operator(ax, onx, AxisIndex::Circulant, xr, gs.first, nullptr, 0.0);
    ++terms;
    if (ony % 2 == 1 && onx % 2 == 1) {   // Re((Cyr + i Cyi) q (Cxr + i Cxi)^T): the imaginary parts' product, with a minus
      append_axis_operator(ay, ony, AxisIndex::Circulant, yi, 1.0, nullptr, 0.0);
      append_axis_operator(ax, onx, AxisIndex::Circulant, xi, -gs.first, nullptr, 0.0);
      ++terms;
    }
  }
  z->f_terms = terms;
  // tiles: every tile of k_zoom_sweep; the x pass's tiles with a masked bin, then all of them (the reference's plane)
  const int ztu = (ony + ZS_TU - 1) / ZS_TU, ztv = (onx + ZS_TV - 1) / ZS_TV;
  std::vector<int> all(ztu * ztv);
  for (int i = 0; i < ztu * ztv; ++i) all[i] = i;
  const int ftu = (ony + FS_T - 1) / FS_T, ftv = (onx + FS_T - 1) / FS_T;
  std::vector<int> ft;
  for (int tu = 0; tu < ftu; ++tu)
    for (int tv = 0; tv < ftv; ++tv) {
      bool any = false;
      for (int u = tu * FS_T; u < std::min(ony, (tu + 1) * FS_T) && !any; ++u)
        for (int v = tv * FS_T; v < std::min(onx, (tv + 1) * FS_T) && !any; ++v)
          any = mask[(size_t)((u + ony / 2) % ony) * onx + (v + onx / 2) % onx] != 0;
      if (any) ft.push_back(tu * ftv + tv);
    }
  z->f_tiles_v = ftv;
  z->f_n_tiles = (int)ft.size();
  z->f_all_off = (int)ft.size();
  z->f_all_tiles = ftu * ftv;
  for (int i = 0; i < ftu * ftv; ++i) ft.push_back(i);
  int rc;
  if ((rc = ensure(c, z->d_ay, ay.size()))) return rc;
  if ((rc = ensure(c, z->d_ax, ax.size()))) return rc;
  if ((rc = ensure(c, z->d_tiles_all, all.size()))) return rc;
  if ((rc = ensure(c, z->d_ftiles, ft.size()))) return rc;
  if ((rc = ensure(c, z->d_fq, plane))) return rc;
  if ((rc = ensure(c, z->d_ft, (size_t)terms * plane))) return rc;
  HH_HIP(c, hipMemcpyAsync(z->d_ay, ay.data(), ay.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HH_HIP(c, hipMemcpyAsync(z->d_ax, ax.data(), ax.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HH_HIP(c, hipMemcpyAsync(z->d_tiles_all, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HH_HIP(c, hipMemcpyAsync(z->d_ftiles, ft.data(), ft.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HH_HIP(c, hipStreamSynchronize(c->stream));   // (the host vectors are locals)
  return HH_OK;
}

// One reference image's fftshifted spectrum *pwr through the filter (L commutes with fftshift); *pwr then names the result.
int filt_reference_plane(hh_ctx* c, const float** pwr) {
  hh_zoom* z = c->zoom;
  if (int rc = filt_y_passes(c, *pwr, 1)) return rc;
  FiltArgs a = filt_args(c, *pwr);
  a.tiles = z->d_ftiles + z->f_all_off;
  a.out = z->d_fq;
  a.n_seg = 0;
  hipLaunchKernelGGL(k_filter_xpass<true>, dim3(z->f_all_tiles, 1), dim3(256), 0, c->stream, a);
  HH_HIP(c, hipGetLastError());
  *pwr = z->d_fq;
  return HH_OK;
}

// Every hh_sweep* entry point with a filter set.  ld: row stride of d_scores (0: n_cand).
int filt_sweep(hh_ctx* c, const double* d_params, int64_t n_cand, float* d_scores, int64_t ld) {
  hh_zoom* z = c->zoom;
  const int64_t stride = ld > 0 ? ld : n_cand;
  const int S = c->n_segments, npart = z->f_n_tiles, J = z->f_terms;
  const size_t plane = (size_t)z->r_ony * z->r_onx;
  const int64_t fit = std::max<int64_t>(1, FS_BYTES / (int64_t)((1 + J) * plane * sizeof(float)));
  const int64_t cap = std::min<int64_t>(n_cand, std::min<int64_t>(fit, FS_BATCH));
  int rc;
  if ((rc = ensure(c, z->d_fq, (size_t)cap * plane))) return rc;
  if ((rc = ensure(c, z->d_ft, (size_t)J * cap * plane))) return rc;
  if ((rc = ensure(c, z->d_fpart, (size_t)S * cap * npart * 3))) return rc;
  c->last_first_pass = 4;
  const int all_tiles = ((z->r_ony + ZS_TU - 1) / ZS_TU) * ((z->r_onx + ZS_TV - 1) / ZS_TV);
  for (int64_t b0 = 0; b0 < n_cand; b0 += cap) {
    const int nb = (int)std::min<int64_t>(cap, n_cand - b0);
    ZoomSweepArgs za = zoom_args(c);
    za.params = d_params + 4 * b0;
    za.tiles = z->d_tiles_all;
    za.q_out = z->d_fq;
    if ((rc = launch_zoom_any<true>(c, za, all_tiles, nb))) return rc;
    if ((rc = filt_y_passes(c, z->d_fq, nb))) return rc;
    FiltArgs a = filt_args(c, z->d_fq);
    a.tiles = z->d_ftiles;
    a.partials = z->d_fpart;
    hipLaunchKernelGGL(k_filter_xpass<false>, dim3(npart, nb), dim3(256), 0, c->stream, a);
    HH_HIP(c, hipGetLastError());
    for (int s = 0; s < S; ++s) {
      hipLaunchKernelGGL(k_finalize, dim3(std::min(1024, (nb + 3) / 4)), dim3(256), 0, c->stream,
                         z->d_fpart + (size_t)s * nb * npart * 3, npart, (int64_t)nb, z->ref[s], d_scores + (size_t)s * stride + b0);
      HH_HIP(c, hipGetLastError());
    }
  }
  return HH_OK;
}

}  // namespace
