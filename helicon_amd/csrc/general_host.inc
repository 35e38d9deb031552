// general_host.inc — host side of the general-size path (included by helicon_hip.hip inside its anonymous namespace,
// after fail / HH_HIP / ensure).  Kernels: general_sizes.inc.

bool gen_factor(int n, GenPlan& plan) {
  plan.n_stages = 0;
  int ns = 1;
  auto push = [&](int r) {
    if (plan.n_stages >= GEN_MAX_STAGES) return false;
    plan.radix[plan.n_stages] = r;
    plan.magic[plan.n_stages] = ns == 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)ns - 1) / (unsigned)ns);
    plan.n_stages++;
    ns *= r;
    return true;
  };
  int m = n;
  // powers of two: eights, with the remainder as fours rather than a lone radix-2 stage (200 = 8 x 5 x 5,
  // 320 = 8 x 8 x 5, 480 = 8 x 4 x 3 x 5, but 400 = 4 x 4 x 5 x 5, not 8 x 2 x 5 x 5)
  int e2 = 0;
  while (m % 2 == 0) { ++e2; m /= 2; }
  int n8 = e2 / 3, n4 = 0, n2 = 0;
  if (e2 % 3 == 2) n4 = 1;
  if (e2 % 3 == 1) { if (n8 > 0) { --n8; n4 = 2; } else n2 = 1; }
  for (int i = 0; i < n8; ++i) if (!push(8)) return false;
  for (int i = 0; i < n4; ++i) if (!push(4)) return false;
  for (int i = 0; i < n2; ++i) if (!push(2)) return false;
  while (m % 3 == 0) { if (!push(3)) return false; m /= 3; }
  while (m % 5 == 0) { if (!push(5)) return false; m /= 5; }
  for (int p = 7; p <= 31 && m > 1; p += 2)
    while (m % p == 0) { if (!push(p)) return false; m /= p; }
  return m == 1;
}

void gen_free(hh_ctx* c) {
  delete c->gen;   // its buffers free themselves
  c->gen = nullptr;
}

int gen_create(hh_ctx* c, int ny, int nx) {
  hh_gen* g = new (std::nothrow) hh_gen();
  if (!g) return fail(c, HH_ERR_NOMEM, "out of host memory");
  c->gen = g;
  g->d = GenDims{ny, nx, ny / 2 + 1, (nx + 3) / 4 * 4};
  // a row length with a prime factor above 31 (37, 74, 127 ...) has no row-transform plan: its sweeps take the direct
  // path (gen_sweep_direct: float64 transforms per candidate), and so does a list whose Stockham launch would need more
  // than the CU's 160 KB of LDS (gen_sweep) — every (ny, nx) in [8, 1024]^2 is served, those slowly.  What stays refused:
  // a rise so small that one column group reaches more than 32 table rows (kg > 32, gen_sweep).
  g->direct_only = !gen_factor(nx, g->plan);
  std::vector<float2> tw;
  for (int pass = 0; pass < 2; ++pass) {
    const int n = pass ? ny : nx;
    tw.resize((size_t)n);
    for (int k = 0; k < n; ++k) {
      const double ang = -2.0 * M_PI * (double)k / (double)n;
      tw[k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    DevBuf<float2>& dst = pass ? g->d_tw_ny : g->d_tw_nx;
    if (int rc = ensure(c, dst, tw.size())) return rc;
    HH_HIP(c, hipMemcpy(dst, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
  }
  return HH_OK;
}

// images (host, S x ny x nx) -> half-plane spectra in g->d_f ([S][nky][nx] double2)
int gen_spectra(hh_ctx* c, const float* images, int count) {
  hh_gen* g = c->gen;
  const GenDims& d = g->d;
  const size_t npix = (size_t)d.ny * d.nx;
  int rc = ensure(c, c->d_img, (size_t)count * npix);
  if (rc) return rc;
  if ((rc = ensure(c, g->d_r, (size_t)count * npix))) return rc;
  if ((rc = ensure(c, g->d_f, (size_t)count * d.nky * d.nx))) return rc;
  HH_HIP(c, hipMemcpyAsync(c->d_img, images, (size_t)count * npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_gen_dft_rows, dim3((d.nx + 127) / 128, d.ny, count), dim3(128), 0, c->stream, c->d_img, d, g->d_r);
  hipLaunchKernelGGL(k_gen_dft_cols, dim3((d.nx + 127) / 128, d.nky, count), dim3(128), 0, c->stream, g->d_r, d, g->d_f);
  HH_HIP(c, hipGetLastError());
  return HH_OK;
}

// helicon.low_high_pass_filter for one ny x nx image (host float32 in and out)
int gen_low_high_pass_filter(hh_ctx* c, const float* image, double low_pass_fraction, double high_pass_fraction, float* out) {
  hh_gen* g = c->gen;
  const GenDims& d = g->d;
  const size_t npix = (size_t)d.ny * d.nx;
  int rc = gen_spectra(c, image, 1);  // g->d_f: half plane [nky][nx]
  if (rc) return rc;
  DevArena mem;
  double2* d_full = mem.get<double2>(npix);
  float* d_out = mem.get<float>(npix);
  if ((rc = arena_ok(c, mem))) return rc;
  hipError_t e = hipSuccess;
  {
    // filters.py:362-369: each filter applies only for a fraction strictly inside (0, 1)
    const bool lp = low_pass_fraction > 0 && low_pass_fraction < 1, hp = high_pass_fraction > 0 && high_pass_fraction < 1;
    const double f2_lp = lp ? std::log(2.0) / (low_pass_fraction * low_pass_fraction) : 0.0;
    const double f2_hp = hp ? std::log(2.0) / (high_pass_fraction * high_pass_fraction) : 0.0;
    const dim3 grid((d.nx + 127) / 128, d.ny);
    hipLaunchKernelGGL(k_gen_filter_full, grid, dim3(128), 0, c->stream, g->d_f, d, f2_lp, f2_hp, d_full);
    hipLaunchKernelGGL(k_gen_idft_cols, grid, dim3(128), 0, c->stream, d_full, d, g->d_r);   // d_r holds ny x nx double2
    hipLaunchKernelGGL(k_gen_idft_rows, grid, dim3(128), 0, c->stream, g->d_r, d, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, HH_ERR_HIP, std::string("hh_low_high_pass_filter: ") + hipGetErrorString(e));
  return HH_OK;
}

int gen_set_reference(hh_ctx* c, const float* images, int n_segments, const uint8_t* mask, int log_flag) {
  hh_gen* g = c->gen;
  const GenDims& d = g->d;
  const int ny = d.ny, nx = d.nx;
  const size_t nh = (size_t)d.nky * nx;
  int rc = gen_spectra(c, images, n_segments);
  if (rc) return rc;
  std::vector<double2> spec((size_t)n_segments * nh);
  HH_HIP(c, hipMemcpyAsync(spec.data(), g->d_f, spec.size() * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
  HH_HIP(c, hipStreamSynchronize(c->stream));
  // Hermitian half-plane weights (any ny, nx): W[ky][kx] = mask(k) + mask(-k), except on the rows that are their own
  // mirror (ky = 0, and ky = ny/2 when ny is even), whose two members both lie in the half plane.
  auto mu = [&](int uy, int ux) {  // mask at unshifted frequency indices; fftshift moves u to (u + n/2) mod n
    return mask[(size_t)((uy + ny / 2) % ny) * nx + ((ux + nx / 2) % nx)] ? 1.f : 0.f;
  };
  std::vector<float> w(nh);
  double sw = 0;
  for (int ky = 0; ky < d.nky; ++ky) {
    const bool self = ky == 0 || 2 * ky == ny;
    for (int kx = 0; kx < nx; ++kx) {
      float v = mu(ky, kx);
      if (!self) v += mu(ny - ky, (nx - kx) % nx);
      w[(size_t)ky * nx + kx] = v;
      sw += v;
    }
  }
  if (!(sw > 0)) return fail(c, HH_ERR_ARG, "hh_set_reference: the mask selects no Fourier bin");
  c->n_segments = 0;
  // several segments: every segment's w (E - Ebar) as one [s_pad][kp] matrix for the contraction (zero rows / columns
  // of padding), beside the per-segment {w, w (E - Ebar)} pairs the one-segment kernels read
  const bool multi = n_segments > 1;
  const int s_pad = (n_segments + 63) / 64 * 64;
  const size_t kp = (nh + GEN_SEG_NK - 1) / GEN_SEG_NK * GEN_SEG_NK;
  std::vector<float> wecm(multi ? (size_t)s_pad * kp : 0, 0.f);
  std::vector<float2> w2((size_t)n_segments * nh);
  c->ref.assign(n_segments, RefConsts{});
  std::vector<double> e(nh);
  for (int s = 0; s < n_segments; ++s) {
    const double2* sp = spec.data() + (size_t)s * nh;
    double se = 0;
    for (size_t i = 0; i < nh; ++i) {
      const double a = std::hypot(sp[i].x, sp[i].y);
      e[i] = log_flag ? std::log1p(a) : a;
      se += (double)w[i] * e[i];
    }
    const double ebar = se / sw;
    double swec = 0, var_e = 0;
    for (size_t i = 0; i < nh; ++i) {
      const double dc = e[i] - ebar;
      const float wec = (float)((double)w[i] * dc);
      w2[(size_t)s * nh + i] = make_float2(w[i], wec);
      if (multi) wecm[(size_t)s * kp + i] = wec;
      swec += (double)wec;
      var_e += (double)w[i] * dc * dc;
    }
    c->ref[s] = RefConsts{sw, swec, var_e};
  }
  if ((rc = ensure(c, g->d_w2, w2.size()))) return rc;
  HH_HIP(c, hipMemcpyAsync(g->d_w2, w2.data(), w2.size() * sizeof(float2), hipMemcpyHostToDevice, c->stream));
  if (multi) {
    if ((rc = ensure(c, g->d_wec, wecm.size()))) return rc;
    if ((rc = ensure(c, g->d_ref, (size_t)n_segments))) return rc;
    HH_HIP(c, hipMemcpyAsync(g->d_wec, wecm.data(), wecm.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HH_HIP(c, hipMemcpyAsync(g->d_ref, c->ref.data(), (size_t)n_segments * sizeof(RefConsts), hipMemcpyHostToDevice, c->stream));
    std::vector<int> slices;   // 512-bin slices of the flat bin axis that carry any weight: the contraction skips the rest
    for (size_t sl = 0; sl < kp / GEN_SEG_NK; ++sl) {
      bool any = false;
      for (size_t i = sl * GEN_SEG_NK; i < std::min(nh, (sl + 1) * GEN_SEG_NK) && !any; ++i) any = w[i] > 0.f;
      if (any) slices.push_back((int)sl);
    }
    if ((rc = ensure(c, g->d_seg_slices, (kp / GEN_SEG_NK)))) return rc;
    HH_HIP(c, hipMemcpyAsync(g->d_seg_slices, slices.data(), slices.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    g->n_seg_slices = (int)slices.size();
    if (s_pad != g->s_pad || kp != g->kp) g->b_pad = 0;   // the batch buffers' shapes change with them
    g->s_pad = s_pad;
    g->kp = kp;
  }
  HH_HIP(c, hipStreamSynchronize(c->stream));
  c->n_segments = n_segments;
  c->log_flag = log_flag ? 1 : 0;
  return HH_OK;
}

// The sweep: the list is cut into maximal runs of candidates that share (twist, csym, rot); consecutive runs go into
// one batch (bounded by GEN_BATCH candidates): one table launch, one factor launch, one fused launch per segment.
constexpr int64_t GEN_BATCH = 65536;
constexpr int64_t GEN_SEG_BYTES = (int64_t)8 << 30;   // several segments: most bytes of masked q one batch may hold

// Candidates with out-of-plane tilt or in-plane rotation on a general image size (simulate_helical_projection takes any
// (ny, nx) with any tilt / psi, utils.py:31-47, 166-170): the shared-twist tables need tilt = psi = 0, so these go the
// direct way, candidate by candidate — the lattice's centres and the pixel raster of hh_simulate, the float64 direct
// transforms of the reference image's own spectrum, Pearson from float64 moments — in batches of as many images as
// 512 MB of scratch hold (and one launch's gridDim.z, 65,535, allows).  Exact and slow (tens of thousands of candidates per second at 200 x 200): the path for the few
// candidates a tilt / psi refinement looks at, not for a grid.
int gen_sweep_direct(hh_ctx* c, const double* d_params, const double* h_params, int64_t n_cand, float* d_scores, int64_t ld) {
  hh_gen* g = c->gen;
  const GenDims& d = g->d;
  const size_t npix = (size_t)d.ny * d.nx, nh = (size_t)d.nky * d.nx;
  const int64_t stride = ld > 0 ? ld : n_cand;
  std::vector<double> hp;
  if (!h_params) {
    hp.resize((size_t)n_cand * 4);
    HH_HIP(c, hipMemcpyAsync(hp.data(), d_params, hp.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HH_HIP(c, hipStreamSynchronize(c->stream));
    h_params = hp.data();
  }
  int64_t batch = std::max<int64_t>(1, std::min<int64_t>(n_cand, ((int64_t)512 << 20) / (int64_t)(npix * 20 + nh * 16)));
  batch = std::min<int64_t>(batch, 65535);   // a batch is the z extent of the transform launches
  int rc = ensure(c, c->d_img, (size_t)batch * npix);
  if (rc) return rc;
  if ((rc = ensure(c, g->d_r, (size_t)batch * npix))) return rc;
  if ((rc = ensure(c, g->d_f, (size_t)batch * nh))) return rc;
  if ((rc = ensure(c, g->d_ref, (size_t)c->n_segments))) return rc;
  HH_HIP(c, hipMemcpyAsync(g->d_ref, c->ref.data(), (size_t)c->n_segments * sizeof(RefConsts), hipMemcpyHostToDevice, c->stream));
  HH_HIP(c, hipStreamSynchronize(c->stream));   // (c->ref may change under a later hh_set_reference)
  for (int64_t g0 = 0; g0 < n_cand; g0 += batch) {
    const int nb = (int)std::min<int64_t>(batch, n_cand - g0);
    for (int i = 0; i < nb; ++i) {
      const double* p = h_params + 4 * (g0 + i);
      double im = std::ceil(c->geom.height / p[1]);   // (decode_candidate's own count, as hh_simulate sizes it)
      if (!(im >= 0.0)) im = -1.0;
      if (im > 1048576.0) im = 1048576.0;
      const int csym = std::max(1, std::min(360, (int)p[2]));
      const int64_t m64 = im < 0 ? 0 : (int64_t)(2 * (int64_t)im + 1) * csym * c->geom.n_units;
      if (m64 > (1 << 26)) return fail(c, HH_ERR_ARG, "rise too small for this image");
      const int m = (int)m64;
      if ((rc = ensure(c, g->d_cent, (size_t)std::max(m, 1)))) return rc;
      // (one centre buffer: the launches of a stream run in order, candidate i's raster is done with it before i + 1's centres)
      if (m > 0)
        hipLaunchKernelGGL(k_gen_centres, dim3((m + 255) / 256), dim3(256), 0, c->stream, d_params + 4 * (g0 + i), c->d_units, c->geom, m, g->d_cent);
      hipLaunchKernelGGL(k_gen_raster, dim3((d.nx + 127) / 128, d.ny), dim3(128), 0, c->stream, g->d_cent, m, c->geom, d, c->d_img + (size_t)i * npix);
    }
    hipLaunchKernelGGL(k_gen_dft_rows, dim3((d.nx + 127) / 128, d.ny, nb), dim3(128), 0, c->stream, c->d_img, d, g->d_r);
    hipLaunchKernelGGL(k_gen_dft_cols, dim3((d.nx + 127) / 128, d.nky, nb), dim3(128), 0, c->stream, g->d_r, d, g->d_f);
    hipLaunchKernelGGL(k_gen_direct_scores, dim3(nb), dim3(256), 0, c->stream, g->d_f, nh, c->log_flag, g->d_w2, c->n_segments, g->d_ref, d_scores,
                       stride, g0);
    HH_HIP(c, hipGetLastError());
  }
  c->last_first_pass = 0;
  g->last_row_kernel[0] = g->last_row_kernel[1] = g->last_row_kernel[2] = 0;
  return HH_OK;
}

int gen_sweep(hh_ctx* c, const double* d_params, const double* h_params, int64_t n_cand, float* d_scores, int64_t ld) {
  hh_gen* g = c->gen;
  const GenDims& d = g->d;
  if (c->geom.has_rot || g->direct_only || std::getenv("HH_GEN_DIRECT")) return gen_sweep_direct(c, d_params, h_params, n_cand, d_scores, ld);   // (HH_GEN_DIRECT: the A/B switch of the tests)
  // The same list as last time (the reference app sweeps one grid over every class average): the run structure, the
  // launch plan and the small device arrays of the last sweep are still right — checked by comparing the list with the
  // copy kept from then (on the device for a device-only list: four bytes come back instead of the list).
  const int npart = d.nky;
  const int64_t stride = ld > 0 ? ld : n_cand;
  // several segments: one pass of the row kernel stores the masked q of a batch, one MFMA contraction scores it against
  // every segment (as the tuned path does, §8 of DESIGN.md); the batch is bounded by the bytes of q
  const bool seg_contract = c->n_segments > 1 && !std::getenv("HH_GEN_SEG_LOOP");
  const int64_t batch_cap = seg_contract ? std::max<int64_t>(64, std::min<int64_t>(GEN_BATCH, GEN_SEG_BYTES / (int64_t)(g->kp * sizeof(float))) / 64 * 64)
                                         : GEN_BATCH;
  bool reuse = false;
  if (g->plan_valid && g->plan_n == n_cand && std::memcmp(&g->plan_geom, &c->geom, sizeof(DevGeom)) == 0 &&
      g->plan_stockham == (std::getenv("HH_GEN_STOCKHAM") != nullptr) && g->plan_batch_cap == batch_cap) {
    if (h_params) {
      reuse = std::memcmp(h_params, g->plan_params.data(), (size_t)n_cand * 4 * sizeof(double)) == 0;
    } else {
      int differ = 1;
      HH_HIP(c, hipMemsetAsync(g->d_differ, 0, sizeof(int), c->stream));
      hipLaunchKernelGGL(k_gen_same_list, dim3((unsigned)std::min<int64_t>(1024, (n_cand * 4 + 255) / 256)), dim3(256), 0, c->stream,
                         reinterpret_cast<const unsigned long long*>(d_params), reinterpret_cast<const unsigned long long*>(g->d_plan_params.get()),
                         n_cand * 4, g->d_differ);
      HH_HIP(c, hipMemcpyAsync(&differ, g->d_differ, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HH_HIP(c, hipStreamSynchronize(c->stream));
      reuse = differ == 0;
    }
  }
  if (!reuse) g->plan_valid = false;
  if (!h_params && reuse) h_params = g->plan_params.data();
  if (!h_params) {  // a device-only list: bring it over once (the run structure is found on the host)
    g->h_params.resize((size_t)n_cand * 4);
    HH_HIP(c, hipMemcpyAsync(g->h_params.data(), d_params, (size_t)n_cand * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HH_HIP(c, hipStreamSynchronize(c->stream));
    h_params = g->h_params.data();
  }
  std::vector<int> run_first, run_count, run_imax, run_of, layer_run, layer_first, layer_count;
  for (int64_t b0 = 0; b0 < n_cand;) {
    GenBatchPlan bp{};
    int64_t b1 = b0;
    int rc;
    if (reuse) {
      bp = g->last;
      b1 = n_cand;
    } else {
    // ---- the batch's runs
    run_first.clear(); run_count.clear(); run_imax.clear(); run_of.clear();
    double rise_all = INFINITY;
    int imax_all = 0;
    while (b1 < n_cand && (int64_t)run_first.size() < 65535) {
      const double* p = h_params + 4 * b1;
      int64_t len = 1;
      double rise_min = INFINITY;
      auto usable = [](double r) { return r > 0.0 && r < INFINITY; };
      if (usable(p[1])) rise_min = p[1];
      while (b1 + len < n_cand) {
        const double* q = p + 4 * len;
        if (!(q[0] == p[0] && q[2] == p[2] && q[3] == p[3])) break;
        if (usable(q[1])) rise_min = std::min(rise_min, q[1]);
        ++len;
      }
      if (b1 + len - b0 > batch_cap && b1 > b0) break;   // the batch is full: this run opens the next one
      len = std::min<int64_t>(len, batch_cap);            // (a run longer than a batch is swept in pieces)
      double im = rise_min < INFINITY ? std::ceil(c->geom.height / rise_min) : 0.0;
      if (im > 1048576.0) return fail(c, HH_ERR_ARG, "rise too small for this image");
      run_first.push_back((int)(b1 - b0));
      run_count.push_back((int)len);
      run_imax.push_back((int)im);
      for (int64_t k = 0; k < len; ++k) run_of.push_back((int)run_first.size() - 1);
      imax_all = std::max(imax_all, (int)im);
      if (rise_min < INFINITY) rise_all = std::min(rise_all, rise_min);
      b1 += len;
    }
    const int nb = (int)(b1 - b0), runs = (int)run_first.size();
    // ---- sizes
    const int rows = (2 * imax_all + 1) * c->geom.n_units;
    const double span4 = (3.0 + 2.0 * c->geom.rpx) * c->geom.apix + 2.0 * c->geom.slack;
    const double kgd = rise_all < INFINITY ? (std::floor(span4 / (double)(float)rise_all) + 2.0) * c->geom.n_units : 1.0;
    if (kgd > 32.0) return fail(c, HH_ERR_ARG, "rise too small for the general-size path (more than 32 table rows per column group)");
    const int kg = (int)kgd;
    const int rows_lds = std::max(rows, kg);
    const size_t lds = (size_t)16 * d.nxp * sizeof(float2) + (size_t)8 * rows_lds * sizeof(float2) +
                       (size_t)((d.nx + 1) & ~1) * sizeof(float2) + (size_t)kg * d.nxp * sizeof(float) +
                       (size_t)(d.nxp / 4 + 4) * sizeof(int);
    if ((rc = ensure(c, g->d_table, (size_t)runs * rows * d.nky))) return rc;
    if ((rc = ensure(c, g->d_eg, (size_t)nb * kg * d.nxp))) return rc;
    if ((rc = ensure(c, g->d_cgs, (size_t)nb * (d.nxp / 4 + 4)))) return rc;
    if ((rc = ensure(c, g->d_runs, (size_t)3 * runs))) return rc;
    if ((rc = ensure(c, g->d_run_of, (size_t)nb))) return rc;
    if ((rc = ensure(c, g->d_partials, (size_t)nb * npart * 3))) return rc;
    // ---- the fused launch's layers: whole runs while they fill whole rounds of resident workgroups, the runs of the
    // last round in shorter pieces (fused_schedule, as for the tuned kernels).  nx = R1 R2 with both <= 32 takes the
    // two-step row kernel (gen_rows.hip), anything else k_gen_fused.
    GenRowsPlan rp{};
    const bool two_step = !std::getenv("HH_GEN_STOCKHAM") && gen_rows_plan(d.nx, rows_lds, kg, &rp);
    void (*const fused_kernel)(GenFusedArgs) = d.nx <= 256 ? k_gen_fused<4> : d.nx <= 512 ? k_gen_fused<8> : k_gen_fused<16>;
    if (two_step) {
      if (g->slots == 0 || g->slots_lds != rp.lds || !g->slots_two_step) {
        int per_cu = 0;
        HH_HIP(c, gen_rows_prepare(rp, &per_cu));
        g->slots = std::max(1, per_cu) * std::max(1, c->n_cu);
        g->slots_lds = rp.lds;
        g->slots_two_step = true;
      }
    } else {
      // a row too wide (or a table slice too tall) for the Stockham kernel's LDS: the whole list goes the direct way, as
      // the lengths without a plan do (batches already launched are scored again: same values, stream-ordered)
      if (lds > 160 * 1024) { g->plan_valid = false; return gen_sweep_direct(c, d_params, h_params, n_cand, d_scores, ld); }
      if ((rc = ensure_lds_attr(c, reinterpret_cast<const void*>(fused_kernel), 160 * 1024))) return rc;
      if (g->slots == 0 || g->slots_lds != lds || g->slots_two_step) {
        int per_cu = 0;
        HH_HIP(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fused_kernel, GEN_THREADS, lds));
        g->slots = std::max(1, per_cu) * std::max(1, c->n_cu);
        g->slots_lds = lds;
        g->slots_two_step = false;
      }
    }
    const int n_kb = two_step ? (d.nky + rp.rows_per_block - 1) / rp.rows_per_block : (d.nky + 7) / 8;
    {
      const int len_typ = *std::max_element(run_count.begin(), run_count.end());
      const FusedSchedule fs = fused_schedule(runs, len_typ, n_kb, g->slots);
      for (int pass = 0; pass < 2; ++pass) {   // (second pass: one layer per run, if the cut-up list would not fit the grid)
        layer_run.clear(); layer_first.clear(); layer_count.clear();
        for (int r = 0; r < runs; ++r) {
          const int groups = pass ? 1 : (r < fs.runs_a ? fs.groups_a : fs.groups_b);
          const int cpw = (run_count[r] + groups - 1) / groups;
          for (int o = 0; o < run_count[r]; o += cpw) {
            layer_run.push_back(r);
            layer_first.push_back(run_first[r] + o);
            layer_count.push_back(std::min(cpw, run_count[r] - o));
          }
        }
        if (layer_run.size() <= 65535) break;
      }
    }
    const int layers = (int)layer_run.size();
    if ((rc = ensure(c, g->d_layers, (size_t)3 * layers))) return rc;
    int* const d_first = g->d_runs;
    int* const d_count = g->d_runs + runs;
    int* const d_imax = g->d_runs + 2 * runs;
    // the previous batch's kernels may still read these small arrays: the copies below are stream-ordered behind them
    HH_HIP(c, hipMemcpyAsync(d_first, run_first.data(), (size_t)runs * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HH_HIP(c, hipMemcpyAsync(d_count, run_count.data(), (size_t)runs * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HH_HIP(c, hipMemcpyAsync(d_imax, run_imax.data(), (size_t)runs * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HH_HIP(c, hipMemcpyAsync(g->d_run_of, run_of.data(), (size_t)nb * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HH_HIP(c, hipMemcpyAsync(g->d_layers, layer_run.data(), (size_t)layers * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HH_HIP(c, hipMemcpyAsync(g->d_layers + layers, layer_first.data(), (size_t)layers * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HH_HIP(c, hipMemcpyAsync(g->d_layers + 2 * layers, layer_count.data(), (size_t)layers * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HH_HIP(c, hipStreamSynchronize(c->stream));  // (pageable host vectors are reused by the next batch)
    bp = GenBatchPlan{nb, runs, rows, kg, rows_lds, n_kb, layers, lds, two_step, rp};
    }
    const int nb = bp.nb, runs = bp.runs, rows = bp.rows, kg = bp.kg, rows_lds = bp.rows_lds, n_kb = bp.n_kb, layers = bp.layers;
    const size_t lds = bp.lds;
    const bool two_step = bp.two_step;
    const GenRowsPlan rp = bp.rp;
    g->last_row_kernel[0] = two_step ? rp.r1 : 0;
    g->last_row_kernel[1] = two_step ? rp.r2 : 0;
    g->last_row_kernel[2] = (int32_t)(two_step ? rp.lds : lds);
    void (*const fused_kernel)(GenFusedArgs) = d.nx <= 256 ? k_gen_fused<4> : d.nx <= 512 ? k_gen_fused<8> : k_gen_fused<16>;
    int* const d_first = g->d_runs;
    int* const d_imax = g->d_runs + 2 * runs;

    GenTableArgs ta{};
    ta.params = d_params + 4 * b0;
    ta.run_first = d_first;
    ta.run_imax = d_imax;
    ta.units = c->d_units;
    ta.tw_ny = g->d_tw_ny;
    ta.table = g->d_table;
    ta.cap = rows;
    ta.g = c->geom;
    ta.d = d;
    hipLaunchKernelGGL(k_gen_run_table, dim3((rows + 3) / 4, runs), dim3(256), 0, c->stream, ta);

    GenFactorArgs fa{};
    fa.params = d_params + 4 * b0;
    fa.units = c->d_units;
    fa.run_of = g->d_run_of;
    fa.run_imax = d_imax;
    fa.eg = g->d_eg;
    fa.cgs = g->d_cgs;
    fa.kg = kg;
    fa.rows_lds = rows_lds;
    fa.g = c->geom;
    fa.d = d;
    hipLaunchKernelGGL(k_gen_column_factors, dim3(nb), dim3(256), (size_t)(rows_lds + 1) * sizeof(float), c->stream, fa);
    HH_HIP(c, hipGetLastError());

    if (seg_contract) {
      const int b_pad = (nb + 63) / 64 * 64;
      const int rows_c = (int)(g->kp / GEN_SEG_NK);
      if (b_pad > g->b_pad || !g->d_q) {
        if ((rc = ensure(c, g->d_q, (size_t)b_pad * g->kp))) return rc;
        if ((rc = ensure(c, g->d_cpart, (size_t)rows_c * b_pad * g->s_pad))) return rc;
        if ((rc = ensure(c, g->d_psum, (size_t)b_pad * 3))) return rc;
        HH_HIP(c, hipMemsetAsync(g->d_q, 0, (size_t)b_pad * g->kp * sizeof(float), c->stream));   // padding stays finite (and zero)
        g->b_pad = b_pad;
      }
      if (two_step) {
        GenRowsArgs ra{};
        ra.table = g->d_table;
        ra.run_imax = d_imax;
        ra.layer_run = g->d_layers;
        ra.layer_first = g->d_layers + layers;
        ra.layer_count = g->d_layers + 2 * layers;
        ra.eg = g->d_eg;
        ra.cgs = g->d_cgs;
        ra.w2 = g->d_w2;                 // the mask weights are the same for every segment
        ra.tw_nx = g->d_tw_nx;
        ra.partials = g->d_partials;
        ra.q_out = g->d_q;
        ra.q_stride = (int64_t)g->kp;
        ra.cap = rows;
        ra.rows_lds = rows_lds;
        ra.kg = kg;
        ra.n_units = c->geom.n_units;
        ra.log_flag = c->log_flag;
        ra.nky = d.nky;
        ra.nx = d.nx;
        ra.nxp = d.nxp;
        HH_HIP(c, gen_rows_launch(rp, n_kb, layers, c->stream, ra));
      } else {
        GenFusedArgs fu{};
        fu.table = g->d_table;
        fu.run_imax = d_imax;
        fu.layer_run = g->d_layers;
        fu.layer_first = g->d_layers + layers;
        fu.layer_count = g->d_layers + 2 * layers;
        fu.eg = g->d_eg;
        fu.cgs = g->d_cgs;
        fu.w2 = g->d_w2;
        fu.tw_nx = g->d_tw_nx;
        fu.partials = g->d_partials;
        fu.q_out = g->d_q;
        fu.q_stride = (int64_t)g->kp;
        fu.cap = rows;
        fu.rows_lds = rows_lds;
        fu.kg = kg;
        fu.n_units = c->geom.n_units;
        fu.log_flag = c->log_flag;
        fu.plan = g->plan;
        fu.d = d;
        hipLaunchKernelGGL(fused_kernel, dim3(n_kb, layers), dim3(GEN_THREADS), lds, c->stream, fu);
      }
      hipLaunchKernelGGL(k_segment_corr, dim3(g->n_seg_slices, (nb + 255) / 256, g->s_pad / 64), dim3(256), 0, c->stream, g->d_q, g->d_wec,
                         (int)GEN_SEG_NK, g->kp, g->b_pad, g->s_pad, g->d_cpart, g->d_seg_slices);
      hipLaunchKernelGGL(k_sum_partials, dim3(std::min(1024, (nb + 3) / 4)), dim3(256), 0, c->stream, g->d_partials, npart, nb, g->d_psum);
      const int total = nb * c->n_segments;
      hipLaunchKernelGGL(k_finalize_segments, dim3((total + 255) / 256), dim3(256), 0, c->stream, g->d_psum, 1, g->d_cpart, g->n_seg_slices,
                         g->b_pad, g->s_pad, nb, c->n_segments, g->d_ref, d_scores, stride, b0);
      HH_HIP(c, hipGetLastError());
    } else
    for (int s = 0; s < c->n_segments; ++s) {
      if (two_step) {
        GenRowsArgs ra{};
        ra.table = g->d_table;
        ra.run_imax = d_imax;
        ra.layer_run = g->d_layers;
        ra.layer_first = g->d_layers + layers;
        ra.layer_count = g->d_layers + 2 * layers;
        ra.eg = g->d_eg;
        ra.cgs = g->d_cgs;
        ra.w2 = g->d_w2 + (size_t)s * d.nky * d.nx;
        ra.tw_nx = g->d_tw_nx;
        ra.partials = g->d_partials;
        ra.cap = rows;
        ra.rows_lds = rows_lds;
        ra.kg = kg;
        ra.n_units = c->geom.n_units;
        ra.log_flag = c->log_flag;
        ra.nky = d.nky;
        ra.nx = d.nx;
        ra.nxp = d.nxp;
        HH_HIP(c, gen_rows_launch(rp, n_kb, layers, c->stream, ra));
      } else {
        GenFusedArgs fu{};
        fu.table = g->d_table;
        fu.run_imax = d_imax;
        fu.layer_run = g->d_layers;
        fu.layer_first = g->d_layers + layers;
        fu.layer_count = g->d_layers + 2 * layers;
        fu.eg = g->d_eg;
        fu.cgs = g->d_cgs;
        fu.w2 = g->d_w2 + (size_t)s * d.nky * d.nx;
        fu.tw_nx = g->d_tw_nx;
        fu.partials = g->d_partials;
        fu.cap = rows;
        fu.rows_lds = rows_lds;
        fu.kg = kg;
        fu.n_units = c->geom.n_units;
        fu.log_flag = c->log_flag;
        fu.plan = g->plan;
        fu.d = d;
        hipLaunchKernelGGL(fused_kernel, dim3(n_kb, layers), dim3(GEN_THREADS), lds, c->stream, fu);
      }
      const int threads = 256;
      hipLaunchKernelGGL(k_finalize, dim3(std::min(1024, (nb + 3) / 4)), dim3(threads), 0, c->stream, g->d_partials, npart,
                         (int64_t)nb, c->ref[s], d_scores + (size_t)s * stride + b0);
      HH_HIP(c, hipGetLastError());
    }
    if (!reuse && b0 == 0 && b1 == n_cand) {   // one batch holds the whole list: keep its plan for the next sweep
      g->last = bp;
      g->plan_n = n_cand;
      g->plan_geom = c->geom;
      g->plan_stockham = std::getenv("HH_GEN_STOCKHAM") != nullptr;
      g->plan_batch_cap = batch_cap;
      g->plan_params.assign(h_params, h_params + (size_t)n_cand * 4);
      if ((rc = ensure(c, g->d_differ, 1))) return rc;
      if ((rc = ensure(c, g->d_plan_params, (size_t)n_cand * 4))) return rc;
      HH_HIP(c, hipMemcpyAsync(g->d_plan_params, d_params, (size_t)n_cand * 4 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      g->plan_valid = true;
    }
    b0 = b1;
  }
  c->last_first_pass = 2;
  return HH_OK;
}

int gen_simulate(hh_ctx* c, const double* params, float* image_out) {
  hh_gen* g = c->gen;
  const GenDims& d = g->d;
  const size_t npix = (size_t)d.ny * d.nx;
  // number of lattice centres (decode_candidate on the host)
  double im = std::ceil(c->geom.height / params[1]);
  if (!(im >= 0.0)) im = -1.0;
  if (im > 1048576.0) im = 1048576.0;
  int csym = (int)params[2];
  csym = std::max(1, std::min(360, csym));
  const int64_t m64 = im < 0 ? 0 : (int64_t)(2 * (int64_t)im + 1) * csym * c->geom.n_units;
  if (m64 > (1 << 26)) return fail(c, HH_ERR_ARG, "hh_simulate: too many lattice centres");
  const int m = (int)m64;
  int rc = ensure(c, c->d_img, npix);
  if (rc) return rc;
  if ((rc = ensure(c, g->d_cent, (size_t)std::max(m, 1)))) return rc;
  DevArena mem;
  double* dp = mem.get<double>(4);
  if ((rc = arena_ok(c, mem))) return rc;
  hipError_t e = hipMemcpyAsync(dp, params, 4 * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    if (m > 0)
      hipLaunchKernelGGL(k_gen_centres, dim3((m + 255) / 256), dim3(256), 0, c->stream, dp, c->d_units, c->geom, m, g->d_cent);
    hipLaunchKernelGGL(k_gen_raster, dim3((d.nx + 127) / 128, d.ny), dim3(128), 0, c->stream, g->d_cent, m, c->geom, d, c->d_img);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(image_out, c->d_img, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  if (e != hipSuccess) return fail(c, HH_ERR_HIP, std::string("hh_simulate: ") + hipGetErrorString(e));
  return HH_OK;
}

int gen_power_spectrum(hh_ctx* c, const float* image, int log_flag, float* pwr_out, float* phase_out) {
  hh_gen* g = c->gen;
  const GenDims& d = g->d;
  const size_t npix = (size_t)d.ny * d.nx;
  int rc = gen_spectra(c, image, 1);
  if (rc) return rc;
  DevArena mem;
  float* d_out = mem.get<float>(2 * npix);
  unsigned* d_mm = mem.get<unsigned>(2);
  if ((rc = arena_ok(c, mem))) return rc;
  const unsigned init[2] = {0x7f800000u, 0u};
  hipError_t e = hipMemcpyAsync(d_mm, init, sizeof(init), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_gen_expand, dim3(d.ny), dim3(256), 0, c->stream, g->d_f, d, log_flag ? 1 : 0, d_out,
                       phase_out ? d_out + npix : nullptr, d_mm);
    hipLaunchKernelGGL(k_normalise, dim3(256), dim3(256), 0, c->stream, d_out, npix, d_mm);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(pwr_out, d_out, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && phase_out)
      e = hipMemcpyAsync(phase_out, d_out + npix, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  if (e != hipSuccess) return fail(c, HH_ERR_HIP, std::string("hh_power_spectrum: ") + hipGetErrorString(e));
  return HH_OK;
}
