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

// The HH_GEN_* switches (the A/B switches of the tests), read once per sweep.
struct GenSwitches {
  bool direct, seg_loop, stockham;
};
GenSwitches gen_switches() {
  return GenSwitches{std::getenv("HH_GEN_DIRECT") != nullptr, std::getenv("HH_GEN_SEG_LOOP") != nullptr,
                     std::getenv("HH_GEN_STOCKHAM") != nullptr};
}

auto gen_fused_kernel(const GenDims& d) -> void (*)(GenFusedArgs) {
  return d.nx <= 256 ? k_gen_fused<4> : d.nx <= 512 ? k_gen_fused<8> : k_gen_fused<16>;
}

// The same list as last time (the reference app sweeps one grid over every class average): the run structure, the
// launch plan and the small device arrays of the last sweep are still right — checked by comparing the list with the
// copy kept from then (on the device for a device-only list: four bytes come back instead of the list).
int gen_same_list(hh_ctx* c, const GenSwitches& sw, int64_t batch_cap, const double* d_params, const double* h_params,
                  int64_t n_cand, bool* reuse) {
  hh_gen* g = c->gen;
  *reuse = false;
  if (!(g->plan_valid && g->plan_n == n_cand && std::memcmp(&g->plan_geom, &c->geom, sizeof(DevGeom)) == 0 &&
        g->plan_stockham == sw.stockham && g->plan_batch_cap == batch_cap))
    return HH_OK;
  if (h_params) {
    *reuse = std::memcmp(h_params, g->plan_params.data(), (size_t)n_cand * 4 * sizeof(double)) == 0;
    return HH_OK;
  }
  int differ = 1;
  HH_HIP(c, hipMemsetAsync(g->d_differ, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(k_gen_same_list, dim3((unsigned)std::min<int64_t>(1024, (n_cand * 4 + 255) / 256)), dim3(256), 0, c->stream,
                     reinterpret_cast<const unsigned long long*>(d_params), reinterpret_cast<const unsigned long long*>(g->d_plan_params.get()),
                     n_cand * 4, g->d_differ);
  HH_HIP(c, hipMemcpyAsync(&differ, g->d_differ, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HH_HIP(c, hipStreamSynchronize(c->stream));
  *reuse = differ == 0;
  return HH_OK;
}

// One batch holds the whole list: keep its plan for the next sweep.
int gen_keep_plan(hh_ctx* c, const GenSwitches& sw, int64_t batch_cap, const GenBatchPlan& bp, const double* d_params,
                  const double* h_params, int64_t n_cand) {
  hh_gen* g = c->gen;
  g->last = bp;
  g->plan_n = n_cand;
  g->plan_geom = c->geom;
  g->plan_stockham = sw.stockham;
  g->plan_batch_cap = batch_cap;
  g->plan_params.assign(h_params, h_params + (size_t)n_cand * 4);
  if (int rc = ensure(c, g->d_differ, 1)) return rc;
  if (int rc = ensure(c, g->d_plan_params, (size_t)n_cand * 4)) return rc;
  HH_HIP(c, hipMemcpyAsync(g->d_plan_params, d_params, (size_t)n_cand * 4 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  g->plan_valid = true;
  return HH_OK;
}

// Plans the batch that starts at candidate b0: its runs and sizes (sweep_plan.h), the buffers they need, the row kernel
// with its resident workgroups — nx = R1 R2 with both <= 32 takes the two-step row kernel (gen_rows.hip), anything else
// k_gen_fused — and the row launch's layers.  runs, layers: the plan's host arrays (reused from batch to batch).
// -> HH_OK, an error, or GEN_TOO_WIDE: a row too wide (or a table slice too tall) for the Stockham kernel's LDS.
constexpr int GEN_TOO_WIDE = 1;
int gen_plan_batch(hh_ctx* c, const GenSwitches& sw, const double* h_params, int64_t n_cand, int64_t b0, int64_t batch_cap,
                   GenRuns& runs_h, GenLayers& layers_h, GenBatchPlan* bp) {
  hh_gen* g = c->gen;
  const GenDims& d = g->d;
  if (!gen_batch_runs(h_params, n_cand, b0, batch_cap, c->geom.height, runs_h))
    return fail(c, HH_ERR_ARG, "rise too small for this image");
  const int nb = (int)(runs_h.end - b0), runs = (int)runs_h.run_first.size();
  const GenSizes z = gen_sizes(sweep_geom(c), runs_h.imax_all, runs_h.rise_all, d.nx, d.nxp);
  if (!z.ok) return fail(c, HH_ERR_ARG, "rise too small for the general-size path (more than 32 table rows per column group)");
  if (int rc = ensure(c, g->d_table, (size_t)runs * z.rows * d.nky)) return rc;
  if (int rc = ensure(c, g->d_eg, (size_t)nb * z.kg * d.nxp)) return rc;
  if (int rc = ensure(c, g->d_cgs, (size_t)nb * (d.nxp / 4 + 4))) return rc;
  if (int rc = ensure(c, g->d_runs, (size_t)3 * runs)) return rc;
  if (int rc = ensure(c, g->d_run_of, (size_t)nb)) return rc;
  if (int rc = ensure(c, g->d_partials, (size_t)nb * d.nky * 3)) return rc;
  GenRowsPlan rp{};
  const bool two_step = !sw.stockham && gen_rows_plan(d.nx, z.rows_lds, z.kg, &rp);
  if (two_step) {
    if (g->slots == 0 || g->slots_lds != rp.lds || !g->slots_two_step) {
      int per_cu = 0;
      HH_HIP(c, gen_rows_prepare(rp, &per_cu));
      g->slots = std::max(1, per_cu) * std::max(1, c->n_cu);
      g->slots_lds = rp.lds;
      g->slots_two_step = true;
    }
  } else {
    if (z.lds > 160 * 1024) return GEN_TOO_WIDE;
    if (int rc = ensure_lds_attr(c, reinterpret_cast<const void*>(gen_fused_kernel(d)), 160 * 1024)) return rc;
    if (g->slots == 0 || g->slots_lds != z.lds || g->slots_two_step) {
      int per_cu = 0;
      HH_HIP(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gen_fused_kernel(d), GEN_THREADS, z.lds));
      g->slots = std::max(1, per_cu) * std::max(1, c->n_cu);
      g->slots_lds = z.lds;
      g->slots_two_step = false;
    }
  }
  const int n_kb = two_step ? (d.nky + rp.rows_per_block - 1) / rp.rows_per_block : (d.nky + 7) / 8;
  const int len_typ = *std::max_element(runs_h.run_count.begin(), runs_h.run_count.end());
  gen_layers(runs_h.run_first, runs_h.run_count, fused_schedule(runs, len_typ, n_kb, g->slots), layers_h);
  const int layers = (int)layers_h.layer_run.size();
  if (int rc = ensure(c, g->d_layers, (size_t)3 * layers)) return rc;
  *bp = GenBatchPlan{nb, runs, z.rows, z.kg, z.rows_lds, n_kb, layers, z.lds, two_step, rp};
  return HH_OK;
}

// The plan's small arrays to the device: d_runs = [run_first, run_count, run_imax], d_run_of, d_layers = [layer_run,
// layer_first, layer_count].  The previous batch's kernels may still read them: the copies are stream-ordered behind them.
int gen_upload_plan(hh_ctx* c, const GenRuns& runs_h, const GenLayers& layers_h, const GenBatchPlan& bp) {
  hh_gen* g = c->gen;
  auto up = [&](int* dst, const std::vector<int>& src, int count) {
    return hipMemcpyAsync(dst, src.data(), (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream);
  };
  HH_HIP(c, up(g->d_runs, runs_h.run_first, bp.runs));
  HH_HIP(c, up(g->d_runs + bp.runs, runs_h.run_count, bp.runs));
  HH_HIP(c, up(g->d_runs + 2 * bp.runs, runs_h.run_imax, bp.runs));
  HH_HIP(c, up(g->d_run_of, runs_h.run_of, bp.nb));
  HH_HIP(c, up(g->d_layers, layers_h.layer_run, bp.layers));
  HH_HIP(c, up(g->d_layers + bp.layers, layers_h.layer_first, bp.layers));
  HH_HIP(c, up(g->d_layers + 2 * bp.layers, layers_h.layer_count, bp.layers));
  HH_HIP(c, hipStreamSynchronize(c->stream));  // (pageable host vectors are reused by the next batch)
  return HH_OK;
}

// The batch's run tables and column factors.  params: the batch's first candidate.
int gen_tables_and_factors(hh_ctx* c, const double* params, const GenBatchPlan& bp) {
  hh_gen* g = c->gen;
  const GenDims& d = g->d;
  int* const d_imax = g->d_runs + 2 * bp.runs;
  GenTableArgs ta{};
  ta.params = params;
  ta.run_first = g->d_runs;
  ta.run_imax = d_imax;
  ta.units = c->d_units;
  ta.tw_ny = g->d_tw_ny;
  ta.table = g->d_table;
  ta.cap = bp.rows;
  ta.g = c->geom;
  ta.d = d;
  hipLaunchKernelGGL(k_gen_run_table, dim3((bp.rows + 3) / 4, bp.runs), dim3(256), 0, c->stream, ta);

  GenFactorArgs fa{};
  fa.params = params;
  fa.units = c->d_units;
  fa.run_of = g->d_run_of;
  fa.run_imax = d_imax;
  fa.eg = g->d_eg;
  fa.cgs = g->d_cgs;
  fa.kg = bp.kg;
  fa.rows_lds = bp.rows_lds;
  fa.g = c->geom;
  fa.d = d;
  hipLaunchKernelGGL(k_gen_column_factors, dim3(bp.nb), dim3(256), (size_t)(bp.rows_lds + 1) * sizeof(float), c->stream, fa);
  HH_HIP(c, hipGetLastError());
  return HH_OK;
}

// The row pass's arguments against segment s's weights, as either row kernel takes them (GenRowsArgs, GenFusedArgs: the
// fields up to log_flag are the same).  q_out: where the pass stores the masked q of the batch (several segments in one
// contraction; the mask weights are the same for every segment, so s = 0 does), or NULL.
template <class Args>
Args gen_row_args(const hh_ctx* c, const GenBatchPlan& bp, int s, float* q_out) {
  const hh_gen* g = c->gen;
  const GenDims& d = g->d;
  Args a{};
  a.table = g->d_table;
  a.run_imax = g->d_runs + 2 * bp.runs;
  a.layer_run = g->d_layers;
  a.layer_first = g->d_layers + bp.layers;
  a.layer_count = g->d_layers + 2 * bp.layers;
  a.eg = g->d_eg;
  a.cgs = g->d_cgs;
  a.w2 = g->d_w2 + (size_t)s * d.nky * d.nx;
  a.tw_nx = g->d_tw_nx;
  a.partials = g->d_partials;
  a.q_out = q_out;
  a.q_stride = q_out ? (int64_t)g->kp : 0;
  a.cap = bp.rows;
  a.rows_lds = bp.rows_lds;
  a.kg = bp.kg;
  a.n_units = c->geom.n_units;
  a.log_flag = c->log_flag;
  if constexpr (std::is_same<Args, GenRowsArgs>::value) {
    a.nky = d.nky;
    a.nx = d.nx;
    a.nxp = d.nxp;
  } else {
    a.plan = g->plan;
    a.d = d;
  }
  return a;
}

// The row pass of the batch, two-step or Stockham as planned.
int gen_row_pass(hh_ctx* c, const GenBatchPlan& bp, int s, float* q_out) {
  if (bp.two_step) {
    HH_HIP(c, gen_rows_launch(bp.rp, bp.n_kb, bp.layers, c->stream, gen_row_args<GenRowsArgs>(c, bp, s, q_out)));
  } else {
    hipLaunchKernelGGL(gen_fused_kernel(c->gen->d), dim3(bp.n_kb, bp.layers), dim3(GEN_THREADS), bp.lds, c->stream,
                       gen_row_args<GenFusedArgs>(c, bp, s, q_out));
  }
  return HH_OK;
}

// Several segments: one pass of the row kernel stores the masked q of the batch, one MFMA contraction scores it against
// every segment (as the tuned path does, §8 of DESIGN.md).
int gen_scores_contracted(hh_ctx* c, const GenBatchPlan& bp, int64_t b0, float* d_scores, int64_t stride) {
  hh_gen* g = c->gen;
  const int nb = bp.nb, b_pad = (nb + 63) / 64 * 64;
  const int rows_c = (int)(g->kp / GEN_SEG_NK);
  if (b_pad > g->b_pad || !g->d_q) {
    if (int rc = ensure(c, g->d_q, (size_t)b_pad * g->kp)) return rc;
    if (int rc = ensure(c, g->d_cpart, (size_t)rows_c * b_pad * g->s_pad)) return rc;
    if (int rc = ensure(c, g->d_psum, (size_t)b_pad * 3)) return rc;
    HH_HIP(c, hipMemsetAsync(g->d_q, 0, (size_t)b_pad * g->kp * sizeof(float), c->stream));   // padding stays finite (and zero)
    g->b_pad = b_pad;
  }
  if (int rc = gen_row_pass(c, bp, 0, g->d_q)) return rc;
  hipLaunchKernelGGL(k_segment_corr, dim3(g->n_seg_slices, (nb + 255) / 256, g->s_pad / 64), dim3(256), 0, c->stream, g->d_q, g->d_wec,
                     (int)GEN_SEG_NK, g->kp, g->b_pad, g->s_pad, g->d_cpart, g->d_seg_slices);
  hipLaunchKernelGGL(k_sum_partials, dim3(std::min(1024, (nb + 3) / 4)), dim3(256), 0, c->stream, g->d_partials, g->d.nky, nb, g->d_psum);
  const int total = nb * c->n_segments;
  hipLaunchKernelGGL(k_finalize_segments, dim3((total + 255) / 256), dim3(256), 0, c->stream, g->d_psum, 1, g->d_cpart, g->n_seg_slices,
                     g->b_pad, g->s_pad, nb, c->n_segments, g->d_ref, d_scores, stride, b0);
  HH_HIP(c, hipGetLastError());
  return HH_OK;
}

// One segment, or HH_GEN_SEG_LOOP: a row pass and a finalize per segment.
int gen_scores_per_segment(hh_ctx* c, const GenBatchPlan& bp, int64_t b0, float* d_scores, int64_t stride) {
  hh_gen* g = c->gen;
  for (int s = 0; s < c->n_segments; ++s) {
    if (int rc = gen_row_pass(c, bp, s, nullptr)) return rc;
    hipLaunchKernelGGL(k_finalize, dim3(std::min(1024, (bp.nb + 3) / 4)), dim3(256), 0, c->stream, g->d_partials, g->d.nky,
                       (int64_t)bp.nb, c->ref[s], d_scores + (size_t)s * stride + b0);
    HH_HIP(c, hipGetLastError());
  }
  return HH_OK;
}

// The sweep: the list is cut into maximal runs of candidates that share (twist, csym, rot); consecutive runs go into
// one batch (bounded by GEN_BATCH candidates): one table launch, one factor launch, one row launch per segment (or one
// for all segments and a contraction).  Per batch: plan -> upload the plan's arrays -> tables + factors -> row pass +
// scores; a list that is the last sweep's single batch skips the first two.
int gen_sweep(hh_ctx* c, const double* d_params, const double* h_params, int64_t n_cand, float* d_scores, int64_t ld) {
  hh_gen* g = c->gen;
  const GenSwitches sw = gen_switches();
  if (c->geom.has_rot || g->direct_only || sw.direct) return gen_sweep_direct(c, d_params, h_params, n_cand, d_scores, ld);
  const int64_t stride = ld > 0 ? ld : n_cand;
  const bool seg_contract = c->n_segments > 1 && !sw.seg_loop;
  const int64_t batch_cap = gen_batch_cap(seg_contract, g->kp);
  bool reuse = false;
  if (int rc = gen_same_list(c, sw, batch_cap, d_params, h_params, n_cand, &reuse)) return rc;
  if (!reuse) g->plan_valid = false;
  if (!h_params && reuse) h_params = g->plan_params.data();
  if (!h_params) {  // a device-only list: bring it over once (the run structure is found on the host)
    g->h_params.resize((size_t)n_cand * 4);
    HH_HIP(c, hipMemcpyAsync(g->h_params.data(), d_params, (size_t)n_cand * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HH_HIP(c, hipStreamSynchronize(c->stream));
    h_params = g->h_params.data();
  }
  GenRuns runs_h;
  GenLayers layers_h;
  for (int64_t b0 = 0; b0 < n_cand;) {
    GenBatchPlan bp = g->last;
    int64_t b1 = n_cand;
    if (!reuse) {
      const int rc = gen_plan_batch(c, sw, h_params, n_cand, b0, batch_cap, runs_h, layers_h, &bp);
      // too wide for the Stockham kernel: the whole list goes the direct way, as the lengths without a plan do (batches
      // already launched are scored again: same values, stream-ordered)
      if (rc == GEN_TOO_WIDE) { g->plan_valid = false; return gen_sweep_direct(c, d_params, h_params, n_cand, d_scores, ld); }
      if (rc) return rc;
      if (int rc2 = gen_upload_plan(c, runs_h, layers_h, bp)) return rc2;
      b1 = runs_h.end;
    }
    g->last_row_kernel[0] = bp.two_step ? bp.rp.r1 : 0;
    g->last_row_kernel[1] = bp.two_step ? bp.rp.r2 : 0;
    g->last_row_kernel[2] = (int32_t)(bp.two_step ? bp.rp.lds : bp.lds);
    if (int rc = gen_tables_and_factors(c, d_params + 4 * b0, bp)) return rc;
    if (int rc = seg_contract ? gen_scores_contracted(c, bp, b0, d_scores, stride) : gen_scores_per_segment(c, bp, b0, d_scores, stride)) return rc;
    if (!reuse && b0 == 0 && b1 == n_cand)
      if (int rc = gen_keep_plan(c, sw, batch_cap, bp, d_params, h_params, n_cand)) return rc;
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
