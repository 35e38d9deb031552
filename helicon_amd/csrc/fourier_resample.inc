// fourier_resample.inc — Fourier resampling of a 3-D map (or a 2-D image): fft_rescale's 3-D branch
// (lib/transforms.py:714-743), fft_crop (:610-660) and proc3d --fft_resample (plugins/proc3d/fft_resample.py:97-109).
//
// All three are one separable transform: a complex, RECTANGULAR operator per axis (out side x in side), applied to the
// volume as stored, then a pointwise epilogue.  The operators are built on the host in float64 and rounded once to f32
// (helicon_amd/fft_resample.py: rescale_operator, resample_operator, crop_operator); this file only applies them:
//     Y[b][m][p] = sum_k A[m][k] X[b][k][p],   A = Ar + i Ai  (M x K),   X real or complex (re / im planes)
// by k_axis_gemm (axis_pass.inc) on the shared exact-f32 MFMA tile (mfma_tile.inc).  A workgroup owns a 64 x 64 output tile and keeps TWO accumulators
// per wavefront (re and im); every K slice of X goes through LDS once and feeds both:
//     real X:     re += Ar X,            im += Ai X                 (2 MFMAs per k pair)
//     complex X:  re += Ar Xr + Na Xi,   im += Ai Xr + Ar Xi        (4; Na = -Ai is a third operator plane from the host,
//                                                                    so the minus sign costs no vector operation)
// Pass order z, y, x, each in the geometry axis_plan.h gives for its axis and its in / out sides, the x pass with the
// operands swapped (TR) so that its stores coalesce.  An axis without an operator is skipped.  The
// last pass applies the epilogue: STORE both planes, ABS = sqrt(re^2 + im^2) * scale, REAL = re * scale (the imaginary
// accumulator and its MFMAs are then not compiled in).  LDS: 3 operator planes of 64 x 33 and 2 input planes of 32 x 65
// floats = 42 KB on a complex input (34 KB under REAL), 25 KB on a real one.

namespace {

double g_fr_kernel_ms = 0.0;   // the last call's passes, by device events

}  // namespace

extern "C" int hh_separable_transform_3d(int device, const float* data, const int32_t in_shape[3], const int32_t out_shape[3],
                                         const float* const op_re[3], const float* const op_im[3], int epilogue, double scale,
                                         float* out0, float* out1) try {
  const char* fn = "hh_separable_transform_3d: ";
  if (!data || !in_shape || !out_shape || !op_re || !op_im || !out0) return fail(nullptr, HH_ERR_ARG, std::string(fn) + "NULL argument");
  if (epilogue != FR_STORE && epilogue != FR_ABS && epilogue != FR_REAL)
    return fail(nullptr, HH_ERR_ARG, std::string(fn) + "epilogue must be 0 (store), 1 (abs) or 2 (real)");
  if (epilogue == FR_STORE && !out1) return fail(nullptr, HH_ERR_ARG, std::string(fn) + "the store epilogue needs out1 (the imaginary plane)");
  int cur[3], dst[3];
  int last = -1;   // the last axis that has an operator
  for (int ax = 0; ax < 3; ++ax) {
    cur[ax] = in_shape[ax];
    dst[ax] = out_shape[ax];
    if (cur[ax] < 1 || cur[ax] > 1024 || dst[ax] < 1 || dst[ax] > 1024)
      return fail(nullptr, HH_ERR_ARG, std::string(fn) + "every side, in and out, must lie in [1, 1024]");
    if (!op_re[ax] && op_im[ax]) return fail(nullptr, HH_ERR_ARG, std::string(fn) + "an operator with an imaginary plane needs its real plane");
    if (!op_re[ax] && cur[ax] != dst[ax]) return fail(nullptr, HH_ERR_ARG, std::string(fn) + "an axis without an operator keeps its side");
    if (op_re[ax]) last = ax;
  }
  g_fr_kernel_ms = 0.0;
  if (last < 0) {   // nothing to multiply: the epilogue of the input itself
    const int64_t total = (int64_t)cur[0] * cur[1] * cur[2];
    for (int64_t i = 0; i < total; ++i) {
      if (epilogue == FR_STORE) { out0[i] = data[i]; out1[i] = 0.f; }
      else if (epilogue == FR_ABS) out0[i] = std::fabs(data[i]) * (float)scale;
      else out0[i] = data[i] * (float)scale;
    }
    return HH_OK;
  }
  if (int rc = use_device("hh_separable_transform_3d", device)) return rc;
  // plan: every pass reads the planes of the one before it and writes planes that have its out side along its axis
  struct Planned {
    int ax, M, K;
    bool cx;          // a complex input
    int epi;
    size_t a_off;     // of ar in `mats`; ai and na follow at M * K each when the operator has an imaginary plane
    bool has_im;
    int shape[3];     // of the output
  };
  std::vector<Planned> passes;
  std::vector<float> mats;
  bool cx = false;
  for (int ax = 0; ax < 3; ++ax) {
    if (!op_re[ax]) continue;
    Planned p{};
    p.ax = ax; p.M = dst[ax]; p.K = cur[ax]; p.cx = cx; p.epi = ax == last ? epilogue : FR_STORE;
    p.has_im = op_im[ax] != nullptr;
    p.a_off = mats.size();
    const size_t mk = (size_t)p.M * p.K;
    mats.insert(mats.end(), op_re[ax], op_re[ax] + mk);
    if (p.has_im) {
      mats.insert(mats.end(), op_im[ax], op_im[ax] + mk);
      mats.resize(mats.size() + mk);
      for (size_t i = 0; i < mk; ++i) mats[p.a_off + 2 * mk + i] = -op_im[ax][i];
    }
    cur[ax] = dst[ax];
    for (int a = 0; a < 3; ++a) p.shape[a] = cur[a];
    passes.push_back(p);
    cx = true;
  }
  DevArena mem;
  const int64_t total_in = (int64_t)in_shape[0] * in_shape[1] * in_shape[2];
  float* d_in = mem.get<float>((size_t)total_in);
  float* d_mats = mem.get<float>(mats.size());
  std::vector<float*> yr(passes.size(), nullptr), yi(passes.size(), nullptr);
  for (size_t i = 0; i < passes.size(); ++i) {
    const size_t total = (size_t)passes[i].shape[0] * passes[i].shape[1] * passes[i].shape[2];
    yr[i] = mem.get<float>(total);
    if (passes[i].epi == FR_STORE) yi[i] = mem.get<float>(total);
  }
  if (int rc = arena_ok(nullptr, mem)) return rc;
  DevEvents<2> evs;   // around the call's passes
  HH_HIP(nullptr, evs.create());
  hipError_t e = hipMemcpy(d_mats, mats.data(), mats.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_in, data, (size_t)total_in * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipEventRecord(evs[0], nullptr);
  int in_dims[3] = {in_shape[0], in_shape[1], in_shape[2]};
  for (size_t i = 0; e == hipSuccess && i < passes.size(); ++i) {
    const Planned& p = passes[i];
    const size_t mk = (size_t)p.M * p.K;
    const float* const ar = d_mats + p.a_off;
    const float* const op[3] = {ar, p.has_im ? ar + mk : nullptr, p.has_im ? ar + 2 * mk : nullptr};
    const float* const x[2] = {i ? yr[i - 1] : d_in, i ? yi[i - 1] : nullptr};   // complex after the first pass
    float* const y[2] = {yr[i], yi[i]};
    launch_axis_pass(axis_geom(in_dims, p.ax, p.M, 1), op, x, y, p.epi, (float)scale, nullptr);
    e = hipGetLastError();
    for (int a = 0; a < 3; ++a) in_dims[a] = p.shape[a];
  }
  if (e == hipSuccess) e = hipEventRecord(evs[1], nullptr);
  const size_t out_bytes = (size_t)dst[0] * dst[1] * dst[2] * sizeof(float);
  if (e == hipSuccess) e = hipMemcpy(out0, yr.back(), out_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess && epilogue == FR_STORE) e = hipMemcpy(out1, yi.back(), out_bytes, hipMemcpyDeviceToHost);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, evs[0], evs[1]);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string(fn) + hipGetErrorString(e));
  g_fr_kernel_ms = ms;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_separable_transform_3d")

extern "C" int hh_separable_transform_kernel_ms(double* ms) try {
  if (!ms) return fail(nullptr, HH_ERR_ARG, "hh_separable_transform_kernel_ms: NULL argument");
  *ms = g_fr_kernel_ms;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_separable_transform_kernel_ms")
