// fourier_resample.inc — Fourier resampling of a 3-D map (or a 2-D image): fft_rescale's 3-D branch
// (lib/transforms.py:714-743), fft_crop (:610-660) and proc3d --fft_resample (plugins/proc3d/fft_resample.py:97-109).
//
// All three are one separable transform: a complex, RECTANGULAR operator per axis (out side x in side), applied to the
// volume as stored, then a pointwise epilogue.  The operators are built on the host in float64 and rounded once to f32
// (helicon_amd/fft_resample.py: rescale_operator, resample_operator, crop_operator); this file only applies them:
//     Y[b][m][p] = sum_k A[m][k] X[b][k][p],   A = Ar + i Ai  (M x K),   X real or complex (re / im planes)
// on the shared exact-f32 MFMA tile (mfma_tile.inc).  A workgroup owns a 64 x 64 output tile and keeps TWO accumulators
// per wavefront (re and im); every K slice of X goes through LDS once and feeds both:
//     real X:     re += Ar X,            im += Ai X                 (2 MFMAs per k pair)
//     complex X:  re += Ar Xr + Na Xi,   im += Ai Xr + Ar Xi        (4; Na = -Ai is a third operator plane from the host,
//                                                                    so the minus sign costs no vector operation)
// Pass order z, y, x as in map_filter.inc, same stride scheme (sk along the operator's index, sp along P, sb per batch),
// the x pass with the operands swapped (TR) so that its stores coalesce.  An axis without an operator is skipped.  The
// last pass applies the epilogue: STORE both planes, ABS = sqrt(re^2 + im^2) * scale, REAL = re * scale (the imaginary
// accumulator and its MFMAs are then not compiled in).  LDS: 3 operator planes of 64 x 33 and 2 input planes of 32 x 65
// floats = 42 KB on a complex input (34 KB under REAL), 25 KB on a real one.

namespace {

enum { FR_STORE = 0, FR_ABS = 1, FR_REAL = 2 };

struct AxisPass {
  const float* ar;    // [M][K] row-major operator planes: real, imaginary (null: a real operator) ...
  const float* ai;
  const float* na;    // ... and -imaginary (read on a complex input only)
  const float* xr;    // input planes; xi is read by the CX kernels only
  const float* xi;
  float* yr;          // output planes; yi is written under FR_STORE only
  float* yi;
  int M, K;
  int64_t np;             // columns P of the product
  int64_t sk;             // element stride along the operator's index, the same in X (k) and Y (m)
  int64_t sp_in, sp_out;  // element strides along P
  int64_t sb_in, sb_out;  // element strides of one batch (the y pass: one z slice)
  float scale;
};

template <bool TR, bool CX, int EPI>
__global__ __launch_bounds__(256) void k_axis_gemm(AxisPass g) {
  constexpr bool IM = EPI != FR_REAL;      // the imaginary accumulator exists
  constexpr int QI = 1, QN = IM ? 2 : 1, NA = 1 + (IM ? 1 : 0) + (CX ? 1 : 0);   // operator planes in LDS: Ar, [Ai], [-Ai]
  constexpr int XI = CX ? 1 : 0;
  __shared__ float as[NA][MF_T][MF_K + 1];
  __shared__ float bs[CX ? 2 : 1][MF_K][MF_T + 1];
  const Tile64 t = tile64();
  const int tid = t.tid, r = t.r, h = t.h, wm = t.wm, wp = t.wp;
  const int m0 = blockIdx.y * MF_T;
  const int64_t p0 = (int64_t)blockIdx.x * MF_T, bin = (int64_t)blockIdx.z * g.sb_in, bout = (int64_t)blockIdx.z * g.sb_out;
  const float* xr = g.xr + bin;
  const float* xi = CX ? g.xi + bin : nullptr;
  f32x16 re = {0}, im = {0};
  for (int k0 = 0; k0 < g.K; k0 += MF_K) {
    stage_rows(as[0], g.ar, g.K, m0, g.M, k0, g.K, tid);
    if constexpr (IM || CX) {
      if (g.ai) {
        if constexpr (IM) stage_rows(as[QI], g.ai, g.K, m0, g.M, k0, g.K, tid);
        if constexpr (CX) stage_rows(as[QN], g.na, g.K, m0, g.M, k0, g.K, tid);
      } else {   // a real operator: a zero imaginary plane
        for (int e = tid; e < MF_T * MF_K; e += TILE_THREADS) {
          if constexpr (IM) as[QI][e / MF_K][e % MF_K] = 0.f;
          if constexpr (CX) as[QN][e / MF_K][e % MF_K] = 0.f;
        }
      }
    }
    for (int e = tid; e < MF_T * MF_K; e += TILE_THREADS) {   // its own: the stride along P, one index for both planes
      int kk, pp;
      if (g.sp_in == 1) { kk = e / MF_T; pp = e % MF_T; }   // P contiguous: lanes along P
      else { pp = e / MF_K; kk = e % MF_K; }                // the x pass: lanes along k
      const int k = k0 + kk;
      const int64_t p = p0 + pp;
      const bool in = k < g.K && p < g.np;
      const int64_t off = (int64_t)k * g.sk + p * g.sp_in;
      bs[0][kk][pp] = in ? xr[off] : 0.f;
      if constexpr (CX) bs[XI][kk][pp] = in ? xi[off] : 0.f;
    }
    __syncthreads();
    tile_mac<TR>(re, as[0], bs[0], t);
    if constexpr (IM) tile_mac<TR>(im, as[QI], bs[0], t);
    if constexpr (CX) {
      tile_mac<TR>(re, as[QN], bs[XI], t);
      if constexpr (IM) tile_mac<TR>(im, as[0], bs[XI], t);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = acc_row(i, h);
    const int m = m0 + wm + (TR ? r : row);
    const int64_t p = p0 + wp + (TR ? row : r);
    if (m < g.M && p < g.np) {
      const int64_t off = bout + (int64_t)m * g.sk + p * g.sp_out;
      if (EPI == FR_STORE) {
        g.yr[off] = re[i];
        g.yi[off] = im[i];
      } else if (EPI == FR_ABS) {
        g.yr[off] = sqrtf(re[i] * re[i] + im[i] * im[i]) * g.scale;
      } else {
        g.yr[off] = re[i] * g.scale;
      }
    }
  }
}

template <bool TR, bool CX>
void launch_axis_gemm(int epi, dim3 grid, const AxisPass& g) {
  if (epi == FR_STORE) hipLaunchKernelGGL((k_axis_gemm<TR, CX, FR_STORE>), grid, dim3(256), 0, nullptr, g);
  else if (epi == FR_ABS) hipLaunchKernelGGL((k_axis_gemm<TR, CX, FR_ABS>), grid, dim3(256), 0, nullptr, g);
  else hipLaunchKernelGGL((k_axis_gemm<TR, CX, FR_REAL>), grid, dim3(256), 0, nullptr, g);
}

struct FrEvents {   // the two events around a call's passes
  hipEvent_t ev[2] = {};
  ~FrEvents() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

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
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(nullptr, HH_ERR_HIP, std::string(fn) + "no such HIP device (there is no CPU fallback)");
  HH_HIP(nullptr, hipSetDevice(device));
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
  FrEvents evs;
  for (hipEvent_t& e : evs.ev) HH_HIP(nullptr, hipEventCreate(&e));
  hipError_t e = hipMemcpy(d_mats, mats.data(), mats.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_in, data, (size_t)total_in * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipEventRecord(evs.ev[0], nullptr);
  int in_dims[3] = {in_shape[0], in_shape[1], in_shape[2]};
  for (size_t i = 0; e == hipSuccess && i < passes.size(); ++i) {
    const Planned& p = passes[i];
    const size_t mk = (size_t)p.M * p.K;
    AxisPass g{};
    g.ar = d_mats + p.a_off;
    g.ai = p.has_im ? g.ar + mk : nullptr;
    g.na = p.has_im ? g.ar + 2 * mk : nullptr;
    g.xr = i ? yr[i - 1] : d_in;
    g.xi = i ? yi[i - 1] : nullptr;
    g.yr = yr[i];
    g.yi = yi[i];
    g.M = p.M;
    g.K = p.K;
    g.scale = (float)scale;
    const int64_t ny_in = in_dims[1], nx_in = in_dims[2], ny_out = p.shape[1], nx_out = p.shape[2];
    dim3 grid;
    const unsigned mt = (unsigned)((p.M + MF_T - 1) / MF_T);
    if (p.ax == 0) {          // (onz x nz) . (nz x ny nx)
      g.np = ny_in * nx_in; g.sk = g.np; g.sp_in = g.sp_out = 1; g.sb_in = g.sb_out = 0;
      grid = dim3((unsigned)((g.np + MF_T - 1) / MF_T), mt, 1);
    } else if (p.ax == 1) {   // per z slice: (ony x ny) . (ny x nx)
      g.np = nx_in; g.sk = nx_in; g.sp_in = g.sp_out = 1; g.sb_in = ny_in * nx_in; g.sb_out = ny_out * nx_out;
      grid = dim3((unsigned)((g.np + MF_T - 1) / MF_T), mt, (unsigned)in_dims[0]);
    } else {                  // (nz ny x nx) . (onx x nx)^T
      g.np = (int64_t)in_dims[0] * ny_in; g.sk = 1; g.sp_in = nx_in; g.sp_out = nx_out; g.sb_in = g.sb_out = 0;
      grid = dim3((unsigned)((g.np + MF_T - 1) / MF_T), mt, 1);
    }
    if (p.ax == 2) {
      if (p.cx) launch_axis_gemm<true, true>(p.epi, grid, g);
      else launch_axis_gemm<true, false>(p.epi, grid, g);
    } else {
      if (p.cx) launch_axis_gemm<false, true>(p.epi, grid, g);
      else launch_axis_gemm<false, false>(p.epi, grid, g);
    }
    e = hipGetLastError();
    for (int a = 0; a < 3; ++a) in_dims[a] = p.shape[a];
  }
  if (e == hipSuccess) e = hipEventRecord(evs.ev[1], nullptr);
  const size_t out_bytes = (size_t)dst[0] * dst[1] * dst[2] * sizeof(float);
  if (e == hipSuccess) e = hipMemcpy(out0, yr.back(), out_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess && epilogue == FR_STORE) e = hipMemcpy(out1, yi.back(), out_bytes, hipMemcpyDeviceToHost);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, evs.ev[0], evs.ev[1]);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string(fn) + hipGetErrorString(e));
  g_fr_kernel_ms = ms;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_separable_transform_3d")

extern "C" int hh_separable_transform_kernel_ms(double* ms) try {
  if (!ms) return fail(nullptr, HH_ERR_ARG, "hh_separable_transform_kernel_ms: NULL argument");
  *ms = g_fr_kernel_ms;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_separable_transform_kernel_ms")
