// axis_pass.inc — the separable axis passes: a dense operator applied along one axis of a volume as stored (no transposes),
// on the shared exact-f32 MFMA tile (mfma_tile.inc).  The geometry of a pass (its two views, strides and grid) and the
// operator builders are host arithmetic in axis_plan.h; this file holds the two kernels and the one launch of each.
//
//   k_circ_gemm   Y = A [X0; X1]: one accumulator and ONE fmaf chain over k, A square (n x n, or n x 2n over a [re; im]
//                 plane pair).  Users: the 3-D map filter (map_filter.inc, all three axes), the forward z / y passes of FSC
//                 and FRC (fourier_correlation.inc: fc_passes), the true FSC's inverse z / y passes (true_fsc.inc:
//                 tf_create) and the filtered sweep's y pass (filtered_sweep.inc: filt_y_passes).
//   k_axis_gemm   Y = (Ar + i Ai) (Xr + i Xi): a rectangular complex operator (M x K), re and im accumulators fed from one
//                 staged slice, the products interleaved per K slice, a fused epilogue.  User: Fourier resampling
//                 (fourier_resample.inc: hh_separable_transform_3d) and the 2-D transforms of image alignment (align.inc).
//
// The two bodies differ in how the sum over k is ordered, so neither can stand in for the other (DESIGN.md, "Separable axis
// passes").  Included into helicon_hip.hip after fail / HH_HIP and ahead of every file that launches a pass.

namespace {

constexpr int MF_T = 64;   // output tile of a workgroup: 64 rows of the operator x 64 columns of the volume
constexpr int MF_K = 32;   // K slice staged through LDS per step
static_assert(MF_T == AXIS_TILE, "axis_plan.h sizes the grid for this tile");

struct CircPass {
  const float* a;    // [n][ka] row-major operator block (ka = n, or 2n for [Cr | -Ci] / [Ci | Cr] on a complex input)
  const float* b0;   // input plane for k < n
  const float* b1;   // input plane for n <= k < 2n (imaginary part), or null when ka == n
  float* y;          // output plane
  int n, ka;
  int64_t np;        // columns P of the product
  int64_t sk, sp;    // element strides of B / Y along the operator's index and along P
  int64_t sb;        // element stride of one batch (the y pass: one z slice)
};

// Y[b][m][p] = sum_k A[m][k] B[b][k][p] on the shared tile (mfma_tile.inc), one 32 x 32 accumulator per wavefront.  TR swaps
// the MFMA's operands so that the accumulator's lane index runs along m: with the x pass's strides (sk = 1) the stores coalesce.
template <bool TR>
__global__ __launch_bounds__(256) void k_circ_gemm(CircPass g) {
  __shared__ float as[MF_T][MF_K + 1];
  __shared__ float bs[MF_K][MF_T + 1];
  const Tile64 t = tile64();
  const int tid = t.tid, r = t.r, h = t.h, wm = t.wm, wp = t.wp;
  const int m0 = blockIdx.y * MF_T;
  const int64_t p0 = (int64_t)blockIdx.x * MF_T, boff = (int64_t)blockIdx.z * g.sb;
  const float* b0 = g.b0 + boff;
  const float* b1 = g.b1 ? g.b1 + boff : nullptr;
  f32x16 acc = {0};
  for (int k0 = 0; k0 < g.ka; k0 += MF_K) {
    stage_rows(as, g.a, g.ka, m0, g.n, k0, g.ka, tid);
    for (int e = tid; e < MF_T * MF_K; e += 256) {   // its own: the stride along P and the split of K over b0 / b1
      int kk, pp;
      if (g.sp == 1) { kk = e / MF_T; pp = e % MF_T; }   // P contiguous: lanes along P
      else { pp = e / MF_K; kk = e % MF_K; }             // the x pass: lanes along k
      const int k = k0 + kk;
      const int64_t p = p0 + pp;
      float v = 0.f;
      if (k < g.ka && p < g.np) v = k < g.n ? b0[(int64_t)k * g.sk + p * g.sp] : b1[(int64_t)(k - g.n) * g.sk + p * g.sp];
      bs[kk][pp] = v;
    }
    __syncthreads();
    tile_mac<TR>(acc, as, bs, t);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = acc_row(i, h);
    const int m = m0 + wm + (TR ? r : row);
    const int64_t p = p0 + wp + (TR ? row : r);
    if (m < g.n && p < g.np) g.y[boff + (int64_t)m * g.sk + p * g.sp] = acc[i];
  }
}

// One k_circ_gemm pass in the geometry `v` (a square operator: v.M == v.K): y = a . [b0; b1], a the n x ka block.
void launch_circ_pass(const AxisGeom& v, const float* a, int ka, const float* b0, const float* b1, float* y, hipStream_t stream) {
  if (v.M != v.K) throw std::logic_error("launch_circ_pass: k_circ_gemm takes a square operator");
  CircPass g{};
  g.a = a;
  g.b0 = b0;
  g.b1 = b1;
  g.y = y;
  g.n = v.M;
  g.ka = ka;
  g.np = v.np; g.sk = v.sk; g.sp = v.sp_in; g.sb = v.sb_in;
  const dim3 grid((unsigned)v.gx, (unsigned)v.gy, (unsigned)v.gz);
  if (v.tr) hipLaunchKernelGGL(k_circ_gemm<true>, grid, dim3(256), 0, stream, g);
  else hipLaunchKernelGGL(k_circ_gemm<false>, grid, dim3(256), 0, stream, g);
}

// k_axis_gemm's epilogues.  FR_CROSS: P = E conj(Y) / max(|P|, scale) with E = (er, ei) a resident spectrum of one batch's
// shape, the phase-normalised cross-power spectrum of image alignment (align.inc); only P is stored.
enum { FR_STORE = 0, FR_ABS = 1, FR_REAL = 2, FR_CROSS = 3 };

struct AxisPass {
  const float* ar;    // [M][K] row-major operator planes: real, imaginary (null: a real operator) ...
  const float* ai;
  const float* na;    // ... and -imaginary (read on a complex input only)
  const float* xr;    // input planes; xi is read by the CX kernels only
  const float* xi;
  float* yr;          // output planes; yi is written under FR_STORE and FR_CROSS only
  float* yi;
  const float* er;    // FR_CROSS only: the planes of E, indexed as one batch of Y
  const float* ei;
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
      } else if (EPI == FR_CROSS) {
        const float er = g.er[off - bout], ei = g.ei[off - bout];
        const float pr = er * re[i] + ei * im[i], pi = ei * re[i] - er * im[i];
        const float d = fmaxf(hypotf(pr, pi), g.scale);
        g.yr[off] = pr / d;
        g.yi[off] = pi / d;
      } else {
        g.yr[off] = re[i] * g.scale;
      }
    }
  }
}

template <bool TR, bool CX>
void launch_axis_gemm(int epi, dim3 grid, const AxisPass& g, hipStream_t stream) {
  if (epi == FR_STORE) hipLaunchKernelGGL((k_axis_gemm<TR, CX, FR_STORE>), grid, dim3(256), 0, stream, g);
  else if (epi == FR_ABS) hipLaunchKernelGGL((k_axis_gemm<TR, CX, FR_ABS>), grid, dim3(256), 0, stream, g);
  else if (epi == FR_CROSS) hipLaunchKernelGGL((k_axis_gemm<TR, CX, FR_CROSS>), grid, dim3(256), 0, stream, g);
  else hipLaunchKernelGGL((k_axis_gemm<TR, CX, FR_REAL>), grid, dim3(256), 0, stream, g);
}

// One k_axis_gemm pass in the geometry `v`: op = {Ar, Ai, -Ai} (Ai and -Ai null: a real operator), x = {re, im} (im null:
// a real input), y = {re, im} (im written under FR_STORE and FR_CROSS only); cross = {re, im} of FR_CROSS's resident spectrum.
void launch_axis_pass(const AxisGeom& v, const float* const (&op)[3], const float* const (&x)[2], float* const (&y)[2], int epi,
                      float scale, hipStream_t stream, const float* const* cross = nullptr) {
  if ((epi == FR_CROSS) != (cross != nullptr)) throw std::logic_error("launch_axis_pass: FR_CROSS and its spectrum go together");
  AxisPass g{};
  if (cross) { g.er = cross[0]; g.ei = cross[1]; }
  g.ar = op[0]; g.ai = op[1]; g.na = op[2];
  g.xr = x[0]; g.xi = x[1];
  g.yr = y[0]; g.yi = y[1];
  g.M = v.M;
  g.K = v.K;
  g.np = v.np; g.sk = v.sk; g.sp_in = v.sp_in; g.sp_out = v.sp_out; g.sb_in = v.sb_in; g.sb_out = v.sb_out;
  g.scale = scale;
  const dim3 grid((unsigned)v.gx, (unsigned)v.gy, (unsigned)v.gz);
  const bool cx = x[1] != nullptr;
  if (v.tr) {
    if (cx) launch_axis_gemm<true, true>(epi, grid, g, stream);
    else launch_axis_gemm<true, false>(epi, grid, g, stream);
  } else {
    if (cx) launch_axis_gemm<false, true>(epi, grid, g, stream);
    else launch_axis_gemm<false, false>(epi, grid, g, stream);
  }
}

}  // namespace
