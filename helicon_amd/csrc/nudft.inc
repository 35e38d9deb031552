// nudft.inc — the type-2 non-uniform DFT of a stack of images at arbitrary points: what the pixel-size calibration
// (plugins/images2star/calibratepixelsize.py:88-156) asks of finufft.nufft2d2(x, y, f, eps = 1e-6), evaluated as the direct
// sum finufft approximates (isign = -1, centred modes, x paired with the FIRST image axis):
//     F[b][p] = sum_a sum_c f[b][a][c] exp(-i (x[p] (a - ny // 2) + y[p] (c - nx // 2)))
// The calibration's points lie on a polar band, so the sum does not separate over a tensor grid as fourier_zoom.inc's does; it
// is a matrix product per image instead, points x columns against columns x rows, on the exact-f32 MFMA (mfma_tile.inc):
//     T[a][p] = sum_c f[a][c] E[c][p],   E = exp(-i y[p] (c - nx // 2))          (re and im accumulators from one staged slice)
//     F[p]    = sum_a T[a][p] exp(-i x[p] (a - ny // 2))                          (on the accumulator tile, in registers)
// Neither E nor T leaves the registers.  A workgroup owns 64 points of one image (of a few images in turn when they are
// small) and walks the image in tiles of 64 rows.
//
// Phases.  Indices reach +-8192 and rates 4.44 rad / pixel, so every phase is reduced in float64 and in turns,
// frac(u k) with u = angle / 2 pi, before a sine or cosine is taken.  A lane holds the table exp(-i y j) of the NU_K / 2 column
// offsets j it supplies to the MFMA; per slice of NU_K columns it takes ONE float64 sincospi (the slice's first column) and
// forms each entry of E by one complex multiplication with its table: no chain, so no error builds up along the side.  The
// row factor is formed the same way: one float64 sincospi per row tile and a table of the accumulator's 16 row offsets, kept
// per point in LDS (it is read once per fold: every NU_FOLD columns of a row tile).
//
// The mean.  The product runs on f - mean(f) (float64 mean per image, subtracted in float64, rounded once); the mean's own
// term is separable, mean * sum_a e^{-i x (a - ny // 2)} * sum_c e^{-i y (c - nx // 2)}, and is evaluated in float64 per point
// (k_nudft_axis) and added in the epilogue: the result is the full sum, axis leakage included.
//
// Order.  A slice's products go into accumulators of their own (a chain of NU_K terms) which are then added, as in
// fc_pair_product, in float32 over at most NU_FOLD columns: then the row factor takes the tile into the float64 sum.  (Where
// the addends repeat, a float32 sum rounds the same way at every step: over the 512 slices of a 16384-column row a delta on
// the mean's floor, seen from the origin, lost 4e-6 of sum |f - mean|.)  Row tiles follow each other in ascending order; the
// four partial sums of a point (two accumulator row halves x two wavefronts) are added in a fixed order.  A lane's arithmetic
// depends on its own point and image only, so a value does not depend on the other points or images of the call, on its
// place among them, or on the run.

namespace {

constexpr int NUDFT_CHUNK = 32768;    // points of one launch (grid x = NUDFT_CHUNK / 64) and images of one launch (grid y)
constexpr int NU_T = 64;              // points, and image rows, of a workgroup's tile
constexpr int NU_K = 32;              // columns of one accumulator slice (one base sincospi each)
constexpr int NU_KS = 128;            // columns staged at once
constexpr int NU_FOLD = 512;          // columns whose slices are added in float32 before the row factor folds them into float64
constexpr int NU_MAX_SIDE = 16384;
constexpr double NU_2PI = 6.283185307179586476925286766559;

thread_local double nu_last_kernel_ms = 0.0;

// exp(-2 pi i u k), the phase reduced in turns in float64: |u k - rint(u k)| <= 1 / 2 is exact
__device__ __forceinline__ double2 nu_unit(double u, int k) {
  double t = u * (double)k;
  t -= rint(t);
  double s, c;
  sincospi(-2.0 * t, &s, &c);
  return make_double2(c, s);
}
__device__ __forceinline__ float2 nu_unit_f(double u, int k) {
  const double2 v = nu_unit(u, k);
  return make_float2((float)v.x, (float)v.y);
}

// |F| of the abs output and of the ring maximum: one instruction sequence
__device__ __forceinline__ float nu_abs(double re, double im) { return (float)sqrt(re * re + im * im); }

struct NuArgs {
  const float* img;      // [images of the launch][ny][nx], the image's mean removed
  const double* mean;    // [images of the launch]
  const double* x;       // [n_pts] the launch's points, radians per pixel
  const double* y;
  const double2* axis;   // [n_pts] sum_a e^{-i x (a - ny // 2)} * sum_c e^{-i y (c - nx // 2)}
  int ny, nx, n_pts, mode, group;
  int n_img, ipw;          // images of the launch; images one workgroup takes in turn
  int64_t p0, n_pts_all;   // the launch's first point in the call; points of the call (the output's row length)
  void* out;               // the launch's first image: float2 / float [image][n_pts_all], or unsigned [group]
};

__global__ __launch_bounds__(256) void k_nudft_center(float* __restrict__ img, const double* __restrict__ mean, int64_t plane) {
  float* const p = img + (int64_t)blockIdx.y * plane;
  const double m = mean[blockIdx.y];
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < plane; e += (int64_t)gridDim.x * 256) p[e] = (float)((double)p[e] - m);
}

__global__ __launch_bounds__(128) void k_nudft_axis(const double* __restrict__ x, const double* __restrict__ y, int n_pts, int ny, int nx,
                                                    double2* __restrict__ axis) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  const double ux = x[p] / NU_2PI, uy = y[p] / NU_2PI;
  double xr = 0, xi = 0, yr = 0, yi = 0;
  for (int a = 0; a < ny; ++a) {
    const double2 v = nu_unit(ux, a - ny / 2);
    xr += v.x;
    xi += v.y;
  }
  for (int c = 0; c < nx; ++c) {
    const double2 v = nu_unit(uy, c - nx / 2);
    yr += v.x;
    yi += v.y;
  }
  axis[p] = make_double2(xr * yr - xi * yi, xr * yi + xi * yr);
}

// A thread's share of a stage: rows row0 + 2 j of column col.  The address is clamped into the image (a side is at most 2^14,
// so the offset fits 32 bits) and the loads are unconditional, so that they issue back to back and stay in flight under the
// products; nu_store zeroes what lies outside the image when it writes the stage to LDS.
__device__ __forceinline__ void nu_fetch(float (&pre)[NU_T / 2], const float* __restrict__ img, int ny, int nx, int row0, int col) {
  const int colc = min(col, nx - 1);
#pragma unroll
  for (int j = 0; j < NU_T / 2; ++j) pre[j] = img[min(row0 + 2 * j, ny - 1) * nx + colc];
}
__device__ __forceinline__ void nu_store(float (&as)[NU_T][NU_KS + 1], const float (&pre)[NU_T / 2], int ny, int nx, int srow, int scol,
                                         int row0, int col) {
#pragma unroll
  for (int j = 0; j < NU_T / 2; ++j) as[srow + 2 * j][scol] = (row0 + 2 * j < ny && col < nx) ? pre[j] : 0.f;
}

// One workgroup: 64 points of `ipw` images in turn (its tables serve them all).  Lane (r, h) of the wavefront at (wm, wp)
// supplies the image's row wm + r and the point wp + r to the MFMA, and holds, of its point, the accumulator rows
// wm + acc_row(i, h).  A stage of NU_KS columns is read into registers under the products of the stage before it, and
// the base of the next slice is taken under the products of this one.
__global__ __launch_bounds__(256, 2) void k_nudft(NuArgs g) {
  __shared__ float as[NU_T][NU_KS + 1];
  __shared__ double2 red[4][NU_T];
  __shared__ float2 rtab[16][NU_T];   // exp(-i x j) of the accumulator's 16 row offsets j, per point
  const Tile64 t = tile64();
  const int pl = blockIdx.x * NU_T + t.wp + t.r;
  const bool live = pl < g.n_pts;
  const double ux = live ? g.x[pl] / NU_2PI : 0.0, uy = live ? g.y[pl] / NU_2PI : 0.0;
  const int ny = g.ny, nx = g.nx;
  float2 etab[NU_K / 2];
#pragma unroll
  for (int m = 0; m < NU_K / 2; ++m) etab[m] = nu_unit_f(uy, 2 * m + t.h);
  {  // the row table of the tile's 64 points, four entries a thread; the first stage's barrier publishes it
    const int pp = blockIdx.x * NU_T + (t.tid & 63);
    const double up = pp < g.n_pts ? g.x[pp] / NU_2PI : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = (t.tid >> 6) * 4 + q;
      rtab[i][t.tid & 63] = nu_unit_f(up, (i & 3) + 8 * (i >> 2));
    }
  }
  const int srow = t.tid >> 7, scol = t.tid & (NU_KS - 1);   // staging: this thread carries rows srow + 2 j of column scol
  const int b_end = min(g.n_img, ((int)blockIdx.y + 1) * g.ipw);
  for (int b = blockIdx.y * g.ipw; b < b_end; ++b) {
    const float* const img = g.img + (int64_t)b * ny * nx;
    double fre = 0.0, fim = 0.0;
    for (int a0 = 0; a0 < ny; a0 += NU_T) {
      f32x16 tre = {0}, tim = {0};
      float pre[NU_T / 2];
      nu_fetch(pre, img, ny, nx, a0 + srow, scol);
      float2 eb = nu_unit_f(uy, -(nx / 2));
      // the row factor of the accumulator tile: rows a0 + wm + 4 h + {0..3, 8..11, 16..19, 24..27}
      const float2 rb = nu_unit_f(ux, a0 + t.wm + 4 * t.h - ny / 2);
      for (int c0 = 0; c0 < nx; c0 += NU_KS) {
        nu_store(as, pre, ny, nx, srow, scol, a0 + srow, c0 + scol);
        __syncthreads();
        if (c0 + NU_KS < nx) nu_fetch(pre, img, ny, nx, a0 + srow, c0 + NU_KS + scol);
        const int kend = min(NU_KS, nx - c0);   // columns past nx are staged as zeros: their E entries do not matter
        for (int ks = 0; ks < kend; ks += NU_K) {
          const float2 en = nu_unit_f(uy, c0 + ks + NU_K - nx / 2);
          f32x16 sre = {0}, sim = {0};
#pragma unroll
          for (int m = 0; m < NU_K / 2; ++m) {
            const float av = as[t.wm + t.r][ks + 2 * m + t.h];
            const float er = eb.x * etab[m].x - eb.y * etab[m].y, ei = eb.x * etab[m].y + eb.y * etab[m].x;
            sre = __builtin_amdgcn_mfma_f32_32x32x2f32(av, er, sre, 0, 0, 0);
            sim = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ei, sim, 0, 0, 0);
          }
          tre += sre;
          tim += sim;
          eb = en;
        }
        if ((c0 + NU_KS) % NU_FOLD == 0 || c0 + NU_KS >= nx) {   // fold: once a row tile for a side up to NU_FOLD
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float2 rt = rtab[i][t.wp + t.r];
            const float rr = rb.x * rt.x - rb.y * rt.y, ri = rb.x * rt.y + rb.y * rt.x;
            fre += (double)tre[i] * (double)rr - (double)tim[i] * (double)ri;
            fim += (double)tre[i] * (double)ri + (double)tim[i] * (double)rr;
          }
          tre = f32x16{0};
          tim = f32x16{0};
        }
        __syncthreads();
      }
    }
    // red is free: the image's stages, each with two barriers, lie between this store and the last image's reads
    red[(t.wave >> 1) * 2 + t.h][t.wp + t.r] = make_double2(fre, fim);
    __syncthreads();
    const int p = blockIdx.x * NU_T + t.tid;
    if (t.tid < NU_T && p < g.n_pts) {
      double re = red[0][t.tid].x, im = red[0][t.tid].y;
#pragma unroll
      for (int q = 1; q < 4; ++q) {
        re += red[q][t.tid].x;
        im += red[q][t.tid].y;
      }
      const double m = g.mean[b];
      const double2 s = g.axis[p];
      re += m * s.x;
      im += m * s.y;
      const float ab = nu_abs(re, im);
      const int64_t pa = g.p0 + p, o = (int64_t)b * g.n_pts_all + pa;
      if (g.mode == 0) static_cast<float2*>(g.out)[o] = make_float2((float)re, (float)im);
      else if (g.mode == 1) static_cast<float*>(g.out)[o] = ab;
      else atomicMax(static_cast<unsigned*>(g.out) + pa % g.group, __float_as_uint(ab));   // ab >= 0: unsigned order = float order
    }
  }
}

}  // namespace

extern "C" int hh_nudft_chunk(void) { return NUDFT_CHUNK; }

extern "C" int hh_nudft_kernel_ms(double* ms) try {
  if (!ms) return fail(nullptr, HH_ERR_ARG, "hh_nudft_kernel_ms: NULL argument");
  *ms = nu_last_kernel_ms;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_nudft_kernel_ms")

extern "C" int hh_nudft2d2(int device, int32_t n_img, int32_t ny, int32_t nx, const float* images, int64_t n_pts, const double* x,
                           const double* y, int mode, int32_t group, void* out) try {
  if (!images || !x || !y || !out || n_img < 1 || n_pts < 1) return fail(nullptr, HH_ERR_ARG, "hh_nudft2d2: bad argument");
  if (ny < 1 || nx < 1 || ny > NU_MAX_SIDE || nx > NU_MAX_SIDE)
    return fail(nullptr, HH_ERR_ARG, "hh_nudft2d2: image sides " + std::to_string(ny) + " x " + std::to_string(nx) + " outside [1, " +
                                         std::to_string(NU_MAX_SIDE) + "]");
  if (mode < 0 || mode > 2) return fail(nullptr, HH_ERR_ARG, "hh_nudft2d2: mode " + std::to_string(mode) + " is none of 0 (complex64), 1 (abs), 2 (ring maximum)");
  if (mode == 2 && (group < 1 || (int64_t)group > n_pts))
    return fail(nullptr, HH_ERR_ARG, "hh_nudft2d2: the ring maximum needs a group in [1, n_pts]");
  if (int rc = use_device("hh_nudft2d2", device)) return rc;
  const int64_t plane = (int64_t)ny * nx;
  std::vector<double> mean((size_t)n_img);
  for (int32_t b = 0; b < n_img; ++b) {
    const float* const p = images + (int64_t)b * plane;
    double acc = 0.0;
    for (int64_t e = 0; e < plane; ++e) acc += (double)p[e];
    mean[(size_t)b] = acc / (double)plane;
  }
  const size_t n_out = mode == 2 ? (size_t)group : (size_t)n_img * (size_t)n_pts;
  const size_t out_bytes = n_out * (mode == 0 ? sizeof(float2) : sizeof(float));
  const int pts_max = (int)std::min<int64_t>(n_pts, NUDFT_CHUNK);
  DevArena mem;
  float* d_img = mem.get<float>((size_t)n_img * (size_t)plane);
  double* d_mean = mem.get<double>((size_t)n_img);
  double* d_x = mem.get<double>((size_t)n_pts);
  double* d_y = mem.get<double>((size_t)n_pts);
  double2* d_axis = mem.get<double2>((size_t)pts_max);
  unsigned char* d_out = mem.get<unsigned char>(out_bytes);
  if (int rc = arena_ok(nullptr, mem)) return rc;
  DevEvents<2> ev;
  hipError_t e = ev.create();
  if (e == hipSuccess) e = hipMemcpy(d_img, images, (size_t)n_img * (size_t)plane * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_mean, mean.data(), mean.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_x, x, (size_t)n_pts * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_y, y, (size_t)n_pts * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess && mode == 2) e = hipMemset(d_out, 0, out_bytes);
  if (e == hipSuccess) {
    (void)hipEventRecord(ev[0], nullptr);
    const unsigned cblocks = (unsigned)std::min<int64_t>((plane + 255) / 256, 1024);
    for (int32_t b0 = 0; b0 < n_img; b0 += NUDFT_CHUNK) {
      const int nb = std::min<int32_t>(NUDFT_CHUNK, n_img - b0);
      hipLaunchKernelGGL(k_nudft_center, dim3(cblocks, nb), dim3(256), 0, nullptr, d_img + (int64_t)b0 * plane, d_mean + b0, plane);
    }
    for (int64_t p0 = 0; p0 < n_pts; p0 += NUDFT_CHUNK) {
      const int np = (int)std::min<int64_t>(NUDFT_CHUNK, n_pts - p0);
      hipLaunchKernelGGL(k_nudft_axis, dim3((np + 127) / 128), dim3(128), 0, nullptr, d_x + p0, d_y + p0, np, ny, nx, d_axis);
      for (int32_t b0 = 0; b0 < n_img; b0 += NUDFT_CHUNK) {
        const int nb = std::min<int32_t>(NUDFT_CHUNK, n_img - b0);
        NuArgs g{};
        g.img = d_img + (int64_t)b0 * plane;
        g.mean = d_mean + b0;
        g.x = d_x + p0;
        g.y = d_y + p0;
        g.axis = d_axis;
        g.ny = ny; g.nx = nx; g.n_pts = np; g.mode = mode; g.group = mode == 2 ? group : 1;
        g.p0 = p0; g.n_pts_all = n_pts;
        // small images: a workgroup keeps its tables over up to 8 images, while the launch still has thousands of workgroups
        const int tiles = (np + NU_T - 1) / NU_T;
        g.n_img = nb;
        g.ipw = (int)std::min<int64_t>(8, std::max<int64_t>(1, (int64_t)nb * tiles / 4096));
        g.out = mode == 2 ? (void*)d_out : (void*)(d_out + (size_t)b0 * (size_t)n_pts * (mode == 0 ? sizeof(float2) : sizeof(float)));
        hipLaunchKernelGGL(k_nudft, dim3(tiles, (nb + g.ipw - 1) / g.ipw), dim3(TILE_THREADS), 0, nullptr, g);
      }
    }
    (void)hipEventRecord(ev[1], nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    float ms = 0.f;
    e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    nu_last_kernel_ms = ms;
  }
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_nudft2d2: ") + hipGetErrorString(e));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_nudft2d2")
