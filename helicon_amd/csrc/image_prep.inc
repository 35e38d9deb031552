// image_prep.inc — the rest of the pre-sweep image preparation (SURVEY §8(f)4): what the reference does to a micrograph
// segment between reading it and handing it to the sweep / the least-squares scorer, where it goes through scikit-image:
//
//   hh_warp_affine_2d             helicon.transform_image (lib/transforms.py:238-312)       skimage.transform.warp, 2-D fast path
//   hh_rescale_2d                 binning (webApps/denovo3D/app.py:1911-1922) and
//                                 helicon.down_scale (lib/filters.py:375-412)               skimage.transform.rescale -> resize
//   hh_affine_transform_2d_cubic  auto_horizontalize's last step (webApps/denovo3D/utils.py:383-424):
//                                 rotate_shift_image(order = 3)                             scipy.ndimage.affine_transform(order = 3)
//   hh_ssim_2d, hh_joint_histogram  helicon.ssim_score / ms_ssim_score / mutual_information_score (lib/analysis.py:487-613):
//                                 the non-cosine scores of lsq_reconstruct (solver:484-524)     skimage.metrics
//   hh_helix_moments              helicon.estimate_helix_rotation_center_diameter
//                                 (lib/analysis.py:645-728)                                 skimage.morphology.closing + weighted moments
//
// scikit-image is not installed next to the reference in this build environment, so these are PINNED BY DERIVATION: each
// kernel restates what scikit-image 0.25 does for the call the reference makes — for rescale / resize that is a fixed
// sequence of scipy.ndimage calls (gaussian_filter, then zoom(grid_mode = True)), which oracle/prep.py makes on the
// installed SciPy; for warp it is the Cython loop of _warp_fast (float32 arithmetic for a float32 image, as there).
// Included into helicon_hip.hip after the resampling kernels it shares (k_spline_prefilter, spline_mirror).

namespace {

// ---- range of an image (skimage's clip step: _clip_warp_output works from the INPUT image's minimum and maximum) ---------
template <typename T>
__global__ __launch_bounds__(1024) void k_prep_minmax(const T* __restrict__ in, int64_t n, double* __restrict__ out /*[2]*/) {
  __shared__ double smin[1024], smax[1024];
  double lo = INFINITY, hi = -INFINITY;
  bool nan = false;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const double v = (double)in[i];
    nan |= v != v;
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
  smin[threadIdx.x] = nan ? NAN : lo;
  smax[threadIdx.x] = nan ? NAN : hi;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double a = smin[threadIdx.x], b = smin[threadIdx.x + s], c = smax[threadIdx.x], d = smax[threadIdx.x + s];
      smin[threadIdx.x] = (a != a || b != b) ? NAN : fmin(a, b);   // np.min / np.max propagate NaN
      smax[threadIdx.x] = (c != c || d != d) ? NAN : fmax(c, d);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = smin[0]; out[1] = smax[0]; }
}

// np.clip(out, min, max) with skimage's "preserve cval" rule: with mode = "constant" and a cval outside the image's range the
// pixels that are exactly cval keep it.  A NaN bound leaves the image alone (skimage: "if np.isnan(min_val): ... return").
template <typename T>
__global__ __launch_bounds__(256) void k_prep_clip(T* __restrict__ img, int64_t n, const double* __restrict__ range, int constant_mode, double cval) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double lo = range[0], hi = range[1];
  if (lo != lo || hi != hi) return;
  const bool preserve = constant_mode && !(lo <= cval && cval <= hi);
  const T v = img[i];
  if (preserve && v == (T)cval) return;
  img[i] = v < (T)lo ? (T)lo : (v > (T)hi ? (T)hi : v);
}

// ---- skimage.transform.warp, the 2-D fast path (_warp_fast: transform/_warps_cy.pyx) --------------------------------------
// For every output pixel (tfr, tfc):  (c, r) = H (tfc, tfr, 1)  [divided by the third row's product unless H is affine], then
// order 0: the pixel at (round(r), round(c)); order 1: bilinear_interpolation (interpolation.pxd) — corners at floor and CEIL
// of the coordinate, top = (1 - dc) tl + dc tr and bottom likewise in the image's own type, the vertical mix in float64.
// A corner outside the image is cval (mode "constant", get_pixel2d).  T is the image's type: skimage instantiates the loop
// for float32 and float64 and casts the matrix to that type.
template <typename T>
struct WarpArgs {
  T h[9];
  T cval;
  int rows, cols, order, affine;
};

template <typename T>
__global__ __launch_bounds__(256) void k_warp_affine(const T* __restrict__ in, WarpArgs<T> a, T* __restrict__ out) {
#pragma clang fp contract(off)
  const int tfc = blockIdx.x * 256 + threadIdx.x, tfr = blockIdx.y;
  if (tfc >= a.cols) return;
  const T x = (T)tfc, y = (T)tfr;
  T c = a.h[0] * x + a.h[1] * y + a.h[2];
  T r = a.h[3] * x + a.h[4] * y + a.h[5];
  if (!a.affine) {
    const T z = a.h[6] * x + a.h[7] * y + a.h[8];
    c = c / z;
    r = r / z;
  }
  auto pixel = [&](long rr, long cc) -> T {
    return (rr < 0 || rr >= a.rows || cc < 0 || cc >= a.cols) ? a.cval : in[(size_t)rr * a.cols + cc];
  };
  T v;
  if (a.order == 0) {
    v = pixel((long)round((double)r), (long)round((double)c));
  } else {
    const long minr = (long)floor((double)r), minc = (long)floor((double)c);
    const long maxr = (long)ceil((double)r), maxc = (long)ceil((double)c);
    const T dr = r - (T)minr, dc = c - (T)minc;
    const T tl = pixel(minr, minc), tr = pixel(minr, maxc), bl = pixel(maxr, minc), br = pixel(maxr, maxc);
    const double top = (double)(((T)1 - dc) * tl + dc * tr);
    const double bottom = (double)(((T)1 - dc) * bl + dc * br);
    v = (T)((double)((T)1 - dr) * top + (double)dr * bottom);
  }
  out[(size_t)tfr * a.cols + tfc] = v;
}

// ---- scipy.ndimage.gaussian_filter1d along one axis (mode "mirror") -----------------------------------------------------------
// ni_filters.c, NI_Correlate1D with a symmetric kernel: tmp = line[0] w[0] + sum_{j = -lw}^{-1} (line[j] + line[-j]) w[j] in
// float64 on a line extended by reflection about the end points' centres; the result is stored in the image's type after
// EVERY axis (gaussian_filter runs axis 0 into the output array and axis 1 in place on it).
template <typename T>
__global__ __launch_bounds__(256) void k_gauss_axis(const T* __restrict__ in, T* __restrict__ out, int rows, int cols, int axis,
                                                    const double* __restrict__ w /*[lw + 1]: w[j] = weight at distance j*/, int lw) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= cols) return;
  const int len = axis == 0 ? rows : cols, pos = axis == 0 ? y : x;
  auto at = [&](int i) -> double {
    const int m = spline_mirror(i, len);
    return (double)(axis == 0 ? in[(size_t)m * cols + x] : in[(size_t)y * cols + m]);
  };
  double tmp = at(pos) * w[0];
  for (int j = lw; j >= 1; --j) tmp += (at(pos - j) + at(pos + j)) * w[j];
  out[(size_t)y * cols + x] = (T)tmp;
}

// ---- scipy.ndimage.zoom(order, mode = "mirror", grid_mode = True) (ni_interpolation.c, NI_ZoomShift) --------------------------
// Output index k of an axis samples the input at cc = (k + 0.5) zoom - 0.5 (zoom = input length / output length), folded by
// reflection if it leaves [0, len - 1]; order 3: the four cubic B-spline taps from floor(cc) - 1 on the PREFILTERED image
// (k_spline_prefilter, float64), a tap outside the line mirrored; order 1: the two taps floor(cc), floor(cc) + 1 on the image
// itself.  Sum over (tap_y, tap_x), x inner, each term (coefficient * w_y) * w_x; stored in the image's type.
__device__ __forceinline__ double zoom_mirror_coord(double in, int len) {
  if (in < 0) {
    if (len <= 1) return 0.0;
    const int sz2 = 2 * len - 2;
    in = (double)sz2 * (double)(long long)(-in / (double)sz2) + in;
    return in <= (double)(1 - len) ? in + (double)sz2 : -in;
  }
  if (in > (double)(len - 1)) {
    if (len <= 1) return 0.0;
    const int sz2 = 2 * len - 2;
    in -= (double)sz2 * (double)(long long)(in / (double)sz2);
    if (in >= (double)len) in = (double)sz2 - in;
  }
  return in;
}

template <typename TC /*coefficients*/, typename T>
__global__ __launch_bounds__(256) void k_zoom_grid(const TC* __restrict__ c, int rows, int cols, int out_rows, int out_cols, double zoom_y,
                                                   double zoom_x, int order, T* __restrict__ out) {
#pragma clang fp contract(off)
  const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
  if (ox >= out_cols) return;
  const double cc[2] = {zoom_mirror_coord(((double)oy + 0.5) * zoom_y - 0.5, rows), zoom_mirror_coord(((double)ox + 0.5) * zoom_x - 0.5, cols)};
  const int dims[2] = {rows, cols};
  double w[2][4];
  int id[2][4];
  const int taps = order + 1;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const double f = floor(cc[d]);
    const double y = cc[d] - f, z = 1.0 - y;
    int start;
    if (order == 3) {
      w[d][1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
      w[d][2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
      w[d][0] = z * z * z / 6.0;
      w[d][3] = 1.0 - w[d][0] - w[d][1] - w[d][2];
      start = (int)f - 1;
    } else {
      w[d][0] = 1.0 - y;
      w[d][1] = y;
      w[d][2] = w[d][3] = 0.0;
      start = (int)f;
    }
    for (int q = 0; q < 4; ++q) id[d][q] = spline_mirror(start + q, dims[d]);
  }
  double t = 0.0;
  for (int qy = 0; qy < taps; ++qy)
    for (int qx = 0; qx < taps; ++qx) t += ((double)c[(size_t)id[0][qy] * cols + id[1][qx]] * w[0][qy]) * w[1][qx];
  out[(size_t)oy * out_cols + ox] = (T)t;
}

template <typename T>
__global__ void k_prep_to_f64(const T* __restrict__ in, int64_t n, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) out[t] = (double)in[t];
}

// ---- scipy.ndimage.affine_transform(order = 3, mode = "constant", cval = 0) of a 2-D image ------------------------------------
// (what rotate_shift_image(order = 3) calls, lib/transforms.py:315-369): the coordinate rule of k_affine_bilinear, the taps of
// k_map_cubic in two dimensions on the mirror-prefiltered image.
__global__ __launch_bounds__(256) void k_affine_cubic(const double* __restrict__ c, int ny, int nx, double m00, double m01, double m10,
                                                      double m11, double o0, double o1, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= nx) return;
  const double cc[2] = {m00 * (double)y + m01 * (double)x + o0, m10 * (double)y + m11 * (double)x + o1};
  float v = 0.f;
  if (cc[0] >= 0.0 && cc[0] <= (double)(ny - 1) && cc[1] >= 0.0 && cc[1] <= (double)(nx - 1)) {
    const int dims[2] = {ny, nx};
    double w[2][4];
    int id[2][4];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const double f = floor(cc[d]);
      const double yy = cc[d] - f, z = 1.0 - yy;
      w[d][1] = (yy * yy * (yy - 2.0) * 3.0 + 4.0) / 6.0;
      w[d][2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
      w[d][0] = z * z * z / 6.0;
      w[d][3] = 1.0 - w[d][0] - w[d][1] - w[d][2];
      for (int q = 0; q < 4; ++q) id[d][q] = spline_mirror((int)f - 1 + q, dims[d]);
    }
    double t = 0.0;
    for (int qy = 0; qy < 4; ++qy)
      for (int qx = 0; qx < 4; ++qx) t += (c[(size_t)id[0][qy] * nx + id[1][qx]] * w[0][qy]) * w[1][qx];
    v = (float)t;
  }
  out[(size_t)y * nx + x] = v;
}

// ---- helicon.estimate_helix_rotation_center_diameter (lib/analysis.py:645-728) -------------------------------------------------
// skimage.morphology.closing(data > threshold, mode = "ignore") with the default footprint (the 3 x 3 cross): a dilation that
// ignores what lies outside the image (any in-bounds neighbour set), then an erosion that does too (every in-bounds neighbour
// set).  STEP 0 writes the dilation of the thresholded image, STEP 1 its erosion.
template <typename T, int STEP>
__global__ __launch_bounds__(256) void k_closing_cross(const T* __restrict__ data, const unsigned char* __restrict__ prev, int rows, int cols,
                                                       double threshold, unsigned char* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= cols) return;
  auto get = [&](int yy, int xx) -> int {
    if (yy < 0 || yy >= rows || xx < 0 || xx >= cols) return STEP == 0 ? 0 : 1;
    if (STEP == 0) return (double)data[(size_t)yy * cols + xx] > threshold ? 1 : 0;
    return prev[(size_t)yy * cols + xx];
  };
  const int a = get(y, x), b = get(y - 1, x), c = get(y + 1, x), d = get(y, x - 1), e = get(y, x + 1);
  out[(size_t)y * cols + x] = (unsigned char)(STEP == 0 ? (a | b | c | d | e) : (a & b & c & d & e));
}

// _weighted_params (lib/analysis.py:685-708) over the closed mask, float64: w = I - min(I over the mask) + 1e-8; the weighted
// centroid; the weighted central second moments.  One workgroup (the images are a few hundred pixels a side): three sweeps,
// each reduced through LDS.  out = {pixels in the mask, cy, cx, i_yy, i_xx, i_xy, first row, last row}.
template <typename T>
__global__ __launch_bounds__(1024) void k_helix_moments(const T* __restrict__ data, const unsigned char* __restrict__ mask, int rows, int cols,
                                                        double* __restrict__ out /*[8]*/) {
#pragma clang fp contract(off)
  __shared__ double red[4][1024];
  const int tid = threadIdx.x;
  const int64_t n = (int64_t)rows * cols;
  auto reduce = [&](int k, auto op) {   // red[j][0] = op over the 1024 entries, j < k
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
      if (tid < s)
        for (int j = 0; j < k; ++j) red[j][tid] = op(j, red[j][tid], red[j][tid + s]);
      __syncthreads();
    }
  };
  // sweep 1: count, the mask's minimum, its first and last row
  double cnt = 0, lo = INFINITY, y0 = INFINITY, y1 = -INFINITY;
  for (int64_t i = tid; i < n; i += 1024)
    if (mask[i]) {
      cnt += 1.0;
      lo = fmin(lo, (double)data[i]);
      const double y = (double)(i / cols);
      y0 = fmin(y0, y);
      y1 = fmax(y1, y);
    }
  red[0][tid] = cnt; red[1][tid] = lo; red[2][tid] = y0; red[3][tid] = y1;
  reduce(4, [](int j, double a, double b) { return j == 0 ? a + b : (j == 3 ? fmax(a, b) : fmin(a, b)); });
  const double count = red[0][0], wmin = red[1][0], first = red[2][0], last = red[3][0];
  __syncthreads();
  // sweep 2: the weights' sum and first moments
  double cw = 0, sy = 0, sx = 0;
  for (int64_t i = tid; i < n; i += 1024)
    if (mask[i]) {
      const double w = (double)data[i] - wmin + 1e-8;
      cw += w;
      sy += (double)(i / cols) * w;
      sx += (double)(i % cols) * w;
    }
  red[0][tid] = cw; red[1][tid] = sy; red[2][tid] = sx;
  reduce(3, [](int, double a, double b) { return a + b; });
  const double tw = red[0][0], cy = red[1][0] / tw, cx = red[2][0] / tw;
  __syncthreads();
  // sweep 3: central second moments
  double myy = 0, mxx = 0, mxy = 0;
  for (int64_t i = tid; i < n; i += 1024)
    if (mask[i]) {
      const double w = (double)data[i] - wmin + 1e-8;
      const double uy = (double)(i / cols) - cy, ux = (double)(i % cols) - cx;
      myy += uy * uy * w;
      mxx += ux * ux * w;
      mxy += uy * ux * w;
    }
  red[0][tid] = myy; red[1][tid] = mxx; red[2][tid] = mxy;
  reduce(3, [](int, double a, double b) { return a + b; });
  if (tid == 0) {
    out[0] = count;
    out[1] = cy;
    out[2] = cx;
    out[3] = red[0][0] / tw;
    out[4] = red[1][0] / tw;
    out[5] = red[2][0] / tw;
    out[6] = first;
    out[7] = last;
  }
}

// ---- skimage.metrics.structural_similarity(im1, im2, data_range) with its defaults (7 x 7 uniform window, sample covariance,
// K1 = 0.01, K2 = 0.03), float32 images: what helicon.ssim_score / ms_ssim_score (lib/analysis.py:487-582) call for the
// non-cosine scores of lsq_reconstruct (solver:484-524).  scipy.ndimage.uniform_filter runs axis 0, then axis 1, each in float64
// with a float32 result; the mean is taken over the image without its 3-pixel rim, where the window never leaves the image —
// so only that part is formed.  STEP 0: the five axis-0 means (x, y, xx, yy, xy) of rows [3, rows - 3); STEP 1: the axis-1
// means, the SSIM map in float32 with numpy's operation order, and its float64 sum.
__global__ __launch_bounds__(256) void k_ssim_axis0(const float* __restrict__ a, const float* __restrict__ b, int rows, int cols,
                                                    float* __restrict__ out /*[5][rows][cols]*/) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y + 3;
  if (x >= cols || y >= rows - 3) return;
  double s[5] = {0, 0, 0, 0, 0};
  for (int d = -3; d <= 3; ++d) {
    const float p = a[(size_t)(y + d) * cols + x], q = b[(size_t)(y + d) * cols + x];
    s[0] += (double)p; s[1] += (double)q; s[2] += (double)(p * p); s[3] += (double)(q * q); s[4] += (double)(p * q);
  }
  const size_t plane = (size_t)rows * cols;
  for (int k = 0; k < 5; ++k) out[k * plane + (size_t)y * cols + x] = (float)(s[k] / 7.0);
}
__global__ __launch_bounds__(256) void k_ssim_map(const float* __restrict__ m /*[5][rows][cols]*/, int rows, int cols, float cov_norm, float c1,
                                                  float c2, double* __restrict__ sum) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int x = blockIdx.x * 256 + threadIdx.x + 3, y = blockIdx.y + 3;
  double val = 0.0;
  if (x < cols - 3 && y < rows - 3) {
    const size_t plane = (size_t)rows * cols;
    float u[5];
    for (int k = 0; k < 5; ++k) {
      double t = 0;
      for (int d = -3; d <= 3; ++d) t += (double)m[k * plane + (size_t)y * cols + x + d];
      u[k] = (float)(t / 7.0);
    }
    const float ux = u[0], uy = u[1];
    const float vx = cov_norm * (u[2] - ux * ux), vy = cov_norm * (u[3] - uy * uy), vxy = cov_norm * (u[4] - ux * uy);
    const float a1 = 2.f * ux * uy + c1, a2 = 2.f * vxy + c2, b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
    val = (double)((a1 * a2) / (b1 * b2));
  }
  red[threadIdx.x] = val;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) sum[blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// ---- np.histogramdd([a, b], bins) counts for skimage.metrics.normalized_mutual_information (helicon.mutual_information_score,
// lib/analysis.py:585-613): bin = the last edge not above the value (np.searchsorted(edges, v, "right") - 1), the outermost edge
// belonging to the last bin; edges are the host's np.linspace(min, max, bins + 1) in float64.
__global__ __launch_bounds__(256) void k_joint_hist(const float* __restrict__ a, const float* __restrict__ b, int64_t n, const double* __restrict__ ea,
                                                    const double* __restrict__ eb, int bins, unsigned long long* __restrict__ hist) {
  auto bin_of = [&](const double* e, double v) {
    int lo = 0, hi = bins + 1;              // count of edges <= v
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (e[mid] <= v) lo = mid + 1; else hi = mid; }
    int k = lo - 1;
    if (v == e[bins]) k = bins - 1;
    return k;
  };
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int ka = bin_of(ea, (double)a[i]), kb = bin_of(eb, (double)b[i]);
    if (ka >= 0 && ka < bins && kb >= 0 && kb < bins) atomicAdd(&hist[(size_t)ka * bins + kb], 1ull);
  }
}

// ---- host side, one function per element type -------------------------------------------------------------------------------------
template <typename T>
int prep_warp(const T* data, int rows, int cols, const double* inverse_matrix, int order, double cval, int clip, T* out) {
  const size_t n = (size_t)rows * cols;
  DevArena mem;
  T* d_in = mem.get<T>(n);
  T* d_out = mem.get<T>(n);
  double* d_range = mem.get<double>(2);
  if (int rc = arena_ok(nullptr, mem)) return rc;
  hipError_t e = hipMemcpy(d_in, data, n * sizeof(T), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    WarpArgs<T> a{};
    for (int i = 0; i < 9; ++i) a.h[i] = (T)inverse_matrix[i];   // matrix.astype(image.dtype)
    a.cval = (T)cval;
    a.rows = rows; a.cols = cols; a.order = order;
    a.affine = a.h[6] == (T)0 && a.h[7] == (T)0 && a.h[8] == (T)1;
    hipLaunchKernelGGL(k_warp_affine<T>, dim3((cols + 255) / 256, rows), dim3(256), 0, 0, d_in, a, d_out);
    if (clip) {
      hipLaunchKernelGGL(k_prep_minmax<T>, dim3(1), dim3(1024), 0, 0, d_in, (int64_t)n, d_range);
      hipLaunchKernelGGL(k_prep_clip<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_out, (int64_t)n, d_range, 1, cval);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, n * sizeof(T), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_warp_affine_2d: ") + hipGetErrorString(e));
  return HH_OK;
}

template <typename T>
int prep_rescale(const T* data, int rows, int cols, int out_rows, int out_cols, int order, int anti_aliasing, int clip, T* out) {
  const size_t n = (size_t)rows * cols, m = (size_t)out_rows * out_cols;
  DevArena mem;
  T* d_in = mem.get<T>(n);
  T* d_a = mem.get<T>(n);
  T* d_b = mem.get<T>(n);
  T* d_out = mem.get<T>(m);
  double* d_c = mem.get<double>(n);
  double* d_range = mem.get<double>(2);
  if (int rc = arena_ok(nullptr, mem)) return rc;
  hipError_t e = hipMemcpy(d_in, data, n * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_rescale_2d: ") + hipGetErrorString(e));
  const T* cur = d_in;
  // resize(): factors = input shape / output shape; anti_aliasing_sigma = max(0, (factors - 1) / 2); gaussian_filter skips an
  // axis whose sigma is <= 1e-15 and runs the others in axis order, the first from the input, the next in place
  const double factors[2] = {(double)rows / (double)out_rows, (double)cols / (double)out_cols};
  if (anti_aliasing) {
    T* dst[2] = {d_a, d_b};
    int pass = 0;
    for (int axis = 0; axis < 2; ++axis) {
      const double sigma = std::max(0.0, (factors[axis] - 1.0) / 2.0);
      if (!(sigma > 1e-15)) continue;
      const int lw = (int)(4.0 * sigma + 0.5);   // truncate = 4.0
      std::vector<double> w((size_t)lw + 1);
      double sum = 0.0;
      for (int j = -lw; j <= lw; ++j) sum += std::exp(-0.5 / (sigma * sigma) * (double)j * (double)j);
      for (int j = 0; j <= lw; ++j) w[(size_t)j] = std::exp(-0.5 / (sigma * sigma) * (double)j * (double)j) / sum;
      double* d_wa = mem.get<double>(w.size());
      if (int rc = arena_ok(nullptr, mem)) return rc;
      e = hipMemcpy(d_wa, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice);
      if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_rescale_2d: ") + hipGetErrorString(e));
      hipLaunchKernelGGL(k_gauss_axis<T>, dim3((cols + 255) / 256, rows), dim3(256), 0, 0, cur, dst[pass], rows, cols, axis, d_wa, lw);
      cur = dst[pass];
      ++pass;
    }
  }
  const double zoom_y = (double)rows / (double)out_rows, zoom_x = (double)cols / (double)out_cols;
  if (order == 3) {
    hipLaunchKernelGGL(k_prep_to_f64<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, cur, (int64_t)n, d_c);
    // spline_filter: axis 0 (lines = columns), then axis 1 (lines = rows)
    hipLaunchKernelGGL(k_spline_prefilter, dim3((unsigned)((cols + 127) / 128)), dim3(128), 0, 0, d_c, (int64_t)cols, rows, (int64_t)cols, (int64_t)cols);
    hipLaunchKernelGGL(k_spline_prefilter, dim3((unsigned)((rows + 127) / 128)), dim3(128), 0, 0, d_c, (int64_t)rows, cols, (int64_t)1, (int64_t)1);
    hipLaunchKernelGGL((k_zoom_grid<double, T>), dim3((out_cols + 255) / 256, out_rows), dim3(256), 0, 0, d_c, rows, cols, out_rows, out_cols, zoom_y,
                       zoom_x, 3, d_out);
  } else {
    hipLaunchKernelGGL((k_zoom_grid<T, T>), dim3((out_cols + 255) / 256, out_rows), dim3(256), 0, 0, cur, rows, cols, out_rows, out_cols, zoom_y, zoom_x,
                       1, d_out);
  }
  if (clip) {   // the range of the image as it came in (before the filter)
    hipLaunchKernelGGL(k_prep_minmax<T>, dim3(1), dim3(1024), 0, 0, d_in, (int64_t)n, d_range);
    hipLaunchKernelGGL(k_prep_clip<T>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, d_out, (int64_t)m, d_range, 0, 0.0);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, m * sizeof(T), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_rescale_2d: ") + hipGetErrorString(e));
  return HH_OK;
}

template <typename T>
int prep_moments(const T* data, int rows, int cols, double threshold, double* out) {
  const size_t n = (size_t)rows * cols;
  DevArena mem;
  T* d_in = mem.get<T>(n);
  unsigned char* d_dil = mem.get<unsigned char>(n);
  unsigned char* d_clo = mem.get<unsigned char>(n);
  double* d_out = mem.get<double>(8);
  if (int rc = arena_ok(nullptr, mem)) return rc;
  hipError_t e = hipMemcpy(d_in, data, n * sizeof(T), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const dim3 grid((cols + 255) / 256, rows);
    // `data > threshold` is NumPy's comparison of an array with a Python scalar: made in the IMAGE's type, so the threshold is
    // rounded to it first (a float32 pixel equal to float32(0.3) is not above 0.3)
    threshold = (double)(T)threshold;
    hipLaunchKernelGGL((k_closing_cross<T, 0>), grid, dim3(256), 0, 0, d_in, (const unsigned char*)nullptr, rows, cols, threshold, d_dil);
    hipLaunchKernelGGL((k_closing_cross<T, 1>), grid, dim3(256), 0, 0, d_in, d_dil, rows, cols, threshold, d_clo);
    hipLaunchKernelGGL(k_helix_moments<T>, dim3(1), dim3(1024), 0, 0, d_in, d_clo, rows, cols, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, 8 * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_helix_moments: ") + hipGetErrorString(e));
  return HH_OK;
}

}  // namespace

extern "C" {

int hh_warp_affine_2d(int device, const void* data, int is_f64, int rows, int cols, const double inverse_matrix[9], int order, double cval,
                      int clip, void* out) try {
  if (!data || !out || !inverse_matrix || rows < 1 || cols < 1 || (order != 0 && order != 1))
    return fail(nullptr, HH_ERR_ARG, "hh_warp_affine_2d: bad argument (orders 0 and 1 are provided)");
  if (int rc = use_device("hh_warp_affine_2d", device)) return rc;
  return is_f64 ? prep_warp(static_cast<const double*>(data), rows, cols, inverse_matrix, order, cval, clip, static_cast<double*>(out))
                : prep_warp(static_cast<const float*>(data), rows, cols, inverse_matrix, order, cval, clip, static_cast<float*>(out));
} HH_CATCH_CTX(nullptr, "hh_warp_affine_2d")

int hh_rescale_2d(int device, const void* data, int is_f64, int rows, int cols, int out_rows, int out_cols, int order, int anti_aliasing,
                  int clip, void* out) try {
  if (!data || !out || rows < 1 || cols < 1 || out_rows < 1 || out_cols < 1 || (order != 1 && order != 3))
    return fail(nullptr, HH_ERR_ARG, "hh_rescale_2d: bad argument (orders 1 and 3 are provided)");
  if (int rc = use_device("hh_rescale_2d", device)) return rc;
  return is_f64 ? prep_rescale(static_cast<const double*>(data), rows, cols, out_rows, out_cols, order, anti_aliasing, clip, static_cast<double*>(out))
                : prep_rescale(static_cast<const float*>(data), rows, cols, out_rows, out_cols, order, anti_aliasing, clip, static_cast<float*>(out));
} HH_CATCH_CTX(nullptr, "hh_rescale_2d")

int hh_affine_transform_2d_cubic(int device, const float* data, int ny, int nx, const double matrix[4], const double offset[2], float* out) try {
  if (!data || !out || !matrix || !offset || ny < 1 || nx < 1) return fail(nullptr, HH_ERR_ARG, "hh_affine_transform_2d_cubic: bad argument");
  if (int rc = use_device("hh_affine_transform_2d_cubic", device)) return rc;
  const size_t n = (size_t)ny * nx;
  DevArena mem;
  float* d_in = mem.get<float>(n);
  float* d_out = mem.get<float>(n);
  double* d_c = mem.get<double>(n);
  if (int rc = arena_ok(nullptr, mem)) return rc;
  hipError_t e = hipMemcpy(d_in, data, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_prep_to_f64<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, (int64_t)n, d_c);
    hipLaunchKernelGGL(k_spline_prefilter, dim3((unsigned)((nx + 127) / 128)), dim3(128), 0, 0, d_c, (int64_t)nx, ny, (int64_t)nx, (int64_t)nx);
    hipLaunchKernelGGL(k_spline_prefilter, dim3((unsigned)((ny + 127) / 128)), dim3(128), 0, 0, d_c, (int64_t)ny, nx, (int64_t)1, (int64_t)1);
    hipLaunchKernelGGL(k_affine_cubic, dim3((nx + 255) / 256, ny), dim3(256), 0, 0, d_c, ny, nx, matrix[0], matrix[1], matrix[2], matrix[3], offset[0],
                       offset[1], d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, n * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_affine_transform_2d_cubic: ") + hipGetErrorString(e));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_affine_transform_2d_cubic")

int hh_helix_moments(int device, const void* data, int is_f64, int rows, int cols, double threshold, double out[8]) try {
  if (!data || !out || rows < 1 || cols < 1) return fail(nullptr, HH_ERR_ARG, "hh_helix_moments: bad argument");
  if (int rc = use_device("hh_helix_moments", device)) return rc;
  return is_f64 ? prep_moments(static_cast<const double*>(data), rows, cols, threshold, out)
                : prep_moments(static_cast<const float*>(data), rows, cols, threshold, out);
} HH_CATCH_CTX(nullptr, "hh_helix_moments")

int hh_ssim_2d(int device, const float* a, const float* b, int rows, int cols, double data_range, double* out) try {
  if (!a || !b || !out || rows < 7 || cols < 7 || !(data_range > 0))
    return fail(nullptr, HH_ERR_ARG, "hh_ssim_2d: bad argument (the 7 x 7 window must fit the image, data_range > 0)");
  if (int rc = use_device("hh_ssim_2d", device)) return rc;
  const size_t n = (size_t)rows * cols;
  DevArena mem;
  const dim3 g0((cols + 255) / 256, rows - 6), g1((cols - 6 + 255) / 256, rows - 6);
  const int nsum = (int)(g1.x * g1.y);
  float* d_a = mem.get<float>(n);
  float* d_b = mem.get<float>(n);
  float* d_m = mem.get<float>(5 * n);
  double* d_sum = mem.get<double>((size_t)nsum);
  if (int rc = arena_ok(nullptr, mem)) return rc;
  hipError_t e = hipMemcpy(d_a, a, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_b, b, n * sizeof(float), hipMemcpyHostToDevice);
  std::vector<double> sums((size_t)nsum);
  if (e == hipSuccess) {
    // numpy's scalars: cov_norm = 49 / 48 and C = (K R)^2 enter float32 arithmetic as float32 (R is a float32 range)
    const float r = (float)data_range, k1r = 0.01f * r, k2r = 0.03f * r;
    hipLaunchKernelGGL(k_ssim_axis0, g0, dim3(256), 0, 0, d_a, d_b, rows, cols, d_m);
    hipLaunchKernelGGL(k_ssim_map, g1, dim3(256), 0, 0, d_m, rows, cols, (float)(49.0 / 48.0), k1r * k1r, k2r * k2r, d_sum);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(sums.data(), d_sum, sums.size() * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_ssim_2d: ") + hipGetErrorString(e));
  double t = 0;
  for (double v : sums) t += v;
  *out = t / ((double)(rows - 6) * (double)(cols - 6));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_ssim_2d")

int hh_joint_histogram(int device, const float* a, const float* b, int64_t n, const double* edges_a, const double* edges_b, int bins,
                       int64_t* hist) try {
  if (!a || !b || !edges_a || !edges_b || !hist || n < 1 || bins < 1 || bins > 4096)
    return fail(nullptr, HH_ERR_ARG, "hh_joint_histogram: bad argument");
  if (int rc = use_device("hh_joint_histogram", device)) return rc;
  DevArena mem;
  const size_t nb = (size_t)bins * bins;
  float* d_a = mem.get<float>((size_t)n);
  float* d_b = mem.get<float>((size_t)n);
  double* d_ea = mem.get<double>((size_t)bins + 1);
  double* d_eb = mem.get<double>((size_t)bins + 1);
  unsigned long long* d_h = mem.get<unsigned long long>(nb);
  if (int rc = arena_ok(nullptr, mem)) return rc;
  hipError_t e = hipMemcpy(d_a, a, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_b, b, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_ea, edges_a, ((size_t)bins + 1) * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_eb, edges_b, ((size_t)bins + 1) * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_h, 0, nb * sizeof(unsigned long long));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_joint_hist, dim3((unsigned)std::min<int64_t>(1024, (n + 255) / 256)), dim3(256), 0, 0, d_a, d_b, n, d_ea, d_eb, bins, d_h);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(hist, d_h, nb * sizeof(int64_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_joint_histogram: ") + hipGetErrorString(e));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_joint_histogram")

}  // extern "C"
