// fourier_zoom.inc — compute_power_spectra with a Fourier-space zoom (cutoff_res / output_size): lib/transforms.py:663-713
// (fft_rescale, 2-D branch) + :771-820.  The reference evaluates the image's Fourier transform at ony x onx frequencies
//     f_y[u] = fftfreq(ony)[u] * 2 * apix / cutoff_res_y,      f_x[v] = fftfreq(onx)[v] * 2 * apix / cutoff_res_x
// (cycles per pixel) with finufft.nufft2d2 — type 2, e^{-i m x}, modes m = index - n // 2, eps = 1e-6 — then multiplies by
// (-1)^(u + v), fftshifts, takes |F| (log1p), min-max normalises, and returns the phase of the shifted transform.
// finufft is an approximation (to 1e-6) of the direct sum, which is what runs here, in float64 and separably:
//     R[a][v] = sum_b image[a][b] e^{-2 pi i f_x[v] (b - nx // 2)}          (k_zoom_rows)
//     F[u][v] = sum_a R[a][v]     e^{-2 pi i f_y[u] (a - ny // 2)}          (k_zoom_cols: + sign, shift, |.|, phase, min / max)
// O(ny nx onx + ony ny onx) complex multiply-adds: 0.27 G at 512 -> 512, a millisecond or so of float64 — the zoom is a
// once-per-image preparation step, not part of the sweep.  Pinned by derivation (finufft is not installed where the
// fixtures are made): the oracle's direct sum reproduces np.fft.fft2 for the default arguments, where fft_rescale
// provably equals it (DESIGN.md section 1), and the device is held to the oracle elsewhere.

namespace {

struct ZoomDims {
  int ny, nx, ony, onx;
  double sy, sx;   // 2 apix / cutoff_res (1 = the image's own Nyquist: no zoom)
};

__device__ __forceinline__ double zoom_freq(int idx, int n, double scale, double apix2, double cutoff) {
  const int sv = idx <= (n - 1) / 2 ? idx : idx - n;   // np.fft.fftfreq's signed index
  (void)scale;
  return (double)sv / (double)n * 2.0 * apix2 / cutoff;   // fftfreq(n) * 2 * apix / cutoff, the reference's order
}

__global__ __launch_bounds__(128) void k_zoom_rows(const float* __restrict__ img, ZoomDims d, double apix, double cutoff_x,
                                                   double2* __restrict__ r) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x, a = blockIdx.y;
  if (v >= d.onx) return;
  const double f = zoom_freq(v, d.onx, d.sx, apix, cutoff_x);
  const float* const row = img + (size_t)a * d.nx;
  double re = 0, im = 0;
  for (int b = 0; b < d.nx; ++b) {
    double sn, cs;
    sincospi(-2.0 * f * (double)(b - d.nx / 2), &sn, &cs);
    re += (double)row[b] * cs;
    im += (double)row[b] * sn;
  }
  r[(size_t)a * d.onx + v] = make_double2(re, im);
}

__global__ __launch_bounds__(128) void k_zoom_cols(const double2* __restrict__ r, ZoomDims d, double apix, double cutoff_y, int log_flag,
                                                   float* __restrict__ pwr, float* __restrict__ phase, unsigned* __restrict__ minmax) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x, u = blockIdx.y;
  float q = 0.f;
  if (v < d.onx) {
    const double f = zoom_freq(u, d.ony, d.sy, apix, cutoff_y);
    double re = 0, im = 0;
    for (int a = 0; a < d.ny; ++a) {
      double sn, cs;
      sincospi(-2.0 * f * (double)(a - d.ny / 2), &sn, &cs);
      const double2 w = r[(size_t)a * d.onx + v];
      re += w.x * cs - w.y * sn;
      im += w.x * sn + w.y * cs;
    }
    if ((u + v) & 1) { re = -re; im = -im; }             // phase_shift[1::2, :] *= -1; phase_shift[:, 1::2] *= -1
    const int su = (u + d.ony / 2) % d.ony, sv = (v + d.onx / 2) % d.onx;   // np.fft.fftshift
    const double a2 = sqrt(re * re + im * im);
    q = (float)(log_flag ? log1p(a2) : a2);
    pwr[(size_t)su * d.onx + sv] = q;
    if (phase) phase[(size_t)su * d.onx + sv] = (float)atan2(im, re);
  }
  // min / max of the finite values this block produced (idle lanes repeat a real one: q of lane 0 of the wavefront)
  float lmin = v < d.onx ? q : INFINITY, lmax = v < d.onx ? q : 0.f;
  for (int off = 32; off > 0; off >>= 1) {
    lmin = fminf(lmin, __shfl_down(lmin, off, 64));
    lmax = fmaxf(lmax, __shfl_down(lmax, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&minmax[0], __float_as_uint(lmin));   // values are >= 0: unsigned order = float order
    atomicMax(&minmax[1], __float_as_uint(lmax));
  }
}

}  // namespace

extern "C" int hh_power_spectrum_zoom(int device, const float* image, int ny, int nx, int ony, int onx, double apix, double cutoff_y,
                                      double cutoff_x, int log_flag, float* pwr_out, float* phase_out) try {
  if (!image || !pwr_out || ny < 1 || nx < 1 || ony < 1 || onx < 1 || !(apix > 0) || !(cutoff_y > 0) || !(cutoff_x > 0))
    return fail(nullptr, HH_ERR_ARG, "hh_power_spectrum_zoom: bad argument");
  if ((int64_t)ny * nx > (1LL << 26) || (int64_t)ony * onx > (1LL << 26))
    return fail(nullptr, HH_ERR_ARG, "hh_power_spectrum_zoom: image or output larger than 2^26 pixels");
  if (int rc = use_device("hh_power_spectrum_zoom", device)) return rc;
  const ZoomDims d{ny, nx, ony, onx, 2 * apix / cutoff_y, 2 * apix / cutoff_x};
  const size_t n_in = (size_t)ny * nx, n_out = (size_t)ony * onx;
  DevArena mem;
  float* d_img = mem.get<float>(n_in);
  double2* d_r = mem.get<double2>((size_t)ny * onx);
  float* d_out = mem.get<float>(2 * n_out);
  unsigned* d_mm = mem.get<unsigned>(2);
  if (int rc = arena_ok(nullptr, mem)) return rc;
  const unsigned init[2] = {0x7f800000u, 0u};
  hipError_t e = hipMemcpy(d_img, image, n_in * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_mm, init, sizeof(init), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_zoom_rows, dim3((onx + 127) / 128, ny), dim3(128), 0, 0, d_img, d, apix, cutoff_x, d_r);
    hipLaunchKernelGGL(k_zoom_cols, dim3((onx + 127) / 128, ony), dim3(128), 0, 0, d_r, d, apix, cutoff_y, log_flag ? 1 : 0, d_out,
                       phase_out ? d_out + n_out : nullptr, d_mm);
    hipLaunchKernelGGL(k_normalise, dim3(256), dim3(256), 0, 0, d_out, n_out, d_mm);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(pwr_out, d_out, n_out * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess && phase_out) e = hipMemcpy(phase_out, d_out + n_out, n_out * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(nullptr, HH_ERR_HIP, std::string("hh_power_spectrum_zoom: ") + hipGetErrorString(e));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_power_spectrum_zoom")
