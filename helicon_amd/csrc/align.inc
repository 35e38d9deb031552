// align.inc — batched 2-D image alignment (helicon.align_images, lib/alignment.py:8-239): one evaluation of the reference's
// objective for many (moving plane, scale, angle) candidates on a context that keeps the prepared planes on the device.
//
// Per chunk of AL_CHUNK candidates, nothing returned to the host in between:
//   warp     k_align_warp: the batched k_warp_affine (order 1, mode "constant", cval 0, clip to the plane's own range), float32
//            coordinates, a stack W[chunk][ny][nx]
//   forward  x pass (real -> half spectrum, k_axis_gemm's contiguous view over all rows of the stack), then the y pass with
//            the FR_CROSS epilogue: P = Fref conj(F) / max(|P|, 100 FLT_EPSILON) (scikit-image's normalization = "phase" on
//            float32 images); only P is stored
//   inverse  y pass (complex), then k_align_c2r along x with irfft's semantics (k_tfsc_c2r's product) and the per-candidate
//            arg-max of |c| fused in: a 64-bit key (bits of |c|, ~flat index) combined with atomicMax — a maximum does not
//            depend on the order of its operands, the first flat index wins a tie as in np.argmax
//   score    k_align_score: the inverse matrix with its translation column moved by the device's own shift (float64, then
//            cast), the moving plane and its taper sampled at the same coordinates in "wrap" mode, the six moments of
//            (ref, warped)[taper_warped > 0] in float64 and in a fixed order (block_sums, then AL_GROUPS partials left to
//            right); neither warped plane is stored
//
// scikit-image is not installed beside the reference here: the "wrap" rule, like the constant-mode warp of image_prep.inc, is
// PINNED BY DERIVATION from _warp_fast / interpolation.pxd (coord_map applied to each of the four integer neighbours).
// Included into helicon_hip.hip after true_fsc.inc (tf_c2r_table) and image_prep.inc (k_prep_minmax).

constexpr int AL_CHUNK = 64;     // candidates of one launch group
constexpr int AL_GROUPS = 16;    // workgroups that share one candidate's score pass (fixed: the sums' order must not depend on the batch)
constexpr int AL_PHASES = 5;     // warp, forward, inverse, arg-max pass, score

struct hh_align {
  int device = 0, ny = 0, nx = 0, ncol = 0, n_moving = 0;
  int64_t plane = 0, spec = 0;      // ny nx and ny ncol
  DevBuf<float> ref;                // [ny][nx]
  DevBuf<float> ref_spec;           // [re | im][ny][ncol]
  DevBuf<float> moving, taper;      // [M][ny][nx] each
  DevBuf<double> range;             // [2 M][2]: (min, max) of the moving planes, then of the taper planes
  DevBuf<float> mats;               // the operator tables
  size_t o_xc = 0, o_xs = 0, o_yc = 0, o_yn = 0, o_yp = 0, o_ic = 0, o_ip = 0, o_in = 0, o_cw = 0, o_sw = 0;
  DevBuf<float> w;                  // [AL_CHUNK][ny][nx]
  DevBuf<float> s1, s2;             // [re | im][AL_CHUNK][ny][ncol] each
  DevBuf<double> part;              // [AL_CHUNK][AL_GROUPS][6]
  DevBuf<double> d_inv, d_score;    // per call: [n][6], [n]
  DevBuf<int> d_idx, d_shift, d_nmask;
  DevBuf<float> d_peak;
  DevBuf<unsigned long long> d_key;
  DevEvents<AL_PHASES + 1> ev;
  bool profile = false;
  double phase_ms[AL_PHASES] = {0, 0, 0, 0, 0};
  ~hh_align() { (void)hipSetDevice(device); }
};

namespace {

// skimage's coord_map for mode "wrap" (interpolation.pxd)
__device__ __forceinline__ long al_wrap(long i, long dim) {
  if (i < 0) return (dim - 1) - ((-i - 1) % dim);
  if (i > dim - 1) return i % dim;
  return i;
}

__device__ __forceinline__ float al_clip(float v, double lo, double hi, bool preserve_zero) {
  if (lo != lo || hi != hi) return v;
  if (preserve_zero && v == 0.f) return v;
  return v < (float)lo ? (float)lo : (v > (float)hi ? (float)hi : v);
}

// bilinear_interpolation (interpolation.pxd) of a float32 image: corners at floor and CEIL, the horizontal mixes in float32,
// the vertical mix in float64.  WRAP: every corner through coord_map; else a corner outside the image is 0.
template <bool WRAP>
__device__ __forceinline__ float al_bilinear(const float* __restrict__ in, int rows, int cols, float r, float c) {
#pragma clang fp contract(off)
  const long minr = (long)floor((double)r), minc = (long)floor((double)c);
  const long maxr = (long)ceil((double)r), maxc = (long)ceil((double)c);
  const float dr = r - (float)minr, dc = c - (float)minc;
  auto pixel = [&](long rr, long cc) -> float {
    if (WRAP) return in[(size_t)al_wrap(rr, rows) * cols + al_wrap(cc, cols)];
    return (rr < 0 || rr >= rows || cc < 0 || cc >= cols) ? 0.f : in[(size_t)rr * cols + cc];
  };
  const float tl = pixel(minr, minc), tr = pixel(minr, maxc), bl = pixel(maxr, minc), br = pixel(maxr, maxc);
  const double top = (double)((1.f - dc) * tl + dc * tr);
  const double bottom = (double)((1.f - dc) * bl + dc * br);
  return (float)((double)(1.f - dr) * top + (double)dr * bottom);
}

// (c, r) = H (x, y, 1) in the image's type, as k_warp_affine forms it
__device__ __forceinline__ void al_coords(const float (&h)[6], int x, int y, float& c, float& r) {
#pragma clang fp contract(off)
  const float fx = (float)x, fy = (float)y;
  c = h[0] * fx + h[1] * fy + h[2];
  r = h[3] * fx + h[4] * fy + h[5];
}

// xform.inverse with a post-translation of (sy, sx) added to the transform: the translation column in float64, then the cast
__device__ __forceinline__ void al_shifted(const double* __restrict__ inv, int sy, int sx, float (&h)[6]) {
#pragma clang fp contract(off)
  const double h2 = inv[2] - (inv[0] * (double)sx + inv[1] * (double)sy);
  const double h5 = inv[5] - (inv[3] * (double)sx + inv[4] * (double)sy);
  h[0] = (float)inv[0]; h[1] = (float)inv[1]; h[2] = (float)h2;
  h[3] = (float)inv[3]; h[4] = (float)inv[4]; h[5] = (float)h5;
}

// the shift of phase_cross_correlation: the arg-max's index, minus the side where it is strictly above fix(side / 2)
__device__ __forceinline__ void al_key_shift(unsigned long long key, int ny, int nx, int& sy, int& sx) {
  const unsigned flat = ~(unsigned)(key & 0xffffffffull);
  const int y = (int)(flat / (unsigned)nx), x = (int)(flat % (unsigned)nx);
  sy = y > ny / 2 ? y - ny : y;
  sx = x > nx / 2 ? x - nx : x;
}

// W[b] = warp(moving[idx[b]], inv[b]), mode "constant", clipped to the plane's range (k_prep_clip's rule with cval = 0)
__global__ __launch_bounds__(256) void k_align_warp(const float* __restrict__ moving, const double* __restrict__ range,
                                                    const double* __restrict__ inv, const int* __restrict__ idx, int ny, int nx,
                                                    float* __restrict__ w) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= nx) return;
  const int m = idx[b];
  const int64_t plane = (int64_t)ny * nx;
  float h[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) h[i] = (float)inv[(int64_t)b * 6 + i];   // matrix.astype(image.dtype)
  float c, r;
  al_coords(h, x, y, c, r);
  const double lo = range[2 * m], hi = range[2 * m + 1];
  const float v = al_bilinear<false>(moving + m * plane, ny, nx, r, c);
  w[b * plane + (int64_t)y * nx + x] = al_clip(v, lo, hi, !(lo <= 0.0 && 0.0 <= hi));
}

// one plane's second warp (mode "wrap"), stored: the accessor of the aligned image and of the tests
__global__ __launch_bounds__(256) void k_align_warp_wrap(const float* __restrict__ in, const double* __restrict__ range,
                                                         const double* __restrict__ inv, int sy, int sx, int ny, int nx,
                                                         float* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= nx) return;
  float h[6];
  al_shifted(inv, sy, sx, h);
  float c, r;
  al_coords(h, x, y, c, r);
  out[(int64_t)y * nx + x] = al_clip(al_bilinear<true>(in, ny, nx, r, c), range[0], range[1], false);
}

struct AlC2R {
  const float* re;            // [rows][ncol] planes after the inverse y pass, rows = candidates x ny
  const float* im;
  const float* cw;            // [ncol][nx]  w_k cos(2 pi k x / nx) / nx
  const float* sw;            // [ncol][nx] -w_k sin(2 pi k x / nx) / nx
  float* y;                   // [rows][nx] the surface c, or null: not stored
  unsigned long long* key;    // [candidates], zeroed: max over the candidate's pixels of (bits of |c|, ~flat index)
  int rows, nx, ncol, ny;
};

// k_tfsc_c2r's product; the epilogue folds every |c| of the tile into its candidate's key.
__global__ __launch_bounds__(256) void k_align_c2r(AlC2R g) {
  __shared__ float as[2][FC_T][FC_K + 1];   // re, im
  __shared__ float os[2][FC_K][FC_T + 1];   // cw, sw
  const Tile64 t = tile64();
  const int r = t.r, h = t.h, wm = t.wm, wp = t.wp;
  const int row0 = blockIdx.x * FC_T, col0 = blockIdx.y * FC_T;
  const float* const src[2] = {g.re, g.im};
  const float* const op[2] = {g.cw, g.sw};
  const bool active = col0 + wp < g.nx && row0 + wm < g.rows;
  f32x16 acc = {0};
  for (int k0 = 0; k0 < g.ncol; k0 += FC_K) {
#pragma unroll
    for (int q = 0; q < 2; ++q) stage_rows(as[q], src[q], g.ncol, row0, g.rows, k0, g.ncol, t.tid);
    stage_cols(os, op, g.nx, k0, g.ncol, col0, g.nx, t.tid);
    __syncthreads();
    if (active) {
#pragma unroll
      for (int kk = 0; kk < FC_K; kk += 2) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[0][wm + r][kk + h], os[0][kk + h][wp + r], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[1][wm + r][kk + h], os[1][kk + h][wp + r], acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!active) return;   // (per wavefront: wm and wp are)
  const int col = col0 + wp + r;
  const int first = row0 + wm, last = min(first + 31, g.rows - 1);
  const bool one = first / g.ny == last / g.ny;   // the wavefront's rows lie in one candidate
  unsigned long long best = 0ull;
  int cur = -1;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = first + acc_row(i, h);
    if (row >= g.rows || col >= g.nx) continue;
    if (g.y) g.y[(int64_t)row * g.nx + col] = acc[i];
    const int cand = row / g.ny;
    const unsigned flat = (unsigned)(row - cand * g.ny) * (unsigned)g.nx + (unsigned)col;
    const unsigned long long key = ((unsigned long long)__float_as_uint(fabsf(acc[i])) << 32) | (unsigned long long)(~flat);
    if (cand != cur) {
      if (cur >= 0 && !one) atomicMax(&g.key[cur], best);
      cur = cand;
      best = key;
    } else if (key > best) {
      best = key;
    }
  }
  if (one) {
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned lo = __shfl_down((unsigned)best, o, 64), hi = __shfl_down((unsigned)(best >> 32), o, 64);
      const unsigned long long other = ((unsigned long long)hi << 32) | lo;
      if (other > best) best = other;
    }
    if (t.lane == 0 && best) atomicMax(&g.key[first / g.ny], best);
  } else if (cur >= 0) {
    atomicMax(&g.key[cur], best);
  }
}

struct AlScore {
  const float* ref;             // [ny][nx]
  const float* moving;          // [M][ny][nx]
  const float* taper;
  const double* range;          // [2 M][2]
  const double* inv;            // [chunk][6]
  const int* idx;               // [chunk]
  const unsigned long long* key;
  double* part;                 // [chunk][AL_GROUPS][6]
  int ny, nx, n_moving;
};

// Workgroup (g, b): every AL_GROUPS-th stripe of 256 pixels of candidate b; n, sum a, sum b, sum aa, sum bb, sum ab over the
// pixels whose warped taper is > 0 (a: the reference, b: the warped moving plane).
__global__ __launch_bounds__(256) void k_align_score(AlScore s) {
  __shared__ double red[4][6];
  const int b = blockIdx.y, m = s.idx[b], tid = threadIdx.x;
  const int64_t plane = (int64_t)s.ny * s.nx;
  int sy, sx;
  al_key_shift(s.key[b], s.ny, s.nx, sy, sx);
  float h[6];
  al_shifted(s.inv + (int64_t)b * 6, sy, sx, h);
  const float* const mov = s.moving + m * plane;
  const float* const tap = s.taper + m * plane;
  const double mlo = s.range[2 * m], mhi = s.range[2 * m + 1];
  const double tlo = s.range[2 * (s.n_moving + m)], thi = s.range[2 * (s.n_moving + m) + 1];
  double sum[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t e = (int64_t)blockIdx.x * 256 + tid; e < plane; e += (int64_t)AL_GROUPS * 256) {
    const int y = (int)(e / s.nx), x = (int)(e % s.nx);
    float c, r;
    al_coords(h, x, y, c, r);
    const float tw = al_clip(al_bilinear<true>(tap, s.ny, s.nx, r, c), tlo, thi, false);
    if (tw > 0.f) {
      const double vb = (double)al_clip(al_bilinear<true>(mov, s.ny, s.nx, r, c), mlo, mhi, false);
      const double va = (double)s.ref[e];
      sum[0] += 1.0; sum[1] += va; sum[2] += vb; sum[3] += va * va; sum[4] += vb * vb; sum[5] += va * vb;
    }
  }
  block_sums<6, 4>(sum, red, tid, s.part + ((int64_t)b * AL_GROUPS + blockIdx.x) * 6);
}

// cross_correlation_coefficient (lib/analysis.py:793-799) from the moments: 0 when the norm is 0, NaN on an empty mask
__global__ __launch_bounds__(64) void k_align_finish(const double* __restrict__ part, const unsigned long long* __restrict__ key, int n, int ny, int nx,
                                                     int* __restrict__ shift, double* __restrict__ score, float* __restrict__ peak,
                                                     int* __restrict__ nmask) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n) return;
  double t[6];
  for (int e = 0; e < 6; ++e) {
    double v = part[((int64_t)b * AL_GROUPS) * 6 + e];
    for (int g = 1; g < AL_GROUPS; ++g) v += part[((int64_t)b * AL_GROUPS + g) * 6 + e];
    t[e] = v;
  }
  int sy, sx;
  al_key_shift(key[b], ny, nx, sy, sx);
  shift[2 * b] = sy;
  shift[2 * b + 1] = sx;
  peak[b] = __uint_as_float((unsigned)(key[b] >> 32));
  nmask[b] = (int)t[0];
  double sc;
  if (t[0] == 0.0) {
    sc = NAN;
  } else {
    const double va = fmax(t[3] - t[1] * t[1] / t[0], 0.0), vb = fmax(t[4] - t[2] * t[2] / t[0], 0.0);
    const double norm = sqrt(va * vb);
    sc = norm == 0.0 ? 0.0 : (t[5] - t[1] * t[2] / t[0]) / norm;
  }
  score[b] = sc;
}

// the forward transform of `count` planes [count][ny][nx] -> x pass into s1, y pass into (yr, yi); epi FR_CROSS divides the
// product with the resident reference spectrum
void al_forward(hh_align* c, const float* w, int64_t count, float* yr, float* yi, int epi) {
  const int ny = c->ny, nx = c->nx, ncol = c->ncol;
  float* const xr = c->s1;
  float* const xi = c->s1 + AL_CHUNK * c->spec;
  const float* const m = c->mats;
  {
    const float* const op[3] = {m + c->o_xc, m + c->o_xs, nullptr};
    const float* const x[2] = {w, nullptr};
    float* const y[2] = {xr, xi};
    launch_axis_pass(axis_geom(AxisView{1, nx, ncol, count * ny, true}), op, x, y, FR_STORE, 1.f, nullptr);
  }
  const float* const op[3] = {m + c->o_yc, m + c->o_yn, m + c->o_yp};
  const float* const x[2] = {xr, xi};
  float* const y[2] = {yr, yi};
  const float* const ref[2] = {c->ref_spec, c->ref_spec + c->spec};
  launch_axis_pass(axis_geom(AxisView{count, ny, ny, ncol, false}), op, x, y, epi, epi == FR_CROSS ? 100.f * __FLT_EPSILON__ : 1.f, nullptr,
                   epi == FR_CROSS ? ref : nullptr);
}

// stages 1-3 of `count` <= AL_CHUNK candidates whose matrices / plane indices / keys start at the given device pointers;
// surface: where to store c ([count][ny][nx]) or null
int al_correlate(hh_align* c, int64_t count, const double* d_inv, const int* d_idx, unsigned long long* d_key, float* surface) {
  const int ny = c->ny, nx = c->nx, ncol = c->ncol;
  auto mark = [&](int i) { return c->profile ? hipEventRecord(c->ev[i], nullptr) : hipSuccess; };
  HH_HIP(nullptr, mark(0));
  hipLaunchKernelGGL(k_align_warp, dim3((nx + 255) / 256, ny, (unsigned)count), dim3(256), 0, nullptr, c->moving.get(), c->range.get(), d_inv, d_idx, ny,
                     nx, c->w.get());
  HH_HIP(nullptr, mark(1));
  float* const pr = c->s2;
  float* const pi = c->s2 + AL_CHUNK * c->spec;
  al_forward(c, c->w, count, pr, pi, FR_CROSS);
  HH_HIP(nullptr, mark(2));
  float* const zr = c->s1;
  float* const zi = c->s1 + AL_CHUNK * c->spec;
  {
    const float* const m = c->mats;
    const float* const op[3] = {m + c->o_ic, m + c->o_ip, m + c->o_in};
    const float* const x[2] = {pr, pi};
    float* const y[2] = {zr, zi};
    launch_axis_pass(axis_geom(AxisView{count, ny, ny, ncol, false}), op, x, y, FR_STORE, 1.f, nullptr);
  }
  HH_HIP(nullptr, mark(3));
  AlC2R r{};
  r.re = zr; r.im = zi;
  r.cw = c->mats + c->o_cw; r.sw = c->mats + c->o_sw;
  r.y = surface;
  r.key = d_key;
  r.rows = (int)(count * ny); r.nx = nx; r.ncol = ncol; r.ny = ny;
  hipLaunchKernelGGL(k_align_c2r, dim3((unsigned)((r.rows + FC_T - 1) / FC_T), (unsigned)((nx + FC_T - 1) / FC_T)), dim3(256), 0, nullptr, r);
  HH_HIP(nullptr, mark(4));
  HH_HIP(nullptr, hipGetLastError());
  return HH_OK;
}

int al_add_phase_times(hh_align* c) {
  if (!c->profile) return HH_OK;
  HH_HIP(nullptr, hipEventSynchronize(c->ev[AL_PHASES]));
  for (int i = 0; i < AL_PHASES; ++i) {
    float ms = 0.f;
    HH_HIP(nullptr, hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
    c->phase_ms[i] += ms;
  }
  return HH_OK;
}

int al_reserve(hh_align* c, size_t n) {
  if (int rc = ensure(nullptr, c->w, (size_t)AL_CHUNK * c->plane)) return rc;
  if (int rc = ensure(nullptr, c->s1, (size_t)2 * AL_CHUNK * c->spec)) return rc;
  if (int rc = ensure(nullptr, c->s2, (size_t)2 * AL_CHUNK * c->spec)) return rc;
  if (int rc = ensure(nullptr, c->part, (size_t)AL_CHUNK * AL_GROUPS * 6)) return rc;
  if (int rc = ensure(nullptr, c->d_inv, n * 6)) return rc;
  if (int rc = ensure(nullptr, c->d_idx, n)) return rc;
  if (int rc = ensure(nullptr, c->d_key, n)) return rc;
  if (int rc = ensure(nullptr, c->d_score, n)) return rc;
  if (int rc = ensure(nullptr, c->d_shift, 2 * n)) return rc;
  if (int rc = ensure(nullptr, c->d_nmask, n)) return rc;
  if (int rc = ensure(nullptr, c->d_peak, n)) return rc;
  return HH_OK;
}

int al_create(hh_align* c, const float* ref, const float* moving, const float* taper) {
  const int ny = c->ny, nx = c->nx, ncol = c->ncol, M = c->n_moving;
  const size_t plane = (size_t)c->plane;
  std::vector<float> mats;
  {
    std::vector<double> cs, sn;
    unit_circle(nx, cs, sn);
    c->o_xc = append_axis_operator(mats, nx, AxisIndex::Dft, cs, 1.0, nullptr, 0.0);    // its first ncol rows are the operator
    c->o_xs = append_axis_operator(mats, nx, AxisIndex::Dft, sn, -1.0, nullptr, 0.0);
    c->o_cw = tf_c2r_table(mats, nx, ncol, cs, 1.0 / nx, false);
    c->o_sw = tf_c2r_table(mats, nx, ncol, sn, -1.0 / nx, true);
    unit_circle(ny, cs, sn);
    const double q = 1.0 / ny;
    c->o_yc = append_axis_operator(mats, ny, AxisIndex::Dft, cs, 1.0, nullptr, 0.0);
    c->o_yn = append_axis_operator(mats, ny, AxisIndex::Dft, sn, -1.0, nullptr, 0.0);
    c->o_yp = append_axis_operator(mats, ny, AxisIndex::Dft, sn, 1.0, nullptr, 0.0);
    c->o_ic = append_axis_operator(mats, ny, AxisIndex::Dft, cs, q, nullptr, 0.0);
    c->o_ip = append_axis_operator(mats, ny, AxisIndex::Dft, sn, q, nullptr, 0.0);
    c->o_in = append_axis_operator(mats, ny, AxisIndex::Dft, sn, -q, nullptr, 0.0);
  }
  if (int rc = ensure(nullptr, c->mats, mats.size())) return rc;
  if (int rc = ensure(nullptr, c->ref, plane)) return rc;
  if (int rc = ensure(nullptr, c->ref_spec, (size_t)2 * c->spec)) return rc;
  if (int rc = ensure(nullptr, c->moving, (size_t)M * plane)) return rc;
  if (int rc = ensure(nullptr, c->taper, (size_t)M * plane)) return rc;
  if (int rc = ensure(nullptr, c->range, (size_t)4 * M)) return rc;
  if (int rc = al_reserve(c, 1)) return rc;
  HH_HIP(nullptr, c->ev.create());
  HH_HIP(nullptr, hipMemcpy(c->mats, mats.data(), mats.size() * sizeof(float), hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipMemcpy(c->ref, ref, plane * sizeof(float), hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipMemcpy(c->moving, moving, (size_t)M * plane * sizeof(float), hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipMemcpy(c->taper, taper, (size_t)M * plane * sizeof(float), hipMemcpyHostToDevice));
  for (int m = 0; m < M; ++m) {
    hipLaunchKernelGGL(k_prep_minmax<float>, dim3(1), dim3(1024), 0, nullptr, c->moving + m * plane, (int64_t)plane, c->range + 2 * m);
    hipLaunchKernelGGL(k_prep_minmax<float>, dim3(1), dim3(1024), 0, nullptr, c->taper + m * plane, (int64_t)plane, c->range + 2 * (M + m));
  }
  al_forward(c, c->ref, 1, c->ref_spec, c->ref_spec + c->spec, FR_STORE);
  HH_HIP(nullptr, hipGetLastError());
  HH_HIP(nullptr, hipDeviceSynchronize());
  return HH_OK;
}

}  // namespace

extern "C" int hh_align_chunk(void) { return AL_CHUNK; }

extern "C" int hh_align_create(int device, int32_t ny, int32_t nx, const float* ref_work, int32_t n_moving, const float* moving_work,
                               const float* taper, hh_align** out) try {
  if (!out) return fail(nullptr, HH_ERR_ARG, "hh_align_create: NULL argument");
  *out = nullptr;
  if (!ref_work || !moving_work || !taper) return fail(nullptr, HH_ERR_ARG, "hh_align_create: NULL argument");
  if (ny < 2 || ny > 1024 || nx < 2 || nx > 1024) return fail(nullptr, HH_ERR_ARG, "hh_align_create: the sides must lie in [2, 1024]");
  if (n_moving < 1 || n_moving > 65536) return fail(nullptr, HH_ERR_ARG, "hh_align_create: n_moving must lie in [1, 65536]");
  if (int rc = use_device("hh_align_create", device)) return rc;
  std::unique_ptr<hh_align> c(new hh_align);
  c->device = device; c->ny = ny; c->nx = nx; c->ncol = nx / 2 + 1; c->n_moving = n_moving;
  c->plane = (int64_t)ny * nx; c->spec = (int64_t)ny * c->ncol;
  if (int rc = al_create(c.get(), ref_work, moving_work, taper)) return rc;
  *out = c.release();
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_align_create")

extern "C" int hh_align_destroy(hh_align* ctx) try {
  delete ctx;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_align_destroy")

extern "C" int hh_align_eval(hh_align* ctx, int64_t n, const int32_t* moving_index, const double* inv_matrix, int32_t* shift_out,
                             double* score_out, float* peak_out, int32_t* nmask_out) try {
  if (!ctx || !moving_index || !inv_matrix || !shift_out || !score_out) return fail(nullptr, HH_ERR_ARG, "hh_align_eval: NULL argument");
  if (n < 1) return fail(nullptr, HH_ERR_ARG, "hh_align_eval: n must be >= 1");
  hh_align* const c = ctx;
  for (int64_t i = 0; i < n; ++i)
    if (moving_index[i] < 0 || moving_index[i] >= c->n_moving) return fail(nullptr, HH_ERR_ARG, "hh_align_eval: a moving index outside the context's planes");
  for (int64_t i = 0; i < 6 * n; ++i)
    if (!std::isfinite(inv_matrix[i])) return fail(nullptr, HH_ERR_ARG, "hh_align_eval: a matrix entry that is NaN or infinite");
  HH_HIP(nullptr, hipSetDevice(c->device));
  if (int rc = al_reserve(c, (size_t)n)) return rc;
  HH_HIP(nullptr, hipMemcpy(c->d_inv, inv_matrix, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipMemcpy(c->d_idx, moving_index, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipMemsetAsync(c->d_key, 0, (size_t)n * sizeof(unsigned long long), nullptr));
  for (int64_t b0 = 0; b0 < n; b0 += AL_CHUNK) {
    const int64_t nb = std::min<int64_t>(AL_CHUNK, n - b0);
    if (int rc = al_correlate(c, nb, c->d_inv + b0 * 6, c->d_idx + b0, c->d_key + b0, nullptr)) return rc;
    AlScore s{};
    s.ref = c->ref; s.moving = c->moving; s.taper = c->taper; s.range = c->range;
    s.inv = c->d_inv + b0 * 6; s.idx = c->d_idx + b0; s.key = c->d_key + b0;
    s.part = c->part;
    s.ny = c->ny; s.nx = c->nx; s.n_moving = c->n_moving;
    hipLaunchKernelGGL(k_align_score, dim3(AL_GROUPS, (unsigned)nb), dim3(256), 0, nullptr, s);
    hipLaunchKernelGGL(k_align_finish, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, nullptr, c->part.get(), c->d_key + b0, (int)nb, c->ny, c->nx,
                       c->d_shift + 2 * b0, c->d_score + b0, c->d_peak + b0, c->d_nmask + b0);
    HH_HIP(nullptr, hipGetLastError());
    if (c->profile) {
      HH_HIP(nullptr, hipEventRecord(c->ev[AL_PHASES], nullptr));
      if (int rc = al_add_phase_times(c)) return rc;
    }
  }
  HH_HIP(nullptr, hipMemcpy(shift_out, c->d_shift, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost));
  HH_HIP(nullptr, hipMemcpy(score_out, c->d_score, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (peak_out) HH_HIP(nullptr, hipMemcpy(peak_out, c->d_peak, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  if (nmask_out) HH_HIP(nullptr, hipMemcpy(nmask_out, c->d_nmask, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_align_eval")

extern "C" int hh_align_correlation(hh_align* ctx, int32_t moving_index, const double* inv_matrix, float* out) try {
  if (!ctx || !inv_matrix || !out) return fail(nullptr, HH_ERR_ARG, "hh_align_correlation: NULL argument");
  hh_align* const c = ctx;
  if (moving_index < 0 || moving_index >= c->n_moving) return fail(nullptr, HH_ERR_ARG, "hh_align_correlation: a moving index outside the context's planes");
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(inv_matrix[i])) return fail(nullptr, HH_ERR_ARG, "hh_align_correlation: a matrix entry that is NaN or infinite");
  HH_HIP(nullptr, hipSetDevice(c->device));
  if (int rc = al_reserve(c, 1)) return rc;
  const int idx = moving_index;
  HH_HIP(nullptr, hipMemcpy(c->d_inv, inv_matrix, 6 * sizeof(double), hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipMemcpy(c->d_idx, &idx, sizeof(int), hipMemcpyHostToDevice));
  HH_HIP(nullptr, hipMemsetAsync(c->d_key, 0, sizeof(unsigned long long), nullptr));
  const bool prof = c->profile;
  c->profile = false;
  const int rc = al_correlate(c, 1, c->d_inv, c->d_idx, c->d_key, c->w);   // the stack is free once the x pass has read it
  c->profile = prof;
  if (rc) return rc;
  HH_HIP(nullptr, hipMemcpy(out, c->w, (size_t)c->plane * sizeof(float), hipMemcpyDeviceToHost));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_align_correlation")

extern "C" int hh_align_warp_wrap(hh_align* ctx, const float* plane, int32_t moving_index, int which, const double* inv_matrix,
                                  const int32_t* shift, float* out) try {
  if (!ctx || !inv_matrix || !shift || !out) return fail(nullptr, HH_ERR_ARG, "hh_align_warp_wrap: NULL argument");
  hh_align* const c = ctx;
  if (!plane && (moving_index < 0 || moving_index >= c->n_moving || which < 0 || which > 1))
    return fail(nullptr, HH_ERR_ARG, "hh_align_warp_wrap: a moving index outside the context's planes, or which not 0 (image) / 1 (taper)");
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(inv_matrix[i])) return fail(nullptr, HH_ERR_ARG, "hh_align_warp_wrap: a matrix entry that is NaN or infinite");
  HH_HIP(nullptr, hipSetDevice(c->device));
  const size_t n = (size_t)c->plane;
  DevArena mem;
  float* d_in = mem.get<float>(plane ? n : 1);
  float* d_out = mem.get<float>(n);
  double* d_range = mem.get<double>(2);
  double* d_inv = mem.get<double>(6);
  if (int rc = arena_ok(nullptr, mem)) return rc;
  const float* src;
  const double* range;
  if (plane) {
    HH_HIP(nullptr, hipMemcpy(d_in, plane, n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_prep_minmax<float>, dim3(1), dim3(1024), 0, nullptr, d_in, (int64_t)n, d_range);
    src = d_in;
    range = d_range;
  } else {
    src = (which ? c->taper : c->moving) + (size_t)moving_index * n;
    range = c->range + 2 * ((which ? c->n_moving : 0) + moving_index);
  }
  HH_HIP(nullptr, hipMemcpy(d_inv, inv_matrix, 6 * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_align_warp_wrap, dim3((c->nx + 255) / 256, c->ny), dim3(256), 0, nullptr, src, range, d_inv, (int)shift[0], (int)shift[1], c->ny,
                     c->nx, d_out);
  HH_HIP(nullptr, hipGetLastError());
  HH_HIP(nullptr, hipMemcpy(out, d_out, n * sizeof(float), hipMemcpyDeviceToHost));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_align_warp_wrap")

extern "C" int hh_align_profile(hh_align* ctx, int enable, double* phase_ms) try {
  if (!ctx) return fail(nullptr, HH_ERR_ARG, "hh_align_profile: NULL argument");
  if (phase_ms)
    for (int i = 0; i < AL_PHASES; ++i) phase_ms[i] = ctx->phase_ms[i];
  if (enable >= 0) {
    ctx->profile = enable != 0;
    for (double& v : ctx->phase_ms) v = 0.0;
  }
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_align_profile")
