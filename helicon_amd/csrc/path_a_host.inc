// path_a_host.inc — host side + C ABI of the Path-A slice (kernels and struct hh_pa: path_a.inc).

namespace {

int pa_fail(hh_pa* p, int code, const std::string& msg) {
  if (p) p->err = msg; else g_create_error = msg;
  return code;
}
#define PA_HIP(p, call)                                                                         \
  do {                                                                                          \
    hipError_t e__ = (call);                                                                    \
    if (e__ != hipSuccess) return pa_fail(p, HH_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

// scipy.spatial.transform.Rotation.from_euler(<lower-case axes>, angles, degrees=True).as_matrix(): elementary
// quaternions composed in order (extrinsic), matrix entries from the un-normalised quaternion
void pa_quat_axis(char axis, double deg, double q[4]) {
  const double a = deg * (M_PI / 180.0);
  q[0] = q[1] = q[2] = 0.0;
  q[axis - 'x'] = std::sin(a / 2);
  q[3] = std::cos(a / 2);
}
void pa_quat_mul(const double p[4], const double q[4], double out[4]) {  // p * q
  const double cx = p[1] * q[2] - p[2] * q[1], cy = p[2] * q[0] - p[0] * q[2], cz = p[0] * q[1] - p[1] * q[0];
  out[0] = p[3] * q[0] + q[3] * p[0] + cx;
  out[1] = p[3] * q[1] + q[3] * p[1] + cy;
  out[2] = p[3] * q[2] + q[3] * p[2] + cz;
  out[3] = p[3] * q[3] - (p[0] * q[0] + p[1] * q[1] + p[2] * q[2]);
}
void pa_quat_matrix(const double q[4], double m[9]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
  const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
  m[0] = x2 - y2 - z2 + w2; m[1] = 2 * (xy - zw);      m[2] = 2 * (xz + yw);
  m[3] = 2 * (xy + zw);     m[4] = -x2 + y2 - z2 + w2; m[5] = 2 * (yz - xw);
  m[6] = 2 * (xz - yw);     m[7] = 2 * (yz + xw);      m[8] = -x2 - y2 + z2 + w2;
}
void pa_euler1(char axis, double deg, double m[9]) {
  double q[4];
  pa_quat_axis(axis, deg, q);
  pa_quat_matrix(q, m);
}

// floor(vdC_2(i) * n): qmc.Halton(d=1, scramble=False).integers(0, n, n)
std::vector<int64_t> pa_halton(int64_t n) {
  std::vector<int64_t> out((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    double f = 0.5, r = 0.0;
    for (int64_t k = i; k; k >>= 1, f *= 0.5)
      if (k & 1) r += f;
    out[(size_t)i] = (int64_t)std::floor(r * (double)n);
  }
  return out;
}

// get_cylindrical_mask(nz, ny, nx, rmin, rmax) as a rank table (-1 outside); returns the voxel count
int64_t pa_mask_rank(int nz, int ny, int nx, double rmin, double rmax, std::vector<int>& rank) {
  if (rmax < 0) rmax = ny / 2 - 1;
  rank.assign((size_t)nz * ny * nx, -1);
  int64_t n = 0;
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const long long X = i - nx / 2, Y = j - ny / 2, r2 = X * X + Y * Y;
        bool in = (double)r2 < rmax * rmax;
        if (0 < rmin && rmin < rmax) in = in && (double)r2 >= rmin * rmin;
        if (in) rank[((size_t)k * ny + j) * nx + i] = (int)n++;
      }
  return n;
}

// sorted_hsym_csym_pairs (solver:1749-1791) in the order build_A_helical_sym_matrix walks them (Halton re-indexing,
// solver:1785-1790): for every pair the two inverse-applied z rotations and the two axial shifts (rise * h)
struct PaSymOp {
  double ma[9], mb[9];
  double shift_a, shift_b;
};
std::vector<PaSymOp> pa_sym_ops(int nz, double twist, double rise, int csym, size_t max_ops = (size_t)-1) {
  const int hmax = std::max(1, (int)std::ceil((double)nz / (2 * rise)));
  struct Hc { int h, c; };
  std::vector<Hc> hcs;
  for (int h = -hmax; h <= hmax; ++h)
    for (int c = 0; c < csym; ++c) hcs.push_back({h, c});
  struct Row { double angle; int a, b, c, d; Hc p, q; };
  std::vector<Row> rows;
  for (size_t i = 0; i < hcs.size(); ++i)
    for (size_t j = i + 1; j < hcs.size(); ++j) {
      const double a1 = twist * hcs[i].h + hcs[i].c * 360.0 / csym, a2 = twist * hcs[j].h + hcs[j].c * 360.0 / csym;
      double md = std::fmod(a2 - a1 + 180.0, 360.0);   // Python's %: result takes the sign of the divisor
      if (md < 0) md += 360.0;
      const double ang = std::fabs(md - 180.0);
      const double angle = std::nearbyint(ang * 100.0) / 100.0;   // round(x, 2), see pa_sym_pairs
      rows.push_back({angle, std::abs(hcs[i].h + hcs[j].h), std::abs(hcs[i].h - hcs[j].h), std::abs(hcs[i].h), std::abs(hcs[j].h),
                      hcs[i], hcs[j]});
    }
  std::stable_sort(rows.begin(), rows.end(), [](const Row& x, const Row& y) {
    if (x.angle != y.angle) return x.angle < y.angle;
    if (x.a != y.a) return x.a < y.a;
    if (x.b != y.b) return x.b < y.b;
    if (x.c != y.c) return x.c < y.c;
    return x.d < y.d;
  });
  const std::vector<int64_t> order = pa_halton((int64_t)rows.size());
  std::vector<PaSymOp> out;
  out.reserve(std::min(order.size(), max_ops));
  for (int64_t oi : order) {
    if (out.size() >= max_ops) break;
    const Row& p = rows[(size_t)oi];
    PaSymOp op;
    pa_euler1('z', twist * p.p.h + p.p.c * 360.0 / csym, op.ma);
    pa_euler1('z', twist * p.q.h + p.q.c * 360.0 / csym, op.mb);
    op.shift_a = rise * p.p.h;
    op.shift_b = rise * p.q.h;
    out.push_back(op);
  }
  return out;
}

// build_A_helical_sym_matrix, nearest neighbour (solver_linear_regression.py:1142-1298): the (i, j) voxel pairs in
// the reference's order, with its order-dependent de-duplication
// With out16: the trilinear branch (solver:910-1140) instead — 16-entry rows, quirks included: a pair counts only when
// |dz|, |dy| and |dx| of the two truncated positions are all >= 3, de-duplication is by the ranks of the ROUNDED
// positions, and the weights of corners 110 and 111 are xf yf (1 - xf) and xf yf zf.
void pa_sym_pairs(int nz, int ny, int nx, double twist, double rise, int csym, double rmin, double rmax, int64_t min_pairs,
                  std::vector<int2>& out, std::vector<PaEll16>* out16 = nullptr) {
#pragma clang fp contract(off)
  out.clear();
  if (out16) out16->clear();
  std::vector<int> rank;
  const int64_t n_x = pa_mask_rank(nz, ny, nx, rmin, rmax, rank);
  // sorted_hsym_csym_pairs
  const int hmax = std::max(1, (int)std::ceil((double)nz / (2 * rise)));
  struct Hc { int h, c; };
  std::vector<Hc> hcs;
  for (int h = -hmax; h <= hmax; ++h)
    for (int c = 0; c < csym; ++c) hcs.push_back({h, c});
  struct Row { double angle; int a, b, c, d; Hc p, q; size_t order; };
  std::vector<Row> rows;
  for (size_t i = 0; i < hcs.size(); ++i)
    for (size_t j = i + 1; j < hcs.size(); ++j) {
      const double a1 = twist * hcs[i].h + hcs[i].c * 360.0 / csym, a2 = twist * hcs[j].h + hcs[j].c * 360.0 / csym;
      double md = std::fmod(a2 - a1 + 180.0, 360.0);   // Python's %: result takes the sign of the divisor
      if (md < 0) md += 360.0;
      const double ang = std::fabs(md - 180.0);
      // round(x, 2) as CPython does it for floats (correctly rounded decimal repr): nearbyint(x * 100) / 100 agrees
      // whenever x * 100 is not within an ulp of a tie; the key only orders pairs
      const double angle = std::nearbyint(ang * 100.0) / 100.0;
      rows.push_back({angle, std::abs(hcs[i].h + hcs[j].h), std::abs(hcs[i].h - hcs[j].h), std::abs(hcs[i].h), std::abs(hcs[j].h),
                      hcs[i], hcs[j], rows.size()});
    }
  std::stable_sort(rows.begin(), rows.end(), [](const Row& x, const Row& y) {
    if (x.angle != y.angle) return x.angle < y.angle;
    if (x.a != y.a) return x.a < y.a;
    if (x.b != y.b) return x.b < y.b;
    if (x.c != y.c) return x.c < y.c;
    return x.d < y.d;
  });
  const std::vector<int64_t> order = pa_halton((int64_t)rows.size());
  std::vector<long long> seen_keys;
  std::unordered_set<long long> seen;
  seen.insert(-1);
  auto position_of = [&](const double* m, const Hc& s, int k, int j, int i, double& Z, double& Y, double& X) {
    const double x = (double)(i - nx / 2), y = (double)(j - ny / 2), z = (double)(k - nz / 2);
    const double rx = x * m[0] + y * m[1] + z * m[2], ry = x * m[3] + y * m[4] + z * m[5], rz = x * m[6] + y * m[7] + z * m[8];
    X = rx + (double)(nx / 2);
    Y = ry + (double)(ny / 2);
    Z = rz + (double)(nz / 2) + rise * s.h;
  };
  auto image_of = [&](const double* m, const Hc& s, int k, int j, int i, long long& zi, long long& yi, long long& xi) {
    double Z, Y, X;
    position_of(m, s, k, j, i, Z, Y, X);
    xi = (long long)std::nearbyint(X);
    yi = (long long)std::nearbyint(Y);
    zi = (long long)std::nearbyint(Z);
  };
  // the 2 x 2 x 2 cell of one truncated position: false when it leaves the box or the cylinder
  auto cell_of = [&](double Z, double Y, double X, long long t[3], int idx[8], float w[8], float sgn) {
    t[0] = (long long)Z; t[1] = (long long)Y; t[2] = (long long)X;
    if (t[0] < 0 || t[0] + 1 > nz - 1 || t[1] < 0 || t[1] + 1 > ny - 1 || t[2] < 0 || t[2] + 1 > nx - 1) return false;
    for (int c = 0; c < 8; ++c) {
      idx[c] = rank[((size_t)(t[0] + (c >> 2)) * ny + (t[1] + ((c >> 1) & 1))) * nx + (t[2] + (c & 1))];
      if (idx[c] < 0) return false;
    }
    const double zf = Z - (double)t[0], yf = Y - (double)t[1], xf = X - (double)t[2];
    const double ww[8] = {(1 - zf) * (1 - yf) * (1 - xf), (1 - zf) * (1 - yf) * xf, (1 - zf) * yf * (1 - xf), (1 - zf) * yf * xf,
                          zf * (1 - yf) * (1 - xf),       zf * (1 - yf) * xf,       xf * yf * (1 - xf),       xf * yf * zf};
    for (int c = 0; c < 8; ++c) w[c] = sgn * (float)ww[c];  // the reference stores float32
    return true;
  };
  int64_t row_count = 0;
  for (int64_t oi : order) {
    const Row& p = rows[(size_t)oi];
    double ma[9], mb[9];
    pa_euler1('z', twist * p.p.h + p.p.c * 360.0 / csym, ma);
    pa_euler1('z', twist * p.q.h + p.q.c * 360.0 / csym, mb);
    int64_t added = 0;
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
          if (rank[((size_t)k * ny + j) * nx + i] < 0) continue;
          long long za, ya, xa, zb, yb, xb;
          if (out16) {
            double Za, Ya, Xa, Zb, Yb, Xb;
            position_of(ma, p.p, k, j, i, Za, Ya, Xa);
            position_of(mb, p.q, k, j, i, Zb, Yb, Xb);
            PaEll16 e;
            long long ta[3], tb[3];
            if (!cell_of(Za, Ya, Xa, ta, e.idx, e.w, 1.f) || !cell_of(Zb, Yb, Xb, tb, e.idx + 8, e.w + 8, -1.f)) continue;
            if (std::llabs(ta[0] - tb[0]) < 3 || std::llabs(ta[1] - tb[1]) < 3 || std::llabs(ta[2] - tb[2]) < 3) continue;
            // rank[round(Z), round(Y), round(X)] as NumPy indexes it: a coordinate in (-1, -0.5) truncates to cell 0
            // but rounds to -1, which wraps to the last index of its axis
            auto wrapped = [](double v, int dim) {
              const long long r = (long long)std::nearbyint(v);
              return (size_t)(r < 0 ? r + dim : r);
            };
            const int ir = rank[(wrapped(Za, nz) * ny + wrapped(Ya, ny)) * nx + wrapped(Xa, nx)];
            const int jr = rank[(wrapped(Zb, nz) * ny + wrapped(Yb, ny)) * nx + wrapped(Xb, nx)];
            const long long pid = (long long)ir * n_x + jr;
            if (seen.count(pid)) continue;
            seen.insert(pid);
            seen.insert((long long)jr * n_x + ir);
            out16->push_back(e);
            ++added;
            continue;
          }
          image_of(ma, p.p, k, j, i, za, ya, xa);
          image_of(mb, p.q, k, j, i, zb, yb, xb);
          if (za < 0 || za > nz - 1 || zb < 0 || zb > nz - 1 || ya < 0 || ya > ny - 1 || yb < 0 || yb > ny - 1 || xa < 0 ||
              xa > nx - 1 || xb < 0 || xb > nx - 1)
            continue;
          const int ia = rank[((size_t)za * ny + ya) * nx + xa], ib = rank[((size_t)zb * ny + yb) * nx + xb];
          if (ia < 0 || ib < 0) continue;
          const long long pid = (long long)ia * n_x + ib;
          if (seen.count(pid)) continue;
          seen.insert(pid);
          seen.insert((long long)ib * n_x + ia);
          out.push_back(make_int2(ia, ib));
          ++added;
        }
    row_count += added;
    if (row_count >= min_pairs) break;
  }
}

// Set-up transfers (index tables, flags, column sums) go through a pinned staging buffer OF THE OBJECT, in pieces: copying
// straight from / to std::vector storage makes the runtime pin those pages, and their release when the vector dies stalls
// a later GPU operation of the process (the same sporadic ~95 ms as with the caller's arrays, see hh_pa).  (Round 2 had
// one process-wide buffer behind a mutex held across the copy and its synchronisation: concurrent hh_pa_create calls of
// a thread pool serialised on it.)
constexpr size_t PA_STAGE_BYTES = (size_t)2 << 20;

hipError_t pa_copy(hh_pa* p, void* dst, const void* src, size_t bytes, bool to_device) {
  if (!p->h_stage) {
    const hipError_t e = hipHostMalloc(&p->h_stage, PA_STAGE_BYTES, hipHostMallocDefault);
    if (e != hipSuccess) { p->h_stage = nullptr; return e; }
  }
  for (size_t o = 0; o < bytes; o += PA_STAGE_BYTES) {
    const size_t nb = std::min(PA_STAGE_BYTES, bytes - o);
    hipError_t e;
    if (to_device) {
      std::memcpy(p->h_stage, static_cast<const char*>(src) + o, nb);
      e = hipMemcpyAsync(static_cast<char*>(dst) + o, p->h_stage, nb, hipMemcpyHostToDevice, p->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    } else {
      e = hipMemcpyAsync(p->h_stage, static_cast<const char*>(src) + o, nb, hipMemcpyDeviceToHost, p->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
      if (e == hipSuccess) std::memcpy(static_cast<char*>(dst) + o, p->h_stage, nb);
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// grow-only device buffer (device_mem.h); a failure is this object's HH_ERR_NOMEM
template <class T>
int pa_ensure(hh_pa* p, DevBuf<T>& b, size_t count) {
  return b.ensure(count) ? HH_OK : pa_fail(p, HH_ERR_NOMEM, dev_alloc_failed(b.bytes_for(count)));
}

int pa_alloc_vectors(hh_pa* p) {
  const int64_t big = p->m_data + p->m_sym + p->n;
  for (DevBuf<double>* v : {&p->d_x, &p->d_v, &p->d_h, &p->d_hbar, &p->d_scale, &p->d_root})
    if (int rc = pa_ensure(p, *v, (size_t)std::max<int64_t>(p->n, 1))) return rc;
  for (DevBuf<double>* v : {&p->d_y, &p->d_u, &p->d_w})
    if (int rc = pa_ensure(p, *v, (size_t)std::max<int64_t>(big, 1))) return rc;
  if (int rc = pa_ensure(p, p->d_red, 1024)) return rc;
  PA_HIP(p, hipHostMalloc(&p->h_a, (size_t)std::max<int64_t>(big, 1) * sizeof(double), hipHostMallocDefault));
  PA_HIP(p, hipHostMalloc(&p->h_b, (size_t)std::max<int64_t>(p->n, 1) * sizeof(double), hipHostMallocDefault));
  PA_HIP(p, hipHostMalloc(&p->h_c, (size_t)std::max<int64_t>(p->n, 1) * sizeof(double), hipHostMallocDefault));
  PA_HIP(p, hipHostMalloc(&p->h_out, (size_t)std::max<int64_t>(big, 1) * sizeof(double), hipHostMallocDefault));
  PA_HIP(p, hipHostMalloc(&p->h_red, 1024 * sizeof(double), hipHostMallocDefault));
  return HH_OK;
}

// host vector -> device through a pinned staging buffer (queued; the stage must not be reused before the next sync)
int pa_upload(hh_pa* p, double* dev, const double* host, int64_t count, double* stage) {
  std::memcpy(stage, host, (size_t)count * sizeof(double));
  PA_HIP(p, hipMemcpyAsync(dev, stage, (size_t)count * sizeof(double), hipMemcpyHostToDevice, p->stream));
  return HH_OK;
}
// device vector -> host through the pinned staging buffer (synchronises the stream)
int pa_download(hh_pa* p, double* host, const double* dev, int64_t count) {
  PA_HIP(p, hipMemcpyAsync(p->h_out, dev, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  PA_HIP(p, hipStreamSynchronize(p->stream));
  std::memcpy(host, p->h_out, (size_t)count * sizeof(double));
  return HH_OK;
}

inline dim3 pa_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// y = Op x with Op = [A diag(d); diag(root)] (d, root: device pointers or NULL); all device pointers
void pa_op(hh_pa* p, const double* x, const double* d, const double* root, double* y) {
  const int64_t rows = p->m_data * PA_G + p->m_sym + (root ? p->n : 0);   // threads: PA_G per data row, one per other row
  if (p->g.linear)
    hipLaunchKernelGGL(k_pa_matvec_lin, pa_grid(rows), dim3(256), 0, p->stream, p->g, p->d_ops, p->d_rank, p->d_ray_of_row,
                       p->m_data, p->d_sym16, p->m_sym, x, d, root, p->n, y);
  else
    hipLaunchKernelGGL(k_pa_matvec, pa_grid(rows), dim3(256), 0, p->stream, p->d_map, p->d_ray_of_row, p->g.D2, p->m_data,
                       p->d_pairs, p->m_sym, x, d, root, p->n, y);
}
// the scatter half of Op^T, into `acc` (zero-filled here) as fixed point with the given scale
template <bool ABS>
void pa_scatter(hh_pa* p, const double* y, double scale, double* acc) {
  (void)hipMemsetAsync(acc, 0, (size_t)p->n * sizeof(double), p->stream);
  if (p->m_data + p->m_sym <= 0) return;
  const int64_t rows = p->m_data * PA_G + p->m_sym;   // threads
  if (p->g.linear)
    hipLaunchKernelGGL(k_pa_rmatvec_lin<ABS>, pa_grid(rows), dim3(256), 0, p->stream, p->g, p->d_ops, p->d_rank, p->d_ray_of_row,
                       p->m_data, p->d_sym16, p->m_sym, y, scale, reinterpret_cast<long long*>(acc));
  else
    hipLaunchKernelGGL(k_pa_rmatvec<ABS>, pa_grid(rows), dim3(256), 0, p->stream, p->d_map, p->d_ray_of_row, p->g.D2, p->m_data,
                       p->d_pairs, p->m_sym, y, scale, reinterpret_cast<long long*>(acc));
}
// g = Op^T y; ymax >= max |y[:m_data + m_sym]| (1 for the unit vectors of LSMR)
void pa_op_t(hh_pa* p, const double* y, const double* d, const double* root, double* g, double ymax) {
  const double bound = p->colsum * ymax;
  const int e = bound > 0 ? 61 - (int)std::ceil(std::log2(bound)) : 0;
  pa_scatter<false>(p, y, std::ldexp(1.0, e), g);
  hipLaunchKernelGGL(k_pa_finish_rmatvec, pa_grid(p->n), dim3(256), 0, p->stream, g, std::ldexp(1.0, -e), d, root,
                     y + p->m_data + p->m_sym, p->n);
}
int pa_norm(hh_pa* p, const double* v, int64_t n, double* out) {
  const int blocks = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (n + 255) / 256));
  hipLaunchKernelGGL(k_pa_sumsq, dim3(blocks), dim3(256), 0, p->stream, v, n, p->d_red);
  double* const h = p->h_red;
  PA_HIP(p, hipMemcpyAsync(h, p->d_red, (size_t)blocks * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  PA_HIP(p, hipStreamSynchronize(p->stream));
  double s = 0;
  for (int i = 0; i < blocks; ++i) s += h[i];
  *out = std::sqrt(s);
  return HH_OK;
}

void pa_sym_ortho(double a, double b, double& c, double& s, double& r) {
  auto sign = [](double v) { return (double)((v > 0) - (v < 0)); };
  if (b == 0) { c = sign(a); s = 0; r = std::fabs(a); }
  else if (a == 0) { c = 0; s = sign(b); r = std::fabs(b); }
  else if (std::fabs(b) > std::fabs(a)) { const double tau = a / b; s = sign(b) / std::sqrt(1 + tau * tau); c = s * tau; r = b / s; }
  else { const double tau = b / a; c = sign(a) / std::sqrt(1 + tau * tau); s = c * tau; r = a / c; }
}

}  // namespace

extern "C" {

const char* hh_pa_last_error(const hh_pa* p) { return p ? p->err.c_str() : g_create_error.c_str(); }

void hh_pa_destroy(hh_pa* p) try {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  for (double* v : {p->h_a, p->h_b, p->h_c, p->h_out, p->h_red})
    if (v) (void)hipHostFree(v);
  if (p->h_stage) (void)hipHostFree(p->h_stage);
  const hipStream_t stream = p->stream;
  delete p;                                   // frees the device buffers: before their stream goes
  if (stream) (void)hipStreamDestroy(stream);
} catch (...) {
}

int hh_pa_create(hh_pa** out, int device, const float* image, int ny, int nx, const hh_pa_params* q) try {
  if (!out || !image || !q) return pa_fail(nullptr, HH_ERR_ARG, "hh_pa_create: NULL argument");
  *out = nullptr;
  int d2 = q->reconstruct_diameter_2d_pixel > 0 ? q->reconstruct_diameter_2d_pixel : ny;
  int l2 = q->reconstruct_length_2d_pixel > 0 ? q->reconstruct_length_2d_pixel : nx;
  if (d2 > ny || l2 > nx || d2 < 2 || l2 < 2) return pa_fail(nullptr, HH_ERR_ARG, "hh_pa_create: 2-D region does not fit the image");
  if (!(q->rise_pixel > 0) || q->csym < 1 || q->twist_degree == 0.0)
    return pa_fail(nullptr, HH_ERR_ARG, "hh_pa_create: rise must be positive, csym >= 1, twist non-zero");
  if (q->interpolation != 0 && q->interpolation != 1)
    return pa_fail(nullptr, HH_ERR_ARG, "hh_pa_create: interpolation must be 0 (nearest neighbour) or 1 (trilinear)");
  if (q->fsc_half < 0 || q->fsc_half > 2 || (q->fsc_half > 0 && (q->fsc_mode < 1 || (q->fsc_mode == 1 && (!q->fsc_ids || q->n_fsc_ids < 0)))))
    return pa_fail(nullptr, HH_ERR_ARG, "hh_pa_create: half sets need fsc_half 1 or 2 and fsc_mode 2, 3, 4, or 1 with the first half's "
                                        "pixel ids in fsc_ids (the caller's random split)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return pa_fail(nullptr, HH_ERR_HIP, "hh_pa_create: no such HIP device (Path A has no CPU fallback)");
  hh_pa* p = new (std::nothrow) hh_pa();
  if (!p) return pa_fail(nullptr, HH_ERR_NOMEM, "out of host memory");
  p->device = device;
  DevBuf<unsigned char> d_has;      // set-up scratch: released on every way out
  struct Guard { hh_pa* p; ~Guard() { if (p) hh_pa_destroy(p); } } guard{p};
  auto bail = [&](int rc) {
    g_create_error = p->err;
    guard.p = nullptr;
    hh_pa_destroy(p);
    return rc;
  };
#define PA_ENSURE(buf, count) do { if (int rc__ = pa_ensure(p, buf, count)) return bail(rc__); } while (0)
#define PA_TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { p->err = std::string(#call) + ": " + hipGetErrorString(e__); return bail(HH_ERR_HIP); } } while (0)
  PA_TRY(hipSetDevice(device));
  PA_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  const int l3 = q->reconstruct_length_3d_pixel > 0 ? q->reconstruct_length_3d_pixel : l2;
  PaGeom& g = p->g;
  g.linear = q->interpolation;
  g.L2 = l2; g.D2 = d2; g.mz = l3; g.my = d2; g.mx = d2;
  g.scale = q->scale2d_to_3d;
  g.dy = q->dy_pixel;
  pa_euler1('y', 90.0, g.m_y90);
  {
    double qy[4], qx[4], qq[4];
    pa_quat_axis('y', q->tilt_degree, qy);
    pa_quat_axis('x', q->psi_degree, qx);
    pa_quat_mul(qx, qy, qq);  // extrinsic "yx": the later rotation multiplies from the left
    pa_quat_matrix(qq, g.m_yx);
  }
  // the unknowns: voxels of the cylinder in the (L3d, D2d, D2d) box, C-order rank (solver:1375-1387)
  std::vector<int> rank;
  const double rmin = q->reconstruct_diameter_3d_inner_pixel / 2.0;
  const double rmax = (double)(q->reconstruct_diameter_3d_pixel / 2 - 1);
  p->n = pa_mask_rank(g.mz, g.my, g.mx, rmin, rmax, rank);
  if (p->n <= 0) { p->err = "hh_pa_create: the cylinder holds no voxel"; return bail(HH_ERR_ARG); }
  PA_ENSURE(p->d_rank, rank.size());
  PA_TRY(pa_copy(p, p->d_rank, rank.data(), rank.size() * sizeof(int), true));
  int* const d_rank = p->d_rank;
  // symmetry operations in the reference's order (solver:1556-1571)
  const int hmax = std::max(1, (int)(std::ceil((double)(l3 + l2)) / 2 / q->rise_pixel));
  struct Hc { int h, c; };
  std::vector<Hc> hcs;
  for (int h = -hmax; h <= hmax; ++h)
    for (int c = 0; c < q->csym; ++c) hcs.push_back({h, c});
  std::stable_sort(hcs.begin(), hcs.end(), [](const Hc& a, const Hc& b) {
    return std::abs(a.h) != std::abs(b.h) ? std::abs(a.h) < std::abs(b.h) : a.c < b.c;
  });
  const std::vector<int64_t> order = pa_halton((int64_t)hcs.size());
  std::vector<PaOp> ops(order.size());
  for (size_t i = 0; i < order.size(); ++i) {
    const Hc& s = hcs[(size_t)order[i]];
    pa_euler1('z', q->twist_degree * s.h + 360.0 * s.c / q->csym, ops[i].m_z);
    ops[i].shift = s.h * q->rise_pixel;
  }
  PA_ENSURE(p->d_ops, ops.size());
  PA_TRY(pa_copy(p, p->d_ops, ops.data(), ops.size() * sizeof(PaOp), true));
  PaOp* const d_ops = p->d_ops;
  // index map, chunk of operations by chunk, until the row target is passed (solver:1647)
  const size_t rays_per_op = (size_t)l2 * d2, per_op = rays_per_op * d2;
  const int n_ops = (int)ops.size();
  std::vector<unsigned char> has;
  std::vector<int> ray_of_row;
  PA_ENSURE(d_has, rays_per_op * 64);
  int64_t n_b = 0;
  int used = 0;
  bool done = false;
  while (used < n_ops && !done) {
    const int chunk = std::min(64, n_ops - used);
    if (g.linear) {  // nothing to keep per sample: only which rays meet the cylinder
      hipLaunchKernelGGL(k_pa_has_lin, pa_grid((int64_t)(rays_per_op * chunk)), dim3(256), 0, p->stream, g, d_ops, used,
                         rays_per_op * chunk, d_rank, d_has);
    } else {
    const size_t cap_ops = p->d_map.size() / per_op;
    if ((size_t)(used + chunk) > cap_ops) {  // grow the map (keep what is already there)
      const size_t ncap = std::max<size_t>(cap_ops * 2, (size_t)(used + chunk));
      DevBuf<int> nm;
      PA_ENSURE(nm, ncap * per_op);
      if (p->d_map) {
        const hipError_t ec = hipMemcpy(nm, p->d_map, (size_t)used * per_op * sizeof(int), hipMemcpyDeviceToDevice);
        if (ec != hipSuccess) { p->err = std::string("hh_pa_create: ") + hipGetErrorString(ec); return bail(HH_ERR_HIP); }
      }
      p->d_map = std::move(nm);
    }
    hipLaunchKernelGGL(k_pa_index, pa_grid((int64_t)(per_op * chunk)), dim3(256), 0, p->stream, g, d_ops, used, chunk, d_rank,
                       p->d_map + (size_t)used * per_op);
    hipLaunchKernelGGL(k_pa_has, pa_grid((int64_t)(rays_per_op * chunk)), dim3(256), 0, p->stream,
                       p->d_map + (size_t)used * per_op, rays_per_op * chunk, d2, d_has);
    }
    has.resize(rays_per_op * chunk);
    PA_TRY(pa_copy(p, has.data(), d_has, has.size(), false));
    for (int o = 0; o < chunk && !done; ++o) {
      // rows of this operation, in (k, j) order; b = pixel_vals[j, k], pid = k * ny + j (solver:1548-1549)
      for (int k = 0; k < l2; ++k)
        for (int j = 0; j < d2; ++j)
          if (has[((size_t)o * l2 + k) * d2 + j]) {
            ray_of_row.push_back((int)(((size_t)(used + o) * l2 + k) * d2 + j));
            p->b_data.push_back(image[(size_t)(j - d2 / 2 + ny / 2) * nx + (k - l2 / 2 + nx / 2)]);
            p->b_pid.push_back(k * d2 + j);
          }
      n_b = (int64_t)ray_of_row.size();
      p->n_ops_used = used + o + 1;
      if (q->min_projection_lines > 0 && n_b > q->min_projection_lines) done = true;
    }
    used += chunk;
  }
  d_has.reset();
  if (q->fsc_half > 0) {
    // split_A_b (solver:175-203): the data rows of one half of the image's pixels — every second pixel id (mode 2),
    // the lower half of the ids (mode 3), or the outer thirds against the middle third (mode 4 and above)
    std::vector<int32_t> ids(p->b_pid);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const size_t n = ids.size();
    std::vector<int32_t> set1;
    if (q->fsc_mode == 1) { set1.assign(q->fsc_ids, q->fsc_ids + q->n_fsc_ids); std::sort(set1.begin(), set1.end()); }
    else if (q->fsc_mode == 2) { for (size_t i = 0; i < n; i += 2) set1.push_back(ids[i]); }
    else if (q->fsc_mode == 3) { set1.assign(ids.begin(), ids.begin() + n / 2); }
    else { set1.assign(ids.begin(), ids.begin() + n / 3); set1.insert(set1.end(), ids.begin() + n * 2 / 3, ids.end()); }
    size_t w = 0;
    for (size_t r = 0; r < ray_of_row.size(); ++r) {
      const bool in1 = std::binary_search(set1.begin(), set1.end(), p->b_pid[r]);
      if (in1 == (q->fsc_half == 1)) {
        ray_of_row[w] = ray_of_row[r];
        p->b_data[w] = p->b_data[r];
        p->b_pid[w] = p->b_pid[r];
        ++w;
      }
    }
    ray_of_row.resize(w);
    p->b_data.resize(w);
    p->b_pid.resize(w);
  }
  p->m_data = (int64_t)ray_of_row.size();
  if (p->m_data == 0) { p->err = "hh_pa_create: no projection ray meets the cylinder"; return bail(HH_ERR_ARG); }
  PA_ENSURE(p->d_ray_of_row, ray_of_row.size());
  PA_TRY(pa_copy(p, p->d_ray_of_row, ray_of_row.data(), ray_of_row.size() * sizeof(int), true));
  // symmetry constraints (box (L3d, D3d, D3d) of lsq_reconstruct, solver:116-173)
  std::vector<int2> pairs;
  std::vector<PaEll16> rows16;
  if (q->min_sym_pairs > 0)
    pa_sym_pairs(l3, q->reconstruct_diameter_3d_pixel, q->reconstruct_diameter_3d_pixel, q->twist_degree, q->rise_pixel, q->csym,
                 rmin, rmax, q->min_sym_pairs, pairs, g.linear ? &rows16 : nullptr);
  p->m_sym = (int64_t)(g.linear ? rows16.size() : pairs.size());
  if (p->m_sym && g.linear) {
    PA_ENSURE(p->d_sym16, rows16.size());
    PA_TRY(pa_copy(p, p->d_sym16, rows16.data(), rows16.size() * sizeof(PaEll16), true));
  } else if (p->m_sym) {
    PA_ENSURE(p->d_pairs, pairs.size());
    PA_TRY(pa_copy(p, p->d_pairs, pairs.data(), pairs.size() * sizeof(int2), true));
  }
#undef PA_TRY
#undef PA_ENSURE
  const int rc = pa_alloc_vectors(p);
  if (rc) return bail(rc);
  {  // largest column sum of |A|, itself in fixed point (2^20: exact for hit counts, 1e-6 for trilinear weights)
    pa_scatter<true>(p, nullptr, std::ldexp(1.0, 20), p->d_x);
    std::vector<long long> sums((size_t)p->n);
    if (pa_copy(p, sums.data(), p->d_x, sums.size() * sizeof(long long), false) != hipSuccess) {
      p->err = "hh_pa_create: column sums failed";
      return bail(HH_ERR_HIP);
    }
    p->colsum = std::ldexp((double)*std::max_element(sums.begin(), sums.end()), -20) * (1.0 + 1e-3) + 1e-3;
  }
  guard.p = nullptr;
  *out = p;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_pa_create")

int hh_pa_dims(const hh_pa* p, int64_t dims[4]) try {
  if (!p || !dims) return HH_ERR_ARG;
  dims[0] = p->n; dims[1] = p->m_data; dims[2] = p->m_sym; dims[3] = p->n_ops_used;
  return HH_OK;
} HH_CATCH_PA(p, "hh_pa_dims")

int hh_pa_get_rhs(const hh_pa* p, float* b, int32_t* pid) try {
  if (!p) return HH_ERR_ARG;
  if (b) std::memcpy(b, p->b_data.data(), p->b_data.size() * sizeof(float));
  if (pid) std::memcpy(pid, p->b_pid.data(), p->b_pid.size() * sizeof(int32_t));
  return HH_OK;
} HH_CATCH_PA(p, "hh_pa_get_rhs")

// y = [A diag(d); diag(root)] x   (host float64 vectors; d and root may be NULL; y: m_data + m_sym (+ n with root))
int hh_pa_matvec(hh_pa* p, const double* x, const double* d, const double* root, double* y) try {
  if (!p || !x || !y) return pa_fail(p, HH_ERR_ARG, "hh_pa_matvec: NULL argument");
  PA_HIP(p, hipSetDevice(p->device));
  const int64_t rows = p->m_data + p->m_sym + (root ? p->n : 0);
  int rc;
  if ((rc = pa_upload(p, p->d_x, x, p->n, p->h_a))) return rc;
  if (d && (rc = pa_upload(p, p->d_scale, d, p->n, p->h_b))) return rc;
  if (root && (rc = pa_upload(p, p->d_root, root, p->n, p->h_c))) return rc;
  pa_op(p, p->d_x, d ? p->d_scale : nullptr, root ? p->d_root : nullptr, p->d_y);
  PA_HIP(p, hipGetLastError());
  return pa_download(p, y, p->d_y, rows);
} HH_CATCH_PA(p, "hh_pa_matvec")

// g = [A diag(d); diag(root)]^T y
int hh_pa_rmatvec(hh_pa* p, const double* y, const double* d, const double* root, double* g) try {
  if (!p || !y || !g) return pa_fail(p, HH_ERR_ARG, "hh_pa_rmatvec: NULL argument");
  PA_HIP(p, hipSetDevice(p->device));
  const int64_t rows = p->m_data + p->m_sym + (root ? p->n : 0);
  int rc;
  if ((rc = pa_upload(p, p->d_y, y, rows, p->h_a))) return rc;
  if (d && (rc = pa_upload(p, p->d_scale, d, p->n, p->h_b))) return rc;
  if (root && (rc = pa_upload(p, p->d_root, root, p->n, p->h_c))) return rc;
  double ymax = 0;
  for (int64_t i = 0; i < p->m_data + p->m_sym; ++i) ymax = std::max(ymax, std::fabs(y[i]));
  if (!std::isfinite(ymax)) return pa_fail(p, HH_ERR_ARG, "hh_pa_rmatvec: y is not finite");
  pa_op_t(p, p->d_y, d ? p->d_scale : nullptr, root ? p->d_root : nullptr, p->d_x, ymax);
  PA_HIP(p, hipGetLastError());
  return pa_download(p, g, p->d_x, p->n);
} HH_CATCH_PA(p, "hh_pa_rmatvec")

// LSMR (scipy.sparse.linalg.lsmr, damp = 0, x0 = 0) for min || Op x - rhs ||, Op = [A diag(d); diag(root)], with every
// vector on the device.  rhs: host, m_data + m_sym (+ n with root).  info = {istop, itn}; norms = {normr, normar}.
int hh_pa_lsmr(hh_pa* p, const double* rhs, const double* d, const double* root, double atol, double btol, double conlim,
               int maxiter, double* x_out, int info[2], double norms[2]) try {
  if (!p || !rhs || !x_out) return pa_fail(p, HH_ERR_ARG, "hh_pa_lsmr: NULL argument");
  PA_HIP(p, hipSetDevice(p->device));
  const int64_t n = p->n, m = p->m_data + p->m_sym + (root ? n : 0);
  const double* dd = nullptr;
  const double* dr = nullptr;
  int rc;
  if (d) { if ((rc = pa_upload(p, p->d_scale, d, n, p->h_b))) return rc; dd = p->d_scale; }
  if (root) { if ((rc = pa_upload(p, p->d_root, root, n, p->h_c))) return rc; dr = p->d_root; }
  double *u = p->d_u, *v = p->d_v, *h = p->d_h, *hbar = p->d_hbar, *x = p->d_x, *w = p->d_w;
  if ((rc = pa_upload(p, u, rhs, m, p->h_a))) return rc;
  PA_HIP(p, hipMemsetAsync(x, 0, (size_t)n * sizeof(double), p->stream));
  PA_HIP(p, hipMemsetAsync(hbar, 0, (size_t)n * sizeof(double), p->stream));
  double normb, beta, alpha = 0;
  if ((rc = pa_norm(p, u, m, &normb))) return rc;
  beta = normb;
  if (beta > 0) {
    hipLaunchKernelGGL(k_pa_scale, pa_grid(m), dim3(256), 0, p->stream, u, 1.0 / beta, m);
    pa_op_t(p, u, dd, dr, v, 1.0);
    if ((rc = pa_norm(p, v, n, &alpha))) return rc;
  } else {
    PA_HIP(p, hipMemsetAsync(v, 0, (size_t)n * sizeof(double), p->stream));
  }
  if (alpha > 0) hipLaunchKernelGGL(k_pa_scale, pa_grid(n), dim3(256), 0, p->stream, v, 1.0 / alpha, n);
  PA_HIP(p, hipMemcpyAsync(h, v, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
  int itn = 0, istop = 0;
  double zetabar = alpha * beta, alphabar = alpha, rho = 1, rhobar = 1, cbar = 1, sbar = 0;
  double betadd = beta, betad = 0, rhodold = 1, tautildeold = 0, thetatilde = 0, zeta = 0, dsum = 0;
  double normA2 = alpha * alpha, maxrbar = 0, minrbar = 1e100, normA = std::sqrt(normA2), condA = 1, normx = 0;
  const double ctol = conlim > 0 ? 1.0 / conlim : 0.0;
  double normr = beta, normar = alpha * beta;
  if (normar != 0 && normb != 0) {
    while (itn < maxiter) {
      ++itn;
      pa_op(p, v, dd, dr, w);                                                            // u = A v - alpha u
      hipLaunchKernelGGL(k_pa_scale_add, pa_grid(m), dim3(256), 0, p->stream, u, -alpha, w, m);
      if ((rc = pa_norm(p, u, m, &beta))) return rc;
      if (beta > 0) {
        hipLaunchKernelGGL(k_pa_scale, pa_grid(m), dim3(256), 0, p->stream, u, 1.0 / beta, m);
        pa_op_t(p, u, dd, dr, w, 1.0);                                                       // v = A^T u - beta v
        hipLaunchKernelGGL(k_pa_scale_add, pa_grid(n), dim3(256), 0, p->stream, v, -beta, w, n);
        if ((rc = pa_norm(p, v, n, &alpha))) return rc;
        if (alpha > 0) hipLaunchKernelGGL(k_pa_scale, pa_grid(n), dim3(256), 0, p->stream, v, 1.0 / alpha, n);
      }
      double chat, shat, alphahat, c, s;
      pa_sym_ortho(alphabar, 0.0, chat, shat, alphahat);
      const double rhoold = rho;
      pa_sym_ortho(alphahat, beta, c, s, rho);
      const double thetanew = s * alpha;
      alphabar = c * alpha;
      const double rhobarold = rhobar, zetaold = zeta;
      const double thetabar = sbar * rho, rhotemp = cbar * rho;
      pa_sym_ortho(cbar * rho, thetanew, cbar, sbar, rhobar);
      zeta = cbar * zetabar;
      zetabar = -sbar * zetabar;
      hipLaunchKernelGGL(k_pa_scale_add, pa_grid(n), dim3(256), 0, p->stream, hbar, -(thetabar * rho / (rhoold * rhobarold)), h, n);
      hipLaunchKernelGGL(k_pa_axpy, pa_grid(n), dim3(256), 0, p->stream, x, zeta / (rho * rhobar), hbar, n);
      hipLaunchKernelGGL(k_pa_scale_add, pa_grid(n), dim3(256), 0, p->stream, h, -(thetanew / rho), v, n);
      const double betaacute = chat * betadd, betacheck = -shat * betadd;
      const double betahat = c * betaacute;
      betadd = -s * betaacute;
      const double thetatildeold = thetatilde;
      double ctildeold, stildeold, rhotildeold;
      pa_sym_ortho(rhodold, thetabar, ctildeold, stildeold, rhotildeold);
      thetatilde = stildeold * rhobar;
      rhodold = ctildeold * rhobar;
      betad = -stildeold * betad + ctildeold * betahat;
      tautildeold = (zetaold - thetatildeold * tautildeold) / rhotildeold;
      const double taud = (zeta - thetatilde * tautildeold) / rhodold;
      dsum += betacheck * betacheck;
      normr = std::sqrt(dsum + (betad - taud) * (betad - taud) + betadd * betadd);
      normA2 += beta * beta;
      normA = std::sqrt(normA2);
      normA2 += alpha * alpha;
      maxrbar = std::max(maxrbar, rhobarold);
      if (itn > 1) minrbar = std::min(minrbar, rhobarold);
      condA = std::max(maxrbar, rhotemp) / std::min(minrbar, rhotemp);
      normar = std::fabs(zetabar);
      if ((rc = pa_norm(p, x, n, &normx))) return rc;
      const double test1 = normr / normb;
      const double test2 = (normA * normr) != 0 ? normar / (normA * normr) : INFINITY;
      const double test3 = 1 / condA;
      const double t1 = test1 / (1 + normA * normx / normb);
      const double rtol = btol + atol * normA * normx / normb;
      if (itn >= maxiter) istop = 7;
      if (1 + test3 <= 1) istop = 6;
      if (1 + test2 <= 1) istop = 5;
      if (1 + t1 <= 1) istop = 4;
      if (test3 <= ctol) istop = 3;
      if (test2 <= atol) istop = 2;
      if (test1 <= rtol) istop = 1;
      if (istop > 0) break;
    }
  }
  PA_HIP(p, hipGetLastError());
  if ((rc = pa_download(p, x_out, x, n))) return rc;
  PA_HIP(p, hipStreamSynchronize(p->stream));
  if (info) { info[0] = istop; info[1] = itn; }
  if (norms) { norms[0] = normr; norms[1] = normar; }
  return HH_OK;
} HH_CATCH_PA(p, "hh_pa_lsmr")

}  // extern "C"
