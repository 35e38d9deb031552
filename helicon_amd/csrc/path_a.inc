// path_a.inc — Path A (the reference's shipped denovo3D scorer) on the GPU, first slice (included by helicon_hip.hip).
//
// Reference: webApps/denovo3D/solver_linear_regression.py — build_A_data_matrix (1304-1654, nearest neighbour),
// build_A_helical_sym_matrix (847-1298, nearest neighbour), back_project_2d_coords_to_3d_coords (1657-1746),
// sorted_hsym_csym_pairs (1749-1791), lsq_reconstruct (31-547); lib/analysis.py:731-774 get_cylindrical_mask.
//
// The reference spends its time building two sparse matrices in (numba-compiled) Python loops and then calls
// scipy's LSMR.  Here the data matrix is never built: a row of A_data is one projection ray (symmetry operation o,
// image column k, image row j) and its entries are the voxels the ray's D2d depth samples fall into, so the device
// keeps only the int32 voxel index of every sample ("index map", -1 outside the cylinder) and
//     y = A x      gathers  x[idx]  along each ray                      (k_pa_matvec)
//     g = A^T y    scatters y[row]  to the samples' voxels, f64 atomics  (k_pa_rmatvec)
// The symmetry constraints x[i] - x[j] = 0 are a list of index pairs.  LSMR (Fong & Saunders 2011, the
// recurrences and stopping rules of scipy.sparse.linalg.lsmr) runs with all its vectors on the device, for A itself
// and for the trust-region step's augmented operator [A diag(d); diag(root)].  Coordinates are computed in float64
// with the reference's operation order and no contraction, so the rounding decisions (np.rint: ties to even) are
// the reference's: the implicit matrix equals the reference's CSR matrix entry for entry.
// Host-side glue (the bounded trust-region iteration of scipy.optimize.lsq_linear, positivity rule, score):
// helicon_amd/solver.py.

namespace {

struct PaGeom {
  int linear;            // 0: nearest neighbour (solver:1511-1553), 1: trilinear (solver:1414-1503)
  int L2, D2;            // image columns / rows used (nz', ny = nx of the back-projected grid)
  int mz, my, mx;        // mask box: (L3d, D2d, D2d)
  double m_y90[9];       // Ry(90) as scipy builds it (row-major); applied inverse
  double m_yx[9];        // Rx(psi) Ry(tilt); applied inverse
  double scale, dy;
};

struct PaOp {            // one symmetry operation of build_A_data_matrix
  double m_z[9];         // Rz(twist h + 360 c / csym); applied inverse
  double shift;          // h * rise_pixel
};

// inverse application of a rotation matrix, scipy's order of operations: out_j = v0 m[0][j] + v1 m[1][j] + v2 m[2][j]
__host__ __device__ __forceinline__ void pa_rot_inv(const double* m, double& x, double& y, double& z) {
#pragma clang fp contract(off)
  const double a = x * m[0] + y * m[3] + z * m[6];
  const double b = x * m[1] + y * m[4] + z * m[7];
  const double c = x * m[2] + y * m[5] + z * m[8];
  x = a; y = b; z = c;
}

// coordinates (in voxels of the mask box) of depth sample i of the ray through image column k, row j under one
// symmetry operation — back_project_2d_coords_to_3d_coords + solver:1389-1394, 1576-1581, float64, reference order
__host__ __device__ __forceinline__ void pa_coords(const PaGeom& g, const PaOp& op, int k, int j, int i, double& X, double& Y, double& Z) {
#pragma clang fp contract(off)
  // (X, Y, Z) = (column index, row index, depth index), centred, as float32 -> float64; Ry(90) inverse; scale
  double x = (double)(float)(k - g.L2 / 2), y = (double)(float)(j - g.D2 / 2), z = (double)(float)(i - g.D2 / 2);
  pa_rot_inv(g.m_y90, x, y, z);
  if (g.scale != 1.0) { x *= g.scale; y *= g.scale; z *= g.scale; }
  y -= g.dy;
  pa_rot_inv(g.m_yx, x, y, z);
  pa_rot_inv(op.m_z, x, y, z);
  z -= op.shift;
  X = x + (double)(g.mx / 2);
  Y = y + (double)(g.my / 2);
  Z = z + (double)(g.mz / 2);
}

// trilinear sample (solver:1420-1483): int() truncation towards zero, the whole 2 x 2 x 2 cell inside the cylinder;
// returns false when the sample contributes nothing; idx / w in the order 000, 001, 010, 011, 100, 101, 110, 111 (z, y, x)
__device__ __forceinline__ bool pa_cell(const PaGeom& g, const int* __restrict__ rank, double X, double Y, double Z, int idx[8],
                                        double w[8]) {
#pragma clang fp contract(off)
  const long long zi = (long long)Z, yi = (long long)Y, xi = (long long)X;
  if (zi < 0 || zi + 1 > g.mz - 1 || yi < 0 || yi + 1 > g.my - 1 || xi < 0 || xi + 1 > g.mx - 1) return false;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    idx[c] = rank[((size_t)(zi + (c >> 2)) * g.my + (yi + ((c >> 1) & 1))) * g.mx + (xi + (c & 1))];
    if (idx[c] < 0) return false;
  }
  const double zf = Z - (double)zi, yf = Y - (double)yi, xf = X - (double)xi;
  w[0] = (1 - zf) * (1 - yf) * (1 - xf);
  w[1] = (1 - zf) * (1 - yf) * xf;
  w[2] = (1 - zf) * yf * (1 - xf);
  w[3] = (1 - zf) * yf * xf;
  w[4] = zf * (1 - yf) * (1 - xf);
  w[5] = zf * (1 - yf) * xf;
  w[6] = zf * yf * (1 - xf);
  w[7] = zf * yf * xf;
  return true;
}

// voxel index of every ray sample: map[((o * L2 + k) * D2 + j) * D2 + i], -1 when the sample misses the cylinder
__global__ __launch_bounds__(256) void k_pa_index(PaGeom g, const PaOp* __restrict__ ops, int op0, int n_ops,
                                                  const int* __restrict__ rank, int* __restrict__ map) {
#pragma clang fp contract(off)
  const size_t per_op = (size_t)g.L2 * g.D2 * g.D2;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= per_op * n_ops) return;
  const int o = (int)(t / per_op);
  const size_t s = t % per_op;
  const int i = (int)(s % g.D2), j = (int)((s / g.D2) % g.D2), k = (int)(s / ((size_t)g.D2 * g.D2));
  double X, Y, Z;
  pa_coords(g, ops[op0 + o], k, j, i, X, Y, Z);
  const long long xi = (long long)rint(X), yi = (long long)rint(Y), zi = (long long)rint(Z);
  int idx = -1;
  if (zi >= 0 && zi < g.mz && yi >= 0 && yi < g.my && xi >= 0 && xi < g.mx)
    idx = rank[((size_t)zi * g.my + yi) * g.mx + xi];
  map[(size_t)o * per_op + s] = idx;
}

// has[ray] = the ray has at least one sample inside the mask (a row of A_data exists for it)
__global__ __launch_bounds__(256) void k_pa_has(const int* __restrict__ map, size_t n_rays, int d2, unsigned char* __restrict__ has) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const int* p = map + r * d2;
  unsigned char h = 0;
  for (int i = 0; i < d2; ++i) h |= p[i] >= 0;
  has[r] = h;
}

// y[r] = sum over the ray's samples of (x d)[idx]          (rows [0, m_data))
// y[m_data + q] = (x d)[pi] - (x d)[pj]                     (symmetry rows)
// y[m_data + m_sym + c] = root[c] x[c]                      (augmented rows, only with root)
// PA_G lanes share one projection ray (a data row): the ray's samples are dealt to them and the partial sums meet by
// shuffles, in a fixed order (the result does not depend on anything but PA_G).  One thread per symmetry / augmented row.
constexpr int PA_G = 16;
__device__ __forceinline__ double pa_group_sum(double v) {
#pragma unroll
  for (int off = PA_G / 2; off > 0; off >>= 1) v += __shfl_down(v, off, PA_G);
  return v;  // lane 0 of the group holds the sum
}

__global__ __launch_bounds__(256) void k_pa_matvec(const int* __restrict__ map, const int* __restrict__ ray_of_row, int d2,
                                                   int64_t m_data, const int2* __restrict__ pairs, int64_t m_sym,
                                                   const double* __restrict__ x, const double* __restrict__ dscale,
                                                   const double* __restrict__ root, int64_t n, double* __restrict__ y) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m_data * PA_G) {   // (m_data * PA_G is a multiple of the group size: whole groups take this branch)
    const int64_t r = t / PA_G;
    const int l = (int)(t % PA_G);
    const int* p = map + (size_t)ray_of_row[r] * d2;
    double acc = 0;
    for (int i = l; i < d2; i += PA_G) {
      const int c = p[i];
      if (c >= 0) acc += dscale ? x[c] * dscale[c] : x[c];
    }
    acc = pa_group_sum(acc);
    if (l == 0) y[r] = acc;
    return;
  }
  const int64_t r = m_data + (t - m_data * PA_G);
  if (r < m_data + m_sym) {
    const int2 pr = pairs[r - m_data];
    const double a = dscale ? x[pr.x] * dscale[pr.x] : x[pr.x], b = dscale ? x[pr.y] * dscale[pr.y] : x[pr.y];
    y[r] = a - b;
  } else if (root && r < m_data + m_sym + n) {
    const int64_t c = r - m_data - m_sym;
    y[r] = root[c] * x[c];
  }
}

// g = d (A^T y[:m]) + root y[m:]   — the scatter half.  The sums are accumulated in 64-bit FIXED POINT (integer atomics:
// associative, so the result does not depend on the order the hardware serves them in: the loosely converged
// trust-region solve amplifies a last-bit difference in A^T y to 1e-4 - 1e-3 in the score).  `scale` is a power of two
// chosen by the host from the largest column sum of |A| and max |y| (pa_op_t), so no sum can leave 62 bits; the
// resolution is 2^-61 of that bound.  ABS: accumulate |weight| x 1 instead (the column sums themselves, at create).
__device__ __forceinline__ void pa_acc(long long* acc, int c, double contribution) {
  atomicAdd(reinterpret_cast<unsigned long long*>(acc + c), (unsigned long long)__double2ll_rn(contribution));
}

template <bool ABS>
__global__ __launch_bounds__(256) void k_pa_rmatvec(const int* __restrict__ map, const int* __restrict__ ray_of_row, int d2,
                                                    int64_t m_data, const int2* __restrict__ pairs, int64_t m_sym,
                                                    const double* __restrict__ y, double scale, long long* __restrict__ acc) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m_data * PA_G) {
    const int64_t r = t / PA_G;
    const int l = (int)(t % PA_G);
    const int* p = map + (size_t)ray_of_row[r] * d2;
    const double v = (ABS ? 1.0 : y[r]) * scale;
    // a lane takes a contiguous piece of the ray: consecutive samples often fall into the same voxel, and one
    // atomic serves a run of equal indices
    const int per = (d2 + PA_G - 1) / PA_G, i0 = l * per, i1 = min(d2, i0 + per);
    int prev = -1, count = 0;
    for (int i = i0; i < i1; ++i) {
      const int c = p[i];
      if (c != prev) {
        if (prev >= 0) pa_acc(acc, prev, count * v);
        prev = c;
        count = 0;
      }
      ++count;
    }
    if (prev >= 0) pa_acc(acc, prev, count * v);
    return;
  }
  const int64_t r = m_data + (t - m_data * PA_G);
  if (r < m_data + m_sym) {
    const int2 pr = pairs[r - m_data];
    const double v = (ABS ? 1.0 : y[r]) * scale;
    pa_acc(acc, pr.x, v);
    pa_acc(acc, pr.y, ABS ? v : -v);
  }
}

// acc (fixed point, scale 1 / inv_scale) -> g = d acc + root y_tail, in place (acc and g are the same buffer)
__global__ void k_pa_finish_rmatvec(double* __restrict__ g, double inv_scale, const double* __restrict__ dscale,
                                    const double* __restrict__ root, const double* __restrict__ y_tail, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double v = (double)reinterpret_cast<const long long*>(g)[c] * inv_scale;
  if (dscale) v *= dscale[c];
  if (root) v += root[c] * y_tail[c];
  g[c] = v;
}

// small vector kernels of the LSMR loop (float64)
__global__ void k_pa_scale_add(double* __restrict__ u, double a, const double* __restrict__ w, int64_t n) {  // u = a u + w
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) u[i] = a * u[i] + w[i];
}
__global__ void k_pa_scale(double* __restrict__ u, double a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) u[i] *= a;
}
__global__ void k_pa_axpy(double* __restrict__ x, double a, const double* __restrict__ w, int64_t n) {  // x += a w
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] += a * w[i];
}
__global__ __launch_bounds__(256) void k_pa_sumsq(const double* __restrict__ u, int64_t n, double* __restrict__ out) {
  double s = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) s += u[i] * u[i];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// ---- trilinear interpolation: nothing is stored per sample, the geometry is recomputed in every product (60 float64
// operations per sample are cheaper than reading eight indices and weights back) -------------------------------------
__global__ __launch_bounds__(256) void k_pa_has_lin(PaGeom g, const PaOp* __restrict__ ops, int op0, size_t n_rays,
                                                    const int* __restrict__ rank, unsigned char* __restrict__ has) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  const int j = (int)(r % g.D2), k = (int)((r / g.D2) % g.L2), o = (int)(r / ((size_t)g.D2 * g.L2));
  unsigned char h = 0;
  for (int i = 0; i < g.D2 && !h; ++i) {
    double X, Y, Z, w[8];
    int idx[8];
    pa_coords(g, ops[op0 + o], k, j, i, X, Y, Z);
    h = pa_cell(g, rank, X, Y, Z, idx, w);
  }
  has[r] = h;
}

// symmetry rows of the trilinear branch: 16 (voxel, weight) entries each (solver:1061-1131)
struct PaEll16 {
  int idx[16];
  float w[16];
};

__global__ __launch_bounds__(256) void k_pa_matvec_lin(PaGeom g, const PaOp* __restrict__ ops, const int* __restrict__ rank,
                                                       const int* __restrict__ ray_of_row, int64_t m_data,
                                                       const PaEll16* __restrict__ sym, int64_t m_sym,
                                                       const double* __restrict__ x, const double* __restrict__ dscale,
                                                       const double* __restrict__ root, int64_t n, double* __restrict__ y) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m_data * PA_G) {
    const int64_t r = t / PA_G;
    const int l = (int)(t % PA_G);
    const int ray = ray_of_row[r];
    const int j = ray % g.D2, k = (ray / g.D2) % g.L2, o = ray / (g.D2 * g.L2);
    const PaOp op = ops[o];
    double acc = 0;
    for (int i = l; i < g.D2; i += PA_G) {
      double X, Y, Z, w[8];
      int idx[8];
      pa_coords(g, op, k, j, i, X, Y, Z);
      if (!pa_cell(g, rank, X, Y, Z, idx, w)) continue;
#pragma unroll
      for (int c = 0; c < 8; ++c) acc += w[c] * (dscale ? x[idx[c]] * dscale[idx[c]] : x[idx[c]]);
    }
    acc = pa_group_sum(acc);
    if (l == 0) y[r] = acc;
    return;
  }
  const int64_t r = m_data + (t - m_data * PA_G);
  if (r < m_data + m_sym) {
    const PaEll16& e = sym[r - m_data];
    double acc = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) acc += (double)e.w[c] * (dscale ? x[e.idx[c]] * dscale[e.idx[c]] : x[e.idx[c]]);
    y[r] = acc;
  } else if (root && r < m_data + m_sym + n) {
    const int64_t c = r - m_data - m_sym;
    y[r] = root[c] * x[c];
  }
}

template <bool ABS>
__global__ __launch_bounds__(256) void k_pa_rmatvec_lin(PaGeom g, const PaOp* __restrict__ ops, const int* __restrict__ rank,
                                                        const int* __restrict__ ray_of_row, int64_t m_data,
                                                        const PaEll16* __restrict__ sym, int64_t m_sym,
                                                        const double* __restrict__ y, double scale, long long* __restrict__ acc) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m_data * PA_G) {
    const int64_t r = t / PA_G;
    const int l = (int)(t % PA_G);
    const int ray = ray_of_row[r];
    const int j = ray % g.D2, k = (ray / g.D2) % g.L2, o = ray / (g.D2 * g.L2);
    const PaOp op = ops[o];
    const double v = (ABS ? 1.0 : y[r]) * scale;
    for (int i = l; i < g.D2; i += PA_G) {
      double X, Y, Z, w[8];
      int idx[8];
      pa_coords(g, op, k, j, i, X, Y, Z);
      if (!pa_cell(g, rank, X, Y, Z, idx, w)) continue;
#pragma unroll
      for (int c = 0; c < 8; ++c) pa_acc(acc, idx[c], (ABS ? fabs(w[c]) : w[c]) * v);   // (a weight is negative only in the cell next to index 0)
    }
    return;
  }
  const int64_t r = m_data + (t - m_data * PA_G);
  if (r < m_data + m_sym) {
    const PaEll16& e = sym[r - m_data];
    const double v = (ABS ? 1.0 : y[r]) * scale;
#pragma unroll
    for (int c = 0; c < 16; ++c) pa_acc(acc, e.idx[c], (ABS ? fabs((double)e.w[c]) : (double)e.w[c]) * v);
  }
}

}  // namespace

struct hh_pa {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  PaGeom g{};
  int64_t n = 0, m_data = 0, m_sym = 0;
  int n_ops_used = 0;
  DevBuf<int> d_map;             // [n_ops_used][L2][D2][D2]
  DevBuf<int> d_ray_of_row;      // [m_data] ray index (o * L2 + k) * D2 + j
  DevBuf<int2> d_pairs;          // [m_sym] (nearest neighbour)
  DevBuf<PaEll16> d_sym16;       // [m_sym] (trilinear)
  DevBuf<PaOp> d_ops;            // [n_ops] (kept: the trilinear products recompute the geometry)
  DevBuf<int> d_rank;            // [mz][my][mx] voxel rank, -1 outside the cylinder
  double colsum = 0;             // largest column sum of |A| (sizes the fixed-point scale of A^T y)
  // pinned host staging: vectors cross the boundary through these, never straight from / to the caller's pageable
  // arrays — the runtime pins such pages on the fly, and with the solver's stream of freshly allocated NumPy arrays
  // that cost sporadic ~95 ms stalls (7 of them in one 0.7 s lsq_reconstruct call)
  double* h_a = nullptr;         // [m + n]
  double* h_b = nullptr;         // [n]
  double* h_c = nullptr;         // [n]
  double* h_out = nullptr;       // [m + n]
  double* h_red = nullptr;       // [1024] block sums of a norm
  void* h_stage = nullptr;       // set-up transfers (pa_copy), this object's own
  std::vector<float> b_data;     // [m_data]
  std::vector<int32_t> b_pid;    // [m_data]
  // work vectors (float64)
  DevBuf<double> d_x, d_y, d_u, d_v, d_h, d_hbar, d_w, d_scale, d_root, d_red;
};
