// adaptive_mask.inc — the adaptive mask of the true FSC (commands/trueFSC.py:660-735, _generate_adaptive_mask, as
// helicon_amd.true_fsc.adaptive_mask restates it) built on the device from a float64 volume, or from the float32 maps a
// true-FSC context already holds.
//
//   LP      scipy.ndimage.gaussian_filter(V, sigma) in float64, mode "reflect": three passes z, y, x, each on the previous
//           pass's float64 output; per output t = v[i] w[0], then for j = r ... 1: t += (v[i - j] + v[i + j]) w[j], products
//           and sums rounded one by one (am_mul / am_add: no FMA), indices folded with period 2 n.  The taps w[0 ... r],
//           r = int(4 sigma + 0.5), come from the caller (NumPy's exp and sum), never from this file.
//           k_am_gauss_line: y and z.  Lanes along x, AM_TILE consecutive outputs per thread; the two windows v[i - j] and
//                            v[i + j] slide through registers while j runs down: two loads per j for AM_TILE outputs.
//           k_am_gauss_x:    one wavefront per line; the line and its folded halo staged in LDS.
//   thresh  a fraction of max(LP), a value, the k-th largest voxel, or Otsu's threshold on 256 bins over [min, max] counted by
//           np.linspace's edges (am_edges; bin i holds edges[i] <= x < edges[i + 1], the last bin is closed, zeros left out).
//           k_am_minmax: exact minimum and maximum, per-workgroup partials finished on the host; counts non-finite voxels.
//           k_am_hist:   edges and counts in LDS, integer adds.
//           k_am_digits: radix selection of the k-th largest on order-preserving 64-bit keys, one 8-bit digit per pass from
//                        the top; the host walks the 256 counts.  Integer counts only: no dependence on the schedule.
//   seeds   {LP >= v*} and {LP > thresh}, v* the 1000th largest voxel: EVERY voxel tied at v* (np.argpartition keeps an
//           arbitrary 1000 of them).
//   label   26-connected components of {LP > thresh}: an int32 parent per voxel.
//           k_am_runs:    x-runs by ballot: every foreground voxel points at the first voxel of its run.
//           k_am_unions:  the four preceding lines (z, y-1), (z-1, y-1), (z-1, y), (z-1, y+1) at dx in {-1, 0, 1}: one union
//                         per pair of adjacent runs.  A union links the larger root to the smaller by an agent-scope atomic
//                         min and goes on from the value the atomic returned; a load inside am_find may be stale and is an
//                         agent-scope relaxed atomic load.  Parents only decrease, so the final root of a component is its
//                         smallest flat index whatever the order of execution.
//           k_am_flatten: every voxel gets its root; counts the roots.
//           Every find / union loop spends from a step budget; a budget that runs out, or a parent that is not a smaller
//           foreground index, sets the error word and the call returns HH_ERR_INTERNAL.
//   pick    keep[root] = 1 from the seeds (k_am_keep); mask = keep[root[v]] (k_am_pick); nothing kept: the mask is {LP > thresh}.
//
// Scratch per voxel: two float64 planes, the int32 parents, two byte planes (three when the mask is downloaded): 22 or 23
// bytes, allocated and released per call.

namespace {

constexpr int AM_MAX_SIDE = 1024;
constexpr int64_t AM_MAX_VOXELS = (int64_t)1 << 28;   // int32 parents
constexpr int AM_MAX_RADIUS = 4096;
constexpr int AM_HALO = 1024;       // the x pass stages at most this much halo on each side; taps beyond it fold on the fly
constexpr int AM_TILE = 8;
constexpr int AM_STEP_CAP = 1 << 22;   // steps one union (or one flattening find) may take before it is a defect
constexpr int AM_SEEDS = 1000;
constexpr int AM_GRID = 1024;          // workgroups of the reductions (per-workgroup partials)
enum { AM_W_ABOVE = 0, AM_W_GE, AM_W_ROOTS, AM_W_KEPT, AM_W_BAD, AM_W_ERR, AM_WORDS = 8 };   // the call's counters; then 256 bin counts
enum { AM_EV_START = 0, AM_EV_Z, AM_EV_Y, AM_EV_X, AM_EV_STATS, AM_EV_RUNS, AM_EV_UNIONS, AM_EV_FLATTEN, AM_EV_PICK, AM_EVENTS };

double g_am_stage_ms[8] = {0};   // the last mask call: z, y, x, statistics, runs, unions, flatten, pick

__device__ __forceinline__ double am_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double am_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// scipy's "reflect": d c b a | a b c d | d c b a, period 2 n
__device__ __forceinline__ int am_fold(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// out = in (float64), or float64(a), or (float64(a) + float64(b)) / 2
__global__ __launch_bounds__(256) void k_am_widen(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = b ? am_add((double)a[i], (double)b[i]) / 2.0 : (double)a[i];
}

// One pass along y or z.  Element (o, j, x) lies at o * so + j * sl + x; thread: one (o, x) column and AM_TILE consecutive i.
__global__ __launch_bounds__(256) void k_am_gauss_line(const double* __restrict__ in, double* __restrict__ out, const double* __restrict__ w, int r, int m,
                                                       int mx, int64_t columns, int64_t so, int64_t sl) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= columns) return;
  const int64_t base = (q / mx) * so + (q % mx);
  const int i0 = blockIdx.y * AM_TILE;
  double acc[AM_TILE], lo[AM_TILE], hi[AM_TILE];
  const double w0 = w[0];
#pragma unroll
  for (int t = 0; t < AM_TILE; ++t) acc[t] = am_mul(in[base + am_fold(i0 + t, m) * sl], w0);
  if (r > 0) {
#pragma unroll
    for (int t = 0; t < AM_TILE; ++t) {   // lo[t] = v[i0 + t - j], hi[t] = v[i0 + t + j] at j = r
      lo[t] = in[base + am_fold(i0 + t - r, m) * sl];
      hi[t] = in[base + am_fold(i0 + t + r, m) * sl];
    }
    for (int j = r;;) {
      const double wj = w[j];
#pragma unroll
      for (int t = 0; t < AM_TILE; ++t) acc[t] = am_add(acc[t], am_mul(am_add(lo[t], hi[t]), wj));
      if (--j == 0) break;
#pragma unroll
      for (int t = 0; t < AM_TILE - 1; ++t) lo[t] = lo[t + 1];
      lo[AM_TILE - 1] = in[base + am_fold(i0 + AM_TILE - 1 - j, m) * sl];
#pragma unroll
      for (int t = AM_TILE - 1; t > 0; --t) hi[t] = hi[t - 1];
      hi[0] = in[base + am_fold(i0 + j, m) * sl];
    }
  }
#pragma unroll
  for (int t = 0; t < AM_TILE; ++t)
    if (i0 + t < m) out[base + (int64_t)(i0 + t) * sl] = acc[t];
}

// The pass along x: one wavefront (one workgroup) per line; ext[halo + k] = v[fold(k)] for k in [-halo, nx + halo).
__global__ __launch_bounds__(64) void k_am_gauss_x(const double* __restrict__ in, double* __restrict__ out, const double* __restrict__ w, int r, int nx,
                                                   int halo) {
  extern __shared__ __attribute__((aligned(16))) double am_ext[];
  const int lane = threadIdx.x;
  const double* const src = in + (int64_t)blockIdx.x * nx;
  double* const dst = out + (int64_t)blockIdx.x * nx;
  for (int k = lane; k < nx + 2 * halo; k += 64) am_ext[k] = src[am_fold(k - halo, nx)];
  __syncthreads();
  const double w0 = w[0];
  for (int x = lane; x < nx; x += 64) {
    double t = am_mul(am_ext[halo + x], w0);
    int j = r;
    for (; j > halo; --j) t = am_add(t, am_mul(am_add(am_ext[halo + am_fold(x - j, nx)], am_ext[halo + am_fold(x + j, nx)]), w[j]));
    for (; j >= 1; --j) t = am_add(t, am_mul(am_add(am_ext[halo + x - j], am_ext[halo + x + j]), w[j]));
    dst[x] = t;
  }
}

// dst += the workgroup's sum of `mine` (integers: the order does not matter)
__device__ __forceinline__ void am_block_add(unsigned long long* dst, unsigned mine) {
  __shared__ unsigned total;
  if (threadIdx.x == 0) total = 0u;
  __syncthreads();
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0 && total) atomicAdd(dst, (unsigned long long)total);
  __syncthreads();
}

// per-workgroup minimum and maximum of the finite voxels (pmin, pmax: [gridDim.x]); words[AM_W_BAD] += the others
__global__ __launch_bounds__(256) void k_am_minmax(const double* __restrict__ v, int64_t n, double* __restrict__ pmin, double* __restrict__ pmax,
                                                   unsigned long long* words) {
  __shared__ double smin[256], smax[256];
  double mn = INFINITY, mx = -INFINITY;
  unsigned bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double x = v[i];
    if (isfinite(x)) {
      mn = x < mn ? x : mn;
      mx = x > mx ? x : mx;
    } else {
      ++bad;
    }
  }
  smin[threadIdx.x] = mn;
  smax[threadIdx.x] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double a = smin[threadIdx.x + s], b = smax[threadIdx.x + s];
      if (a < smin[threadIdx.x]) smin[threadIdx.x] = a;
      if (b > smax[threadIdx.x]) smax[threadIdx.x] = b;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    pmin[blockIdx.x] = smin[0];
    pmax[blockIdx.x] = smax[0];
  }
  am_block_add(words + AM_W_BAD, bad);
}

// counts[i] += voxels x != 0 with edges[i] <= x < edges[i + 1] (i = 255: x <= edges[256]); every x lies in [edges[0], edges[256]]
__global__ __launch_bounds__(256) void k_am_hist(const double* __restrict__ v, int64_t n, const double* __restrict__ edges, unsigned long long* counts) {
  __shared__ double e[257];
  __shared__ unsigned c[256];
  for (int k = threadIdx.x; k < 257; k += 256) e[k] = edges[k];
  c[threadIdx.x] = 0u;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double x = v[i];
    if (x == 0.0) continue;
    int lo = 0, hi = 256;   // e[lo] <= x, and x < e[hi] or hi == 256
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (e[mid] <= x) lo = mid; else hi = mid;
    }
    atomicAdd(&c[lo], 1u);
  }
  __syncthreads();
  if (c[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)c[threadIdx.x]);
}

// keys order as the doubles do (-0.0 just below +0.0)
__device__ __forceinline__ unsigned long long am_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// counts[d] += keys whose bits above shift + 8 equal `prefix` and whose digit (key >> shift) & 255 is d
__global__ __launch_bounds__(256) void k_am_digits(const double* __restrict__ v, int64_t n, unsigned long long prefix, int shift, unsigned long long* counts) {
  __shared__ unsigned c[256];
  c[threadIdx.x] = 0u;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned long long k = am_key(v[i]);
    if (shift == 56 || (k >> (shift + 8)) == prefix) atomicAdd(&c[(unsigned)(k >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (c[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)c[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_am_above(const double* __restrict__ lp, int64_t n, double thresh, double vstar, uint8_t* __restrict__ above,
                                                  unsigned long long* words) {
  unsigned n_above = 0, n_ge = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double x = lp[i];
    const bool a = x > thresh;
    above[i] = a ? 1 : 0;
    n_above += a ? 1u : 0u;
    n_ge += x >= vstar ? 1u : 0u;
  }
  am_block_add(words + AM_W_ABOVE, n_above);
  am_block_add(words + AM_W_GE, n_ge);
}

// One wavefront per line: parent[v] = the first voxel of v's x-run, -1 on background.
__global__ __launch_bounds__(256) void k_am_runs(const uint8_t* __restrict__ fg, int nx, int64_t lines, int32_t* __restrict__ parent) {
  const int lane = threadIdx.x & 63;
  const int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (line >= lines) return;   // whole wavefronts leave together
  const uint8_t* const src = fg + line * nx;
  int32_t* const dst = parent + line * nx;
  const int base = (int)(line * nx);
  const unsigned long long under = lane == 0 ? 0ull : ((1ull << lane) - 1ull);
  int carry = -1;   // the start of the run that reaches the end of the previous chunk
  for (int x0 = 0; x0 < nx; x0 += 64) {
    const int x = x0 + lane;
    const bool inside = x < nx && src[x] != 0;
    const unsigned long long b = __ballot(inside);
    const unsigned long long gap = ~b & under;   // background below this lane
    const int start = gap ? x0 + 64 - __clzll((long long)gap) : (carry >= 0 ? carry : x0);
    if (x < nx) dst[x] = inside ? base + start : -1;
    if (b >> 63) {
      const unsigned long long z = ~b;
      carry = z ? x0 + 64 - __clzll((long long)z) : (carry >= 0 ? carry : x0);
    } else {
      carry = -1;
    }
  }
}

__device__ __forceinline__ void am_defect(int* err) { __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of i, or -1 after a defect; the voxel's own pointer is moved to the root found (parents only decrease)
__device__ int am_find(int32_t* parent, int i, int& budget, int* err) {
  const int first = i;
  for (;;) {
    const int p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == i) break;
    if (p < 0 || p > i || --budget <= 0) {
      am_defect(err);
      return -1;
    }
    i = p;
  }
  if (i != first) (void)__hip_atomic_fetch_min(parent + first, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return i;
}

__device__ void am_union(int32_t* parent, int a, int b, int* err) {
  int budget = AM_STEP_CAP;
  for (;;) {
    a = am_find(parent, a, budget, err);
    b = am_find(parent, b, budget, err);
    if (a < 0 || b < 0 || a == b) return;
    if (a < b) {
      const int t = a; a = b; b = t;
    }
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;   // a was a root and now hangs below b
    a = old;                // a had been linked elsewhere meanwhile: that link's target and b are still to be joined
    if (--budget <= 0) {
      am_defect(err);
      return;
    }
  }
}

// One union per pair of adjacent runs: a voxel whose left neighbour belongs to its run has only L[x + 1] left to look at, and
// that only when L[x] is background (otherwise it is the run of L[x], which the left voxel's window held).
__global__ __launch_bounds__(256) void k_am_unions(const uint8_t* __restrict__ fg, int32_t* parent, int nz, int ny, int nx, int64_t n, int* err) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (!fg[i]) continue;
    const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((int64_t)nx * ny));
    const bool left = x > 0 && fg[i - 1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int zz = k == 0 ? z : z - 1, yy = k == 2 ? y : (k == 3 ? y + 1 : y - 1);
      if (zz < 0 || yy < 0 || yy >= ny) continue;
      const int64_t row = ((int64_t)zz * ny + yy) * nx;
      const bool c = fg[row + x] != 0, r = x + 1 < nx && fg[row + x + 1] != 0;
      if (left) {
        if (r && !c) am_union(parent, (int)i, (int)(row + x + 1), err);
      } else if (c) {
        am_union(parent, (int)i, (int)(row + x), err);
      } else {
        if (x > 0 && fg[row + x - 1]) am_union(parent, (int)i, (int)(row + x - 1), err);
        if (r) am_union(parent, (int)i, (int)(row + x + 1), err);
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_am_flatten(const uint8_t* __restrict__ fg, int32_t* parent, int64_t n, unsigned long long* words, int* err) {
  unsigned roots = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (!fg[i]) continue;
    int budget = AM_STEP_CAP;
    if (am_find(parent, (int)i, budget, err) == (int)i) ++roots;
  }
  am_block_add(words + AM_W_ROOTS, roots);
}

// keep[root] = 1 for every component that holds a seed (several writers, one value)
__global__ __launch_bounds__(256) void k_am_keep(const double* __restrict__ lp, const uint8_t* __restrict__ above, const int32_t* __restrict__ root, int64_t n,
                                                 double vstar, uint8_t* keep) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    if (above[i] && lp[i] >= vstar) keep[root[i]] = 1;
}

__global__ __launch_bounds__(256) void k_am_pick(const uint8_t* __restrict__ above, const int32_t* __restrict__ root, const uint8_t* __restrict__ keep, int64_t n,
                                                 uint8_t* __restrict__ mask, unsigned long long* words) {
  unsigned kept = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint8_t m = above[i] ? keep[root[i]] : 0;
    mask[i] = m;
    kept += m;
  }
  am_block_add(words + AM_W_KEPT, kept);
}

// np.linspace(mn, mx, 257)
void am_edges(double mn, double mx, double* e) {
#pragma clang fp contract(off)
  const double delta = mx - mn, step = delta / 256.0;
  for (int i = 0; i < 257; ++i) e[i] = (step == 0.0 ? ((double)i / 256.0) * delta : (double)i * step) + mn;
  e[256] = mx;
}

// otsu_threshold_eman from the histogram on: the first bin skipped, ties to the lowest bin
double am_otsu(const int64_t* counts, double hmin, double hmax) {
#pragma clang fp contract(off)
  const double bin_width = (hmax - hmin) / 256.0;
  double total = 0.0, sum_all = 0.0;
  for (int i = 0; i < 256; ++i) {
    total += (double)counts[i];
    sum_all += (double)i * (double)counts[i];
  }
  if (total == 0.0) return hmin;
  double cum = 0.0, cumv = 0.0, best = 0.0;
  int arg = 0;
  for (int i = 0; i < 256; ++i) {
    cum += (double)counts[i];
    cumv += (double)i * (double)counts[i];
    const double w_b = cum, w_f = total - cum;
    double m_b = 0.0, m_f = 0.0;
    if (w_b > 0 && w_f > 0) {
      m_b = cumv / w_b;
      m_f = (sum_all - cumv) / w_f;
    }
    const double d = m_b - m_f;
    const double between = w_b * w_f * (d * d);
    if (i >= 1 && (arg == 0 || between > best)) {
      best = between;
      arg = i;
    }
  }
  return hmin + (double)(arg + 1) * bin_width;
}

bool am_sides_ok(int nz, int ny, int nx) { return nz >= 1 && ny >= 1 && nx >= 1 && nz <= AM_MAX_SIDE && ny <= AM_MAX_SIDE && nx <= AM_MAX_SIDE; }

// r = int(4 sigma + 0.5), or -1 when sigma is no filter width this file takes
int am_radius(double sigma) {
  if (!std::isfinite(sigma) || !(sigma > 0) || 4.0 * sigma + 0.5 >= (double)(AM_MAX_RADIUS + 1)) return -1;
  return (int)(4.0 * sigma + 0.5);
}

unsigned am_grid(int64_t n, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap)); }

struct AmScratch {
  DevBuf<double> a, b, taps, small;        // small: edges [257], pmin [AM_GRID], pmax [AM_GRID]
  DevBuf<int32_t> parent;
  DevBuf<uint8_t> above, keep, mask;
  DevBuf<unsigned long long> words;        // [AM_WORDS + 256]
  DevEvents<AM_EVENTS> ev;
  int* err() const { return reinterpret_cast<int*>(words + AM_W_ERR); }
};

int am_reserve(AmScratch* s, int64_t n, bool planes, bool labels, bool keep, bool mask, const double* taps, int r) {
  int rc = HH_OK;
  if (planes) {
    rc = ensure(nullptr, s->a, (size_t)n);
    if (!rc) rc = ensure(nullptr, s->b, (size_t)n);
    if (!rc) rc = ensure(nullptr, s->small, (size_t)(257 + 2 * AM_GRID));
  }
  if (!rc && labels) {
    rc = ensure(nullptr, s->parent, (size_t)n);
    if (!rc) rc = ensure(nullptr, s->above, (size_t)n);
  }
  if (!rc && keep) rc = ensure(nullptr, s->keep, (size_t)n);
  if (!rc && mask) rc = ensure(nullptr, s->mask, (size_t)n);
  if (!rc) rc = ensure(nullptr, s->words, (size_t)(AM_WORDS + 256));
  if (!rc && taps) rc = ensure(nullptr, s->taps, (size_t)(r + 1));
  if (rc) return rc;
  HH_HIP(nullptr, hipMemset(s->words, 0, s->words.bytes()));
  if (taps) {
    HH_HIP(nullptr, hipMemcpy(s->taps, taps, (size_t)(r + 1) * sizeof(double), hipMemcpyHostToDevice));
  }
  HH_HIP(nullptr, s->ev.create());
  return HH_OK;
}

// the three passes z, y, x on the default stream: s->a -> s->b -> s->a -> s->b
int am_filter(AmScratch* s, int nz, int ny, int nx, int r) {
  const int64_t cz = (int64_t)ny * nx, cy = (int64_t)nz * nx, lines = (int64_t)nz * ny;
  hipLaunchKernelGGL(k_am_gauss_line, dim3((unsigned)((cz + 255) / 256), (unsigned)((nz + AM_TILE - 1) / AM_TILE)), dim3(256), 0, nullptr, s->a, s->b,
                     s->taps, r, nz, nx, cz, (int64_t)nx, (int64_t)ny * nx);
  HH_HIP(nullptr, hipEventRecord(s->ev[AM_EV_Z], nullptr));
  hipLaunchKernelGGL(k_am_gauss_line, dim3((unsigned)((cy + 255) / 256), (unsigned)((ny + AM_TILE - 1) / AM_TILE)), dim3(256), 0, nullptr, s->b, s->a,
                     s->taps, r, ny, nx, cy, (int64_t)ny * nx, (int64_t)nx);
  HH_HIP(nullptr, hipEventRecord(s->ev[AM_EV_Y], nullptr));
  const int halo = std::min(r, AM_HALO);
  hipLaunchKernelGGL(k_am_gauss_x, dim3((unsigned)lines), dim3(64), (size_t)(nx + 2 * halo) * sizeof(double), nullptr, s->a, s->b, s->taps, r, nx, halo);
  HH_HIP(nullptr, hipEventRecord(s->ev[AM_EV_X], nullptr));
  HH_HIP(nullptr, hipGetLastError());
  return HH_OK;
}

// runs, unions, flatten of s->above into s->parent; words[AM_W_ROOTS] counts the components
int am_label(AmScratch* s, int nz, int ny, int nx) {
  const int64_t n = (int64_t)nz * ny * nx, lines = (int64_t)nz * ny;
  hipLaunchKernelGGL(k_am_runs, dim3((unsigned)((lines + 3) / 4)), dim3(256), 0, nullptr, s->above, nx, lines, s->parent);
  HH_HIP(nullptr, hipEventRecord(s->ev[AM_EV_RUNS], nullptr));
  hipLaunchKernelGGL(k_am_unions, dim3(am_grid(n, 65536)), dim3(256), 0, nullptr, s->above, s->parent, nz, ny, nx, n, s->err());
  HH_HIP(nullptr, hipEventRecord(s->ev[AM_EV_UNIONS], nullptr));
  hipLaunchKernelGGL(k_am_flatten, dim3(am_grid(n, 65536)), dim3(256), 0, nullptr, s->above, s->parent, n, s->words, s->err());
  HH_HIP(nullptr, hipEventRecord(s->ev[AM_EV_FLATTEN], nullptr));
  HH_HIP(nullptr, hipGetLastError());
  return HH_OK;
}

int am_defect_found(const char* fn) {
  return fail(nullptr, HH_ERR_INTERNAL, std::string(fn) + ": the labelling met a parent that is no smaller foreground index, or ran out of its step budget");
}

// the value at index `rank` of lp sorted in descending order
int am_select(AmScratch* s, const double* lp, int64_t n, int64_t rank, double* value) {
  unsigned long long* const counts = s->words + AM_WORDS;
  unsigned long long host[256], prefix = 0;
  int64_t rem = rank;
  for (int shift = 56; shift >= 0; shift -= 8) {
    HH_HIP(nullptr, hipMemsetAsync(counts, 0, sizeof(host), nullptr));
    hipLaunchKernelGGL(k_am_digits, dim3(am_grid(n, AM_GRID)), dim3(256), 0, nullptr, lp, n, prefix, shift, counts);
    HH_HIP(nullptr, hipGetLastError());
    HH_HIP(nullptr, hipMemcpy(host, counts, sizeof(host), hipMemcpyDeviceToHost));
    int d = 255;
    for (; d > 0 && rem >= (int64_t)host[d]; --d) rem -= (int64_t)host[d];
    if (rem >= (int64_t)host[d]) return fail(nullptr, HH_ERR_INTERNAL, "am_select: the digit counts do not hold the rank");
    prefix = (prefix << 8) | (unsigned long long)d;
  }
  const unsigned long long bits = (prefix >> 63) ? (prefix & 0x7fffffffffffffffull) : ~prefix;
  std::memcpy(value, &bits, sizeof(double));
  return HH_OK;
}

constexpr int AM_MODE_OTSU = 0, AM_MODE_FRACTION = 1, AM_MODE_VALUE = 2, AM_MODE_RANK = 3;

// what can be refused without the box: sigma, the taps, the mode and its argument
int am_check_threshold_args(const std::string& f, double sigma, const double* taps, int mode, double value) {
  if (sigma != 0.0 && am_radius(sigma) < 0) return fail(nullptr, HH_ERR_ARG, f + ": sigma must be 0 (no filter) or positive and finite with int(4 sigma + 0.5) <= 4096");
  if (sigma != 0.0 && !taps) return fail(nullptr, HH_ERR_ARG, f + ": NULL taps with sigma > 0");
  if (mode < AM_MODE_OTSU || mode > AM_MODE_RANK) return fail(nullptr, HH_ERR_ARG, f + ": unknown mode (0 Otsu, 1 fraction of the maximum, 2 value, 3 rank)");
  if (mode != AM_MODE_OTSU && !std::isfinite(value)) return fail(nullptr, HH_ERR_ARG, f + ": the threshold argument is NaN or infinite");
  return HH_OK;
}

int am_check_box(const std::string& f, int nz, int ny, int nx, int mode, double value) {
  if (!am_sides_ok(nz, ny, nx)) return fail(nullptr, HH_ERR_ARG, f + ": the sides of the box must lie in [1, 1024]");
  const int64_t n = (int64_t)nz * ny * nx;
  if (n > AM_MAX_VOXELS) return fail(nullptr, HH_ERR_ARG, f + ": more than 2^28 voxels");
  if (n < AM_SEEDS) return fail(nullptr, HH_ERR_ARG, f + ": fewer than 1000 voxels: there is no 1000th largest value");
  if (mode == AM_MODE_RANK && (value < 0 || value > (double)(n - 1) || value != std::floor(value)))
    return fail(nullptr, HH_ERR_ARG, f + ": the rank must be a whole number in [0, N - 1]");
  return HH_OK;
}

// s->a holds the volume; the support goes to d_support (device, n bytes)
int am_build(const char* fn, AmScratch* s, int nz, int ny, int nx, double sigma, int mode, double value, uint8_t* d_support, double* info) {
  const std::string f(fn);
  const int64_t n = (int64_t)nz * ny * nx;
  HH_HIP(nullptr, hipMemsetAsync(s->words, 0, (size_t)(AM_WORDS + 256) * sizeof(unsigned long long), nullptr));
  HH_HIP(nullptr, hipEventRecord(s->ev[AM_EV_START], nullptr));
  const double* lp = s->a;
  if (sigma != 0.0) {
    if (int rc = am_filter(s, nz, ny, nx, am_radius(sigma))) return rc;
    lp = s->b;
  } else {
    for (int e = AM_EV_Z; e <= AM_EV_X; ++e) HH_HIP(nullptr, hipEventRecord(s->ev[e], nullptr));
  }
  // minimum, maximum, non-finite voxels
  double* const d_edges = s->small;
  double *const d_pmin = s->small + 257, *const d_pmax = d_pmin + AM_GRID;
  const unsigned g = am_grid(n, AM_GRID);
  hipLaunchKernelGGL(k_am_minmax, dim3(g), dim3(256), 0, nullptr, lp, n, d_pmin, d_pmax, s->words);
  HH_HIP(nullptr, hipGetLastError());
  std::vector<double> part((size_t)2 * AM_GRID);
  unsigned long long words[AM_WORDS];
  HH_HIP(nullptr, hipMemcpy(part.data(), d_pmin, (size_t)2 * AM_GRID * sizeof(double), hipMemcpyDeviceToHost));
  HH_HIP(nullptr, hipMemcpy(words, s->words, sizeof(words), hipMemcpyDeviceToHost));
  if (words[AM_W_BAD]) return fail(nullptr, HH_ERR_ARG, f + ": the volume holds NaN or infinite values");
  double mn = INFINITY, mx = -INFINITY;
  for (unsigned k = 0; k < g; ++k) {
    mn = std::min(mn, part[k]);
    mx = std::max(mx, part[(size_t)AM_GRID + k]);
  }
  double vstar = 0.0, thresh = 0.0;
  if (int rc = am_select(s, lp, n, AM_SEEDS - 1, &vstar)) return rc;
  if (mode == AM_MODE_FRACTION) {
    thresh = value * mx;
  } else if (mode == AM_MODE_VALUE) {
    thresh = value;
  } else if (mode == AM_MODE_RANK) {
    if (int rc = am_select(s, lp, n, (int64_t)value, &thresh)) return rc;
  } else {
    if (!(mn < mx)) return fail(nullptr, HH_ERR_ARG, f + ": a constant volume has no Otsu threshold (the histogram's range is empty)");
    double edges[257];
    am_edges(mn, mx, edges);
    unsigned long long* const d_counts = s->words + AM_WORDS;
    HH_HIP(nullptr, hipMemcpy(d_edges, edges, sizeof(edges), hipMemcpyHostToDevice));
    HH_HIP(nullptr, hipMemsetAsync(d_counts, 0, 256 * sizeof(unsigned long long), nullptr));
    hipLaunchKernelGGL(k_am_hist, dim3(g), dim3(256), 0, nullptr, lp, n, d_edges, d_counts);
    HH_HIP(nullptr, hipGetLastError());
    unsigned long long counts[256];
    int64_t c64[256];
    HH_HIP(nullptr, hipMemcpy(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost));
    for (int i = 0; i < 256; ++i) c64[i] = (int64_t)counts[i];
    thresh = am_otsu(c64, mn, mx);
  }
  hipLaunchKernelGGL(k_am_above, dim3(g), dim3(256), 0, nullptr, lp, n, thresh, vstar, s->above, s->words);
  HH_HIP(nullptr, hipEventRecord(s->ev[AM_EV_STATS], nullptr));
  if (int rc = am_label(s, nz, ny, nx)) return rc;
  HH_HIP(nullptr, hipMemsetAsync(s->keep, 0, (size_t)n, nullptr));
  hipLaunchKernelGGL(k_am_keep, dim3(g), dim3(256), 0, nullptr, lp, s->above, s->parent, n, vstar, s->keep);
  hipLaunchKernelGGL(k_am_pick, dim3(g), dim3(256), 0, nullptr, s->above, s->parent, s->keep, n, d_support, s->words);
  HH_HIP(nullptr, hipGetLastError());
  HH_HIP(nullptr, hipMemcpy(words, s->words, sizeof(words), hipMemcpyDeviceToHost));
  if (words[AM_W_ERR]) return am_defect_found(fn);
  const bool fallback = words[AM_W_KEPT] == 0;
  if (fallback) HH_HIP(nullptr, hipMemcpyAsync(d_support, s->above, (size_t)n, hipMemcpyDeviceToDevice, nullptr));
  HH_HIP(nullptr, hipEventRecord(s->ev[AM_EV_PICK], nullptr));
  HH_HIP(nullptr, hipEventSynchronize(s->ev[AM_EV_PICK]));
  for (int e = 0; e < 8; ++e) {
    float ms = 0.f;
    HH_HIP(nullptr, hipEventElapsedTime(&ms, s->ev[e], s->ev[e + 1]));
    g_am_stage_ms[e] += ms;
  }
  if (info) {
    info[0] = thresh; info[1] = mn; info[2] = mx; info[3] = vstar;
    info[4] = (double)words[AM_W_ABOVE];
    info[5] = fallback ? (double)words[AM_W_ABOVE] : (double)words[AM_W_KEPT];
    info[6] = (double)words[AM_W_ROOTS];
    info[7] = (double)((fallback ? 1 : 0) | (words[AM_W_GE] > (unsigned long long)AM_SEEDS ? 2 : 0));
  }
  return HH_OK;
}

}  // namespace

// Host only: np.linspace(hmin, hmax, 257) (edges_out, may be NULL) and Otsu's threshold from 256 counts (otsu_threshold_eman's
// arithmetic), the two host steps of the Otsu mode.
extern "C" int hh_am_otsu(const int64_t* counts, double hmin, double hmax, double* edges_out, double* threshold_out) try {
  if (!counts || !threshold_out) return fail(nullptr, HH_ERR_ARG, "hh_am_otsu: NULL argument");
  if (!std::isfinite(hmin) || !std::isfinite(hmax) || hmax < hmin) return fail(nullptr, HH_ERR_ARG, "hh_am_otsu: a finite range hmin <= hmax is needed");
  for (int i = 0; i < 256; ++i)
    if (counts[i] < 0) return fail(nullptr, HH_ERR_ARG, "hh_am_otsu: a negative count");
  if (edges_out) am_edges(hmin, hmax, edges_out);
  *threshold_out = am_otsu(counts, hmin, hmax);
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_am_otsu")

// the device-event times of the mask calls since the last reset: z, y, x passes, statistics, runs, unions, flatten, pick
extern "C" int hh_am_stage_ms(double* out, int reset) try {
  if (out) std::memcpy(out, g_am_stage_ms, sizeof(g_am_stage_ms));
  if (reset) std::memset(g_am_stage_ms, 0, sizeof(g_am_stage_ms));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_am_stage_ms")

extern "C" int hh_am_gaussian_3d(int device, const double* vol, int32_t nz, int32_t ny, int32_t nx, double sigma, const double* taps, double* out) try {
  if (!vol || !taps || !out) return fail(nullptr, HH_ERR_ARG, "hh_am_gaussian_3d: NULL argument");
  if (!am_sides_ok(nz, ny, nx)) return fail(nullptr, HH_ERR_ARG, "hh_am_gaussian_3d: the sides of the box must lie in [1, 1024]");
  const int64_t n = (int64_t)nz * ny * nx;
  if (n > AM_MAX_VOXELS) return fail(nullptr, HH_ERR_ARG, "hh_am_gaussian_3d: more than 2^28 voxels");
  const int r = am_radius(sigma);
  if (r < 0) return fail(nullptr, HH_ERR_ARG, "hh_am_gaussian_3d: sigma must be positive and finite with int(4 sigma + 0.5) <= 4096");
  if (int rc = use_device("hh_am_gaussian_3d", device)) return rc;
  AmScratch s;
  if (int rc = am_reserve(&s, n, true, false, false, false, taps, r)) return rc;
  HH_HIP(nullptr, hipMemcpy(s.a, vol, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  if (int rc = am_filter(&s, nz, ny, nx, r)) return rc;
  HH_HIP(nullptr, hipMemcpy(out, s.b, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_am_gaussian_3d")

extern "C" int hh_am_label_3d(int device, const uint8_t* binary, int32_t nz, int32_t ny, int32_t nx, int32_t* roots_out, int64_t* n_components) try {
  if (!binary || !roots_out || !n_components) return fail(nullptr, HH_ERR_ARG, "hh_am_label_3d: NULL argument");
  if (!am_sides_ok(nz, ny, nx)) return fail(nullptr, HH_ERR_ARG, "hh_am_label_3d: the sides of the box must lie in [1, 1024]");
  const int64_t n = (int64_t)nz * ny * nx;
  if (n > AM_MAX_VOXELS) return fail(nullptr, HH_ERR_ARG, "hh_am_label_3d: more than 2^28 voxels");
  if (int rc = use_device("hh_am_label_3d", device)) return rc;
  AmScratch s;
  if (int rc = am_reserve(&s, n, false, true, false, false, nullptr, 0)) return rc;
  HH_HIP(nullptr, hipMemcpy(s.above, binary, (size_t)n, hipMemcpyHostToDevice));
  if (int rc = am_label(&s, nz, ny, nx)) return rc;
  unsigned long long words[AM_WORDS];
  HH_HIP(nullptr, hipMemcpy(words, s.words, sizeof(words), hipMemcpyDeviceToHost));
  if (words[AM_W_ERR]) return am_defect_found("hh_am_label_3d");
  HH_HIP(nullptr, hipMemcpy(roots_out, s.parent, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  *n_components = (int64_t)words[AM_W_ROOTS];
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_am_label_3d")

extern "C" int hh_am_mask_3d(int device, const void* vol, int is_f64, int32_t nz, int32_t ny, int32_t nx, double sigma, const double* taps, int mode,
                             double value, uint8_t* support_out, double* info) try {
  if (!vol || !support_out) return fail(nullptr, HH_ERR_ARG, "hh_am_mask_3d: NULL argument");
  if (int rc = am_check_threshold_args("hh_am_mask_3d", sigma, taps, mode, value)) return rc;
  if (int rc = am_check_box("hh_am_mask_3d", nz, ny, nx, mode, value)) return rc;
  if (int rc = use_device("hh_am_mask_3d", device)) return rc;
  const int64_t n = (int64_t)nz * ny * nx;
  AmScratch s;
  if (int rc = am_reserve(&s, n, true, true, true, true, sigma != 0.0 ? taps : nullptr, sigma != 0.0 ? am_radius(sigma) : 0)) return rc;
  if (is_f64) {
    HH_HIP(nullptr, hipMemcpy(s.a, vol, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  } else {   // the float32 volume is staged in the second plane and widened into the first
    float* const stage = reinterpret_cast<float*>(s.b.get());
    HH_HIP(nullptr, hipMemcpy(stage, vol, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_am_widen, dim3(am_grid(n, 4096)), dim3(256), 0, nullptr, stage, (const float*)nullptr, s.a, n);
    HH_HIP(nullptr, hipGetLastError());
  }
  if (int rc = am_build("hh_am_mask_3d", &s, nz, ny, nx, sigma, mode, value, s.mask, info)) return rc;
  HH_HIP(nullptr, hipMemcpy(support_out, s.mask, (size_t)n, hipMemcpyDeviceToHost));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_am_mask_3d")

extern "C" int hh_am_context_support(hh_tfsc* ctx, int one_mask, double sigma, const double* taps, int mode, double value, double* info) try {
  if (!ctx) return fail(nullptr, HH_ERR_ARG, "hh_am_context_support: NULL argument");
  if (int rc = am_check_threshold_args("hh_am_context_support", sigma, taps, mode, value)) return rc;
  hh_tfsc* const c = ctx;
  if (int rc = am_check_box("hh_am_context_support", c->n, c->n, c->n, mode, value)) return rc;
  HH_HIP(nullptr, hipSetDevice(c->device));
  if (!c->soft) c->soft = new SmState;
  SmState* const sm = c->soft;
  const int n_sup = one_mask ? 1 : 2;
  const int64_t n = c->per_map;
  if (sm->n_sup != n_sup) {
    sm->sup.reset();
    sm->n_sup = 0;
    if (int rc = ensure(nullptr, sm->sup, (size_t)n_sup * (size_t)n)) return rc;
  }
  AmScratch s;
  if (int rc = am_reserve(&s, n, true, true, true, false, sigma != 0.0 ? taps : nullptr, sigma != 0.0 ? am_radius(sigma) : 0)) return rc;
  sm->n_sup = 0;   // a build that fails leaves the context without a support, not with half of one
  for (int k = 0; k < n_sup; ++k) {
    const float* const first = c->maps + (int64_t)k * n;
    hipLaunchKernelGGL(k_am_widen, dim3(am_grid(n, 4096)), dim3(256), 0, nullptr, first, one_mask ? c->maps + n : (const float*)nullptr, s.a, n);
    HH_HIP(nullptr, hipGetLastError());
    if (int rc = am_build("hh_am_context_support", &s, c->n, c->n, c->n, sigma, mode, value, sm->sup + (int64_t)k * n, info ? info + 8 * k : nullptr)) return rc;
  }
  sm->n_sup = n_sup;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_am_context_support")

extern "C" int hh_am_context_get_support(hh_tfsc* ctx, int which, uint8_t* support_out) try {
  if (!ctx || !support_out) return fail(nullptr, HH_ERR_ARG, "hh_am_context_get_support: NULL argument");
  if (which < 0 || which > 1) return fail(nullptr, HH_ERR_ARG, "hh_am_context_get_support: which must be 0 or 1");
  hh_tfsc* const c = ctx;
  SmState* const sm = c->soft;
  if (!sm || sm->n_sup < 1) return fail(nullptr, HH_ERR_STATE, "hh_am_context_get_support: no support is set");
  HH_HIP(nullptr, hipSetDevice(c->device));
  HH_HIP(nullptr, hipMemcpy(support_out, sm->sup + (sm->n_sup == 2 ? which : 0) * c->per_map, (size_t)c->per_map, hipMemcpyDeviceToHost));
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_am_context_get_support")
