// path_a_batch.inc — Path A for MANY candidates at once, resident on the device (included by helicon_hip.hip after
// path_a_host.inc; uses its geometry, symmetry-pair and rotation helpers).
//
// Reference: webApps/denovo3D/solver_linear_regression.py:31-547 (lsq_reconstruct), :205-269 (solve_equations ->
// scipy.optimize.lsq_linear(method="trf", lsq_solver="lsmr", tol=1e-2, max_iter=200, lsmr_maxiter=1000,
// lsmr_tol="auto")), :484-530 (cosine score); scipy/optimize/_lsq/trf_linear.py and scipy/sparse/linalg/_isolve/lsmr.py
// are the algorithms restated (they are third-party code, scipy 1.15.3; the restatement is pinned through
// oracle/path_a.py and the reference's own lsq_reconstruct outputs, fixtures G5 / G9 / G11).
//
// One hh_pab holds K candidates of ONE image and ONE reconstruction box (K (twist, rise, csym, tilt, psi, dy) tuples:
// what the reference's thread pool hands to K process_one_task calls, app.py:2473-2476).  Every phase of the solve is
// one launch for all K candidates (grid.y = candidate):
//   * A x, A^T y  (tilt = psi = 0, the app's own setting, app.py:2344-2346)  k_pabs_matvec / k_pabs_rmatvec: every ray
//              of (operation o, image column k) lies in ONE z slice of the cylinder, and the voxels of a slice are
//              contiguous in rank order.  Rows are kept slice-major, a workgroup owns one slice: it stages the slice of x
//              in LDS (coalesced) and gathers there (A x), or accumulates the slice of A^T y in LDS in 64-bit fixed
//              point (integer atomics: one result whatever the order) from the same compact uint16 map — the divergent
//              8-byte gathers that bound the first version (546k per product, one L1 line each) never leave the CU.
//              Symmetry rows connect slices: A x gathers them from L2, A^T y through their transposed lists.
//   * A x, A^T y  (any tilt / psi)  k_pab_matvec gathers along the int32 map from L2; k_pab_rmatvec gathers along the
//              transposed pattern (voxel -> rows, CSR, lists sorted by row) built on the device at create
//   * LSMR     one iteration = forward product (+ u update + |u|^2), transposed product (+ v update + |v|^2), the
//              h / hbar / x update (+ |x|^2), each followed by a one-wavefront-per-candidate scalar kernel holding the
//              Golub-Kahan / rotation recurrences and the stopping tests; a converged candidate's blocks exit at once
//   * lsq_linear's trust-region-reflective iteration: scaling vectors, the three trial steps and their 1-D quadratic
//     models, backtracking, feasibility — the same vector / scalar kernel pair with a lambda per step
// The host only queues launches; it reads one word ("is any candidate still iterating?") every few LSMR iterations and
// once per trust-region iteration.  Norms and inner products are per-block partial sums reduced in index order by the
// scalar kernels: a solve is bit-reproducible for a given batch composition... and, because no quantity of one
// candidate depends on another's, for any batch composition.

namespace {

// A candidate's place in lsq_linear.  Candidates of a group advance independently: every kernel of the solve is masked by
// this, and a pass of the host loop launches each phase's kernels once (those that have candidates) and a few LSMR
// iterations for everyone who is inside a solve.
enum PabPhase { PH_LSMR0 = 0, PH_AFTER0, PH_PRE, PH_LSMR, PH_POST, PH_BT, PH_FIN, PH_DONE, PH_COUNT };
constexpr int PAB_VEC_ELEMS = 4;     // elements per thread of the element-wise kernels (k_pab_vec)
constexpr int PABS_TAIL_ROWS = 8;    // symmetry / augmented rows per thread in the sliced forward product
constexpr int PAB_FLAG_WORDS = 16;   // [0, PH_COUNT): candidates per phase (k_pab_count_phases); [8]: self-check failures
constexpr int PAB_SLOTS = 8;
constexpr int PAB_TRACE_ROWS = 8192;        // reduction slots per candidate
constexpr int PAB_LANES = 16;       // lanes sharing one projection ray in A x

// n-sized vectors
enum { NV_X, NV_G, NV_VS, NV_DG, NV_D, NV_ROOT, NV_GH, NV_PH, NV_P, NV_RH, NV_RR, NV_ST, NV_XN, NV_LV, NV_LH, NV_LHBAR, NV_LX, NV_XF,
       NV_COUNT };
// m-sized vectors (allocated with room for the n augmented rows)
enum { MV_B, MV_R, MV_LU, MV_T1, MV_T2, MV_COUNT };

struct alignas(128) PabState {   // one cache line set per candidate: neighbours are written by other workgroups (other XCDs)
  // the problem
  int64_t m_data, m_sym, row0, sym0, t0;
  double lb, ub, bmax;
  int bounded, clip;
  // LSMR
  int phase, aug, start;   // where the candidate is in lsq_linear (PabPhase); LSMR operator is [A diag(d); diag(root)]; LSMR to be started
  int run, l_on, l_skip, pend, istop, itn;
  double colsum, fx_scale, fx_inv, fx_scale_r, fx_inv_r, rmax;   // fixed-point scales of the sliced A^T y (unit vectors / residual)
  double atol, btol, normb, alpha, beta, inv_alpha, inv_beta, neg_alpha, neg_beta;
  double zetabar, alphabar, rho, rhobar, cbar, sbar, betadd, betad, rhodold, tautildeold, thetatilde, zeta, dsum;
  double normA2, maxrbar, minrbar, normx, normr, normar, normA, condA;
  double c_hbar, c_x, c_h;
  // trust region
  int t_on, status, pending, has_pending, n_outer, inb, rsu_pos, choice, bt, bt_on, bt_fix, lsmr_calls, lsmr_iters, first_iters;
  double g_norm, theta, ltol, p_dot_g, p_stride, r_su, r_sl, r_stride, r_value, p_value, ag_su, ag_stride, ag_value, cost,
      cost_change, bt_alpha;
  double score;
  // proximal-gradient solver of the scikit-learn models (hh_pab_solve_prox)
  int p_it, p_conv, p_nnz, p_pad;
  double p_alpha, p_rho, p_L, p_t, p_beta, p_mu_w, p_sum, p_rn2, p_ybar, p_lam, p_obj, p_dw, p_wmax, p_lam0;
};

struct PabView {
  int K, d2, d2p;        // d2p: row stride of map16 (d2 rounded up to 64 samples)
  int trace_c;           // debugging (HH_PAB_TRACE=c): candidate whose stopping-test inputs are recorded, else -1
  double* trace;         // [PAB_TRACE_ROWS][8]
  int fence;             // debugging (HH_PAB_FENCE): agent-scope acquire at the start and release at the end of every kernel
  int sliced, mz, nslice;
  const int* list;       // candidates of THIS launch: slot s of the grid works on candidate list[s] (NULL: candidate s)
  int n_list;            // slots in the launch
  int64_t n, N, MA;
  PabState* st;
  unsigned* ctl;         // [K] pab_ctl_pack of every candidate's state
  double* nv;
  double* mv;
  const int* map;        // [sum m_data][d2]                       (general path)
  const uint16_t* map16; // [sum m_data][d2] index inside the slice (sliced path; 0xFFFF = outside the cylinder)
  const int* maprow;     // [sum m_data] the row of map16 a data row reads (sliced path): rows of one operation and image row share one, see k_pab_share_rows
  const int* srow;       // [K][mz + 1] rows of slice z: [srow[z], srow[z + 1])  (sliced path: rows are slice-major)
  const int2* pairs;     // [sum m_sym]
  const int* tptr;       // [K][n + 1]
  const int* tent;       // [sum nnz]: row, top bit = negative sign (sliced path: symmetry rows only)
  // trilinear projector (path_a_linear.inc)
  int linear;
  const PaGeom* lin_geom;      // [K]
  const PaOp* lin_ops;         // concatenated
  const int64_t* lin_op0;      // [K]
  const int* ray_of_row;       // [sum m_data] ray (o * L2 + k) * D2 + j of every data row, device (slice-major) order
  const unsigned* sidx2;       // [my * mx] in-plane index of (y, x) | (y, x + 1) << 16, 0xFFFF outside the disc
  const PaEll16* sym16;        // [sum m_sym]
  const int2* tent2;           // [sum nnz] transposed symmetry lists: (row, float32 weight bits)
  long long* acc64;            // [K][N] fixed-point accumulator of A^T y (zero between products)
  // separable form of the trilinear data rows (path_a_factored.inc)
  int fac_G, fac_ng, fac_max_gl, fac_max_lists;   // home layers per group (0: direct kernels), groups, strides of the tables
  int fac_split;                                  // workgroups per group (its columns dealt out)
  const int* fac_ngl;                    // [K][ng] lists present in a group
  const struct PabfGroupList* fac_gl;    // [K][ng][max_gl]
  const struct PabfEntry* fac_entries;   // [K][max_lists][D2][D2]
  const unsigned char* fac_count;        // [K][max_lists][D2]
  int fwd_main;                // blocks of a forward product that own planes of x (the deferred update's self-check)
  // banded form of the trilinear data rows (path_a_banded.inc): T bands of disc rows per home layer
  int band_T;                  // bands (0: not this form)
  const int* band_y;           // [T + 1] first disc row of every band (band_y[T] = my)
  const int* band_v;           // [my + 1] in-plane index of the first voxel of every disc row
  double* bpart;               // [K][T][bstride] the bands' parts of the data rows of A x
  int64_t bstride;
  double* red;           // [K][PAB_SLOTS][RB]
  int RB;
  int* flags;            // [4]
  __device__ __forceinline__ double* nvec(int id, int c) const { return nv + ((size_t)id * K + c) * N; }
  __device__ __forceinline__ double* mvec(int id, int c) const { return mv + ((size_t)id * K + c) * MA; }
  __device__ __forceinline__ double* redp(int c, int slot) const { return red + ((size_t)c * PAB_SLOTS + slot) * RB; }
};

// Launch shape of every per-candidate kernel: grid = (8, blocks, ceil(slots / 8)); slot s = blockIdx.x + 8 blockIdx.z works
// on candidate list[s].  A launch covers only the candidates that have something to do in it (round 4): the host keeps,
// per pass of the solve, the list of candidates that are not finished and the list of those outside an LSMR solve
// (k_pab_lists), and sizes the grid by the list.  Before, every launch covered all K candidates of the group and the
// workgroups of the (on average 86 %) idle ones left after reading their control word — at K = 256 that was 31,000
// workgroups per launch doing nothing, and it is what kept groups small and made the tail of a group (its slowest
// candidate iterates 7 x the average) the wall time.
// Placement: workgroups are dealt to the 8 XCDs round-robin by linear id, whose fastest index is blockIdx.x, so all
// workgroups of a slot (and its scalar steps, grid = slots: workgroup s -> XCD s % 8) share an XCD and its L2 during a
// pass.  That is a locality measure only; CORRECTNESS does not rest on it: every per-candidate array starts on a 128-byte
// line (PabState alignas(128), N and M multiples of 64 doubles), vectors cross launches through the launch boundary's
// release / acquire, and the small words every workgroup of the next launch reads first — control word, state, partial
// sums — are written and read with agent-scope atomics (they bypass the compute unit's scalar and vector caches: see
// pab_state_load).  A candidate may sit on another slot, hence another XCD, in the next pass.
#define PAB_SLOT ((int)(blockIdx.x + 8 * blockIdx.z))
#define PAB_CAND (PAB_SLOT < w.n_list ? (w.list ? w.list[PAB_SLOT] : PAB_SLOT) : -1)
#define PAB_BLOCK ((int)blockIdx.y)
#define PAB_NBLOCKS ((int)gridDim.y)
inline dim3 pab_grid(int blocks, int slots) { return dim3(8, (unsigned)blocks, (unsigned)((slots + 7) / 8)); }

// A workgroup's partial result: neighbouring workgroups write neighbouring 8-byte words of one cache line, possibly from
// different XCDs, whose L2s are not coherent with each other — the store is an agent-scope atomic (write-through, the
// line is not kept dirty in the writer's L2), so a later write-back of that L2 cannot carry a stale copy of a
// neighbour's word over the neighbour's new one.
__device__ __forceinline__ void pab_store_partial(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The per-candidate state is small, hot and rewritten by every scalar step.  A workgroup never reads it with plain
// loads: those may be served from a cache of THIS compute unit (scalar or vector) that still holds the line as it was
// two launches ago, when the same step last ran here — seen as a lost update of the test-only LSMR recurrences
// (dsum, betad, ...: `normr` off by one iteration, nothing else) in about one candidate-solve in a thousand at K = 256.
// So: every workgroup copies the state into LDS with agent-scope loads, the scalar steps write it back with agent-scope
// stores.
// The few state bits every kernel's predicate looks at, packed into one word per candidate (PabView::ctl): a workgroup
// reads it first (one agent-scope load, the same address for all lanes) and leaves at once when its candidate has nothing
// to do in this launch; only the workgroups that stay pay for the copy of the whole state.  The scalar steps refresh it.
struct PabCtl {
  int phase, l_on, l_skip, pend, start, t_on, inb, rsu_pos, bt_on, bt_fix;
};
__device__ __forceinline__ unsigned pab_ctl_pack(const PabState& s) {
  return (unsigned)s.phase | (s.l_on ? 1u << 4 : 0) | (s.l_skip ? 1u << 5 : 0) | (s.pend ? 1u << 6 : 0) | (s.start ? 1u << 7 : 0) |
         (s.t_on ? 1u << 8 : 0) | (s.inb ? 1u << 9 : 0) | (s.rsu_pos ? 1u << 10 : 0) | (s.bt_on ? 1u << 11 : 0) | (s.bt_fix ? 1u << 12 : 0);
}
__device__ __forceinline__ PabCtl pab_ctl_load(const unsigned* ctl, int c) {
  const unsigned k = __hip_atomic_load(const_cast<unsigned*>(ctl + c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return PabCtl{(int)(k & 15u), (int)((k >> 4) & 1), (int)((k >> 5) & 1), (int)((k >> 6) & 1), (int)((k >> 7) & 1), (int)((k >> 8) & 1),
                (int)((k >> 9) & 1), (int)((k >> 10) & 1), (int)((k >> 11) & 1), (int)((k >> 12) & 1)};
}
static_assert(sizeof(PabState) % 8 == 0, "PabState is copied in 8-byte words");
__device__ __forceinline__ void pab_state_load(PabState* lds, const PabState* src) {
  const unsigned long long* g = reinterpret_cast<const unsigned long long*>(src);
  unsigned long long* l = reinterpret_cast<unsigned long long*>(lds);
  for (int i = threadIdx.x; i < (int)(sizeof(PabState) / 8); i += blockDim.x)
    l[i] = __hip_atomic_load(const_cast<unsigned long long*>(g + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
}
__device__ __forceinline__ void pab_state_store(PabState* dst, const PabState* lds) {
  __syncthreads();
  unsigned long long* g = reinterpret_cast<unsigned long long*>(dst);
  const unsigned long long* l = reinterpret_cast<const unsigned long long*>(lds);
  for (int i = threadIdx.x; i < (int)(sizeof(PabState) / 8); i += blockDim.x)
    __hip_atomic_store(g + i, l[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
enum { RED_SUM = 0, RED_MIN = 1, RED_MAX = 2 };
template <int NRED>
struct PabRed {
  int kind[NRED > 0 ? NRED : 1];
  int slot[NRED > 0 ? NRED : 1];
  int nb[NRED > 0 ? NRED : 1];
};
__device__ __forceinline__ double pab_ident(int kind) { return kind == RED_SUM ? 0.0 : kind == RED_MIN ? INFINITY : -INFINITY; }
__device__ __forceinline__ double pab_comb(int kind, double a, double b) {
  return kind == RED_SUM ? a + b : kind == RED_MIN ? fmin(a, b) : fmax(a, b);
}
// block of 256 -> one value in thread 0, fixed tree
__device__ __forceinline__ double pab_block_reduce(int kind, double v, double* lds4) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = pab_comb(kind, v, __shfl_down(v, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return pab_comb(kind, pab_comb(kind, lds4[0], lds4[1]), pab_comb(kind, lds4[2], lds4[3]));
}
// block of PABS_THREADS (16 wavefronts) -> one value, fixed tree; lds16: 16 doubles
constexpr int PABS_THREADS = 1024;   // workgroup of the sliced products: 16 wavefronts share one staged slice
constexpr int PABS_LANES = 8;        // lanes per projection ray there: 8 samples (one 16-byte load of the map) per lane and step
__device__ __forceinline__ double pabs_block_reduce(int kind, double v, double* lds16) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = pab_comb(kind, v, __shfl_down(v, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds16[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = lds16[0];
#pragma unroll
  for (int k = 1; k < PABS_THREADS / 64; ++k) r = pab_comb(kind, r, lds16[k]);
  return r;
}

// ---- generic element-wise step: body(c, i, state, acc[]) for i < count(c), per-block partial reductions -------------
enum { CNT_N = 0, CNT_M = 1, CNT_MDATA = 2, CNT_MAUG = 3 };
template <int NRED, class P, class F>
__global__ __launch_bounds__(256) void k_pab_vec(PabView w, int count_kind, PabRed<NRED> red, P pred, F body) {
  const int c = PAB_CAND, bx = PAB_BLOCK, nbx = PAB_NBLOCKS;
  if (c < 0) return;
  if (w.fence > 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (!pred(pab_ctl_load(w.ctl, c))) return;
  __shared__ PabState s_lds;
  pab_state_load(&s_lds, &w.st[c]);
  const PabState& s = s_lds;
  __shared__ double lds4[4];
  double acc[NRED > 0 ? NRED : 1];
#pragma unroll
  for (int k = 0; k < NRED; ++k) acc[k] = pab_ident(red.kind[k]);
  const int64_t cnt = count_kind == CNT_N ? w.n : count_kind == CNT_M ? s.m_data + s.m_sym : count_kind == CNT_MDATA ? s.m_data
                                                                                                : s.m_data + s.m_sym + w.n;
  // a workgroup owns PAB_VEC_ELEMS x 256 consecutive elements (its number, not the grid's size, decides which: what a
  // candidate's partial sums are must not depend on the other candidates of the batch)
#pragma unroll
  for (int u = 0; u < PAB_VEC_ELEMS; ++u) {
    const int64_t i = ((int64_t)bx * PAB_VEC_ELEMS + u) * 256 + threadIdx.x;
    if (i < cnt) body(w, c, i, s, acc);
  }
#pragma unroll
  for (int k = 0; k < NRED; ++k) {
    const double v = pab_block_reduce(red.kind[k], acc[k], lds4);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, red.slot[k])[bx], v);
  }
}

// ---- generic scalar step: one wavefront per candidate reduces the partials in index order, lane 0 runs the body -------
template <int NRED, class P, class F>
__global__ __launch_bounds__(64) void k_pab_scalar(PabView w, PabRed<NRED> red, P pred, F body) {
  if ((int)blockIdx.x >= w.n_list) return;
  const int c = w.list ? w.list[blockIdx.x] : (int)blockIdx.x;
  if (w.fence) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (!pred(pab_ctl_load(w.ctl, c))) return;
  __shared__ PabState s_lds;
  pab_state_load(&s_lds, &w.st[c]);
  PabState& s = s_lds;
  double val[NRED > 0 ? NRED : 1];
#pragma unroll
  for (int k = 0; k < NRED; ++k) {
    const double* p = w.redp(c, red.slot[k]);
    double v = pab_ident(red.kind[k]);
    // agent-scope loads: the partials were written by other workgroups in the previous launch; a plain load may be served
    // from this CU's vector L1, which holds the PREVIOUS iteration's value of the same word when this step ran here then
    for (int i = threadIdx.x; i < red.nb[k]; i += 64)
      v = pab_comb(red.kind[k], v, __hip_atomic_load(const_cast<double*>(&p[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = pab_comb(red.kind[k], v, __shfl_down(v, off, 64));
    val[k] = v;
  }
  if (threadIdx.x == 0) {
    body(w, c, s, val);
    __hip_atomic_store(w.ctl + c, pab_ctl_pack(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  pab_state_store(&w.st[c], &s_lds);
  if (w.fence) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
}

// ---- A x (nearest neighbour) -------------------------------------------------------------------------------------------
// MODE 0: dst = Op src.  MODE 1 (LSMR): dst = (dst inv_beta) neg_alpha + Op src, |dst|^2 -> slot 0.
// MODE 2 (residual): dst = A src - b, |dst|^2 -> slot 0.   Op = [A diag(d); diag(root)] when dsc / rootv >= 0.
template <int MODE, class P>
__global__ __launch_bounds__(256) void k_pab_matvec(PabView w, int src, int dsc, int rootv, int dst, P pred) {
#pragma clang fp contract(off)
  const int c = PAB_CAND, bx = PAB_BLOCK, nbx = PAB_NBLOCKS;
  if (c < 0) return;
  if (w.fence > 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (!pred(pab_ctl_load(w.ctl, c))) return;
  __shared__ PabState s_lds;
  pab_state_load(&s_lds, &w.st[c]);
  const PabState& s = s_lds;
  __shared__ double lds4[4];
  const bool op_aug = MODE != 1 || s.aug;   // LSMR: the candidate's own operator (plain first solve / trust-region step)
  const double* __restrict__ x = w.nvec(src, c);
  const double* __restrict__ d = dsc >= 0 && op_aug ? w.nvec(dsc, c) : nullptr;
  const double* __restrict__ root = rootv >= 0 && op_aug ? w.nvec(rootv, c) : nullptr;
  double* __restrict__ y = w.mvec(dst, c);
  const int64_t t = (int64_t)bx * 256 + threadIdx.x;
  const int64_t nd = s.m_data * PAB_LANES;
  double sq = 0;
  int64_t r = -1;
  double val = 0;
  if (t < nd) {
    const int64_t row = t / PAB_LANES;
    const int l = (int)(t % PAB_LANES);
    const int* __restrict__ p = w.map + (size_t)(s.row0 + row) * w.d2;
    double acc = 0;
    for (int i = l; i < w.d2; i += PAB_LANES) {
      const int v = p[i];
      if (v >= 0) {
        const double xv = MODE == 1 ? x[v] * s.inv_alpha : x[v];
        acc += d ? xv * d[v] : xv;
      }
    }
#pragma unroll
    for (int off = PAB_LANES / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, PAB_LANES);
    if (l == 0) { r = row; val = acc; }
  } else {
    const int64_t q = s.m_data + (t - nd);
    if (q < s.m_data + s.m_sym) {
      const int2 pr = w.pairs[s.sym0 + (q - s.m_data)];
      const double xa = MODE == 1 ? x[pr.x] * s.inv_alpha : x[pr.x], xb = MODE == 1 ? x[pr.y] * s.inv_alpha : x[pr.y];
      const double a = d ? xa * d[pr.x] : xa, b = d ? xb * d[pr.y] : xb;
      r = q; val = a - b;
    } else if (root && q < s.m_data + s.m_sym + w.n) {
      const int64_t v = q - s.m_data - s.m_sym;
      r = q; val = root[v] * (MODE == 1 ? x[v] * s.inv_alpha : x[v]);
    }
  }
  if (r >= 0) {
    if (MODE == 1) val = (y[r] * s.inv_beta) * s.neg_alpha + val;
    if (MODE == 2) val = val - w.mvec(MV_B, c)[r];
    y[r] = val;
    sq = val * val;
  }
  if (MODE != 0) {
    const double v = pab_block_reduce(RED_SUM, sq, lds4);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 0)[bx], v);
  }
}

// ---- A^T y as a gather over the transposed pattern ----------------------------------------------------------------------
// MODE 0: dst = A^T y[:m].  MODE 1 (LSMR): dst = dst neg_beta + Op^T (y inv_beta), |dst|^2 -> slot 1.
template <int MODE, class P>
__global__ __launch_bounds__(256) void k_pab_rmatvec(PabView w, int src, int dsc, int rootv, int dst, P pred) {
#pragma clang fp contract(off)
  const int c = PAB_CAND, bx = PAB_BLOCK, nbx = PAB_NBLOCKS;
  if (c < 0) return;
  if (w.fence > 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (!pred(pab_ctl_load(w.ctl, c))) return;
  __shared__ PabState s_lds;
  pab_state_load(&s_lds, &w.st[c]);
  const PabState& s = s_lds;
  __shared__ double lds4[4];
  const double* __restrict__ y = w.mvec(src, c);
  double* __restrict__ g = w.nvec(dst, c);
  const int* __restrict__ tp = w.tptr + (size_t)c * (w.n + 1);
  const int* __restrict__ te = w.tent + s.t0;
  const double sc = MODE == 1 ? s.inv_beta : 1.0;
  double sq = 0;
  for (int64_t v = (int64_t)bx * 256 + threadIdx.x; v < w.n; v += (int64_t)nbx * 256) {
    double acc = 0;
    const int e1 = tp[v + 1];
    for (int e = tp[v]; e < e1; ++e) {
      const int ent = te[e];
      const double yy = MODE == 1 ? y[ent & 0x7fffffff] * sc : y[ent & 0x7fffffff];
      acc += ent < 0 ? -yy : yy;
    }
    if (dsc >= 0 && (MODE != 1 || s.aug)) acc *= w.nvec(dsc, c)[v];
    if (rootv >= 0 && (MODE != 1 || s.aug)) {
      const double tail = y[s.m_data + s.m_sym + v];
      acc += w.nvec(rootv, c)[v] * (MODE == 1 ? tail * sc : tail);
    }
    if (MODE == 1) acc = (g[v] * s.inv_alpha) * s.neg_beta + acc;
    g[v] = acc;
    sq += acc * acc;
  }
  if (MODE == 1) {
    const double r = pab_block_reduce(RED_SUM, sq, lds4);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 1)[bx], r);
  }
}

// the h / hbar / x update of the LSMR iteration whose coefficients are in the state (deferred to the next forward
// product, which reads v anyway): v = the normalised v of that iteration; returns the new x
__device__ __forceinline__ double pab_deferred_update(const PabView& w, int c, int64_t gi, const PabState& s, double v) {
#pragma clang fp contract(off)
  double hbar = w.nvec(NV_LHBAR, c)[gi] * s.c_hbar;
  const double h = w.nvec(NV_LH, c)[gi];
  hbar = hbar + h;
  const double x = w.nvec(NV_LX, c)[gi] + s.c_x * hbar;
  double hn = h * s.c_h;
  hn = hn + v;
  w.nvec(NV_LHBAR, c)[gi] = hbar;
  w.nvec(NV_LX, c)[gi] = x;
  w.nvec(NV_LH, c)[gi] = hn;
  return x;
}

// ---- the sliced products (tilt = psi = 0): one workgroup per z slice ---------------------------------------------------
// Map rows are padded to d2p = a multiple of 64 samples (0xFFFF beyond d2): a lane takes 8 consecutive samples with one
// 16-byte load, 8 lanes a step of 64 samples, and a wavefront's loads of a step are one contiguous kilobyte.
__device__ __forceinline__ void pabs_unpack(const uint4& q, unsigned m[8]) {
  m[0] = q.x & 0xffffu; m[1] = q.x >> 16; m[2] = q.y & 0xffffu; m[3] = q.y >> 16;
  m[4] = q.z & 0xffffu; m[5] = q.z >> 16; m[6] = q.w & 0xffffu; m[7] = q.w >> 16;
}

// A x.  MODE 0: dst = Op src.  MODE 1 (LSMR): src is v un-normalised (v = src inv_alpha); with st.pend the deferred
// h / hbar / x update runs while the slice is staged (|x|^2 -> slot 2); dst = (dst inv_beta) neg_alpha + Op v, |dst|^2
// -> slot 0.  MODE 2: dst = A src - b, |dst|^2 -> slot 0, max |dst| -> slot 1.
template <int MODE, class P>
__global__ __launch_bounds__(PABS_THREADS) void k_pabs_matvec(PabView w, int src, int dsc, int rootv, int dst, P pred) {
#pragma clang fp contract(off)
  const int c = PAB_CAND, bx = PAB_BLOCK, nbx = PAB_NBLOCKS;
  if (c < 0) return;
  if (w.fence > 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (!pred(pab_ctl_load(w.ctl, c))) return;
  __shared__ PabState s_lds;
  pab_state_load(&s_lds, &w.st[c]);
  const PabState& s = s_lds;
  extern __shared__ double xs[];   // [nslice]
  __shared__ double lds16[PABS_THREADS / 64];
  const bool op_aug = MODE != 1 || s.aug;   // LSMR: the candidate's own operator (plain first solve / trust-region step)
  const double* __restrict__ x = w.nvec(src, c);
  const double* __restrict__ d = dsc >= 0 && op_aug ? w.nvec(dsc, c) : nullptr;
  const double* __restrict__ root = rootv >= 0 && op_aug ? w.nvec(rootv, c) : nullptr;
  double* __restrict__ y = w.mvec(dst, c);
  double sq = 0, sqx = 0, mx = 0;
  if (bx < w.mz) {
    const int z = bx;
    const int64_t base = (int64_t)z * w.nslice;
    const int* __restrict__ sr = w.srow + (size_t)c * (w.mz + 1);
    const int r0 = sr[z], r1 = sr[z + 1];
    const int l = threadIdx.x & (PABS_LANES - 1), slot = threadIdx.x / PABS_LANES;
    constexpr int ROWS = PABS_THREADS / PABS_LANES;   // rows per pass
    const int steps = w.d2p / 64;
    // the first pass's operands are requested before the slice is staged
    int r = r0 + slot;
    // (a row reads the map of maprow[row]: the rows of one operation and image row share a copy; the index for the pass after
    // next is asked for a pass ahead, so that the map load of the next pass does not wait for it)
    const int* __restrict__ mrow = w.maprow + s.row0;
    int mr0 = r < r1 ? mrow[r] : 0, mr1 = r + ROWS < r1 ? mrow[r + ROWS] : 0;
    const uint4* __restrict__ mp = reinterpret_cast<const uint4*>(w.map16 + (size_t)mr0 * w.d2p) + l;
    uint4 q = make_uint4(~0u, ~0u, ~0u, ~0u);
    double yold = 0, bold = 0;
    if (r < r1) {
      q = mp[0];
      if (MODE == 1 && l == 0) yold = y[r];
      if (MODE == 2 && l == 0) bold = w.mvec(MV_B, c)[r];
    }
    // (element by element: two or four elements per thread asked for together were built and compared back to back on one box —
    // four take the kernel from 44 to 86 VGPRs and from two workgroups per compute unit to one; two, under a 64-VGPR cap with 28
    // bytes of scratch: 1,024 candidates 1.355 -> 1.40 s)
    for (int v = threadIdx.x; v < w.nslice; v += PABS_THREADS) {
      const int64_t gi = base + v;
      double xv = x[gi];
      if (MODE == 1) {
        xv = xv * s.inv_alpha;
        if (s.pend) {
          const double xn = pab_deferred_update(w, c, gi, s, xv);
          sqx += xn * xn;
        }
      }
      xs[v] = d ? xv * d[gi] : xv;
    }
    __syncthreads();
    for (int rb = r0; rb < r1; rb += ROWS) {
      r = rb + slot;
      const int mr2 = r + 2 * ROWS < r1 ? mrow[r + 2 * ROWS] : 0;
      double acc = 0;
      uint4 qn = make_uint4(~0u, ~0u, ~0u, ~0u);
      double yn = 0, bn = 0;
      for (int st = 0; st < steps; ++st) {
        // next operand: the next step of this row, or the first step of the next pass's row
        const bool last = st + 1 == steps;
        const int rn = last ? r + ROWS : r;
        if (rn < r1) {
          const uint4* __restrict__ np = reinterpret_cast<const uint4*>(w.map16 + (size_t)(last ? mr1 : mr0) * w.d2p) + l + (last ? 0 : (st + 1) * PABS_LANES);
          qn = *np;
          if (last && l == 0) {
            if (MODE == 1) yn = y[rn];
            if (MODE == 2) bn = w.mvec(MV_B, c)[rn];
          }
        } else {
          qn = make_uint4(~0u, ~0u, ~0u, ~0u);
        }
        unsigned m[8];
        pabs_unpack(q, m);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (m[k] != 0xffffu) acc += xs[m[k]];
        q = qn;
      }
#pragma unroll
      for (int off = PABS_LANES / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, PABS_LANES);
      if (l == 0 && r < r1) {
        double val = acc;
        if (MODE == 1) val = (yold * s.inv_beta) * s.neg_alpha + val;
        if (MODE == 2) val = val - bold;
        y[r] = val;
        sq += val * val;
        mx = fmax(mx, fabs(val));
      }
      yold = yn;
      bold = bn;
      mr0 = mr1;
      mr1 = mr2;
    }
  } else {
#pragma unroll
    for (int u = 0; u < PABS_TAIL_ROWS; ++u) {
      const int64_t qi = s.m_data + (((int64_t)(bx - w.mz) * PABS_TAIL_ROWS + u) * PABS_THREADS + threadIdx.x);
      int64_t r = -1;
      double val = 0;
      if (qi < s.m_data + s.m_sym) {
        const int2 pr = w.pairs[s.sym0 + (qi - s.m_data)];
        const double xa = MODE == 1 ? x[pr.x] * s.inv_alpha : x[pr.x], xb = MODE == 1 ? x[pr.y] * s.inv_alpha : x[pr.y];
        const double a = d ? xa * d[pr.x] : xa, b = d ? xb * d[pr.y] : xb;
        r = qi; val = a - b;
      } else if (root && qi < s.m_data + s.m_sym + w.n) {
        const int64_t v = qi - s.m_data - s.m_sym;
        r = qi; val = root[v] * (MODE == 1 ? x[v] * s.inv_alpha : x[v]);
      }
      if (r >= 0) {
        if (MODE == 1) val = (y[r] * s.inv_beta) * s.neg_alpha + val;
        if (MODE == 2) val = val - w.mvec(MV_B, c)[r];
        y[r] = val;
        sq += val * val;
        mx = fmax(mx, fabs(val));
      }
    }
  }
  if (MODE != 0) {
    const double v = pabs_block_reduce(RED_SUM, sq, lds16);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 0)[bx], v);
  }
  if (MODE == 1) {
    const double v = pabs_block_reduce(RED_SUM, sqx, lds16);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 2)[bx], v);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 3)[bx], (bx < w.mz && s.pend) ? 1.0 : 0.0);   // self-check, see scalar 1
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 4)[bx], (double)s.itn);                        // self-check: freshness tag
  }
  if (MODE == 2) {
    const double v = pabs_block_reduce(RED_MAX, mx, lds16);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 1)[bx], v);
  }
}

// A^T y.  The slice of the result is accumulated in LDS as 64-bit fixed point from the forward map (integer atomics:
// associative, one result for any order); the scale is a power of two from the largest column sum of |A_data| and the
// bound on |y| (1 for LSMR's unit vectors, max |r| for the residual).  Symmetry rows through their transposed lists.
// MODE 0: dst = A^T y[:m] (scale st.fx_scale_r).  MODE 1 (LSMR): dst = (dst inv_alpha) neg_beta + Op^T (y inv_beta),
// |dst|^2 -> slot 1.  ABSCOUNT: count hits per voxel instead, the slice's largest count -> atomicMax(colmax[c]).
template <int MODE, bool ABSCOUNT, class P>
__global__ __launch_bounds__(PABS_THREADS) void k_pabs_rmatvec(PabView w, int src, int dsc, int rootv, int dst, int* __restrict__ colmax, P pred) {
#pragma clang fp contract(off)
  const int c = PAB_CAND, bx = PAB_BLOCK, nbx = PAB_NBLOCKS;
  if (c < 0) return;
  if (w.fence > 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (!pred(pab_ctl_load(w.ctl, c))) return;
  __shared__ PabState s_lds;
  pab_state_load(&s_lds, &w.st[c]);
  const PabState& s = s_lds;
  extern __shared__ long long accs[];   // [nslice]
  __shared__ double lds16[PABS_THREADS / 64];
  const int z = bx;
  const int64_t base = (int64_t)z * w.nslice;
  const double* __restrict__ y = ABSCOUNT ? nullptr : w.mvec(src, c);
  const double sc = MODE == 1 ? s.inv_beta : 1.0;
  const double scale = ABSCOUNT ? 1.0 : MODE == 1 ? s.fx_scale : s.fx_scale_r;
  const double inv_scale = ABSCOUNT ? 1.0 : MODE == 1 ? s.fx_inv : s.fx_inv_r;
  const int* __restrict__ sr = w.srow + (size_t)c * (w.mz + 1);
  const int r0 = sr[z], r1 = sr[z + 1];
  const int l = threadIdx.x & (PABS_LANES - 1), slot = threadIdx.x / PABS_LANES;
  constexpr int ROWS = PABS_THREADS / PABS_LANES;
  const int steps = w.d2p / 64;
  // first operands in flight while the accumulator is cleared
  uint4 q = make_uint4(~0u, ~0u, ~0u, ~0u);
  double yv = 0;
  // (shared map rows: see k_pabs_matvec; without the table every row reads its own map)
  const int* __restrict__ mrow = w.maprow ? w.maprow + s.row0 : nullptr;
  const int ra = r0 + slot;
  int mr0 = mrow && ra < r1 ? mrow[ra] : (int)(s.row0 + ra), mr1 = mrow && ra + ROWS < r1 ? mrow[ra + ROWS] : (int)(s.row0 + ra + ROWS);
  if (ra < r1) {
    q = *(reinterpret_cast<const uint4*>(w.map16 + (size_t)mr0 * w.d2p) + l);
    if (!ABSCOUNT) yv = y[ra];
  }
  for (int v = threadIdx.x; v < w.nslice; v += PABS_THREADS) accs[v] = 0;
  __syncthreads();
  for (int r = ra; r < r1; r += ROWS) {
    const int mr2 = mrow && r + 2 * ROWS < r1 ? mrow[r + 2 * ROWS] : (int)(s.row0 + r + 2 * ROWS);
    const long long qv = ABSCOUNT ? 1 : __double2ll_rn((MODE == 1 ? yv * sc : yv) * scale);
    double yn = 0;
    for (int st = 0; st < steps; ++st) {
      const bool last = st + 1 == steps;
      const int rn = last ? r + ROWS : r;
      uint4 qn = make_uint4(~0u, ~0u, ~0u, ~0u);
      if (rn < r1) {
        qn = *(reinterpret_cast<const uint4*>(w.map16 + (size_t)(last ? mr1 : mr0) * w.d2p) + l + (last ? 0 : (st + 1) * PABS_LANES));
        if (last && !ABSCOUNT) yn = y[rn];
      }
      unsigned m[8];
      pabs_unpack(q, m);
      // consecutive samples often fall into the same voxel: one atomic serves a run of equal indices
      unsigned prev = 0xffffu;
      int count = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (m[k] != prev) {
          if (prev != 0xffffu) atomicAdd(reinterpret_cast<unsigned long long*>(&accs[prev]), (unsigned long long)(count * qv));
          prev = m[k];
          count = 0;
        }
        ++count;
      }
      if (prev != 0xffffu) atomicAdd(reinterpret_cast<unsigned long long*>(&accs[prev]), (unsigned long long)(count * qv));
      q = qn;
    }
    yv = yn;
    mr0 = mr1;
    mr1 = mr2;
  }
  __syncthreads();
  if (ABSCOUNT) {
    double mx = 0;
    for (int v = threadIdx.x; v < w.nslice; v += PABS_THREADS) mx = fmax(mx, (double)accs[v]);
    const double m = pabs_block_reduce(RED_MAX, mx, lds16);
    if (threadIdx.x == 0) atomicMax(&colmax[c], (int)m);
    return;
  }
  double* __restrict__ g = w.nvec(dst, c);
  const int* __restrict__ tp = w.tptr + (size_t)c * (w.n + 1);
  const int* __restrict__ te = w.tent + s.t0;
  double sq = 0;
  for (int v = threadIdx.x; v < w.nslice; v += PABS_THREADS) {
    const int64_t gi = base + v;
    double acc = (double)accs[v] * inv_scale;
    const int e1 = tp[gi + 1];
    for (int e = tp[gi]; e < e1; ++e) {
      const int ent = te[e];
      const double yy = MODE == 1 ? y[ent & 0x7fffffff] * sc : y[ent & 0x7fffffff];
      acc += ent < 0 ? -yy : yy;
    }
    if (dsc >= 0 && (MODE != 1 || s.aug)) acc *= w.nvec(dsc, c)[gi];
    if (rootv >= 0 && (MODE != 1 || s.aug)) {
      const double tail = y[s.m_data + s.m_sym + gi];
      acc += w.nvec(rootv, c)[gi] * (MODE == 1 ? tail * sc : tail);
    }
    if (MODE == 1) acc = (g[gi] * s.inv_alpha) * s.neg_beta + acc;
    g[gi] = acc;
    sq += acc * acc;
  }
  if (MODE == 1) {
    const double r = pabs_block_reduce(RED_SUM, sq, lds16);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 1)[bx], r);
  }
}

// ---- set-up kernels -----------------------------------------------------------------------------------------------------
struct PabGeomRef {          // where a candidate's geometry and operations live
  const PaGeom* geom;        // [K]
  const PaOp* ops;           // concatenated
  const int64_t* op0;        // [K] first operation of candidate c
};

#include "path_a_linear.inc"   // the trilinear projector's kernels (k_pabl_*)
#include "path_a_factored.inc" // ... and its separable form (k_pabf_*), the default
#include "path_a_banded.inc"   // ... and its banded form (k_pabt_*), for boxes whose two planes do not fit the LDS

// has[(c_slot * chunk + o) * rays + ray]: 0 = the ray misses the cylinder under operation lo + o of candidate
// cand[c_slot]; 1 + z = all its samples inside the cylinder lie in slice z; 255 = they lie in more than one slice
// (tilt / psi, or a half-integer axial position: the ~1e-16 off-diagonal entries of scipy's Ry(90) then decide the
// rounding sample by sample — the reference's behaviour, kept) or z > 253
__global__ __launch_bounds__(256) void k_pab_has(PabGeomRef gr, const int* __restrict__ cand, int lo, int chunk, const int* __restrict__ n_ops,
                                                 const int* __restrict__ rank, unsigned char* __restrict__ has) {
#pragma clang fp contract(off)
  const int slot = blockIdx.z, o = blockIdx.y, c = cand[slot];
  const PaGeom g = gr.geom[c];
  const size_t rays = (size_t)g.L2 * g.D2;
  const size_t ray = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (ray >= rays) return;
  int zmin = 1 << 30, zmax = -1;
  if (lo + o < n_ops[c]) {
    const PaOp op = gr.ops[gr.op0[c] + lo + o];
    const int j = (int)(ray % g.D2), k = (int)(ray / g.D2);
    for (int i = 0; i < g.D2; ++i) {
      double X, Y, Z;
      pa_coords(g, op, k, j, i, X, Y, Z);
      const long long xi = (long long)rint(X), yi = (long long)rint(Y), zi = (long long)rint(Z);
      if (zi >= 0 && zi < g.mz && yi >= 0 && yi < g.my && xi >= 0 && xi < g.mx && rank[((size_t)zi * g.my + yi) * g.mx + xi] >= 0) {
        zmin = min(zmin, (int)zi);
        zmax = max(zmax, (int)zi);
      }
    }
  }
  has[((size_t)slot * chunk + o) * rays + ray] = zmax < 0 ? 0 : (zmin == zmax && zmax <= 253) ? (unsigned char)(1 + zmax) : 255;
}

// rows per (slot, operation, slice) from the codes of k_pab_has: counts[(slot * chunk + o) * (mz + 1) + z], z = mz for a
// ray in more than one slice
__global__ __launch_bounds__(256) void k_pab_count_codes(const unsigned char* __restrict__ has, size_t rays, int chunk, int mz,
                                                         int* __restrict__ counts) {
  extern __shared__ int cnt_lds[];   // [mz + 1]
  const int slot = blockIdx.y, o = blockIdx.x;
  for (int z = threadIdx.x; z <= mz; z += 256) cnt_lds[z] = 0;
  __syncthreads();
  const unsigned char* h = has + ((size_t)slot * chunk + o) * rays;
  for (size_t r = threadIdx.x; r < rays; r += 256) {
    const int code = h[r];
    if (code) atomicAdd(&cnt_lds[code == 255 ? mz : code - 1], 1);
  }
  __syncthreads();
  for (int z = threadIdx.x; z <= mz; z += 256) counts[((size_t)slot * chunk + o) * (mz + 1) + z] = cnt_lds[z];
}

// The rows of (slot, operation) in ray order, written where they belong: row index in the reference's order =
// base_ref + rank among the operation's existing rays; device (slice-major) order = base_int[slice] + the same rank
// (the host folds the slice's offset inside the operation into base_int; on the general path base_int = base_ref).
// b = pixel_vals[j, k], pid = k * D2d + j (solver:1548-1549).  One workgroup per (operation, slot), tiles of 1024 rays.
struct PabEmit {
  const unsigned char* has;      // codes of this chunk
  const float* image;            // [ny][nx]
  const long long* base_ref;     // [live][chunk] (relative to the candidate's first row; < 0: operation not used)
  const long long* base_int;     // [live][chunk][mz + 1]
  const long long* row0;         // [live] first row of the slot's candidate
  const int* cand;               // [live]
  int* ray_of_row;               // device order
  float* b_int;                  // device order
  float* b_ref;                  // reference order
  int* pid_ref;                  // reference order
  int* bmax;                     // [K] max of b as ordered int
  int chunk, lo, mz, L2, D2, ny, nx;
};
__device__ __forceinline__ int pab_ordered(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__global__ __launch_bounds__(1024) void k_pab_emit(PabEmit a) {
  const int slot = blockIdx.y, o = blockIdx.x;
  const long long bref = a.base_ref[slot * a.chunk + o];
  if (bref < 0) return;
  const long long* const bint = a.base_int + ((size_t)slot * a.chunk + o) * (a.mz + 1);
  const long long row0 = a.row0[slot];
  const size_t rays = (size_t)a.L2 * a.D2;
  const unsigned char* h = a.has + ((size_t)slot * a.chunk + o) * rays;
  __shared__ int wave_tot[16];
  __shared__ int tile_base;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) tile_base = 0;
  int bm = pab_ordered(-INFINITY);
  for (size_t r0 = 0; r0 < rays; r0 += 1024) {
    const size_t ray = r0 + threadIdx.x;
    const int code = ray < rays ? h[ray] : 0;
    const unsigned long long bal = __ballot(code != 0);
    if (lane == 0) wave_tot[wv] = __popcll(bal);
    __syncthreads();
    int before = tile_base;
    for (int k = 0; k < wv; ++k) before += wave_tot[k];
    if (code) {
      const int rank = before + __popcll(bal & ((1ull << lane) - 1ull));
      const int j = (int)(ray % a.D2), k = (int)(ray / a.D2);
      const int z = code == 255 ? a.mz : code - 1;
      const float b = a.image[(size_t)(j - a.D2 / 2 + a.ny / 2) * a.nx + (k - a.L2 / 2 + a.nx / 2)];
      const long long ir = row0 + bint[z] + rank, rr = row0 + bref + rank;
      a.ray_of_row[ir] = (int)(((size_t)(a.lo + o) * a.L2 + k) * a.D2 + j);
      a.b_int[ir] = b;
      a.b_ref[rr] = b;
      a.pid_ref[rr] = k * a.D2 + j;
      bm = max(bm, pab_ordered(b));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int k = 0; k < 16; ++k) t += wave_tot[k];
      tile_base += t;
    }
    __syncthreads();
  }
  for (int off = 32; off > 0; off >>= 1) bm = max(bm, __shfl_down(bm, off, 64));
  if (lane == 0) atomicMax(&a.bmax[a.cand[slot]], bm);
}

// ---- shared map rows (sliced nearest-neighbour path) ------------------------------------------------------------------------------
// With tilt = psi = 0 the in-plane voxel of a ray's sample depends on (operation, image row j, depth) only, so the rays
// (operation, k, j) of all image columns k have the SAME 16-bit map row — up to the ~1e-16 noise of scipy's Ry(90), which
// moves a sample across a voxel boundary for a few k.  The map is the bulk of what an LSMR iteration reads from HBM (128 of
// ~160 bytes per data row and product); if the rows of one (operation, j) read ONE copy, that copy stays in the caches.
// Nothing is moved: maprow[row] names the row whose map a row reads — the first row of its (operation, j) when their maps
// are equal byte for byte, else the first row that differed from that one, else the row itself.
// STEP 0: first[c][op * D2 + j] = the smallest row of the group.  STEP 1: rows equal to it take it; the others compete for
// second[...].  STEP 2: the others take second[...] if equal, else themselves.
template <int STEP>
__global__ __launch_bounds__(256) void k_pab_share_rows(const PabState* __restrict__ st, const int* __restrict__ ray_of_row,
                                                        const uint16_t* __restrict__ map16, int d2p, int l2, int d2, int max_ops,
                                                        int* __restrict__ first, int* __restrict__ second, int* __restrict__ maprow, int count) {
  const int c = PAB_SLOT, bx = PAB_BLOCK;
  if (c >= count) return;
  const PabState& s = st[c];
  const int lanes = 8, sub = threadIdx.x & (lanes - 1);
  const int64_t r = ((int64_t)bx * 256 + threadIdx.x) / lanes;
  if (r >= s.m_data) return;
  const int64_t row = s.row0 + r;
  const int ray = ray_of_row[row];
  const int op = ray / (l2 * d2), j = ray % d2;
  const size_t key = ((size_t)c * max_ops + op) * d2 + j;
  if (STEP == 0) {
    if (sub == 0) atomicMin(&first[key], (int)r);
    return;
  }
  if (STEP == 2 && maprow[row] >= 0) return;
  const int other = STEP == 1 ? first[key] : second[key];
  bool same = true;
  for (int t = sub * 8; t < d2p; t += lanes * 8) {
    const uint4 a = *reinterpret_cast<const uint4*>(map16 + (size_t)row * d2p + t);
    const uint4 b = *reinterpret_cast<const uint4*>(map16 + (size_t)(s.row0 + other) * d2p + t);
    same = same && a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
  }
  // all eight lanes of the row agree?
  const unsigned long long bal = __ballot(same);
  const int shift = (threadIdx.x & 63) & ~(lanes - 1);
  const bool all_same = ((bal >> shift) & 0xffull) == 0xffull;
  if (sub != 0) return;
  if (all_same) maprow[row] = (int)(s.row0 + other);
  else if (STEP == 1) { maprow[row] = -1; atomicMin(&second[key], (int)r); }
  else maprow[row] = (int)row;
}

// the compact index map: one thread per (row, sample)
// (map16 != NULL: the sliced format — index inside the sample's slice, 0xFFFF outside; bad[0] is set if a sample of a row
// leaves the slice its row was filed under, which cannot happen without tilt / psi)
__global__ __launch_bounds__(256) void k_pab_fill_map(PabGeomRef gr, const PabState* __restrict__ st, const int* __restrict__ ray_of_row,
                                                      const int* __restrict__ rank, int* __restrict__ map, uint16_t* __restrict__ map16,
                                                      const int* __restrict__ srow, int nslice, int d2p, int* __restrict__ bad, int K) {
#pragma clang fp contract(off)
  const int c = PAB_SLOT, bx = PAB_BLOCK;
  if (c >= K) return;
  const PabState& s = st[c];
  const PaGeom g = gr.geom[c];
  const int64_t t = (int64_t)bx * 256 + threadIdx.x;
  if (t >= s.m_data * g.D2) return;
  const int64_t row = t / g.D2;
  const int i = (int)(t % g.D2);
  const int ray = ray_of_row[s.row0 + row];
  const int j = ray % g.D2, k = (ray / g.D2) % g.L2, o = ray / (g.D2 * g.L2);
  double X, Y, Z;
  pa_coords(g, gr.ops[gr.op0[c] + o], k, j, i, X, Y, Z);
  const long long xi = (long long)rint(X), yi = (long long)rint(Y), zi = (long long)rint(Z);
  int idx = -1;
  if (zi >= 0 && zi < g.mz && yi >= 0 && yi < g.my && xi >= 0 && xi < g.mx) idx = rank[((size_t)zi * g.my + yi) * g.mx + xi];
  if (!map16) {
    map[(size_t)(s.row0 + row) * g.D2 + i] = idx;
    return;
  }
  unsigned short local = 0xffffu;
  if (idx >= 0) {
    const int* sr = srow + (size_t)c * (g.mz + 1);
    if (row >= sr[zi] && row < sr[zi + 1]) local = (unsigned short)(idx - (int)zi * nslice);
    else bad[0] = 1;
  }
  map16[(size_t)(s.row0 + row) * d2p + i] = local;   // (the padding beyond D2 was preset to 0xFFFF)
}

// transposed pattern, pass 1 (FILL = false): cnt[c][v + 1] += 1 per entry; pass 3 (FILL = true): entries into their lists
// (DATA = false: symmetry rows only — the sliced path keeps no transposed lists of the data rows)
template <bool FILL, bool DATA>
__global__ __launch_bounds__(256) void k_pab_transpose(PabView w, int* __restrict__ cnt, int* __restrict__ tent) {
  const int c = PAB_CAND, bx = PAB_BLOCK, nbx = PAB_NBLOCKS;
  if (c < 0) return;
  if (w.fence > 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const PabState& s = w.st[c];
  int* __restrict__ cc = cnt + (size_t)c * (w.n + 1);
  const int64_t t = (int64_t)bx * 256 + threadIdx.x;
  const int64_t nd = DATA ? s.m_data * w.d2 : 0;
  if (DATA && t < nd) {
    const int v = w.map[(size_t)s.row0 * w.d2 + t];
    if (v < 0) return;
    const int row = (int)(t / w.d2);
    if (FILL) tent[s.t0 + atomicAdd(&cc[v], 1)] = row;
    else atomicAdd(&cc[v + 1], 1);
  } else if (t - nd < s.m_sym) {
    const int64_t q = t - nd;
    const int2 pr = w.pairs[s.sym0 + q];
    const int row = (int)(s.m_data + q);
    if (FILL) {
      tent[s.t0 + atomicAdd(&cc[pr.x], 1)] = row;
      tent[s.t0 + atomicAdd(&cc[pr.y], 1)] = row | (int)0x80000000;
    } else {
      atomicAdd(&cc[pr.x + 1], 1);
      atomicAdd(&cc[pr.y + 1], 1);
    }
  }
}
// pass 2: inclusive scan of the counts (one block per candidate), tptr = scan, cursor = copy
__global__ __launch_bounds__(1024) void k_pab_scan(int64_t n, int* __restrict__ tptr, int* __restrict__ cursor) {
  const int c = blockIdx.x;
  int* p = tptr + (size_t)c * (n + 1);
  int* q = cursor + (size_t)c * (n + 1);
  __shared__ int part[1024];
  const int per = (int)((n + 1 + 1023) / 1024);
  const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < n + 1 ? lo + per : n + 1;
  int sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += p[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < 1024; ++i) { const int v = part[i]; part[i] = run; run += v; }
  }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int64_t i = lo; i < hi; ++i) { run += p[i]; p[i] = run; q[i] = run; }
}
// pass 4: every voxel's list in ascending row order (the order scipy's CSR transpose sums in)
__global__ __launch_bounds__(256) void k_pab_sort_lists(PabView w, int* __restrict__ tent) {
  const int c = PAB_CAND, bx = PAB_BLOCK, nbx = PAB_NBLOCKS;
  if (c < 0) return;
  if (w.fence > 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const PabState& s = w.st[c];
  const int64_t v = (int64_t)bx * 256 + threadIdx.x;
  if (v >= w.n) return;
  const int* tp = w.tptr + (size_t)c * (w.n + 1);
  int* e = tent + s.t0;
  const int lo = tp[v], hi = tp[v + 1];
  for (int i = lo + 1; i < hi; ++i) {
    const int x = e[i];
    const int key = x & 0x7fffffff;
    int j = i - 1;
    // (a row can appear twice with opposite signs only in a symmetry row x_i - x_i; ties keep + before -)
    while (j >= lo && ((e[j] & 0x7fffffff) > key || ((e[j] & 0x7fffffff) == key && e[j] < 0 && x >= 0))) { e[j + 1] = e[j]; --j; }
    e[j + 1] = x;
  }
}

// ---- symmetry constraints on the device ---------------------------------------------------------------------------------
// build_A_helical_sym_matrix, nearest neighbour (solver:1142-1298), is a sequential rule: walk the symmetry pairs in
// Halton order and the voxels in C order, keep a voxel-image pair (ia, ib) unless (ia, ib) or (ib, ia) was kept before,
// stop after the pair of operations that brings the count to min_sym_pairs.  Equivalent parallel form: number every
// candidate row t = (pair index, voxel index) in that walk; a row is kept iff it has the smallest t among the rows with
// the same unordered {ia, ib}.  A hash table keyed by the unordered pair takes atomicMin(t) (pass 1), a row is kept when
// the table holds its own t (pass 2), and a per-(candidate, pair) scan of the kept flags writes them in walk order
// (pass 3).  Arithmetic of the images: the host's (pa_sym_pairs), expression for expression.
struct PabSymRef {
  const PaSymOp* ops;          // [live][chunk]
  const int* cand;             // [live] candidate of a slot
  const int* n_valid;          // [live] pairs of this chunk that exist for the slot's candidate
  int chunk, p0;               // p0: walk index of the chunk's first pair
  int nz, ny, nx;              // box of lsq_reconstruct's mask (L3d, D3d, D3d)
  const int* rank;             // its voxel ranks (-1 outside the cylinder)
  unsigned long long* keys;    // [K][T]
  unsigned long long* tmin;    // [K][T]
  unsigned T;                  // power of two
  int* err;                    // set when a table is full
};
__device__ __forceinline__ bool pab_sym_images(const PabSymRef& r, const PaSymOp& op, int k, int j, int i, int& ia, int& ib) {
#pragma clang fp contract(off)
  const double x = (double)(i - r.nx / 2), y = (double)(j - r.ny / 2), z = (double)(k - r.nz / 2);
  long long c[2][3];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const double* m = w ? op.mb : op.ma;
    const double rx = x * m[0] + y * m[1] + z * m[2], ry = x * m[3] + y * m[4] + z * m[5], rz = x * m[6] + y * m[7] + z * m[8];
    const double X = rx + (double)(r.nx / 2), Y = ry + (double)(r.ny / 2), Z = rz + (double)(r.nz / 2) + (w ? op.shift_b : op.shift_a);
    c[w][0] = (long long)nearbyint(Z); c[w][1] = (long long)nearbyint(Y); c[w][2] = (long long)nearbyint(X);
    if (c[w][0] < 0 || c[w][0] > r.nz - 1 || c[w][1] < 0 || c[w][1] > r.ny - 1 || c[w][2] < 0 || c[w][2] > r.nx - 1) return false;
  }
  ia = r.rank[((size_t)c[0][0] * r.ny + c[0][1]) * r.nx + c[0][2]];
  ib = r.rank[((size_t)c[1][0] * r.ny + c[1][1]) * r.nx + c[1][2]];
  return ia >= 0 && ib >= 0;
}
__device__ __forceinline__ unsigned long long pab_sym_key(int ia, int ib) {
  const unsigned lo = (unsigned)min(ia, ib), hi = (unsigned)max(ia, ib);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned pab_sym_hash(unsigned long long key, unsigned T) {
  return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & (T - 1);
}
// PASS 1: insert (atomicMin of the walk index); PASS 2: flags[(slot * chunk + pi) * nbox + v] = kept, counts[slot * chunk + pi]
template <int PASS>
__global__ __launch_bounds__(256) void k_pab_sym(PabSymRef r, unsigned char* __restrict__ flags, int* __restrict__ counts) {
  const int slot = blockIdx.z, pi = blockIdx.y;
  const int64_t nbox = (int64_t)r.nz * r.ny * r.nx;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool kept = false;
  if (pi < r.n_valid[slot] && v < nbox && r.rank[v] >= 0) {
    const int i = (int)(v % r.nx), j = (int)((v / r.nx) % r.ny), k = (int)(v / ((int64_t)r.nx * r.ny));
    int ia, ib;
    if (pab_sym_images(r, r.ops[(size_t)slot * r.chunk + pi], k, j, i, ia, ib)) {
      const int c = r.cand[slot];
      unsigned long long* keys = r.keys + (size_t)c * r.T;
      unsigned long long* tmin = r.tmin + (size_t)c * r.T;
      const unsigned long long key = pab_sym_key(ia, ib), t = (unsigned long long)(r.p0 + pi) * (unsigned long long)nbox + (unsigned long long)v;
      unsigned h = pab_sym_hash(key, r.T);
      bool found = false;
      for (unsigned probe = 0; probe < r.T; ++probe, h = (h + 1) & (r.T - 1)) {
        if (PASS == 1) {
          const unsigned long long old = atomicCAS(&keys[h], ~0ull, key);
          if (old == ~0ull || old == key) { atomicMin(&tmin[h], t); found = true; break; }
        } else {
          if (keys[h] == key) { kept = tmin[h] == t; found = true; break; }
          if (keys[h] == ~0ull) break;
        }
      }
      if (!found) r.err[0] = 1;
    }
  }
  if (PASS == 2) {
    if (v < nbox) flags[((size_t)slot * r.chunk + pi) * nbox + v] = kept;
    const unsigned long long b = __ballot(kept);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&counts[slot * r.chunk + pi], __popcll(b));
  }
}
// PASS 3: the kept rows of (slot, pair) in voxel order -> pairs[base + rank among the kept]; base < 0: the pair is not used
__global__ __launch_bounds__(1024) void k_pab_sym_emit(PabSymRef r, const unsigned char* __restrict__ flags, const long long* __restrict__ base,
                                                       int2* __restrict__ pairs) {
  const int slot = blockIdx.y, pi = blockIdx.x;
  const long long b0 = base[slot * r.chunk + pi];
  if (b0 < 0) return;
  const int64_t nbox = (int64_t)r.nz * r.ny * r.nx;
  const unsigned char* f = flags + ((size_t)slot * r.chunk + pi) * nbox;
  __shared__ int part[1024];
  const int64_t per = (nbox + 1023) / 1024;
  const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < nbox ? lo + per : nbox;
  int cnt = 0;
  for (int64_t v = lo; v < hi; ++v) cnt += f[v];
  part[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < 1024; ++t) { const int c = part[t]; part[t] = run; run += c; }
  }
  __syncthreads();
  long long at = b0 + part[threadIdx.x];
  const PaSymOp op = r.ops[(size_t)slot * r.chunk + pi];
  for (int64_t v = lo; v < hi; ++v)
    if (f[v]) {
      const int i = (int)(v % r.nx), j = (int)((v / r.nx) % r.ny), k = (int)(v / ((int64_t)r.nx * r.ny));
      int ia, ib;
      (void)pab_sym_images(r, op, k, j, i, ia, ib);
      pairs[at++] = make_int2(ia, ib);
    }
}

// ---- small device helpers of the trust-region step ------------------------------------------------------------------------
__device__ __forceinline__ double pab_pymod(double a, double b) {  // np.remainder for b > 0
  double t = fmod(a, b);
  if (t != 0 && t < 0) t += b;
  return t;
}
__device__ __forceinline__ double pab_reflect(double y, double lb, double ub) {  // reflective_transformation, finite box
  const double d = ub - lb;
  const double t = pab_pymod(y - lb, 2 * d);
  return lb + fmin(t, 2 * d - t);
}
__device__ __forceinline__ double pab_feasible(double x, double lb, double ub, double rstep) {  // make_strictly_feasible
  double xn = x;
  if (rstep == 0) {
    if (x <= lb) xn = nextafter(lb, ub);
    if (x >= ub) xn = nextafter(ub, lb);
  } else {
    const double lower = x - lb, upper = ub - x;
    const double lt = rstep * fmax(1.0, fabs(lb)), ut = rstep * fmax(1.0, fabs(ub));
    if (lower <= fmin(upper, lt)) xn = lb + rstep * fmax(1.0, fabs(lb));
    if (upper <= fmin(lower, ut)) xn = ub - rstep * fmax(1.0, fabs(ub));
  }
  if (xn < lb || xn > ub) xn = 0.5 * (lb + ub);
  return xn;
}
__device__ __forceinline__ double pab_step_to_bound(double x, double sdir, double lb, double ub) {
  return sdir == 0 ? INFINITY : fmax((lb - x) / sdir, (ub - x) / sdir);
}
__device__ __forceinline__ int pab_active(double x, double lb, double ub) {  // find_active_constraints, rtol = 1e-10
  const double rt = 1e-10;
  const double lower = x - lb, upper = ub - x;
  int a = 0;
  if (lower <= fmin(upper, rt * fmax(1.0, fabs(lb)))) a = -1;
  if (upper <= fmin(lower, rt * fmax(1.0, fabs(ub)))) a = 1;
  return a;
}
__device__ __forceinline__ void pab_sym_ortho(double a, double b, double& c, double& s, double& r) {
  auto sgn = [](double v) { return (double)((v > 0) - (v < 0)); };
  if (b == 0) { c = sgn(a); s = 0; r = fabs(a); }
  else if (a == 0) { c = 0; s = sgn(b); r = fabs(b); }
  else if (fabs(b) > fabs(a)) { const double tau = a / b; s = sgn(b) / sqrt(1 + tau * tau); c = s * tau; r = b / s; }
  else { const double tau = b / a; c = sgn(a) / sqrt(1 + tau * tau); s = c * tau; r = a / c; }
}
// minimize_quadratic_1d(a, b, lb, ub, c): returns the argument, value through `val`
__device__ __forceinline__ double pab_min_quad(double a, double b, double lo, double hi, double c, double& val) {
  double tb = lo, yb = lo * (a * lo + b) + c;
  const double yh = hi * (a * hi + b) + c;
  if (yh < yb) { tb = hi; yb = yh; }
  if (a != 0) {
    const double ext = -0.5 * b / a;
    if (lo < ext && ext < hi) {
      const double ye = ext * (a * ext + b) + c;
      if (ye < yb) { tb = ext; yb = ye; }
    }
  }
  val = yb;
  return tb;
}

}  // namespace

struct hh_pab {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int K = 0;
  int64_t n = 0, N = 0, M = 0, MA = 0;
  int d2 = 0, d2p = 0;
  int sliced = 0, mz = 0, nslice = 0;   // tilt = psi = 0 and a slice fits LDS: the slice-major products
  int linear = 0;                       // trilinear projector (all candidates of a batch alike); needs `sliced`
  DevBuf<unsigned> d_sidx2;
  DevBuf<PaEll16> d_sym16;
  DevBuf<int2> d_tent2;
  DevBuf<long long> d_acc64;
  size_t lin_lds = 0;                   // dynamic LDS of the trilinear products
  int fac_G = 0, fac_ng = 0, fac_max_gl = 0, fac_max_lists = 0;   // separable form (path_a_factored.inc); G = 0: direct kernels
  int fac_split = 1;
  size_t fac_lds = 0;
  int band_T = 0;                       // banded form (path_a_banded.inc); T = 0: not this form
  size_t band_lds = 0;
  DevBuf<int> d_band_y;
  DevBuf<int> d_band_v;
  DevBuf<double> d_bpart;
  int flat = 0;                         // every candidate has tilt = psi = 0
  DevBuf<int> d_fac_ngl;
  DevBuf<PabfGroupList> d_fac_gl;
  DevBuf<PabfEntry> d_fac_entries;
  DevBuf<unsigned char> d_fac_count;
  int RB = 0;
  int nb_n = 0, nb_m = 0, nb_mv = 0, nb_mva = 0;   // grid.x of: vectors over n, over m (+ n), products without / with augmented rows
  int nb_fin = 0;                                  // ... of the trilinear A^T y's gather half (k_pabl_finish)
  std::vector<PabState> st;       // host copy of the static part
  std::vector<float> b_data;      // concatenated
  std::vector<int32_t> b_pid;
  std::vector<int> n_ops_used;
  DevBuf<PabState> d_st;
  DevBuf<unsigned> d_ctl;
  DevBuf<PaGeom> d_geom;
  DevBuf<PaOp> d_ops;
  DevBuf<int64_t> d_op0;
  DevBuf<int> d_rank;
  DevBuf<int> d_map;
  DevBuf<uint16_t> d_map16;
  DevBuf<int> d_maprow;
  DevBuf<int> d_srow;
  DevBuf<int> d_ray_of_row;
  DevBuf<float> d_bref;           // device-side enumeration: b and pixel ids in the reference's row order (hh_pab_get_rhs)
  DevBuf<int> d_pidref;
  DevBuf<int2> d_pairs;
  DevBuf<int> d_tptr;
  DevBuf<int> d_tent;
  DevBuf<double> d_nv;
  DevBuf<double> d_mv;
  DevBuf<double> d_red;
  DevBuf<float> d_xf;
  DevBuf<double> d_trace;
  int trace_c = -1, trace_run = 0;
  DevBuf<int> d_flags;
  DevBuf<int> d_lists;            // [2][K]: candidates not finished / of those, the ones outside an LSMR solve (k_pab_lists)
  const int* cur_list = nullptr;  // the list the next launches cover (NULL: all K)
  int cur_n = 0;
  void* h_stage = nullptr;        // pinned staging of THIS object (no process-wide buffer, no lock)
  size_t stage_bytes = 0;
  int* h_flags = nullptr;
  int64_t total_rows = 0, total_sym = 0, total_nnz = 0;
  // counters of the last solve
  int64_t launches = 0, syncs = 0, ticks = 0, inconsistent = 0;
  size_t device_bytes = 0;
};

namespace {

int pab_fail(hh_pab* p, int code, const std::string& msg) {
  if (p) p->err = msg; else g_create_error = msg;
  return code;
}
#define PAB_HIP(p, call)                                                                        \
  do {                                                                                          \
    hipError_t e__ = (call);                                                                    \
    if (e__ != hipSuccess) return pab_fail(p, HH_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

int pab_stage(hh_pab* p, size_t bytes) {
  if (bytes <= p->stage_bytes) return HH_OK;
  if (p->h_stage) (void)hipHostFree(p->h_stage);
  p->h_stage = nullptr;
  p->stage_bytes = 0;
  const size_t want = std::max<size_t>(bytes, (size_t)1 << 20);
  PAB_HIP(p, hipHostMalloc(&p->h_stage, want, hipHostMallocDefault));
  p->stage_bytes = want;
  return HH_OK;
}
int pab_to_device(hh_pab* p, void* dst, const void* src, size_t bytes) {
  if (!bytes) return HH_OK;
  int rc = pab_stage(p, bytes);
  if (rc) return rc;
  std::memcpy(p->h_stage, src, bytes);
  PAB_HIP(p, hipMemcpyAsync(dst, p->h_stage, bytes, hipMemcpyHostToDevice, p->stream));
  PAB_HIP(p, hipStreamSynchronize(p->stream));
  return HH_OK;
}
int pab_to_host(hh_pab* p, void* dst, const void* src, size_t bytes) {
  if (!bytes) return HH_OK;
  int rc = pab_stage(p, bytes);
  if (rc) return rc;
  PAB_HIP(p, hipMemcpyAsync(p->h_stage, src, bytes, hipMemcpyDeviceToHost, p->stream));
  PAB_HIP(p, hipStreamSynchronize(p->stream));
  std::memcpy(dst, p->h_stage, bytes);
  return HH_OK;
}
// a buffer of the object (at least one element), counted in device_bytes
template <class T>
int pab_alloc(hh_pab* p, DevBuf<T>& out, size_t count) {
  if (!out.ensure(std::max<size_t>(count, 1))) return pab_fail(p, HH_ERR_NOMEM, dev_alloc_failed(out.bytes_for(std::max<size_t>(count, 1))));
  p->device_bytes += out.bytes();
  return HH_OK;
}
int pab_arena_ok(hh_pab* p, const DevArena& mem) {
  return mem.ok() ? HH_OK : pab_fail(p, HH_ERR_NOMEM, dev_alloc_failed(mem.failed_bytes()));
}

inline int pab_slots(const hh_pab* p) { return p->cur_list ? p->cur_n : p->K; }
inline void pab_cover(hh_pab* p, const int* list, int n) { p->cur_list = list; p->cur_n = n; }   // list NULL: every candidate

PabView pab_view(const hh_pab* p) {
  PabView w{};
  w.trace_c = p->trace_c; w.trace = p->d_trace;
  static const int fence = std::getenv("HH_PAB_FENCE") ? std::atoi(std::getenv("HH_PAB_FENCE")) : 0;   // 1: scalar steps, 2: every kernel
  w.fence = fence;
  w.K = p->K; w.d2 = p->d2; w.d2p = p->d2p; w.n = p->n; w.N = p->N; w.MA = p->MA;
  w.sliced = p->sliced; w.mz = p->mz; w.nslice = p->nslice; w.map16 = p->d_map16; w.maprow = p->d_maprow; w.srow = p->d_srow;
  w.st = p->d_st; w.ctl = p->d_ctl; w.nv = p->d_nv; w.mv = p->d_mv; w.map = p->d_map; w.pairs = p->d_pairs; w.tptr = p->d_tptr; w.tent = p->d_tent;
  w.red = p->d_red; w.RB = p->RB; w.flags = p->d_flags;
  w.list = p->cur_list; w.n_list = p->cur_list ? p->cur_n : p->K;
  w.linear = p->linear; w.lin_geom = p->d_geom; w.lin_ops = p->d_ops; w.lin_op0 = p->d_op0; w.ray_of_row = p->d_ray_of_row;
  w.sidx2 = p->d_sidx2; w.sym16 = p->d_sym16; w.tent2 = p->d_tent2; w.acc64 = p->d_acc64;
  w.fac_G = p->fac_G; w.fac_ng = p->fac_ng; w.fac_max_gl = p->fac_max_gl; w.fac_max_lists = p->fac_max_lists;
  w.fac_ngl = p->d_fac_ngl; w.fac_gl = p->d_fac_gl; w.fac_entries = p->d_fac_entries; w.fac_count = p->d_fac_count;
  w.fac_split = p->fac_split;
  w.fwd_main = p->fac_G ? p->fac_ng * p->fac_split : p->mz;
  w.band_T = p->band_T; w.band_y = p->d_band_y; w.band_v = p->d_band_v; w.bpart = p->d_bpart; w.bstride = p->M;
  return w;
}

template <int NRED>
PabRed<NRED> pab_red(std::initializer_list<int> kinds, std::initializer_list<int> slots, int nb) {
  PabRed<NRED> r{};
  int i = 0;
  for (int k : kinds) r.kind[i++] = k;
  i = 0;
  for (int s : slots) r.slot[i++] = s;
  for (int k = 0; k < (NRED > 0 ? NRED : 1); ++k) r.nb[k] = nb;
  return r;
}

// launch helpers (every launch of a solve goes through these: they count).  HH_PAB_SYNC (debugging): wait for every launch.
inline void pab_after_launch(hh_pab* p) {
  static const bool sync_all = std::getenv("HH_PAB_SYNC") != nullptr;
  ++p->launches;
  if (sync_all) (void)hipStreamSynchronize(p->stream);
}
template <int NRED, class P, class F>
void pab_vec(hh_pab* p, int count_kind, const PabRed<NRED>& red, P pred, F body) {
  const int nb = count_kind == CNT_N ? p->nb_n : p->nb_m;
  hipLaunchKernelGGL((k_pab_vec<NRED, P, F>), pab_grid(nb, pab_slots(p)), dim3(256), 0, p->stream, pab_view(p), count_kind, red, pred, body);
  pab_after_launch(p);
}
template <int NRED, class P, class F>
void pab_scalar(hh_pab* p, const PabRed<NRED>& red, P pred, F body) {
  hipLaunchKernelGGL((k_pab_scalar<NRED, P, F>), dim3(pab_slots(p)), dim3(64), 0, p->stream, pab_view(p), red, pred, body);
  pab_after_launch(p);
}
// grid.x of a forward product = number of its partial sums (slot 0)
int pab_nb_fwd(const hh_pab* p, bool aug) { return aug ? p->nb_mva : p->nb_mv; }
int pab_nb_bwd(const hh_pab* p) { return p->linear ? p->nb_fin : p->sliced ? p->mz : p->nb_n; }
// kernels that ask for more than 64 KB of dynamic LDS need the attribute, once per kernel and device
template <class K>
void pab_lds_attr(hh_pab* p, K kernel, size_t bytes) {
  if (bytes <= (size_t)48 << 10) return;
  static std::mutex mu;
  static std::vector<std::pair<const void*, std::pair<int, size_t>>> done;
  const void* key = reinterpret_cast<const void*>(kernel);
  std::lock_guard<std::mutex> lock(mu);
  for (auto& d : done)
    if (d.first == key && d.second.first == p->device && d.second.second >= bytes) return;
  (void)hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  done.push_back({key, {p->device, bytes}});
}
// the separable form's planes per group (fac_G: 1 .. 4, anything else as 4) as a compile-time constant: f(integral_constant)
template <class F>
void pabf_with_G(int G, F f) {
  switch (G) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
template <int MODE, class P>
void pab_matvec(hh_pab* p, int src, int dsc, int rootv, int dst, P pred) {
  const int nb = pab_nb_fwd(p, rootv >= 0);
  if (p->linear && p->fac_G) {
    // (nb = groups + blocks of k_pabf_tail)
    auto launch = [&](auto kernel) {
      pab_lds_attr(p, kernel, p->fac_lds);
      hipLaunchKernelGGL(kernel, pab_grid(p->fac_ng * p->fac_split, pab_slots(p)), dim3(PABS_THREADS), p->fac_lds, p->stream, pab_view(p), src, dsc, rootv, dst, pred);
    };
    pabf_with_G(p->fac_G, [&](auto G) { launch(k_pabf_matvec<MODE, decltype(G)::value, P>); });
    pab_after_launch(p);
    if (nb > p->fac_ng * p->fac_split)
      hipLaunchKernelGGL((k_pabf_tail<MODE, P>), pab_grid(nb - p->fac_ng * p->fac_split, pab_slots(p)), dim3(256), 0, p->stream, pab_view(p), src, dsc, rootv, dst, pred);
  } else if (p->linear && p->band_T) {
    // (the bands' parts of every data row, then the rows summed and the tail: nb = planes + tail blocks as in the LDS form)
    pab_lds_attr(p, k_pabt_gather<MODE, P>, p->band_lds);
    hipLaunchKernelGGL((k_pabt_gather<MODE, P>), pab_grid(p->mz * p->band_T, pab_slots(p)), dim3(PABS_THREADS), p->band_lds, p->stream, pab_view(p), src,
                       dsc, pred);
    pab_after_launch(p);
    hipLaunchKernelGGL((k_pabl_matvec<MODE, P, true>), pab_grid(nb, pab_slots(p)), dim3(PABS_THREADS), 0, p->stream, pab_view(p), src, dsc, rootv, dst, pred);
  } else if (p->linear) {
    pab_lds_attr(p, k_pabl_matvec<MODE, P>, p->lin_lds);
    hipLaunchKernelGGL((k_pabl_matvec<MODE, P>), pab_grid(nb, pab_slots(p)), dim3(PABS_THREADS), p->lin_lds, p->stream, pab_view(p), src, dsc, rootv,
                       dst, pred);
  } else if (p->sliced)
    hipLaunchKernelGGL((k_pabs_matvec<MODE, P>), pab_grid(nb, pab_slots(p)), dim3(PABS_THREADS), (size_t)p->nslice * sizeof(double), p->stream, pab_view(p),
                       src, dsc, rootv, dst, pred);
  else
    hipLaunchKernelGGL((k_pab_matvec<MODE, P>), pab_grid(nb, pab_slots(p)), dim3(256), 0, p->stream, pab_view(p), src, dsc, rootv, dst, pred);
  pab_after_launch(p);
}
template <int MODE, class P>
void pab_rmatvec(hh_pab* p, int src, int dsc, int rootv, int dst, P pred) {
  if (p->linear) {   // scatter the data rows into the fixed-point accumulator, then the gather half (one more launch)
    if (p->fac_G) {
      auto launch = [&](auto kernel) {
        pab_lds_attr(p, kernel, p->fac_lds);
        hipLaunchKernelGGL(kernel, pab_grid(p->fac_ng * p->fac_split, pab_slots(p)), dim3(PABS_THREADS), p->fac_lds, p->stream, pab_view(p), src, pred);
      };
      pabf_with_G(p->fac_G, [&](auto G) { launch(k_pabf_scatter<MODE, false, decltype(G)::value, P>); });
    } else if (p->band_T) {
      pab_lds_attr(p, k_pabt_scatter<MODE, false, P>, p->band_lds);
      hipLaunchKernelGGL((k_pabt_scatter<MODE, false, P>), pab_grid(p->mz * p->band_T, pab_slots(p)), dim3(PABS_THREADS), p->band_lds, p->stream,
                         pab_view(p), src, pred);
    } else {
      pab_lds_attr(p, k_pabl_scatter<MODE, false, P>, p->lin_lds);
      hipLaunchKernelGGL((k_pabl_scatter<MODE, false, P>), pab_grid(p->mz, pab_slots(p)), dim3(PABS_THREADS), p->lin_lds, p->stream, pab_view(p), src, pred);
    }
    pab_after_launch(p);
    hipLaunchKernelGGL((k_pabl_finish<MODE, P>), pab_grid(p->nb_fin, pab_slots(p)), dim3(256), 0, p->stream, pab_view(p), src, dsc, rootv, dst,
                       (long long*)nullptr, pred);
  } else if (p->sliced)
    hipLaunchKernelGGL((k_pabs_rmatvec<MODE, false, P>), pab_grid(p->mz, pab_slots(p)), dim3(PABS_THREADS), (size_t)p->nslice * sizeof(long long), p->stream,
                       pab_view(p), src, dsc, rootv, dst, (int*)nullptr, pred);
  else
    hipLaunchKernelGGL((k_pab_rmatvec<MODE, P>), pab_grid(p->nb_n, pab_slots(p)), dim3(256), 0, p->stream, pab_view(p), src, dsc, rootv, dst, pred);
  pab_after_launch(p);
}
// the power-of-two scale that keeps colsum * bound inside 62 bits
__host__ __device__ inline void pab_fx_scale(double colsum, double bound, double& scale, double& inv) {
  const double b = colsum * bound * (1.0 + 1e-3) + 1e-300;
  int e = 0;
  (void)frexp(b, &e);            // b = f 2^e, f in [0.5, 1)  ->  b < 2^e
  if (e < -900) e = -900;        // (a zero vector: any finite scale will do)
  scale = ldexp(1.0, 61 - e);
  inv = ldexp(1.0, e - 61);
}

// read the flag words (synchronises the stream)
int pab_poll(hh_pab* p, int out[PAB_FLAG_WORDS]) {
  PAB_HIP(p, hipMemcpyAsync(p->h_flags, p->d_flags, PAB_FLAG_WORDS * sizeof(int), hipMemcpyDeviceToHost, p->stream));
  PAB_HIP(p, hipStreamSynchronize(p->stream));
  ++p->syncs;
  for (int i = 0; i < PAB_FLAG_WORDS; ++i) out[i] = p->h_flags[i];
  return HH_OK;
}
// candidates per phase -> flags[0 .. PH_COUNT); the lists of the next pass -> lists[0][..] = candidates that are not done
// (flags[10] of them), lists[1][..] = of those, the ones outside an LSMR solve (flags[11]) — in candidate order (one
// workgroup, a ballot scan per 1024 candidates), so a pass's launch shape depends on the state only
__global__ __launch_bounds__(1024) void k_pab_lists(PabView w, int* __restrict__ lists) {
  __shared__ int wave_cnt[2][16];
  __shared__ int base[2];
  __shared__ int hist[PH_COUNT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x < PH_COUNT) hist[threadIdx.x] = 0;
  if (threadIdx.x < 2) base[threadIdx.x] = 0;
  __syncthreads();
  for (int c0 = 0; c0 < w.K; c0 += 1024) {
    const int c = c0 + threadIdx.x;
    const int ph = c < w.K ? pab_ctl_load(w.ctl, c).phase : PH_DONE;
    if (c < w.K) atomicAdd(&hist[ph], 1);
    const bool in[2] = {ph != PH_DONE, ph != PH_DONE && ph != PH_LSMR0 && ph != PH_LSMR};
    unsigned long long bal[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      bal[k] = __ballot(in[k]);
      if (lane == 0) wave_cnt[k][wv] = __popcll(bal[k]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (in[k]) {
        int at = base[k] + __popcll(bal[k] & ((1ull << lane) - 1ull));
        for (int q = 0; q < wv; ++q) at += wave_cnt[k][q];
        lists[(size_t)k * w.K + at] = c;
      }
    __syncthreads();
    if (threadIdx.x < 2) {
      int t = 0;
      for (int q = 0; q < 16; ++q) t += wave_cnt[threadIdx.x][q];
      base[threadIdx.x] += t;
    }
    __syncthreads();
  }
  if (threadIdx.x < PH_COUNT) w.flags[threadIdx.x] = hist[threadIdx.x];
  if (threadIdx.x < 2) w.flags[10 + threadIdx.x] = base[threadIdx.x];
}

// ---- LSMR for every candidate inside a solve (st.l_on): rhs in MV_LU (m + n entries, zeros past m for the plain operator), result in NV_LX -----------------------------
// scipy.sparse.linalg.lsmr(A, b, atol, btol (in st), conlim = 1e8, maxiter): the same recurrences as hh_pa_lsmr.
// One iteration = 4 launches (5 on the general path):
//   forward   u = A v - alpha u, |u|^2      (+ the PREVIOUS iteration's h / hbar / x update and |x|^2, fused on the sliced
//                                             path, a separate element-wise launch on the general one)
//   scalar 1  the previous iteration's stopping tests (they need that |x|), then beta
//   backward  v = A^T u - beta v, |v|^2     (v is kept un-normalised, with 1 / alpha beside it)
//   scalar 2  alpha, the rotations, the coefficients of this iteration's update
// so a candidate learns that it has converged one forward product late: that product only touches u.
// pab_lsmr_start: candidates with st.start set begin a solve with their own operator (st.aug); pab_lsmr_ticks: `count`
// iterations for everyone inside a solve.  A candidate that stops moves on by itself (PH_LSMR0 -> PH_AFTER0, PH_LSMR ->
// PH_POST).
void pab_lsmr_start(hh_pab* p) {
  auto st = [] __device__(const auto& s) { return s.start != 0; };
  auto st_bwd = [] __device__(const auto& s) { return s.start != 0 && !s.l_skip; };
  const int nb_b = pab_nb_bwd(p);
  pab_vec<0>(p, CNT_N, PabRed<0>{}, st, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double*) {
    w.nvec(NV_LV, c)[i] = 0; w.nvec(NV_LX, c)[i] = 0; w.nvec(NV_LHBAR, c)[i] = 0;
  });
  pab_vec<1>(p, CNT_MAUG, pab_red<1>({RED_SUM}, {0}, p->nb_m), st,
             [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
               const double u = w.mvec(MV_LU, c)[i];
               acc[0] += u * u;
             });
  pab_scalar<1>(p, pab_red<1>({RED_SUM}, {0}, p->nb_m), st, [] __device__(const PabView&, int, PabState& s, const double* v) {
    s.normb = sqrt(v[0]);
    s.beta = s.normb;
    s.l_skip = !(s.beta > 0);
    s.inv_beta = s.beta > 0 ? 1.0 / s.beta : 0.0;
    s.neg_beta = 0.0;          // v = 0 * v + Op^T u
    s.inv_alpha = 1.0;
    s.l_on = 0;
    s.pend = 0;
    s.itn = 0; s.istop = 0;
  });
  pab_rmatvec<1>(p, MV_LU, NV_D, NV_ROOT, NV_LV, st_bwd);
  pab_scalar<1>(p, pab_red<1>({RED_SUM}, {1}, nb_b), st, [] __device__(const PabView&, int, PabState& s, const double* v) {
    s.alpha = s.beta > 0 ? sqrt(v[0]) : 0.0;
    s.inv_alpha = s.alpha > 0 ? 1.0 / s.alpha : 1.0;
    s.neg_alpha = -s.alpha;
    s.zetabar = s.alpha * s.beta; s.alphabar = s.alpha; s.rho = 1; s.rhobar = 1; s.cbar = 1; s.sbar = 0;
    s.betadd = s.beta; s.betad = 0; s.rhodold = 1; s.tautildeold = 0; s.thetatilde = 0; s.zeta = 0; s.dsum = 0;
    s.normA2 = s.alpha * s.alpha; s.maxrbar = 0; s.minrbar = 1e100; s.normx = 0;
    s.normr = s.beta; s.normar = s.alpha * s.beta;
    s.l_on = (s.normar != 0 && s.normb != 0) ? 1 : 0;
    s.l_skip = 0;
    ++s.lsmr_calls;
    if (!s.l_on) s.phase = s.phase == PH_LSMR0 ? PH_AFTER0 : PH_POST;   // x = 0 is the answer
  });
  pab_vec<0>(p, CNT_N, PabRed<0>{}, st, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
#pragma clang fp contract(off)
    w.nvec(NV_LH, c)[i] = w.nvec(NV_LV, c)[i] * s.inv_alpha;   // h = v
  });
  pab_scalar<0>(p, PabRed<0>{}, st, [] __device__(const PabView&, int, PabState& s, const double*) { s.start = 0; });
}

void pab_lsmr_ticks(hh_pab* p, int count, int maxiter) {
  auto on = [] __device__(const auto& s) { return s.l_on != 0; };
  auto on_bwd = [] __device__(const auto& s) { return s.l_on != 0 && !s.l_skip; };
  auto on_pend = [] __device__(const auto& s) { return s.l_on != 0 && s.pend != 0; };
  const int nb_f = pab_nb_fwd(p, true), nb_b = pab_nb_bwd(p);
  const bool sliced = p->sliced != 0;
  for (int t = 0; t < count; ++t) {
    if (!sliced)
      pab_vec<1>(p, CNT_N, pab_red<1>({RED_SUM}, {2}, p->nb_n), on_pend,
                 [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
                   const double x = pab_deferred_update(w, c, i, s, w.nvec(NV_LV, c)[i] * s.inv_alpha);
                   acc[0] += x * x;
                 });
    pab_matvec<1>(p, NV_LV, NV_D, NV_ROOT, MV_LU, on);
    {
      PabRed<5> r2{};
      r2.kind[0] = r2.kind[1] = r2.kind[2] = RED_SUM; r2.slot[0] = 0; r2.slot[1] = 2; r2.slot[2] = 3;
      r2.kind[3] = RED_MIN; r2.kind[4] = RED_MAX; r2.slot[3] = r2.slot[4] = 4;
      r2.nb[0] = nb_f; r2.nb[1] = sliced ? nb_f : p->nb_n; r2.nb[2] = r2.nb[3] = r2.nb[4] = sliced ? nb_f : 0;
      pab_scalar<5>(p, r2, on, [maxiter, sliced] __device__(const PabView& w, int cidx, PabState& s, const double* v) {
        // self-check: every slice workgroup of the forward pass must have seen the same `pend` as this step does,
        // and every partial this step reads must carry this iteration's tag
        if (sliced && v[2] != (s.pend ? (double)w.fwd_main : 0.0)) atomicAdd(&w.flags[8], 1);
        if (sliced && (v[3] != (double)s.itn || v[4] != (double)s.itn)) atomicAdd(&w.flags[8], 1000);
        if (w.trace_c >= 0 && cidx == w.trace_c && s.lsmr_iters < PAB_TRACE_ROWS) {
          double* t = w.trace + (size_t)s.lsmr_iters * 8;
          t[0] = s.pend; t[1] = v[0]; t[2] = v[1]; t[3] = s.normr; t[4] = s.normA; t[5] = s.alpha; t[6] = s.beta; t[7] = s.normar;
        }
        if (s.pend) {   // the stopping tests of the iteration whose update has just been applied
          s.normx = sqrt(v[1]);
          const double normA = s.normA, condA = s.condA;
          const double test1 = s.normr / s.normb;
          const double test2 = (normA * s.normr) != 0 ? s.normar / (normA * s.normr) : INFINITY;
          const double test3 = 1 / condA;
          const double t1 = test1 / (1 + normA * s.normx / s.normb);
          const double rtol = s.btol + s.atol * normA * s.normx / s.normb;
          const double ctol = 1e-8;   // conlim = 1e8
          int istop = 0;
          if (s.itn >= maxiter) istop = 7;
          if (1 + test3 <= 1) istop = 6;
          if (1 + test2 <= 1) istop = 5;
          if (1 + t1 <= 1) istop = 4;
          if (test3 <= ctol) istop = 3;
          if (test2 <= s.atol) istop = 2;
          if (test1 <= rtol) istop = 1;
          s.istop = istop;
          s.pend = 0;
          if (istop > 0) {   // the solve is over: on to the next phase of this candidate
            s.l_on = 0;
            s.phase = s.phase == PH_LSMR0 ? PH_AFTER0 : PH_POST;
            return;
          }
        }
        s.beta = sqrt(v[0]);
        s.l_skip = !(s.beta > 0);
        s.inv_beta = s.beta > 0 ? 1.0 / s.beta : 0.0;
        s.neg_beta = -s.beta;
      });
    }
    pab_rmatvec<1>(p, MV_LU, NV_D, NV_ROOT, NV_LV, on_bwd);
    pab_scalar<1>(p, pab_red<1>({RED_SUM}, {1}, nb_b), on, [] __device__(const PabView&, int, PabState& s, const double* v) {
      ++s.itn;
      ++s.lsmr_iters;
      if (!s.l_skip) {
        s.alpha = sqrt(v[0]);
        s.inv_alpha = s.alpha > 0 ? 1.0 / s.alpha : 1.0;
      }
      s.neg_alpha = -s.alpha;
      const double alpha = s.alpha, beta = s.beta;
      double chat, shat, alphahat, c, sn;
      pab_sym_ortho(s.alphabar, 0.0, chat, shat, alphahat);
      const double rhoold = s.rho;
      pab_sym_ortho(alphahat, beta, c, sn, s.rho);
      const double thetanew = sn * alpha;
      s.alphabar = c * alpha;
      const double rhobarold = s.rhobar, zetaold = s.zeta;
      const double thetabar = s.sbar * s.rho, rhotemp = s.cbar * s.rho;
      pab_sym_ortho(s.cbar * s.rho, thetanew, s.cbar, s.sbar, s.rhobar);
      s.zeta = s.cbar * s.zetabar;
      s.zetabar = -s.sbar * s.zetabar;
      s.c_hbar = -(thetabar * s.rho / (rhoold * rhobarold));
      s.c_x = s.zeta / (s.rho * s.rhobar);
      s.c_h = -(thetanew / s.rho);
      const double betaacute = chat * s.betadd, betacheck = -shat * s.betadd;
      const double betahat = c * betaacute;
      s.betadd = -sn * betaacute;
      const double thetatildeold = s.thetatilde;
      double ctildeold, stildeold, rhotildeold;
      pab_sym_ortho(s.rhodold, thetabar, ctildeold, stildeold, rhotildeold);
      s.thetatilde = stildeold * s.rhobar;
      s.rhodold = ctildeold * s.rhobar;
      s.betad = -stildeold * s.betad + ctildeold * betahat;
      s.tautildeold = (zetaold - thetatildeold * s.tautildeold) / rhotildeold;
      const double taud = (s.zeta - s.thetatilde * s.tautildeold) / s.rhodold;
      s.dsum += betacheck * betacheck;
      s.normr = sqrt(s.dsum + (s.betad - taud) * (s.betad - taud) + s.betadd * s.betadd);
      s.normA2 += beta * beta;
      s.normA = sqrt(s.normA2);
      s.normA2 += alpha * alpha;
      s.maxrbar = fmax(s.maxrbar, rhobarold);
      if (s.itn > 1) s.minrbar = fmin(s.minrbar, rhobarold);
      s.condA = fmax(s.maxrbar, rhotemp) / fmin(s.minrbar, rhotemp);
      s.normar = fabs(s.zetabar);
      s.pend = 1;   // the h / hbar / x update and the tests follow with the next forward pass
    });
    ++p->ticks;
  }
}

// ---- the set-up of a batch (hh_pab_create_ex): phases, in the order they run ------------------------------------------------
// Every phase returns HH_OK, or a code with p->err set; its temporaries are its locals and end with it on every way out.
// PabBuild holds what more than one phase reads.  Two of its members are device / host memory that crosses phases and is
// freed where it is last read: d_b_int (row phases -> pab_build_tables) and rows16_of (pab_build_sym_host -> pab_build_tables).
struct PabBuild {
  const hh_pa_params* qs;
  int count, flags;
  const float* image;
  int ny, nx, d2, l2, l3, d3;
  double rmin, rmax;
  static constexpr int chunk = 8;          // operations per sweep of the row enumeration
  std::vector<int> rank;                   // voxel ranks of the (L3d, D2d, D2d) box
  std::vector<int> n_ops;
  PabGeomRef gr{};
  bool dev_rows = false, dev_sym = false;
  std::vector<int> srow_h;                 // [count][mz + 1] (device rows)
  DevBuf<float> d_b_int;                   // device-order b of the data rows
  std::vector<std::vector<int>> ray_of_row;      // host rows, per candidate: ray, b, pixel id and slice of every row
  std::vector<std::vector<float>> b_of;
  std::vector<std::vector<int32_t>> pid_of;
  std::vector<std::vector<short>> z_of;
  std::vector<std::vector<int2>> pairs_of;       // host symmetry rows, per candidate
  std::vector<std::vector<PaEll16>> rows16_of;   // (trilinear: the 16-entry rows)
  bool timing = std::getenv("HH_PAB_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
  size_t rays() const { return (size_t)l2 * d2; }
  void lap(hh_pab* p, const char* what) {
    if (!timing) return;
    (void)hipStreamSynchronize(p->stream);
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "hh_pab_create[%d]: %-28s %8.2f ms\n", count, what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  }
};

// a buffer of the object holding a host table
template <class T>
int pab_upload(hh_pab* p, DevBuf<T>& buf, const std::vector<T>& v) {
  if (int rc = pab_alloc(p, buf, v.size())) return rc;
  return pab_to_device(p, buf, v.data(), v.size() * sizeof(T));
}

// the arguments of hh_pab_create_ex (no object yet: messages go to g_create_error); the box of the batch -> d2, l2, l3
int pab_check_args(hh_pab** out, const float* image, int ny, int nx, const hh_pa_params* qs, int count, int flags, int& d2, int& l2, int& l3) {
  if (!out || !image || !qs || count < 1) return pab_fail(nullptr, HH_ERR_ARG, "hh_pab_create: bad argument");
  if (flags & ~(HH_PAB_ALLOW_BANDED | HH_PAB_FORCE_BANDED)) return pab_fail(nullptr, HH_ERR_ARG, "hh_pab_create_ex: unknown flags");
  *out = nullptr;
  const hh_pa_params& q0 = qs[0];
  d2 = q0.reconstruct_diameter_2d_pixel > 0 ? q0.reconstruct_diameter_2d_pixel : ny;
  l2 = q0.reconstruct_length_2d_pixel > 0 ? q0.reconstruct_length_2d_pixel : nx;
  l3 = q0.reconstruct_length_3d_pixel > 0 ? q0.reconstruct_length_3d_pixel : l2;
  if (d2 > ny || l2 > nx || d2 < 2 || l2 < 2) return pab_fail(nullptr, HH_ERR_ARG, "hh_pab_create: 2-D region does not fit the image");
  for (int c = 0; c < count; ++c) {
    const hh_pa_params& q = qs[c];
    if (!(q.rise_pixel > 0) || q.csym < 1 || q.twist_degree == 0.0)
      return pab_fail(nullptr, HH_ERR_ARG, "hh_pab_create: rise must be positive, csym >= 1, twist non-zero");
    if ((q.interpolation != 0 && q.interpolation != 1) || q.interpolation != q0.interpolation)
      return pab_fail(nullptr, HH_ERR_ARG, "hh_pab_create: interpolation must be 0 (nearest neighbour) or 1 (trilinear), the same for the whole batch");
    if (q.reconstruct_diameter_2d_pixel != q0.reconstruct_diameter_2d_pixel || q.reconstruct_length_2d_pixel != q0.reconstruct_length_2d_pixel ||
        q.reconstruct_diameter_3d_pixel != q0.reconstruct_diameter_3d_pixel || q.reconstruct_length_3d_pixel != q0.reconstruct_length_3d_pixel ||
        q.reconstruct_diameter_3d_inner_pixel != q0.reconstruct_diameter_3d_inner_pixel)
      return pab_fail(nullptr, HH_ERR_ARG, "hh_pab_create: the candidates of one batch share the reconstruction box");
    if (q.fsc_half < 0 || q.fsc_half > 2 || (q.fsc_half > 0 && (q.fsc_mode < 1 || (q.fsc_mode == 1 && (!q.fsc_ids || q.n_fsc_ids < 0)))))
      return pab_fail(nullptr, HH_ERR_ARG, "hh_pab_create: half sets need fsc_half 1 or 2 and fsc_mode 2, 3, 4, or 1 with fsc_ids");
  }
  return HH_OK;
}

// device and stream; the unknowns (shared by the batch): voxels of the cylinder in the (L3d, D2d, D2d) box, C-order rank
// (solver:1375-1387); the form of the products
int pab_build_form(hh_pab* p, PabBuild& b) {
  const int device = p->device, count = b.count, d2 = b.d2, l3 = b.l3, flags = b.flags;
  PAB_HIP(p, hipSetDevice(device));
  PAB_HIP(p, hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  PAB_HIP(p, hipHostMalloc(reinterpret_cast<void**>(&p->h_flags), PAB_FLAG_WORDS * sizeof(int), hipHostMallocDefault));
  p->n = pa_mask_rank(l3, d2, d2, b.rmin, b.rmax, b.rank);
  if (p->n <= 0) return pab_fail(p, HH_ERR_ARG, "hh_pab_create: the cylinder holds no voxel");
  p->mz = l3;
  p->nslice = (int)(p->n / l3);   // the same disk in every slice
  p->flat = 1;
  for (int c = 0; c < count; ++c) p->flat = p->flat && b.qs[c].tilt_degree == 0.0 && b.qs[c].psi_degree == 0.0;
  const bool flat = p->flat && std::getenv("HH_PAB_GENERAL") == nullptr;
  p->sliced = flat && (int64_t)p->nslice * l3 == p->n && p->nslice < 0xffff && (size_t)p->nslice * sizeof(double) <= (size_t)60 << 10;
  p->linear = b.qs[0].interpolation;
  if (p->linear) {   // two planes of x and the disc's table in LDS; no general (tilt / psi) form of the trilinear products here
    p->lin_lds = (size_t)2 * p->nslice * sizeof(double) + (size_t)d2 * d2 * sizeof(unsigned);
    const bool slice_major = flat && (int64_t)p->nslice * l3 == p->n && p->nslice < 0xffff;
    const bool lds_fits = p->lin_lds <= (size_t)150 << 10;
    // (band_T is set once the bands are cut, in pab_build_banded; this marks the form)
    p->band_T = slice_major && ((flags & HH_PAB_FORCE_BANDED) || (!lds_fits && (flags & HH_PAB_ALLOW_BANDED))) ? -1 : 0;
    p->sliced = slice_major && (lds_fits || p->band_T);
    if (!p->sliced)
      return pab_fail(p, HH_ERR_ARG,
                      slice_major ? "hh_pab_create: not sliceable — the batched trilinear projector's LDS form needs two planes of the cylinder in LDS "
                                    "(hh_pab_create_ex with HH_PAB_ALLOW_BANDED has the banded form)"
                                  : "hh_pab_create: not sliceable — the batched trilinear projector needs tilt = psi = 0 "
                                    "(the single-candidate hh_pa has the general form)");
  }
  return pab_upload(p, p->d_rank, b.rank);
}

// geometry and symmetry operations of every candidate, in the reference's order (solver:1556-1571)
int pab_build_geometry(hh_pab* p, PabBuild& b) {
  const int count = b.count, d2 = b.d2, l2 = b.l2, l3 = b.l3;
  std::vector<PaGeom> geoms((size_t)count);
  std::vector<PaOp> ops;
  std::vector<int64_t> op0((size_t)count);
  b.n_ops.assign((size_t)count, 0);
  for (int c = 0; c < count; ++c) {
    const hh_pa_params& q = b.qs[c];
    PaGeom& g = geoms[(size_t)c];
    g.linear = q.interpolation;
    g.L2 = l2; g.D2 = d2; g.mz = l3; g.my = d2; g.mx = d2;
    g.scale = q.scale2d_to_3d;
    g.dy = q.dy_pixel;
    pa_euler1('y', 90.0, g.m_y90);
    double qy[4], qx[4], qq[4];
    pa_quat_axis('y', q.tilt_degree, qy);
    pa_quat_axis('x', q.psi_degree, qx);
    pa_quat_mul(qx, qy, qq);
    pa_quat_matrix(qq, g.m_yx);
    const int hmax = std::max(1, (int)(std::ceil((double)(l3 + l2)) / 2 / q.rise_pixel));
    struct Hc { int h, c; };
    std::vector<Hc> hcs;
    for (int h = -hmax; h <= hmax; ++h)
      for (int cc = 0; cc < q.csym; ++cc) hcs.push_back({h, cc});
    std::stable_sort(hcs.begin(), hcs.end(), [](const Hc& a, const Hc& b) {
      return std::abs(a.h) != std::abs(b.h) ? std::abs(a.h) < std::abs(b.h) : a.c < b.c;
    });
    const std::vector<int64_t> order = pa_halton((int64_t)hcs.size());
    op0[(size_t)c] = (int64_t)ops.size();
    b.n_ops[(size_t)c] = (int)order.size();
    for (size_t i = 0; i < order.size(); ++i) {
      const Hc& s = hcs[(size_t)order[i]];
      PaOp op;
      pa_euler1('z', q.twist_degree * s.h + 360.0 * s.c / q.csym, op.m_z);
      op.shift = s.h * q.rise_pixel;
      ops.push_back(op);
    }
  }
  if (p->linear) {   // what pabl_ray / pabl_at drop from pa_coords must be exactly what it says
    bool ok = true;
    for (const PaGeom& g : geoms) {
      const double id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      for (int t = 0; t < 9; ++t) ok = ok && g.m_yx[t] == id[t];
    }
    for (const PaOp& op : ops) ok = ok && op.m_z[2] == 0 && op.m_z[5] == 0 && op.m_z[6] == 0 && op.m_z[7] == 0;
    if (!ok) return pab_fail(p, HH_ERR_STATE, "hh_pab_create: the rotations are not of the form the trilinear ray arithmetic assumes (internal)");
  }
  if (int rc = pab_upload(p, p->d_geom, geoms)) return rc;
  if (int rc = pab_upload(p, p->d_ops, ops)) return rc;
  if (int rc = pab_upload(p, p->d_op0, op0)) return rc;
  b.gr = PabGeomRef{p->d_geom, p->d_ops, p->d_op0};
  return HH_OK;
}

// The first pass of both row enumerations: which rays exist, operation chunk by chunk, until every candidate has passed
// its row target (solver:1647).  Per chunk: the live candidates' codes (k_pab_has / k_pabl_has), read_back(live) brings
// what the host looks at, and per_op(slot, candidate, operation of the chunk, lo) takes one operation in and returns the
// candidate's rows so far.
template <class ReadBack, class PerOp>
int pab_rows_first_pass(hh_pab* p, PabBuild& b, int* d_cand, const int* d_nops, unsigned char* d_has, ReadBack read_back, PerOp per_op) {
  const int count = b.count, chunk = b.chunk;
  const size_t rays = b.rays();
  std::vector<int> live((size_t)count);
  for (int c = 0; c < count; ++c) live[(size_t)c] = c;
  for (int lo = 0; !live.empty(); lo += chunk) {
    if (int rc = pab_to_device(p, d_cand, live.data(), live.size() * sizeof(int))) return rc;
    hipLaunchKernelGGL(p->linear ? k_pabl_has : k_pab_has, dim3((unsigned)((rays + 255) / 256), chunk, (unsigned)live.size()), dim3(256), 0, p->stream,
                       b.gr, d_cand, lo, chunk, d_nops, p->d_rank, d_has);
    if (int rc = read_back(live.size())) return rc;
    std::vector<int> next;
    for (size_t sl = 0; sl < live.size(); ++sl) {
      const int c = live[sl];
      bool done = false;
      for (int o = 0; o < chunk && lo + o < b.n_ops[(size_t)c] && !done; ++o) {
        const int64_t rows = per_op(sl, c, o, lo);
        p->n_ops_used[(size_t)c] = lo + o + 1;
        if (b.qs[c].min_projection_lines > 0 && rows > b.qs[c].min_projection_lines) done = true;
      }
      if (!done && lo + chunk < b.n_ops[(size_t)c]) next.push_back(c);
    }
    live.swap(next);
  }
  return HH_OK;
}

// Row enumeration on the device: per chunk of operations the codes are counted per slice, the host decides from the
// counts alone which operations each candidate uses, and a second sweep over the used chunks writes the rows where they
// belong — no per-ray data crosses PCIe.  Leaves d_b_int for pab_build_tables.
int pab_build_rows_device(hh_pab* p, PabBuild& b) {
  const int count = b.count, chunk = b.chunk, ny = b.ny, nx = b.nx, l2 = b.l2, d2 = b.d2;
  const size_t rays = b.rays();
  const int mz1 = p->mz + 1;
  DevArena tmp;
  int* d_cand = tmp.get<int>((size_t)count);
  int* d_nops = tmp.get<int>((size_t)count);
  unsigned char* d_has = tmp.get<unsigned char>((size_t)count * chunk * rays);
  int* d_counts = tmp.get<int>((size_t)count * chunk * mz1);
  int* d_bmax = tmp.get<int>((size_t)count);
  float* d_image = tmp.get<float>((size_t)ny * nx);
  long long* d_bref_t = tmp.get<long long>((size_t)count * chunk);
  long long* d_bint_t = tmp.get<long long>((size_t)count * chunk * mz1);
  long long* d_row0_t = tmp.get<long long>((size_t)count);
  if (int rc = pab_arena_ok(p, tmp)) return rc;
  if (int rc = pab_to_device(p, d_nops, b.n_ops.data(), b.n_ops.size() * sizeof(int))) return rc;
  if (int rc = pab_to_device(p, d_image, b.image, (size_t)ny * nx * sizeof(float))) return rc;
  // pass 1: counts per (candidate, operation, slice)
  std::vector<std::vector<int>> cnt3((size_t)count);   // [operation][mz + 1], the operations used
  std::vector<int64_t> rows_so_far((size_t)count, 0);
  std::vector<int> counts_h;
  const int rc1 = pab_rows_first_pass(
      p, b, d_cand, d_nops, d_has,
      [&](size_t nl) {
        hipLaunchKernelGGL(k_pab_count_codes, dim3(chunk, (unsigned)nl), dim3(256), (size_t)mz1 * sizeof(int), p->stream, d_has, rays, chunk, p->mz,
                           d_counts);
        counts_h.resize(nl * chunk * mz1);
        return pab_to_host(p, counts_h.data(), d_counts, counts_h.size() * sizeof(int));
      },
      [&](size_t sl, int c, int o, int) {
        const int* cz = counts_h.data() + (sl * chunk + o) * mz1;
        int64_t tot = 0;
        for (int z = 0; z < mz1; ++z) tot += cz[z];
        if (cz[p->mz] > 0) p->sliced = 0;   // a ray in two slices: the whole batch takes the general products
        cnt3[(size_t)c].insert(cnt3[(size_t)c].end(), cz, cz + mz1);
        return rows_so_far[(size_t)c] += tot;
      });
  if (rc1) return rc1;
  // the row tables' geometry: first row of every candidate, of every slice (device order), of every operation
  int max_used = 0;
  b.srow_h.assign((size_t)count * mz1, 0);
  for (int c = 0; c < count; ++c) {
    if (rows_so_far[(size_t)c] == 0) return pab_fail(p, HH_ERR_ARG, "hh_pab_create: no projection ray of a candidate meets the cylinder");
    PabState& st = p->st[(size_t)c];
    st.m_data = rows_so_far[(size_t)c];
    st.row0 = p->total_rows;
    p->total_rows += st.m_data;
    max_used = std::max(max_used, p->n_ops_used[(size_t)c]);
    if (p->sliced) {
      int* sr = b.srow_h.data() + (size_t)c * mz1;
      for (int o = 0; o < p->n_ops_used[(size_t)c]; ++o)
        for (int z = 0; z < p->mz; ++z) sr[z + 1] += cnt3[(size_t)c][(size_t)o * mz1 + z];
      for (int z = 0; z < p->mz; ++z) sr[z + 1] += sr[z];
    }
  }
  const size_t rows1 = std::max<size_t>((size_t)p->total_rows, 1);
  if (!p->d_ray_of_row.ensure(rows1) || !b.d_b_int.ensure(rows1) || !p->d_bref.ensure(rows1) || !p->d_pidref.ensure(rows1))
    return pab_fail(p, HH_ERR_NOMEM, "hh_pab_create: " + dev_alloc_failed(rows1 * 4));
  if (hipError_t e2 = hipMemsetAsync(d_bmax, 0x80, (size_t)count * sizeof(int), p->stream))   // very negative ordered keys
    return pab_fail(p, HH_ERR_HIP, std::string("hh_pab_create: ") + hipGetErrorString(e2));
  p->device_bytes += (size_t)p->total_rows * 16;
  // pass 2: the rows themselves, chunk by chunk over the operations that are used
  std::vector<long long> bref_h, bint_h, row0_h;
  std::vector<int> live;
  for (int lo = 0; lo < max_used; lo += chunk) {
    live.clear();
    for (int c = 0; c < count; ++c)
      if (p->n_ops_used[(size_t)c] > lo) live.push_back(c);
    const size_t nl = live.size();
    bref_h.assign(nl * chunk, -1);
    bint_h.assign(nl * chunk * mz1, 0);
    row0_h.resize(nl);
    for (size_t sl = 0; sl < nl; ++sl) {
      const int c = live[sl];
      row0_h[sl] = p->st[(size_t)c].row0;
      pab_row_offsets(cnt3[(size_t)c].data(), p->n_ops_used[(size_t)c], p->mz, p->sliced != 0, b.srow_h.data() + (size_t)c * mz1, lo, chunk,
                      bref_h.data() + sl * chunk, bint_h.data() + sl * chunk * mz1);
    }
    if (int rc = pab_to_device(p, d_cand, live.data(), nl * sizeof(int))) return rc;
    if (int rc = pab_to_device(p, d_bref_t, bref_h.data(), bref_h.size() * sizeof(long long))) return rc;
    if (int rc = pab_to_device(p, d_bint_t, bint_h.data(), bint_h.size() * sizeof(long long))) return rc;
    if (int rc = pab_to_device(p, d_row0_t, row0_h.data(), nl * sizeof(long long))) return rc;
    hipLaunchKernelGGL(p->linear ? k_pabl_has : k_pab_has, dim3((unsigned)((rays + 255) / 256), chunk, (unsigned)nl), dim3(256), 0, p->stream, b.gr,
                       d_cand, lo, chunk, d_nops, p->d_rank, d_has);
    const PabEmit em{d_has, d_image, d_bref_t, d_bint_t, d_row0_t, d_cand, p->d_ray_of_row, b.d_b_int, p->d_bref, p->d_pidref, d_bmax,
                     chunk, lo, p->mz, l2, d2, ny, nx};
    hipLaunchKernelGGL(k_pab_emit, dim3(chunk, (unsigned)nl), dim3(1024), 0, p->stream, em);
  }
  std::vector<int> bm((size_t)count);
  if (int rc = pab_to_host(p, bm.data(), d_bmax, bm.size() * sizeof(int))) return rc;
  for (int c = 0; c < count; ++c) {
    const int key = bm[(size_t)c], bits = key >= 0 ? key : key ^ 0x7fffffff;
    float f;
    std::memcpy(&f, &bits, sizeof(f));
    p->st[(size_t)c].bmax = (double)f;
  }
  return HH_OK;
}

// Row enumeration on the host (half sets, whose pixel-id rules are host code, and HH_PAB_HOST_ROWS: the A/B reference of
// the tests): the per-ray codes come back and the rows are listed here; then the half sets (split_A_b, solver:175-203)
int pab_build_rows_host(hh_pab* p, PabBuild& b) {
  const int count = b.count, chunk = b.chunk, ny = b.ny, nx = b.nx, l2 = b.l2, d2 = b.d2;
  const size_t rays = b.rays();
  b.ray_of_row.assign((size_t)count, {});
  b.b_of.assign((size_t)count, {});
  b.pid_of.assign((size_t)count, {});
  b.z_of.assign((size_t)count, {});
  {
    std::vector<unsigned char> has;
    DevArena tmp;
    int* d_cand = tmp.get<int>((size_t)count);
    int* d_nops = tmp.get<int>((size_t)count);
    unsigned char* d_has = tmp.get<unsigned char>((size_t)count * chunk * rays);
    if (int rc = pab_arena_ok(p, tmp)) return rc;
    if (int rc = pab_to_device(p, d_nops, b.n_ops.data(), b.n_ops.size() * sizeof(int))) return rc;
    const int rc1 = pab_rows_first_pass(
        p, b, d_cand, d_nops, d_has,
        [&](size_t nl) {
          has.resize(nl * chunk * rays);
          return pab_to_host(p, has.data(), d_has, has.size());
        },
        [&](size_t sl, int c, int o, int lo) {
          const unsigned char* h = has.data() + (sl * chunk + o) * rays;
          // rows of this operation, in (k, j) order; b = pixel_vals[j, k], pid = k * ny + j (solver:1548-1549)
          for (int k = 0; k < l2; ++k)
            for (int j = 0; j < d2; ++j)
              if (h[(size_t)k * d2 + j]) {
                const unsigned char code = h[(size_t)k * d2 + j];
                if (code == 255) p->sliced = 0;   // a ray in two slices: the whole batch takes the general products
                b.z_of[(size_t)c].push_back((short)(code - 1));
                b.ray_of_row[(size_t)c].push_back((int)(((size_t)(lo + o) * l2 + k) * d2 + j));
                b.b_of[(size_t)c].push_back(b.image[(size_t)(j - d2 / 2 + ny / 2) * nx + (k - l2 / 2 + nx / 2)]);
                b.pid_of[(size_t)c].push_back(k * d2 + j);
              }
          return (int64_t)b.ray_of_row[(size_t)c].size();
        });
    if (rc1) return rc1;
  }
  b.lap(p, "rays that exist");
  for (int c = 0; c < count; ++c) {
    const hh_pa_params& q = b.qs[c];
    std::vector<int>& rr = b.ray_of_row[(size_t)c];
    std::vector<float>& bb = b.b_of[(size_t)c];
    std::vector<int32_t>& pp = b.pid_of[(size_t)c];
    std::vector<short>& zz = b.z_of[(size_t)c];
    if (q.fsc_half > 0) {
      const std::vector<size_t> keep = pab_half_rows(pp, q.fsc_mode, q.fsc_half, q.fsc_ids, q.n_fsc_ids);
      for (size_t wr = 0; wr < keep.size(); ++wr) {
        const size_t r = keep[wr];
        rr[wr] = rr[r]; bb[wr] = bb[r]; pp[wr] = pp[r]; zz[wr] = zz[r];
      }
      rr.resize(keep.size()); bb.resize(keep.size()); pp.resize(keep.size()); zz.resize(keep.size());
    }
    if (rr.empty()) return pab_fail(p, HH_ERR_ARG, "hh_pab_create: no projection ray of a candidate meets the cylinder");
    PabState& s = p->st[(size_t)c];
    s.m_data = (int64_t)rr.size();
    s.row0 = p->total_rows;
    p->total_rows += s.m_data;
    s.bmax = (double)*std::max_element(bb.begin(), bb.end());
  }
  return HH_OK;
}

// the data rows: on the device unless a candidate is a half set or HH_PAB_HOST_ROWS asks for the host path
int pab_build_rows(hh_pab* p, PabBuild& b) {
  p->n_ops_used.assign((size_t)b.count, 0);
  p->st.assign((size_t)b.count, PabState{});
  b.dev_rows = std::getenv("HH_PAB_HOST_ROWS") == nullptr;
  for (int c = 0; c < b.count; ++c) b.dev_rows = b.dev_rows && b.qs[c].fsc_half == 0;
  if (!b.dev_rows) return pab_build_rows_host(p, b);
  if (int rc = pab_build_rows_device(p, b)) return rc;
  b.lap(p, "rays and rows (device)");
  return HH_OK;
}

// symmetry rows on host threads through the single-candidate builder, one candidate per thread (HH_PAB_HOST_SYM: the A/B
// reference of the tests; trilinear: the 16-entry rows of solver:910-1140).  Leaves rows16_of for pab_build_tables.
int pab_build_sym_host(hh_pab* p, PabBuild& b) {
  const int count = b.count;
  const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const unsigned nt = std::min<unsigned>(hw, (unsigned)count);
  std::atomic<int> next{0};
  std::atomic<bool> threw{false};
  auto work = [&] {   // (a thread's body must not let an exception out: that is std::terminate whatever the caller guards)
    try {
      for (int c = next.fetch_add(1); c < count; c = next.fetch_add(1)) {
        const hh_pa_params& q = b.qs[c];
        if (q.min_sym_pairs > 0)
          pa_sym_pairs(b.l3, b.d3, b.d3, q.twist_degree, q.rise_pixel, q.csym, b.rmin, b.rmax, q.min_sym_pairs, b.pairs_of[(size_t)c],
                       p->linear ? &b.rows16_of[(size_t)c] : nullptr);
      }
    } catch (...) {
      threw = true;
    }
  };
  {
    std::vector<std::thread> pool;
    struct Join { std::vector<std::thread>& p; ~Join() { for (auto& t : p) if (t.joinable()) t.join(); } } join{pool};
    for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
  }
  if (threw) return pab_fail(p, HH_ERR_NOMEM, "hh_pab_create: out of host memory while building the symmetry pairs");
  for (int c = 0; c < count; ++c) {
    PabState& s = p->st[(size_t)c];
    s.m_sym = (int64_t)(p->linear ? b.rows16_of[(size_t)c].size() : b.pairs_of[(size_t)c].size());
    s.sym0 = p->total_sym;
    p->total_sym += s.m_sym;
  }
  return HH_OK;
}

// symmetry pairs on the device (k_pab_sym): the walk of every candidate in chunks of operations, until it has its pairs
int pab_build_sym_device(hh_pab* p, PabBuild& b) {
  const int count = b.count, l3 = b.l3, d3 = b.d3;
  const hh_pa_params* qs = b.qs;
  int64_t want = 0;
  for (int c = 0; c < count; ++c) want = std::max<int64_t>(want, qs[c].min_sym_pairs);
  const int64_t cap = want > 0 ? want + p->n : 0;   // rows of a candidate: < min_sym_pairs before its last pair, which adds <= n
  for (int c = 0; c < count; ++c) p->st[(size_t)c].sym0 = (int64_t)c * cap;
  if (int rc = pab_alloc(p, p->d_pairs, (size_t)count * cap)) return rc;
  if (cap <= 0) return HH_OK;
  const int sym_chunk = 4;
  const int64_t nbox = (int64_t)l3 * d3 * d3;
  int* d_rank_sym = p->d_rank;
  DevArena tmp;
  int rc_rank = HH_OK;
  if (d3 != b.d2) {   // the symmetry box has its own rank table (same cylinder, same ranks, other box)
    std::vector<int> rank3;
    const int64_t n3 = pa_mask_rank(l3, d3, d3, b.rmin, b.rmax, rank3);
    if (n3 != p->n) return pab_fail(p, HH_ERR_ARG, "hh_pab_create: the cylinder does not fit the 2-D region's box");
    d_rank_sym = tmp.get<int>(rank3.size());
    if (tmp.ok()) rc_rank = pab_to_device(p, d_rank_sym, rank3.data(), rank3.size() * sizeof(int));
  }
  unsigned T = 1;
  while ((int64_t)T < 2 * (want + (int64_t)sym_chunk * p->n)) T <<= 1;
  unsigned long long* d_keys = tmp.get<unsigned long long>((size_t)count * T);
  unsigned long long* d_tmin = tmp.get<unsigned long long>((size_t)count * T);
  PaSymOp* d_sops = tmp.get<PaSymOp>((size_t)count * sym_chunk);
  int* d_cand = tmp.get<int>((size_t)count);
  int* d_nvalid = tmp.get<int>((size_t)count);
  int* d_counts = tmp.get<int>((size_t)count * sym_chunk);
  long long* d_base = tmp.get<long long>((size_t)count * sym_chunk);
  unsigned char* d_flags8 = tmp.get<unsigned char>((size_t)count * sym_chunk * nbox);
  int* d_err = tmp.get<int>(1);
  if (rc_rank) return rc_rank;
  if (int rc = pab_arena_ok(p, tmp)) return rc;
  hipError_t e = hipMemsetAsync(d_keys, 0xff, (size_t)count * T * 8, p->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_tmin, 0xff, (size_t)count * T * 8, p->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, sizeof(int), p->stream);
  if (e != hipSuccess) return pab_fail(p, HH_ERR_HIP, std::string("hh_pab_create (symmetry pairs): ") + hipGetErrorString(e));
  // the walk of every candidate (cheap: a few rotations per pair of operations)
  std::vector<std::vector<PaSymOp>> walk((size_t)count);
  std::vector<int> live;
  for (int c = 0; c < count; ++c)
    if (qs[c].min_sym_pairs > 0) {
      walk[(size_t)c] = pa_sym_ops(l3, qs[c].twist_degree, qs[c].rise_pixel, qs[c].csym);
      if (!walk[(size_t)c].empty()) live.push_back(c);
    }
  std::vector<int64_t> kept((size_t)count, 0);
  std::vector<PaSymOp> ops_h;
  std::vector<int> nvalid_h, counts_h;
  std::vector<long long> base_h;
  for (int p0 = 0; !live.empty(); p0 += sym_chunk) {
    const size_t nl = live.size();
    ops_h.assign(nl * sym_chunk, PaSymOp{});
    nvalid_h.assign(nl, 0);
    for (size_t sl = 0; sl < nl; ++sl) {
      const std::vector<PaSymOp>& wk = walk[(size_t)live[sl]];
      nvalid_h[sl] = (int)std::min<size_t>(sym_chunk, wk.size() - (size_t)p0);
      for (int k = 0; k < nvalid_h[sl]; ++k) ops_h[sl * sym_chunk + k] = wk[(size_t)p0 + k];
    }
    if (int rc = pab_to_device(p, d_sops, ops_h.data(), ops_h.size() * sizeof(PaSymOp))) return rc;
    if (int rc = pab_to_device(p, d_cand, live.data(), nl * sizeof(int))) return rc;
    if (int rc = pab_to_device(p, d_nvalid, nvalid_h.data(), nl * sizeof(int))) return rc;
    (void)hipMemsetAsync(d_counts, 0, nl * sym_chunk * sizeof(int), p->stream);
    PabSymRef sr{d_sops, d_cand, d_nvalid, sym_chunk, p0, l3, d3, d3, d_rank_sym, d_keys, d_tmin, T, d_err};
    const dim3 grid((unsigned)((nbox + 255) / 256), sym_chunk, (unsigned)nl);
    hipLaunchKernelGGL(k_pab_sym<1>, grid, dim3(256), 0, p->stream, sr, (unsigned char*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(k_pab_sym<2>, grid, dim3(256), 0, p->stream, sr, d_flags8, d_counts);
    counts_h.resize(nl * sym_chunk);
    if (int rc = pab_to_host(p, counts_h.data(), d_counts, counts_h.size() * sizeof(int))) return rc;
    base_h.assign(nl * sym_chunk, -1);
    std::vector<int> next;
    for (size_t sl = 0; sl < nl; ++sl) {
      const int c = live[sl];
      bool done = false;
      for (int k = 0; k < nvalid_h[sl] && !done; ++k) {   // row_count += added; if row_count >= min_pairs: break (solver:1275)
        base_h[sl * sym_chunk + k] = (long long)(p->st[(size_t)c].sym0 + kept[(size_t)c]);
        kept[(size_t)c] += counts_h[sl * sym_chunk + k];
        if (kept[(size_t)c] >= qs[c].min_sym_pairs) done = true;
      }
      if (!done && (size_t)(p0 + sym_chunk) < walk[(size_t)c].size()) next.push_back(c);
    }
    if (int rc = pab_to_device(p, d_base, base_h.data(), base_h.size() * sizeof(long long))) return rc;
    hipLaunchKernelGGL(k_pab_sym_emit, dim3(sym_chunk, (unsigned)nl), dim3(1024), 0, p->stream, sr, d_flags8, d_base, p->d_pairs);
    live.swap(next);
  }
  int err_h = 0;
  if (int rc = pab_to_host(p, &err_h, d_err, sizeof(int))) return rc;
  if (err_h) return pab_fail(p, HH_ERR_STATE, "hh_pab_create: symmetry-pair table full (internal)");
  for (int c = 0; c < count; ++c) {
    p->st[(size_t)c].m_sym = kept[(size_t)c];
    p->total_sym += kept[(size_t)c];
    if (kept[(size_t)c] > cap) return pab_fail(p, HH_ERR_STATE, "hh_pab_create: more symmetry rows than planned (internal)");
  }
  return HH_OK;
}

// symmetry constraints (box (L3d, D3d, D3d) of lsq_reconstruct, solver:116-173): on the device, or with HH_PAB_HOST_SYM
// (and for the trilinear rows) on host threads
int pab_build_sym(hh_pab* p, PabBuild& b) {
  if (p->linear && !p->sliced)
    return pab_fail(p, HH_ERR_ARG, "hh_pab_create: not sliceable — a ray's samples lie in more than one cell layer (the single-candidate hh_pa has the general form)");
  b.pairs_of.assign((size_t)b.count, {});
  b.rows16_of.assign((size_t)(p->linear ? b.count : 0), {});
  b.dev_sym = std::getenv("HH_PAB_HOST_SYM") == nullptr && !p->linear;
  if (int rc = b.dev_sym ? pab_build_sym_device(p, b) : pab_build_sym_host(p, b)) return rc;
  b.lap(p, b.dev_sym ? "symmetry pairs (device)" : "symmetry pairs (host)");
  return HH_OK;
}

// the launch shapes: padded sizes and grid.x of every kind of launch
int pab_build_shapes(hh_pab* p, PabBuild&) {
  int64_t m_max = 0, md_max = 0, ms_max = 0;
  for (const PabState& s : p->st) {
    m_max = std::max(m_max, s.m_data + s.m_sym);
    md_max = std::max(md_max, s.m_data * PAB_LANES + s.m_sym);
    ms_max = std::max(ms_max, s.m_sym);
  }
  p->N = (p->n + 63) / 64 * 64;
  p->M = (m_max + 63) / 64 * 64;
  p->MA = p->M + p->N;
  // (element-wise kernels: PAB_VEC_ELEMS elements per thread, for the same reason as PABS_TAIL_ROWS)
  p->nb_n = (int)((p->n + 256 * PAB_VEC_ELEMS - 1) / (256 * PAB_VEC_ELEMS));
  p->nb_m = (int)((m_max + p->n + 256 * PAB_VEC_ELEMS - 1) / (256 * PAB_VEC_ELEMS));
  if (p->sliced) {   // one workgroup per slice, then 256 symmetry (/ augmented) rows per workgroup
    // (symmetry / augmented rows: PABS_TAIL_ROWS per thread — a workgroup's fixed costs (control word, state, reductions)
    // are a few microseconds whatever it does, and with one row per thread these workgroups took twice the slice
    // workgroups' share of the device)
    p->nb_mv = p->mz + (int)((ms_max + PABS_THREADS * PABS_TAIL_ROWS - 1) / (PABS_THREADS * PABS_TAIL_ROWS));
    p->nb_mva = p->mz + (int)((ms_max + p->n + PABS_THREADS * PABS_TAIL_ROWS - 1) / (PABS_THREADS * PABS_TAIL_ROWS));
  } else {
    p->nb_mv = (int)((md_max + 255) / 256);
    p->nb_mva = (int)((md_max + p->n + 255) / 256);
  }
  p->nb_fin = (int)((p->n + 256 * PABL_FIN_ELEMS - 1) / (256 * PABL_FIN_ELEMS));
  p->RB = std::max(std::max(std::max(p->nb_n, p->nb_m), p->nb_mva), p->nb_fin);
  if (p->linear)   // (the separable form's symmetry rows are 512 per block: k_pabf_tail)
    p->RB = std::max(p->RB, 16 * p->mz + (int)((ms_max + p->n + 256 * PABF_TAIL_ROWS - 1) / (256 * PABF_TAIL_ROWS)));
  return HH_OK;
}

// Row tables, resident buffers, right-hand sides.  The device keeps the rows slice-major on the sliced path ((z,
// operation, k, j): a stable sort of the reference's (operation, k, j) order by slice); b and the pixel ids handed back
// to the caller stay in the reference's.  Frees rows16_of and d_b_int.
int pab_build_tables(hh_pab* p, PabBuild& b) {
  const int count = b.count, d2 = b.d2;
  const bool dev_rows = b.dev_rows, dev_sym = b.dev_sym;
  std::vector<int> all_rows(dev_rows ? 0 : (size_t)p->total_rows);
  std::vector<float> all_b(dev_rows ? 0 : (size_t)p->total_rows);
  std::vector<int> srow((size_t)count * (p->mz + 1), 0);
  if (dev_rows) srow = b.srow_h;
  if (!dev_rows) {
    p->b_data.resize((size_t)p->total_rows);
    p->b_pid.resize((size_t)p->total_rows);
  }
  std::vector<int2> all_pairs(dev_sym || p->linear ? 0 : (size_t)p->total_sym);
  std::vector<int> order;
  for (int c = 0; c < count; ++c) {
    const PabState& s = p->st[(size_t)c];
    if (!dev_sym && !p->linear) std::copy(b.pairs_of[(size_t)c].begin(), b.pairs_of[(size_t)c].end(), all_pairs.begin() + s.sym0);
    if (dev_rows) continue;
    const std::vector<int>& rr = b.ray_of_row[(size_t)c];
    const std::vector<float>& bb = b.b_of[(size_t)c];
    std::copy(bb.begin(), bb.end(), p->b_data.begin() + s.row0);
    std::copy(b.pid_of[(size_t)c].begin(), b.pid_of[(size_t)c].end(), p->b_pid.begin() + s.row0);
    if (!p->sliced) {
      std::copy(rr.begin(), rr.end(), all_rows.begin() + s.row0);
      std::copy(bb.begin(), bb.end(), all_b.begin() + s.row0);
      continue;
    }
    if (!pab_slice_order(b.z_of[(size_t)c], p->mz, srow.data() + (size_t)c * (p->mz + 1), order))
      return pab_fail(p, HH_ERR_STATE, "hh_pab_create: a row without a slice (internal)");
    for (size_t k = 0; k < rr.size(); ++k) {
      all_rows[(size_t)s.row0 + k] = rr[(size_t)order[k]];
      all_b[(size_t)s.row0 + k] = bb[(size_t)order[k]];
    }
  }
  if (!dev_rows)
    if (int rc = pab_upload(p, p->d_ray_of_row, all_rows)) return rc;
  if (p->linear) {
    if (int rc = pab_alloc(p, p->d_sym16, (size_t)p->total_sym)) return rc;
    for (int c = 0; c < count; ++c)   // candidate by candidate through the staging buffer (7.5 MB each at the bench size)
      if (int rc = pab_to_device(p, p->d_sym16 + p->st[(size_t)c].sym0, b.rows16_of[(size_t)c].data(), b.rows16_of[(size_t)c].size() * sizeof(PaEll16)))
        return rc;
    std::vector<std::vector<PaEll16>>().swap(b.rows16_of);   // the end of rows16_of: before the resident buffers below
  } else if (!dev_sym) {
    if (int rc = pab_upload(p, p->d_pairs, all_pairs)) return rc;
  }
  if (int rc = pab_upload(p, p->d_srow, srow)) return rc;
  if (p->linear) {   // no map at all: the disc's table and the accumulator of A^T y
    std::vector<unsigned> sidx2((size_t)d2 * d2);
    for (int yy = 0; yy < d2; ++yy)
      for (int xx = 0; xx < d2; ++xx) {
        const int a = b.rank[(size_t)yy * d2 + xx], a1 = xx + 1 < d2 ? b.rank[(size_t)yy * d2 + xx + 1] : -1;   // plane 0: rank = index inside the plane
        sidx2[(size_t)yy * d2 + xx] = (unsigned)(a < 0 ? 0xffff : a) | ((unsigned)(a1 < 0 ? 0xffff : a1) << 16);
      }
    if (int rc = pab_upload(p, p->d_sidx2, sidx2)) return rc;
    if (int rc = pab_alloc(p, p->d_acc64, (size_t)count * ((p->n + 63) / 64 * 64))) return rc;
    PAB_HIP(p, hipMemsetAsync(p->d_acc64, 0, (size_t)count * ((p->n + 63) / 64 * 64) * sizeof(long long), p->stream));
  } else if (p->sliced) {
    if (int rc = pab_alloc(p, p->d_map16, (size_t)p->total_rows * p->d2p)) return rc;
    PAB_HIP(p, hipMemsetAsync(p->d_map16, 0xff, (size_t)p->total_rows * p->d2p * sizeof(uint16_t), p->stream));
  } else {
    if (int rc = pab_alloc(p, p->d_map, (size_t)p->total_rows * d2)) return rc;
  }
  if (int rc = pab_alloc(p, p->d_st, (size_t)count)) return rc;
  if (int rc = pab_alloc(p, p->d_ctl, (size_t)count)) return rc;
  PAB_HIP(p, hipMemsetAsync(p->d_ctl, 0, (size_t)count * sizeof(unsigned), p->stream));
  if (int rc = pab_alloc(p, p->d_tptr, (size_t)count * (p->n + 1))) return rc;
  if (int rc = pab_alloc(p, p->d_nv, (size_t)NV_COUNT * count * p->N)) return rc;
  if (int rc = pab_alloc(p, p->d_mv, (size_t)MV_COUNT * count * p->MA)) return rc;
  if (int rc = pab_alloc(p, p->d_red, (size_t)count * PAB_SLOTS * p->RB)) return rc;
  if (int rc = pab_alloc(p, p->d_xf, (size_t)count * p->N)) return rc;   // rows padded to N floats: whole cache lines per candidate
  if (int rc = pab_alloc(p, p->d_flags, PAB_FLAG_WORDS)) return rc;
  if (int rc = pab_alloc(p, p->d_lists, (size_t)2 * count)) return rc;
  PAB_HIP(p, hipMemsetAsync(p->d_nv, 0, (size_t)NV_COUNT * count * p->N * sizeof(double), p->stream));
  PAB_HIP(p, hipMemsetAsync(p->d_mv, 0, (size_t)MV_COUNT * count * p->MA * sizeof(double), p->stream));
  PAB_HIP(p, hipMemsetAsync(p->d_tptr, 0, (size_t)count * (p->n + 1) * sizeof(int), p->stream));
  PAB_HIP(p, hipMemsetAsync(p->d_flags, 0, PAB_FLAG_WORDS * sizeof(int), p->stream));
  if (int rc = pab_to_device(p, p->d_st, p->st.data(), p->st.size() * sizeof(PabState))) return rc;
  // right-hand sides: b of the data rows (float32 pixel values -> float64), zeros for the symmetry rows (the memset above)
  if (!dev_rows) {   // the host path's b takes the place the device path filled
    if (!b.d_b_int.ensure(all_b.size())) return pab_fail(p, HH_ERR_NOMEM, "hh_pab_create: " + dev_alloc_failed(all_b.size() * sizeof(float)));
    if (int rc = pab_to_device(p, b.d_b_int, all_b.data(), all_b.size() * sizeof(float))) return rc;
  }
  const float* bf = b.d_b_int;
  pab_vec<0>(p, CNT_MDATA, PabRed<0>{}, [] __device__(const auto&) { return true; },
             [bf] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
               w.mvec(MV_B, c)[i] = (double)bf[s.row0 + i];
             });
  const hipError_t e = hipStreamSynchronize(p->stream);
  b.d_b_int.reset();   // the end of d_b_int: MV_B is filled
  if (e != hipSuccess) return pab_fail(p, HH_ERR_HIP, "hh_pab_create: right-hand sides failed");
  b.lap(p, "row tables, buffers");
  return HH_OK;
}

// the compact index map (nearest neighbour), and on the sliced path the shared map rows (k_pab_share_rows)
int pab_build_map(hh_pab* p, PabBuild& b) {
  const int count = b.count, d2 = b.d2, l2 = b.l2;
  if (!p->linear) {
    int64_t md = 0;
    for (const PabState& s : p->st) md = std::max(md, s.m_data);
    hipLaunchKernelGGL(k_pab_fill_map, pab_grid((int)((md * d2 + 255) / 256), count), dim3(256), 0, p->stream, b.gr, p->d_st, p->d_ray_of_row,
                       p->d_rank, p->d_map, p->d_map16, p->d_srow, p->nslice, p->d2p, p->d_flags + 9, count);
    PAB_HIP(p, hipGetLastError());
    if (p->sliced) {
      int f[PAB_FLAG_WORDS];
      if (int rc = pab_poll(p, f)) return rc;
      if (f[9]) return pab_fail(p, HH_ERR_STATE, "hh_pab_create: a ray left its slice (internal)");
      // rows of one (operation, image row) read one copy of their map (k_pab_share_rows)
      if (int rc = pab_alloc(p, p->d_maprow, (size_t)std::max<int64_t>(p->total_rows, 1))) return rc;
      int max_ops_used = 0;
      for (int c = 0; c < count; ++c) max_ops_used = std::max(max_ops_used, p->n_ops_used[(size_t)c]);
      const size_t keys = (size_t)count * std::max(max_ops_used, 1) * d2;
      {
        DevArena tmp;
        int* d_first = tmp.get<int>(keys);
        int* d_second = tmp.get<int>(keys);
        if (int rc = pab_arena_ok(p, tmp)) return rc;
        hipError_t es = hipMemsetAsync(d_first, 0x7f, keys * sizeof(int), p->stream);
        if (es == hipSuccess) es = hipMemsetAsync(d_second, 0x7f, keys * sizeof(int), p->stream);
        if (es == hipSuccess) {
          const dim3 grid = pab_grid((int)((md * 8 + 255) / 256), count);
          hipLaunchKernelGGL(k_pab_share_rows<0>, grid, dim3(256), 0, p->stream, p->d_st, p->d_ray_of_row, p->d_map16, p->d2p, l2, d2, max_ops_used, d_first, d_second, p->d_maprow, count);
          hipLaunchKernelGGL(k_pab_share_rows<1>, grid, dim3(256), 0, p->stream, p->d_st, p->d_ray_of_row, p->d_map16, p->d2p, l2, d2, max_ops_used, d_first, d_second, p->d_maprow, count);
          hipLaunchKernelGGL(k_pab_share_rows<2>, grid, dim3(256), 0, p->stream, p->d_st, p->d_ray_of_row, p->d_map16, p->d2p, l2, d2, max_ops_used, d_first, d_second, p->d_maprow, count);
          es = hipStreamSynchronize(p->stream);
        }
        if (es != hipSuccess) return pab_fail(p, HH_ERR_HIP, std::string("hh_pab_create (shared map rows): ") + hipGetErrorString(es));
      }
      if (b.timing) {
        std::vector<int> mr((size_t)p->total_rows);
        if (pab_to_host(p, mr.data(), p->d_maprow, mr.size() * sizeof(int)) == HH_OK) {
          std::vector<int> u(mr);
          std::sort(u.begin(), u.end());
          const size_t distinct = (size_t)(std::unique(u.begin(), u.end()) - u.begin());
          std::fprintf(stderr, "hh_pab_create[%d]: shared map rows: %zu rows read %zu distinct maps (%.1f rows per map)\n", count, mr.size(), distinct,
                       (double)mr.size() / (double)std::max<size_t>(distinct, 1));
        }
      }
    }
  }
  b.lap(p, "index map");
  return HH_OK;
}

// the transposed pattern (sliced path: of the symmetry rows only): count, scan, fill, sort
int pab_build_transposed(hh_pab* p, PabBuild& b) {
  const int count = b.count, d2 = b.d2;
  PabView w = pab_view(p);
  int64_t span = 0;
  for (const PabState& s : p->st) span = std::max(span, p->linear ? s.m_sym * 16 : (p->sliced ? 0 : s.m_data * d2) + s.m_sym);
  const dim3 grid = pab_grid((int)std::max<int64_t>(1, (span + 255) / 256), count);
  DevBuf<int> d_cursor;
  if (!d_cursor.ensure((size_t)count * (p->n + 1)))
    return pab_fail(p, HH_ERR_NOMEM, "hh_pab_create: " + dev_alloc_failed(d_cursor.bytes_for((size_t)count * (p->n + 1))));
  if (p->linear) hipLaunchKernelGGL((k_pabl_transpose<false>), grid, dim3(256), 0, p->stream, w, p->d_tptr, (int2*)nullptr);
  else if (p->sliced) hipLaunchKernelGGL((k_pab_transpose<false, false>), grid, dim3(256), 0, p->stream, w, p->d_tptr, (int*)nullptr);
  else hipLaunchKernelGGL((k_pab_transpose<false, true>), grid, dim3(256), 0, p->stream, w, p->d_tptr, (int*)nullptr);
  hipLaunchKernelGGL(k_pab_scan, dim3(count), dim3(1024), 0, p->stream, p->n, p->d_tptr, d_cursor);
  // list lengths per candidate -> offsets of the concatenated entry array
  std::vector<int> last((size_t)count);
  hipError_t e = pab_stage(p, (size_t)count * sizeof(int)) ? hipErrorOutOfMemory : hipSuccess;
  // the last entry of every candidate's scan = its number of list entries: one strided copy
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(p->h_stage, sizeof(int), p->d_tptr + p->n, (size_t)(p->n + 1) * sizeof(int), sizeof(int), (size_t)count,
                         hipMemcpyDeviceToHost, p->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
  if (e != hipSuccess) return pab_fail(p, HH_ERR_HIP, std::string("hh_pab_create: ") + hipGetErrorString(e));
  std::memcpy(last.data(), p->h_stage, (size_t)count * sizeof(int));
  p->total_nnz = 0;
  for (int c = 0; c < count; ++c) {
    p->st[(size_t)c].t0 = p->total_nnz;
    p->total_nnz += last[(size_t)c];
  }
  if (int rc = p->linear ? pab_alloc(p, p->d_tent2, (size_t)p->total_nnz) : pab_alloc(p, p->d_tent, (size_t)p->total_nnz)) return rc;
  if (int rc = pab_to_device(p, p->d_st, p->st.data(), p->st.size() * sizeof(PabState))) return rc;
  w = pab_view(p);
  // the cursor of voxel v starts at tptr[v] (the scan is inclusive over cnt[v + 1], i.e. exclusive for v)
  if (p->linear) {
    hipLaunchKernelGGL((k_pabl_transpose<true>), grid, dim3(256), 0, p->stream, w, d_cursor, p->d_tent2);
    hipLaunchKernelGGL(k_pabl_sort_lists, pab_grid((int)((p->n + 255) / 256), count), dim3(256), 0, p->stream, w, p->d_tent2);
  } else {
    if (p->sliced) hipLaunchKernelGGL((k_pab_transpose<true, false>), grid, dim3(256), 0, p->stream, w, d_cursor, p->d_tent);
    else hipLaunchKernelGGL((k_pab_transpose<true, true>), grid, dim3(256), 0, p->stream, w, d_cursor, p->d_tent);
    hipLaunchKernelGGL(k_pab_sort_lists, pab_grid((int)((p->n + 255) / 256), count), dim3(256), 0, p->stream, w, p->d_tent);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
  if (e != hipSuccess) return pab_fail(p, HH_ERR_HIP, std::string("hh_pab_create: ") + hipGetErrorString(e));
  b.lap(p, "transposed lists");
  return HH_OK;
}

// ---- the separable form of the trilinear data rows (path_a_factored.inc) ----------------------------------------------------
// per (candidate, operation, image column): axial data, the hash of its samples' cell decisions, its first row and the
// image rows that have a ray — computed on the device, grouped into footprint lists and column groups on the host
// (4k entries per candidate), then the lists' samples are written by the device
int pab_build_separable(hh_pab* p, PabBuild& b) {
  const int count = b.count, d2 = b.d2, l2 = b.l2;
  int G = 4;   // (+ 26 KB for the group's list table, sized below)
  while (G > 1 && (size_t)(G + 1) * p->nslice * sizeof(double) > ((size_t)120 << 10)) --G;
  const int ng = std::max(1, (p->mz - 1 + G - 1) / G);
  int max_ops = 0;
  for (int c = 0; c < count; ++c) max_ops = std::max(max_ops, p->n_ops_used[(size_t)c]);
  const size_t cells = (size_t)count * max_ops * l2;
  std::vector<PabfZinfo> zi(cells);
  std::vector<unsigned long long> hash(cells), jm(cells * 2);
  std::vector<int> rb(cells);
  {
    DevArena tmp;
    PabfZinfo* d_zi = tmp.get<PabfZinfo>(cells);
    unsigned long long* d_hash = tmp.get<unsigned long long>(cells);
    unsigned long long* d_jm = tmp.get<unsigned long long>(cells * 2);
    int* d_rb = tmp.get<int>(cells);
    int* d_nused = tmp.get<int>((size_t)count);
    if (int rc = pab_arena_ok(p, tmp)) return rc;
    hipError_t e = hipMemsetAsync(d_hash, 0, cells * 8, p->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_jm, 0, cells * 16, p->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_rb, 0x7f, cells * 4, p->stream);
    if (e != hipSuccess) return pab_fail(p, HH_ERR_HIP, std::string("hh_pab_create (footprint lists): ") + hipGetErrorString(e));
    if (int rc = pab_to_device(p, d_nused, p->n_ops_used.data(), (size_t)count * sizeof(int))) return rc;
    hipLaunchKernelGGL(k_pabf_zinfo, dim3((unsigned)((l2 + 127) / 128), (unsigned)max_ops, (unsigned)count), dim3(128), 0, p->stream, b.gr, count, max_ops,
                       d_nused, d_zi);
    hipLaunchKernelGGL(k_pabf_cellhash, dim3((unsigned)l2, (unsigned)max_ops, (unsigned)count), dim3(128), 0, p->stream, b.gr, count, max_ops, d_nused,
                       p->d_sidx2, d_hash);
    int64_t md = 0;
    for (const PabState& st : p->st) md = std::max(md, st.m_data);
    hipLaunchKernelGGL(k_pabf_rowbase, pab_grid((int)((md + 255) / 256), count), dim3(256), 0, p->stream, pab_view(p), max_ops, d_rb, d_jm);
    if (int rc = pab_to_host(p, zi.data(), d_zi, cells * sizeof(PabfZinfo))) return rc;
    if (int rc = pab_to_host(p, hash.data(), d_hash, cells * 8)) return rc;
    if (int rc = pab_to_host(p, jm.data(), d_jm, cells * 16)) return rc;
    if (int rc = pab_to_host(p, rb.data(), d_rb, cells * 4)) return rc;
  }
  b.lap(p, "separable form: axial data, cell hashes");
  // lists: (operation, z mask, cell hash) of the (o, k) that have rows; groups: home / G
  std::vector<std::vector<PabfListRef>> lists((size_t)count);
  std::vector<std::vector<std::vector<PabfGroupList>>> groups((size_t)count);
  int max_lists = 1, max_gl = 1;
  for (int c = 0; c < count; ++c) {
    struct Key { int op; unsigned long long m0, m1, h; };
    std::vector<Key> keys;
    std::vector<PabfListRef>& ls = lists[(size_t)c];
    std::vector<std::vector<PabfGroupList>>& gs = groups[(size_t)c];
    gs.assign((size_t)ng, {});
    for (int o = 0; o < p->n_ops_used[(size_t)c]; ++o)
      for (int k = 0; k < l2; ++k) {
        const size_t at = ((size_t)c * max_ops + o) * l2 + k;
        if (rb[at] == 0x7f7f7f7f) continue;   // no ray of this (operation, column) has a row
        const PabfZinfo& z = zi[at];
        int li = -1;
        for (size_t t = 0; t < keys.size(); ++t)
          if (keys[t].op == o && keys[t].m0 == z.zmask[0] && keys[t].m1 == z.zmask[1] && keys[t].h == hash[at]) { li = (int)t; break; }
        if (li < 0) {
          li = (int)keys.size();
          keys.push_back({o, z.zmask[0], z.zmask[1], hash[at]});
          PabfListRef lr{};
          lr.op = o; lr.k = k; lr.zmask[0] = z.zmask[0]; lr.zmask[1] = z.zmask[1];
          ls.push_back(lr);
        }
        const int g = z.home / G;
        if (g >= ng) return pab_fail(p, HH_ERR_STATE, "hh_pab_create: a home layer beyond the groups (internal)");
        std::vector<PabfGroupList>& gg = gs[(size_t)g];
        PabfGroupList* slot = nullptr;
        for (PabfGroupList& cand_ : gg)
          if (cand_.list == li && cand_.nk < PABF_KMAX) { slot = &cand_; break; }
        if (!slot) { gg.push_back(PabfGroupList{}); slot = &gg.back(); slot->list = li; slot->nk = 0; }
        PabfRowRef& r = slot->e[slot->nk++];
        r.rowbase = rb[at];
        r.hp = z.home - g * G;
        r.jmask[0] = jm[2 * at]; r.jmask[1] = jm[2 * at + 1];
        r.cz0 = z.cz0; r.cz1 = z.cz1;
      }
    max_lists = std::max<int>(max_lists, (int)ls.size());
    for (const auto& gg : gs) max_gl = std::max<int>(max_gl, (int)gg.size());
  }
  {
    std::vector<PabfListRef> all_lists((size_t)count * max_lists);
    std::vector<int> n_lists((size_t)count), ngl((size_t)count * ng);
    std::vector<PabfGroupList> all_gl((size_t)count * ng * max_gl);
    for (int c = 0; c < count; ++c) {
      n_lists[(size_t)c] = (int)lists[(size_t)c].size();
      std::copy(lists[(size_t)c].begin(), lists[(size_t)c].end(), all_lists.begin() + (size_t)c * max_lists);
      for (int g = 0; g < ng; ++g) {
        const auto& gg = groups[(size_t)c][(size_t)g];
        ngl[(size_t)c * ng + g] = (int)gg.size();
        std::copy(gg.begin(), gg.end(), all_gl.begin() + ((size_t)c * ng + g) * max_gl);
      }
    }
    DevArena tmp;
    PabfListRef* d_lists = tmp.get<PabfListRef>(all_lists.size());
    int* d_nlists = tmp.get<int>((size_t)count);
    if (int rc = pab_arena_ok(p, tmp)) return rc;
    if (int rc = pab_to_device(p, d_lists, all_lists.data(), all_lists.size() * sizeof(PabfListRef))) return rc;
    if (int rc = pab_to_device(p, d_nlists, n_lists.data(), n_lists.size() * sizeof(int))) return rc;
    if (int rc = pab_upload(p, p->d_fac_ngl, ngl)) return rc;
    if (int rc = pab_upload(p, p->d_fac_gl, all_gl)) return rc;
    if (int rc = pab_alloc(p, p->d_fac_entries, (size_t)count * max_lists * d2 * d2)) return rc;
    if (int rc = pab_alloc(p, p->d_fac_count, (size_t)count * max_lists * d2)) return rc;
    hipLaunchKernelGGL(k_pabf_entries, dim3((unsigned)((d2 + 63) / 64), (unsigned)max_lists, (unsigned)count), dim3(64), 0, p->stream, b.gr, count,
                       max_lists, d_nlists, d_lists, p->d_sidx2, p->d_fac_entries, p->d_fac_count);
    const hipError_t e3 = hipStreamSynchronize(p->stream);
    if (e3 != hipSuccess) return pab_fail(p, HH_ERR_HIP, std::string("hh_pab_create (footprint lists): ") + hipGetErrorString(e3));
  }
  p->fac_G = G; p->fac_ng = ng; p->fac_max_gl = max_gl; p->fac_max_lists = max_lists;
  p->fac_lds = (size_t)(G + 1) * p->nslice * sizeof(double) + (size_t)max_gl * sizeof(PabfGroupList);
  if (p->fac_lds > ((size_t)160 << 10) && (b.flags & HH_PAB_ALLOW_BANDED)) {   // the banded form instead (pab_build_banded)
    p->d_fac_ngl.reset(); p->d_fac_gl.reset(); p->d_fac_entries.reset(); p->d_fac_count.reset();
    p->fac_G = 0;
    p->band_T = -1;
  } else if (p->fac_lds > ((size_t)160 << 10)) {
    return pab_fail(p, HH_ERR_ARG, "hh_pab_create: not sliceable — the planes and the list table of a group do not fit the LDS");
  }
  // the forward product's blocks: the groups, then the symmetry (/ augmented) rows
  if (p->fac_G) {
    int64_t ms_max = 0;
    for (const PabState& st : p->st) ms_max = std::max(ms_max, st.m_sym);
    p->fac_split = std::max(1, std::min(8, (16 + ng - 1) / ng));   // about sixteen workgroups per candidate and product
    p->nb_mv = ng * p->fac_split + (int)((ms_max + 256 * PABF_TAIL_ROWS - 1) / (256 * PABF_TAIL_ROWS));
    p->nb_mva = ng * p->fac_split + (int)((ms_max + p->n + 256 * PABF_TAIL_ROWS - 1) / (256 * PABF_TAIL_ROWS));
    if (p->nb_mva > p->RB) return pab_fail(p, HH_ERR_STATE, "hh_pab_create: more partial sums than planned (internal)");
  }
  if (b.timing && p->fac_G) {
    size_t nl = 0, ngl_tot = 0, nk_tot = 0;
    for (int c = 0; c < count; ++c) {
      nl += lists[(size_t)c].size();
      for (const auto& gg : groups[(size_t)c]) { ngl_tot += gg.size(); for (const auto& e_ : gg) nk_tot += (size_t)e_.nk; }
    }
    std::fprintf(stderr, "hh_pab_create[%d]: separable form: G %d, %d groups, lists per candidate %.1f (max %d), group lists per group %.1f (max %d), "
                         "rows per group list %.2f, operations used (max) %d\n", count, G, ng, (double)nl / count, max_lists,
                 (double)ngl_tot / count / ng, max_gl, ngl_tot ? (double)nk_tot / ngl_tot : 0.0, max_ops);
  }
  b.lap(p, "separable form: lists and column groups");
  return HH_OK;
}

// ---- the banded form (path_a_banded.inc): the disc's rows cut into bands whose planes, halo row and table rows fit --------
int pab_build_banded(hh_pab* p, PabBuild& b) {
  const PabBandCut cut = pab_band_cut(b.rank, b.d2, (b.flags & HH_PAB_FORCE_BANDED) != 0);
  if (cut.row_too_large) return pab_fail(p, HH_ERR_ARG, "hh_pab_create: not sliceable — one row of the disc does not fit the LDS");
  p->band_T = (int)cut.band_y.size() - 1;
  // the launch needs the largest band's bytes — each at most the budget; with the static state the whole must fit a
  // compute unit's 160 KiB
  p->band_lds = cut.band_lds;
  if (p->band_lds > cut.budget || p->band_lds + sizeof(PabState) > ((size_t)160 << 10))
    return pab_fail(p, HH_ERR_STATE, "hh_pab_create: not sliceable — a band of the disc does not fit the LDS (internal)");
  if (int rc = pab_upload(p, p->d_band_y, cut.band_y)) return rc;
  if (int rc = pab_upload(p, p->d_band_v, cut.vrow)) return rc;
  if (int rc = pab_alloc(p, p->d_bpart, (size_t)b.count * p->band_T * p->M)) return rc;
  if (b.timing) std::fprintf(stderr, "hh_pab_create[%d]: banded form: %d bands, %zu bytes of LDS\n", b.count, p->band_T, p->band_lds);
  b.lap(p, "banded form");
  return HH_OK;
}

// Largest column sum of |A_data| per candidate: sizes the fixed-point scale of A^T y.  launch(d_colmax) runs the
// products' column-sum variants into d_colmax [count] (zeroed); colsum_of(max) makes st.colsum of a candidate's maximum.
template <class T, class Launch, class ColsumOf>
int pab_colsums(hh_pab* p, PabBuild& b, Launch launch, ColsumOf colsum_of) {
  const int count = b.count;
  std::vector<T> colmax((size_t)count, 0);
  {
    DevArena tmp;
    T* d_colmax = tmp.get<T>((size_t)count);
    if (int rc = pab_arena_ok(p, tmp)) return rc;
    hipError_t e = hipMemsetAsync(d_colmax, 0, (size_t)count * sizeof(T), p->stream);
    launch(d_colmax);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return pab_fail(p, HH_ERR_HIP, hipGetErrorString(e));
    if (int rc = pab_to_host(p, colmax.data(), d_colmax, colmax.size() * sizeof(T))) return rc;
  }
  for (int c = 0; c < count; ++c) {
    PabState& s = p->st[(size_t)c];
    s.colsum = colsum_of(colmax[(size_t)c]);
    pab_fx_scale(s.colsum, 1.0, s.fx_scale, s.fx_inv);
    s.fx_scale_r = s.fx_scale;
    s.fx_inv_r = s.fx_inv;
  }
  if (int rc = pab_to_device(p, p->d_st, p->st.data(), p->st.size() * sizeof(PabState))) return rc;
  b.lap(p, "column sums");
  return HH_OK;
}
int pab_build_colsums(hh_pab* p, PabBuild& b) {
  const int count = b.count;
  auto all = [] __device__(const auto&) { return true; };
  if (p->linear)   // in 2^-20 units (the trilinear weights are not counts)
    return pab_colsums<long long>(
        p, b,
        [&](long long* d_colmax) {
          if (p->fac_G) {
            pabf_with_G(p->fac_G, [&](auto G) {
              const auto kernel = k_pabf_scatter<0, true, decltype(G)::value, decltype(all)>;
              pab_lds_attr(p, kernel, p->fac_lds);
              hipLaunchKernelGGL(kernel, pab_grid(p->fac_ng * p->fac_split, count), dim3(PABS_THREADS), p->fac_lds, p->stream, pab_view(p), 0, all);
            });
          } else if (p->band_T) {
            pab_lds_attr(p, k_pabt_scatter<0, true, decltype(all)>, p->band_lds);
            hipLaunchKernelGGL((k_pabt_scatter<0, true, decltype(all)>), pab_grid(p->mz * p->band_T, count), dim3(PABS_THREADS), p->band_lds, p->stream,
                               pab_view(p), 0, all);
          } else {
            pab_lds_attr(p, k_pabl_scatter<0, true, decltype(all)>, p->lin_lds);
            hipLaunchKernelGGL((k_pabl_scatter<0, true, decltype(all)>), pab_grid(p->mz, count), dim3(PABS_THREADS), p->lin_lds, p->stream, pab_view(p), 0, all);
          }
          hipLaunchKernelGGL((k_pabl_finish<2, decltype(all)>), pab_grid(p->nb_fin, count), dim3(256), 0, p->stream, pab_view(p), 0, -1, -1, 0, d_colmax, all);
        },
        [](long long m) { return std::ldexp((double)m, -20) * (1.0 + 1e-3) + 1e-3; });   // (as hh_pa sizes it)
  if (p->sliced)   // hit counts
    return pab_colsums<int>(
        p, b,
        [&](int* d_colmax) {
          hipLaunchKernelGGL((k_pabs_rmatvec<0, true, decltype(all)>), pab_grid(p->mz, count), dim3(PABS_THREADS), (size_t)p->nslice * sizeof(long long),
                             p->stream, pab_view(p), 0, -1, -1, 0, d_colmax, all);
        },
        [](int m) { return (double)std::max(1, m); });
  return HH_OK;
}

}  // namespace

extern "C" {

const char* hh_pab_last_error(const hh_pab* p) { return p ? p->err.c_str() : g_create_error.c_str(); }

void hh_pab_destroy(hh_pab* p) try {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->h_stage) (void)hipHostFree(p->h_stage);
  if (p->h_flags) (void)hipHostFree(p->h_flags);
  const hipStream_t stream = p->stream;
  delete p;                                   // frees the device buffers: before their stream goes
  if (stream) (void)hipStreamDestroy(stream);
} catch (...) {
}

int hh_pab_create(hh_pab** out, int device, const float* image, int ny, int nx, const hh_pa_params* qs, int count) try {
  return hh_pab_create_ex(out, device, image, ny, nx, qs, count, 0);
} HH_CATCH_CTX(nullptr, "hh_pab_create")

// flags: HH_PAB_ALLOW_BANDED — the trilinear products take the banded form (path_a_banded.inc) where the LDS form cannot hold
// the box; HH_PAB_FORCE_BANDED — always, with at least three bands (tests on small boxes).  0: hh_pab_create.
int hh_pab_create_ex(hh_pab** out, int device, const float* image, int ny, int nx, const hh_pa_params* qs, int count, int flags) try {
  int d2 = 0, l2 = 0, l3 = 0;
  if (int rc = pab_check_args(out, image, ny, nx, qs, count, flags, d2, l2, l3)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return pab_fail(nullptr, HH_ERR_HIP, "hh_pab_create: no such HIP device (Path A has no CPU fallback)");
  hh_pab* p = new (std::nothrow) hh_pab();
  if (!p) return pab_fail(nullptr, HH_ERR_NOMEM, "out of host memory");
  p->device = device;
  p->K = count;
  p->d2 = d2;
  p->d2p = (d2 + 63) / 64 * 64;
  struct Guard { hh_pab* p; ~Guard() { if (p) hh_pab_destroy(p); } } guard{p};   // an exception on the way releases the half-built object
  PabBuild b{qs, count, flags, image, ny, nx, d2, l2, l3, qs[0].reconstruct_diameter_3d_pixel,
             qs[0].reconstruct_diameter_3d_inner_pixel / 2.0, (double)(qs[0].reconstruct_diameter_3d_pixel / 2 - 1)};
  auto build = [&]() -> int {
    if (int rc = pab_build_form(p, b)) return rc;
    if (int rc = pab_build_geometry(p, b)) return rc;
    if (int rc = pab_build_rows(p, b)) return rc;          // on the device, or on the host and then the half sets
    if (int rc = pab_build_sym(p, b)) return rc;           // on the device, or on host threads
    if (int rc = pab_build_shapes(p, b)) return rc;
    if (int rc = pab_build_tables(p, b)) return rc;        // row tables, resident buffers, right-hand sides
    if (int rc = pab_build_map(p, b)) return rc;
    if (int rc = pab_build_transposed(p, b)) return rc;
    if (p->linear && d2 <= 128 && !p->band_T)
      if (int rc = pab_build_separable(p, b)) return rc;   // (may hand over to the banded form)
    if (p->linear && p->band_T)
      if (int rc = pab_build_banded(p, b)) return rc;
    return pab_build_colsums(p, b);
  };
  if (const int rc = build()) {   // the one way out of a failed set-up
    g_create_error = p->err;
    guard.p = nullptr;
    hh_pab_destroy(p);
    return rc;
  }
  guard.p = nullptr;
  *out = p;
  return HH_OK;
} HH_CATCH_CTX(nullptr, "hh_pab_create")

// dims = {candidates, unknowns, total data rows, total symmetry rows, device bytes}; per candidate: rows[c] = {data rows,
// symmetry rows, symmetry operations used} (rows may be NULL)
int hh_pab_dims(const hh_pab* p, int64_t dims[5], int64_t* rows) try {
  if (!p || !dims) return HH_ERR_ARG;
  dims[0] = p->K; dims[1] = p->n; dims[2] = p->total_rows; dims[3] = p->total_sym; dims[4] = (int64_t)p->device_bytes;
  if (rows)
    for (int c = 0; c < p->K; ++c) {
      rows[3 * c] = p->st[(size_t)c].m_data;
      rows[3 * c + 1] = p->st[(size_t)c].m_sym;
      rows[3 * c + 2] = p->n_ops_used[(size_t)c];
    }
  return HH_OK;
} HH_CATCH_PAB(p, "hh_pab_dims")

// b and pixel id of the data rows of candidate c (solver:1548-1549)
int hh_pab_get_rhs(const hh_pab* p, int c, float* b, int32_t* pid) try {
  if (!p || c < 0 || c >= p->K) return HH_ERR_ARG;
  const PabState& s = p->st[(size_t)c];
  if (p->b_data.empty() && p->d_bref) {   // rows were enumerated on the device: fetch the reference-order tables once
    hh_pab* q = const_cast<hh_pab*>(p);
    (void)hipSetDevice(q->device);
    q->b_data.resize((size_t)q->total_rows);
    q->b_pid.resize((size_t)q->total_rows);
    int rc = pab_to_host(q, q->b_data.data(), q->d_bref, q->b_data.size() * sizeof(float));
    if (rc == HH_OK) rc = pab_to_host(q, q->b_pid.data(), q->d_pidref, q->b_pid.size() * sizeof(int32_t));
    if (rc) { q->b_data.clear(); q->b_pid.clear(); return rc; }
  }
  if (b) std::memcpy(b, p->b_data.data() + s.row0, (size_t)s.m_data * sizeof(float));
  if (pid) std::memcpy(pid, p->b_pid.data() + s.row0, (size_t)s.m_data * sizeof(int32_t));
  return HH_OK;
} HH_CATCH_PAB(p, "hh_pab_get_rhs")

// the symmetry rows of candidate c as voxel-rank pairs (x_i - x_j = 0), in the reference's row order; out: [m_sym][2]
int hh_pab_get_pairs(hh_pab* p, int c, int32_t* out) try {
  if (!p || !out || c < 0 || c >= p->K) return HH_ERR_ARG;
  if (p->linear) return pab_fail(p, HH_ERR_ARG, "hh_pab_get_pairs: the trilinear symmetry rows are 16-entry rows, not voxel pairs");
  PAB_HIP(p, hipSetDevice(p->device));
  const PabState& s = p->st[(size_t)c];
  return pab_to_host(p, out, p->d_pairs + s.sym0, (size_t)s.m_sym * sizeof(int2));
} HH_CATCH_PAB(p, "hh_pab_get_pairs")

// lsq_linear(A_c, b_c, bounds = positive[c] ? (0, max b_c) : none, tol, max_iter, lsmr_maxiter, lsmr_tol = "auto") for
// every candidate, then x -> float32, prediction A_data x (clipped at 0 when clip[c]) and its cosine with b.
// x_out: [K][n] float32 (may be NULL); scores: [K]; info: [K][5] = {status, trust-region iterations, LSMR calls, LSMR
// iterations, of which in the first (unconstrained) solve}
int hh_pab_solve(hh_pab* p, const int32_t* positive, const int32_t* clip, double tol, int max_iter, int lsmr_maxiter, float* x_out,
                 double* scores, int32_t* info) try {
  if (!p || !scores) return pab_fail(p, HH_ERR_ARG, "hh_pab_solve: NULL argument");
  if (!(tol > 0) || max_iter < 1 || lsmr_maxiter < 1) return pab_fail(p, HH_ERR_ARG, "hh_pab_solve: tol, max_iter, lsmr_maxiter must be positive");
  PAB_HIP(p, hipSetDevice(p->device));
  p->launches = p->syncs = p->ticks = p->inconsistent = 0;
  if (const char* tc = std::getenv("HH_PAB_TRACE")) {
    p->trace_c = std::atoi(tc);
    if (!p->d_trace.ensure((size_t)PAB_TRACE_ROWS * 8)) return pab_fail(p, HH_ERR_NOMEM, dev_alloc_failed((size_t)PAB_TRACE_ROWS * 8 * sizeof(double)));
    PAB_HIP(p, hipMemsetAsync(p->d_trace, 0, (size_t)PAB_TRACE_ROWS * 8 * sizeof(double), p->stream));
  }
  PAB_HIP(p, hipMemsetAsync(p->d_flags, 0, PAB_FLAG_WORDS * sizeof(int), p->stream));
  pab_cover(p, nullptr, 0);
  for (int c = 0; c < p->K; ++c) {
    PabState& s = p->st[(size_t)c];
    const bool pos = positive && positive[c];
    s.bounded = pos ? 1 : 0;
    s.lb = pos ? 0.0 : -INFINITY;
    s.ub = pos ? s.bmax : INFINITY;
    s.clip = clip && clip[c] ? 1 : 0;
    s.phase = PH_LSMR0; s.aug = 0; s.start = 1;
    s.run = 1; s.l_on = 0; s.t_on = 0; s.status = 0; s.pending = 0; s.has_pending = 0; s.n_outer = 0; s.lsmr_calls = 0; s.lsmr_iters = 0;
    s.atol = s.btol = 1e-2 * tol;
    s.bt = s.bt_on = s.bt_fix = 0;
    s.score = 0;
  }
  int rc = pab_to_device(p, p->d_st, p->st.data(), p->st.size() * sizeof(PabState));
  if (rc) return rc;
  {  // control words of the starting state: PH_LSMR0, start
    std::vector<unsigned> ctl((size_t)p->K, (unsigned)PH_LSMR0 | (1u << 7));
    if ((rc = pab_to_device(p, p->d_ctl, ctl.data(), ctl.size() * sizeof(unsigned)))) return rc;
  }
  auto all = [] __device__(const auto&) { return true; };
  auto trf = [] __device__(const auto& s) { return s.t_on != 0; };
  const double EPS = 2.220446049250313e-16;
  // ---- lsq_linear, every candidate at its own pace ------------------------------------------------------------------------
  // Phases of a candidate (PabPhase): the unconstrained LSMR solve -> bounds check (done, or a strictly feasible start)
  // -> per trust-region iteration: scaling and tolerances, the LSMR solve of the step, the step's selection (Newton /
  // reflected / anti-gradient, 1-D models), backtracking if the model lied, the new x / residual / gradient / status.
  // One pass of the loop below launches every phase's kernels once (skipping phases without candidates, as of the
  // previous pass's count) and then a few LSMR iterations for everyone inside a solve; a candidate that finishes a phase
  // is picked up by the next one in the SAME pass.  The host reads the phase counts once per pass.
  auto after0 = [] __device__(const auto& s) { return s.phase == PH_AFTER0; };
  auto after0_trf = [] __device__(const auto& s) { return s.phase == PH_AFTER0 && s.t_on != 0; };
  auto pre = [] __device__(const auto& s) { return s.phase == PH_PRE; };
  auto starting = [] __device__(const auto& s) { return s.start != 0; };
  auto post = [] __device__(const auto& s) { return s.phase == PH_POST; };
  auto sel = [] __device__(const auto& s) { return s.phase == PH_POST && !s.inb; };
  auto sel_r = [] __device__(const auto& s) { return s.phase == PH_POST && !s.inb && s.rsu_pos; };
  auto bt_on = [] __device__(const auto& s) { return s.phase == PH_BT && s.bt_on != 0; };
  auto bt_any = [] __device__(const auto& s) { return s.phase == PH_BT && s.bt_on == 0; };      // trial accepted
  auto bt_fix = [] __device__(const auto& s) { return s.phase == PH_BT && s.bt_on == 0 && s.bt_fix != 0; };
  auto fin = [] __device__(const auto& s) { return s.phase == PH_FIN; };
  auto after_first_solve = [&] {
  // in bounds? (np.all((x >= lb) & (x <= ub)))
  pab_vec<1>(p, CNT_N, pab_red<1>({RED_SUM}, {0}, p->nb_n), after0, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
    const double x = w.nvec(NV_LX, c)[i];
    acc[0] += (x >= s.lb && x <= s.ub) ? 0.0 : 1.0;
  });
  pab_scalar<1>(p, pab_red<1>({RED_SUM}, {0}, p->nb_n), after0, [] __device__(const PabView&, int, PabState& s, const double* v) {
    if (!s.bounded || v[0] == 0) { s.t_on = 0; s.status = 3; }
    else s.t_on = 1;
    s.run = 0;
    s.first_iters = s.lsmr_iters;
  });
  // x: the unconstrained solution, or (trust region) its reflection made strictly feasible (rstep = 0.1)
  pab_vec<0>(p, CNT_N, PabRed<0>{}, after0, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
#pragma clang fp contract(off)
    const double x = w.nvec(NV_LX, c)[i];
    w.nvec(NV_X, c)[i] = s.t_on ? pab_feasible(pab_reflect(x, s.lb, s.ub), s.lb, s.ub, 0.1) : x;
  });
  // r = A x - b, g = A^T r, cost
  pab_matvec<2>(p, NV_X, -1, -1, MV_R, after0_trf);
  pab_scalar<2>(p, pab_red<2>({RED_SUM, RED_MAX}, {0, 1}, p->nb_mv), after0_trf, [] __device__(const PabView& w, int, PabState& s, const double* v) {
    s.cost = 0.5 * v[0];
    if (w.sliced) { s.rmax = v[1]; pab_fx_scale(s.colsum, s.rmax, s.fx_scale_r, s.fx_inv_r); }   // for g = A^T r below
  });
  pab_rmatvec<0>(p, MV_R, -1, -1, NV_G, after0_trf);
  pab_scalar<0>(p, PabRed<0>{}, after0, [] __device__(const PabView&, int, PabState& s, const double*) {
    s.phase = s.t_on ? PH_PRE : PH_DONE;
  });
  };
  auto begin_iteration = [&] {
  // Coleman-Li scaling, g_norm, the scaled quantities
  pab_vec<1>(p, CNT_N, pab_red<1>({RED_MAX}, {0}, p->nb_n), pre, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
    const double x = w.nvec(NV_X, c)[i], g = w.nvec(NV_G, c)[i];
    double v = 1.0, dv = 0.0;
    if (g < 0) { v = s.ub - x; dv = -1.0; }
    if (g > 0) { v = x - s.lb; dv = 1.0; }
    const double dg = g * dv, d = sqrt(v);
    w.nvec(NV_VS, c)[i] = v;
    w.nvec(NV_DG, c)[i] = dg;
    w.nvec(NV_D, c)[i] = d;
    w.nvec(NV_ROOT, c)[i] = sqrt(dg);
    w.nvec(NV_GH, c)[i] = d * g;
    acc[0] = fmax(acc[0], fabs(g * v));
  });
  pab_scalar<1>(p, pab_red<1>({RED_MAX}, {0}, p->nb_n), pre, [tol, EPS, max_iter] __device__(const PabView&, int, PabState& s, const double* v) {
    s.g_norm = v[0];
    if (s.n_outer >= max_iter) { s.status = 0; s.t_on = 0; s.phase = PH_DONE; return; }   // the loop's range is exhausted
    if (s.g_norm < tol) { s.status = 1; s.t_on = 0; s.phase = PH_DONE; return; }
    const double eta = 1e-2 * fmin(0.5, s.g_norm);
    s.ltol = fmax(EPS, fmin(0.1, eta * s.g_norm));
    s.atol = s.btol = s.ltol;
    s.theta = 1 - fmin(0.005, s.g_norm);
    s.has_pending = 0;
    s.aug = 1;
    s.start = 1;
    s.phase = PH_LSMR;
  });
  // p_h = -lsmr([A diag(d); diag(root)], [r; 0])
  pab_vec<0>(p, CNT_MAUG, PabRed<0>{}, starting, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
    w.mvec(MV_LU, c)[i] = i < s.m_data + s.m_sym ? w.mvec(MV_R, c)[i] : 0.0;
  });
  pab_lsmr_start(p);
  };
  auto select_step = [&] {
  // p = d p_h; p . g; is x + p inside?; the step to the boundary along p
  pab_vec<3>(p, CNT_N, pab_red<3>({RED_SUM, RED_SUM, RED_MIN}, {0, 1, 2}, p->nb_n), post,
             [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
               const double ph = -w.nvec(NV_LX, c)[i];
               const double pp = w.nvec(NV_D, c)[i] * ph;
               const double x = w.nvec(NV_X, c)[i];
               w.nvec(NV_PH, c)[i] = ph;
               w.nvec(NV_P, c)[i] = pp;
               acc[0] += pp * w.nvec(NV_G, c)[i];
               const double xp = x + pp;
               acc[1] += (xp >= s.lb && xp <= s.ub) ? 0.0 : 1.0;
               acc[2] = fmin(acc[2], pab_step_to_bound(x, pp, s.lb, s.ub));
             });
  pab_scalar<3>(p, pab_red<3>({RED_SUM, RED_SUM, RED_MIN}, {0, 1, 2}, p->nb_n), post, [] __device__(const PabView&, int, PabState& s, const double* v) {
    s.p_dot_g = v[0];
    if (s.p_dot_g > 0) { s.pending = -1; s.has_pending = 1; }
    s.inb = v[1] == 0;
    s.p_stride = v[2];
  });
  
  
  // the reflected direction: r_h = p_h with the sign flipped where the boundary is hit; p, p_h to the boundary
  pab_vec<1>(p, CNT_N, pab_red<1>({RED_MIN}, {0}, p->nb_n), sel, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
    const double x = w.nvec(NV_X, c)[i];
    double pp = w.nvec(NV_P, c)[i], ph = w.nvec(NV_PH, c)[i];
    const double step = pab_step_to_bound(x, pp, s.lb, s.ub);
    double rh = ph;
    if (step == s.p_stride && pp != 0) rh = -rh;      // hits = (steps == min) * sign(p)
    const double rr = w.nvec(NV_D, c)[i] * rh;
    pp = pp * s.p_stride;
    ph = ph * s.p_stride;
    w.nvec(NV_RH, c)[i] = rh;
    w.nvec(NV_RR, c)[i] = rr;
    w.nvec(NV_P, c)[i] = pp;
    w.nvec(NV_PH, c)[i] = ph;
    acc[0] = fmin(acc[0], pab_step_to_bound(x + pp, rr, s.lb, s.ub));
  });
  pab_scalar<1>(p, pab_red<1>({RED_MIN}, {0}, p->nb_n), sel, [] __device__(const PabView&, int, PabState& s, const double* v) {
    s.r_su = v[0];
    s.r_sl = (1 - s.theta) * s.r_su;
    s.r_su *= s.theta;
    s.rsu_pos = s.r_su > 0;
    if (!s.rsu_pos) s.r_value = INFINITY;
  });
  // build_quadratic_1d(A_h, g_h, r_h, s0 = p_h, diag = diag_h)
  pab_matvec<0>(p, NV_RH, NV_D, -1, MV_T1, sel_r);
  pab_matvec<0>(p, NV_PH, NV_D, -1, MV_T2, sel_r);
  pab_vec<3>(p, CNT_M, pab_red<3>({RED_SUM, RED_SUM, RED_SUM}, {0, 1, 2}, p->nb_m), sel_r,
             [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
               const double v = w.mvec(MV_T1, c)[i], u = w.mvec(MV_T2, c)[i];
               acc[0] += v * v; acc[1] += u * v; acc[2] += u * u;
             });
  pab_vec<5>(p, CNT_N, pab_red<5>({RED_SUM, RED_SUM, RED_SUM, RED_SUM, RED_SUM}, {3, 4, 5, 6, 7}, p->nb_n), sel_r,
             [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
#pragma clang fp contract(off)
               const double rh = w.nvec(NV_RH, c)[i], ph = w.nvec(NV_PH, c)[i], dg = w.nvec(NV_DG, c)[i], gh = w.nvec(NV_GH, c)[i];
               acc[0] += (rh * dg) * rh; acc[1] += gh * rh; acc[2] += gh * ph; acc[3] += (ph * dg) * rh; acc[4] += (ph * dg) * ph;
             });
  {
    PabRed<8> r8{};
    for (int k = 0; k < 8; ++k) { r8.kind[k] = RED_SUM; r8.slot[k] = k; r8.nb[k] = k < 3 ? p->nb_m : p->nb_n; }
    pab_scalar<8>(p, r8, sel_r, [] __device__(const PabView&, int, PabState& s, const double* v) {
      const double a = 0.5 * (v[0] + v[3]);
      const double b = v[4] + v[1] + v[6];
      const double c = 0.5 * v[2] + v[5] + 0.5 * v[7];
      s.r_stride = pab_min_quad(a, b, s.r_sl, s.r_su, c, s.r_value);
    });
  }
  // r_h = p_h + r_h r_stride, r = d r_h (when the reflected step exists); p_h, p scaled by theta
  pab_vec<0>(p, CNT_N, PabRed<0>{}, sel, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
#pragma clang fp contract(off)
    double ph = w.nvec(NV_PH, c)[i];
    if (s.rsu_pos) {
      const double rh = ph + w.nvec(NV_RH, c)[i] * s.r_stride;
      w.nvec(NV_RH, c)[i] = rh;
      w.nvec(NV_RR, c)[i] = w.nvec(NV_D, c)[i] * rh;
    }
    ph = ph * s.theta;
    w.nvec(NV_PH, c)[i] = ph;
    w.nvec(NV_P, c)[i] = w.nvec(NV_P, c)[i] * s.theta;
  });
  // p_value = evaluate_quadratic(A_h, g_h, p_h, diag_h); the anti-gradient direction and its step to the boundary
  pab_matvec<0>(p, NV_PH, NV_D, -1, MV_T1, sel);
  pab_vec<1>(p, CNT_M, pab_red<1>({RED_SUM}, {0}, p->nb_m), sel, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
    const double v = w.mvec(MV_T1, c)[i];
    acc[0] += v * v;
  });
  pab_vec<3>(p, CNT_N, pab_red<3>({RED_SUM, RED_SUM, RED_MIN}, {1, 2, 3}, p->nb_n), sel,
             [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
               const double ph = w.nvec(NV_PH, c)[i], dg = w.nvec(NV_DG, c)[i], gh = w.nvec(NV_GH, c)[i];
               acc[0] += (ph * dg) * ph;
               acc[1] += ph * gh;
               const double agh = -gh;
               w.nvec(NV_ST, c)[i] = agh;                 // ag_h (scratch: the step vector is written later)
               acc[2] = fmin(acc[2], pab_step_to_bound(w.nvec(NV_X, c)[i], w.nvec(NV_D, c)[i] * agh, s.lb, s.ub));
             });
  {
    PabRed<4> r4{};
    for (int k = 0; k < 4; ++k) { r4.kind[k] = k == 3 ? RED_MIN : RED_SUM; r4.slot[k] = k; r4.nb[k] = k == 0 ? p->nb_m : p->nb_n; }
    pab_scalar<4>(p, r4, sel, [] __device__(const PabView&, int, PabState& s, const double* v) {
      s.p_value = 0.5 * (v[0] + v[1]) + v[2];
      s.ag_su = v[3] * s.theta;
    });
  }
  pab_matvec<0>(p, NV_ST, NV_D, -1, MV_T2, sel);
  pab_vec<1>(p, CNT_M, pab_red<1>({RED_SUM}, {0}, p->nb_m), sel, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
    const double v = w.mvec(MV_T2, c)[i];
    acc[0] += v * v;
  });
  pab_vec<2>(p, CNT_N, pab_red<2>({RED_SUM, RED_SUM}, {1, 2}, p->nb_n), sel, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
#pragma clang fp contract(off)
    const double agh = w.nvec(NV_ST, c)[i], dg = w.nvec(NV_DG, c)[i], gh = w.nvec(NV_GH, c)[i];
    acc[0] += (agh * dg) * agh;
    acc[1] += gh * agh;
  });
  {
    PabRed<3> r3{};
    for (int k = 0; k < 3; ++k) { r3.kind[k] = RED_SUM; r3.slot[k] = k; r3.nb[k] = k == 0 ? p->nb_m : p->nb_n; }
    pab_scalar<3>(p, r3, sel, [] __device__(const PabView&, int, PabState& s, const double* v) {
      const double a = 0.5 * (v[0] + v[1]), b = v[2];
      s.ag_stride = pab_min_quad(a, b, 0.0, s.ag_su, 0.0, s.ag_value);
      s.choice = (s.p_value < s.r_value && s.p_value < s.ag_value) ? 0 : (s.r_value < s.p_value && s.r_value < s.ag_value) ? 1 : 2;
    });
  }
  // the step, and cost_change = -evaluate_quadratic(A, g, step)
  pab_vec<1>(p, CNT_N, pab_red<1>({RED_SUM}, {1}, p->nb_n), post, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
    double st;
    if (s.inb || s.choice == 0) st = w.nvec(NV_P, c)[i];
    else if (s.choice == 1) st = w.nvec(NV_RR, c)[i];
    else st = (w.nvec(NV_D, c)[i] * w.nvec(NV_ST, c)[i]) * s.ag_stride;
    w.nvec(NV_ST, c)[i] = st;
    acc[0] += st * w.nvec(NV_G, c)[i];
  });
  pab_matvec<0>(p, NV_ST, -1, -1, MV_T1, post);
  pab_vec<1>(p, CNT_M, pab_red<1>({RED_SUM}, {0}, p->nb_m), post, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
    const double v = w.mvec(MV_T1, c)[i];
    acc[0] += v * v;
  });
  {
    PabRed<2> r2{};
    r2.kind[0] = r2.kind[1] = RED_SUM; r2.slot[0] = 0; r2.slot[1] = 1; r2.nb[0] = p->nb_m; r2.nb[1] = p->nb_n;
    pab_scalar<2>(p, r2, post, [] __device__(const PabView& w, int, PabState& s, const double* v) {
      s.cost_change = -(0.5 * v[0] + v[1]);
      s.bt = s.cost_change < 0;
      s.bt_on = s.bt;
      s.bt_alpha = 1.0;
      s.bt_fix = 0;
      s.phase = s.bt ? PH_BT : PH_FIN;
    });
  }
  };
  auto backtrack = [&] {
  // backtracking (trf_linear.backtracking): one trial per pass — halve alpha until the reflected step gives enough decrease
  pab_vec<1>(p, CNT_N, pab_red<1>({RED_SUM}, {1}, p->nb_n), bt_on, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
    const double x = w.nvec(NV_X, c)[i];
    const double xn = pab_reflect(x + s.bt_alpha * w.nvec(NV_P, c)[i], s.lb, s.ub);
    const double st = xn - x;
    w.nvec(NV_XN, c)[i] = xn;
    w.nvec(NV_ST, c)[i] = st;
    acc[0] += st * w.nvec(NV_G, c)[i];
  });
  pab_matvec<0>(p, NV_ST, -1, -1, MV_T1, bt_on);
  pab_vec<1>(p, CNT_M, pab_red<1>({RED_SUM}, {0}, p->nb_m), bt_on, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
    const double v = w.mvec(MV_T1, c)[i];
    acc[0] += v * v;
  });
  PabRed<2> r2{};
  r2.kind[0] = r2.kind[1] = RED_SUM; r2.slot[0] = 0; r2.slot[1] = 1; r2.nb[0] = p->nb_m; r2.nb[1] = p->nb_n;
  pab_scalar<2>(p, r2, bt_on, [] __device__(const PabView& w, int, PabState& s, const double* v) {
    s.cost_change = -(0.5 * v[0] + v[1]);
    if (s.cost_change > -0.1 * s.bt_alpha * s.p_dot_g) s.bt_on = 0;
    else s.bt_alpha *= 0.5;
  });
  // an active bound at x_new: step back by theta and make strictly feasible
  pab_vec<1>(p, CNT_N, pab_red<1>({RED_SUM}, {0}, p->nb_n), bt_any, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
    acc[0] += pab_active(w.nvec(NV_XN, c)[i], s.lb, s.ub) != 0 ? 1.0 : 0.0;
  });
  pab_scalar<1>(p, pab_red<1>({RED_SUM}, {0}, p->nb_n), bt_any, [] __device__(const PabView&, int, PabState& s, const double* v) {
    s.bt_fix = v[0] != 0;
  });
  pab_vec<1>(p, CNT_N, pab_red<1>({RED_SUM}, {1}, p->nb_n), bt_fix, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
    const double x = w.nvec(NV_X, c)[i];
    const double xn = pab_feasible(pab_reflect(x + (s.theta * s.bt_alpha) * w.nvec(NV_P, c)[i], s.lb, s.ub), s.lb, s.ub, 0.0);
    const double st = xn - x;
    w.nvec(NV_XN, c)[i] = xn;
    w.nvec(NV_ST, c)[i] = st;
    acc[0] += st * w.nvec(NV_G, c)[i];
  });
  pab_matvec<0>(p, NV_ST, -1, -1, MV_T1, bt_fix);
  pab_vec<1>(p, CNT_M, pab_red<1>({RED_SUM}, {0}, p->nb_m), bt_fix, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
    const double v = w.mvec(MV_T1, c)[i];
    acc[0] += v * v;
  });
  PabRed<2> r2b{};
  r2b.kind[0] = r2b.kind[1] = RED_SUM; r2b.slot[0] = 0; r2b.slot[1] = 1; r2b.nb[0] = p->nb_m; r2b.nb[1] = p->nb_n;
  pab_scalar<2>(p, r2b, bt_fix, [] __device__(const PabView&, int, PabState& s, const double* v) { s.cost_change = -(0.5 * v[0] + v[1]); });

  pab_scalar<0>(p, PabRed<0>{}, bt_any, [] __device__(const PabView&, int, PabState& s, const double*) { s.phase = PH_FIN; });
  };
  auto finish_iteration = [&] {
  // x = make_strictly_feasible(x + step, rstep = 0) — unless the step came from backtracking, which (scipy) keeps the old x
  pab_vec<0>(p, CNT_N, PabRed<0>{}, fin, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
#pragma clang fp contract(off)
    if (s.bt) return;
    w.nvec(NV_X, c)[i] = pab_feasible(w.nvec(NV_X, c)[i] + w.nvec(NV_ST, c)[i], s.lb, s.ub, 0.0);
  });
  pab_matvec<2>(p, NV_X, -1, -1, MV_R, fin);
  pab_scalar<2>(p, pab_red<2>({RED_SUM, RED_MAX}, {0, 1}, p->nb_mv), fin, [tol] __device__(const PabView& w, int, PabState& s, const double* v) {
    if (s.cost_change < tol * s.cost) { s.pending = 2; s.has_pending = 1; }
    s.cost = 0.5 * v[0];
    ++s.n_outer;
    if (s.has_pending) { s.status = s.pending; s.t_on = 0; s.phase = PH_DONE; }   // (a finished candidate needs no new gradient)
    else if (w.sliced) { s.rmax = v[1]; pab_fx_scale(s.colsum, s.rmax, s.fx_scale_r, s.fx_inv_r); }
  });
  pab_rmatvec<0>(p, MV_R, -1, -1, NV_G, fin);
  pab_scalar<0>(p, PabRed<0>{}, fin, [] __device__(const PabView&, int, PabState& s, const double*) { s.phase = PH_PRE; });
  };
  pab_vec<0>(p, CNT_MAUG, PabRed<0>{}, all, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
    w.mvec(MV_LU, c)[i] = i < s.m_data + s.m_sym ? w.mvec(MV_B, c)[i] : 0.0;
  });
  pab_lsmr_start(p);
  int cnt[PAB_FLAG_WORDS] = {0};
  cnt[PH_LSMR0] = p->K;
  cnt[10] = p->K;
  const int ticks_per_pass = 8;
  const long long pass_cap = (long long)(max_iter + 2) * ((long long)lsmr_maxiter / ticks_per_pass + 4);
  long long pass = 0;
  for (; pass < pass_cap; ++pass) {
    // the trust-region steps cover the candidates that were outside a solve when the lists were made (a candidate that
    // finishes a step is picked up by the next one in the SAME pass, and enters its next solve in it); the LSMR
    // iterations cover everyone who is not done
    const bool any_glue = cnt[PH_AFTER0] + cnt[PH_POST] + cnt[PH_BT] + cnt[PH_FIN] + cnt[PH_PRE] > 0;
    if (pass > 0) pab_cover(p, p->d_lists + p->K, cnt[11]);
    if (cnt[PH_AFTER0] > 0) after_first_solve();
    if (cnt[PH_POST] > 0) select_step();
    if (cnt[PH_POST] + cnt[PH_BT] > 0) backtrack();
    if (cnt[PH_POST] + cnt[PH_BT] + cnt[PH_FIN] > 0) finish_iteration();
    if (any_glue) begin_iteration();
    if (pass > 0) pab_cover(p, p->d_lists, cnt[10]);
    pab_lsmr_ticks(p, ticks_per_pass, lsmr_maxiter);
    pab_cover(p, nullptr, 0);
    hipLaunchKernelGGL(k_pab_lists, dim3(1), dim3(1024), 0, p->stream, pab_view(p), p->d_lists);
    if ((rc = pab_poll(p, cnt))) return rc;
    if (cnt[PH_DONE] == p->K) break;
  }
  pab_cover(p, nullptr, 0);
  if (pass >= pass_cap) return pab_fail(p, HH_ERR_STATE, "hh_pab_solve: the solve did not finish (internal)");
  // ---- x -> float32, prediction, cosine score (solver:484-530) ---------------------------------------------------------------
  {
    float* const xf = p->d_xf;
    const int64_t n = p->N;
    pab_vec<0>(p, CNT_N, PabRed<0>{}, all, [xf, n] __device__(const PabView& w, int c, int64_t i, const PabState&, double*) {
      const float f = (float)w.nvec(NV_X, c)[i];
      xf[(size_t)c * n + i] = f;
      w.nvec(NV_XF, c)[i] = (double)f;
    });
    pab_matvec<0>(p, NV_XF, -1, -1, MV_T1, all);
    pab_vec<3>(p, CNT_MDATA, pab_red<3>({RED_SUM, RED_SUM, RED_SUM}, {0, 1, 2}, p->nb_m), all,
               [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
                 double pr = w.mvec(MV_T1, c)[i];
                 if (s.clip && pr < 0) pr = 0;
                 const double b = w.mvec(MV_B, c)[i];
                 acc[0] += pr * b; acc[1] += pr * pr; acc[2] += b * b;
               });
    pab_scalar<3>(p, pab_red<3>({RED_SUM, RED_SUM, RED_SUM}, {0, 1, 2}, p->nb_m), all, [] __device__(const PabView&, int, PabState& s, const double* v) {
      const double norm = sqrt(v[1]) * sqrt(v[2]);
      s.score = norm == 0 ? 0.0 : v[0] / norm;
    });
  }
  PAB_HIP(p, hipGetLastError());
  {
    int f[PAB_FLAG_WORDS];
    if ((rc = pab_poll(p, f))) return rc;
    p->inconsistent = f[8];
  }
  // The solver's own consistency check (scalar step 1 of every LSMR iteration: every slice workgroup of the forward
  // product saw the `pend` / iteration tag this step sees).  A solve that failed it hands nothing back.
  if (p->inconsistent)
    return pab_fail(p, HH_ERR_STATE, "hh_pab_solve: the solver's self-check failed (" + std::to_string(p->inconsistent) +
                                         "): a workgroup read per-candidate state older than the previous launch wrote; no result is returned");
  std::vector<PabState> back((size_t)p->K);
  if ((rc = pab_to_host(p, back.data(), p->d_st, back.size() * sizeof(PabState)))) return rc;
  for (int c = 0; c < p->K; ++c) {
    scores[c] = back[(size_t)c].score;
    if (info) {
      info[5 * c] = back[(size_t)c].status;
      info[5 * c + 1] = back[(size_t)c].n_outer;
      info[5 * c + 2] = back[(size_t)c].lsmr_calls;
      info[5 * c + 3] = back[(size_t)c].lsmr_iters;
      info[5 * c + 4] = back[(size_t)c].first_iters;
    }
  }
  if (p->trace_c >= 0 && std::getenv("HH_PAB_TRACE_FILE")) {
    std::vector<double> tr((size_t)PAB_TRACE_ROWS * 8);
    if ((rc = pab_to_host(p, tr.data(), p->d_trace, tr.size() * sizeof(double)))) return rc;
    const std::string path = std::string(std::getenv("HH_PAB_TRACE_FILE")) + "." + std::to_string(p->trace_run++);
    if (FILE* f = std::fopen(path.c_str(), "wb")) { std::fwrite(tr.data(), sizeof(double), tr.size(), f); std::fclose(f); }
  }
  if (x_out) {   // [K][N] on the device -> [K][n] for the caller
    if ((rc = pab_stage(p, (size_t)p->K * p->N * sizeof(float)))) return rc;
    PAB_HIP(p, hipMemcpyAsync(p->h_stage, p->d_xf, (size_t)p->K * p->N * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    PAB_HIP(p, hipStreamSynchronize(p->stream));
    for (int c = 0; c < p->K; ++c)
      std::memcpy(x_out + (size_t)c * p->n, static_cast<const float*>(p->h_stage) + (size_t)c * p->N, (size_t)p->n * sizeof(float));
  }
  return HH_OK;
} HH_CATCH_PAB(p, "hh_pab_solve")

// The trilinear products recompute a ray's coordinates with the per-ray part of pa_coords hoisted (pabl_ray / pabl_at,
// path_a_linear.inc) and rely on the result being pa_coords' own, bit for bit: the reference's int() truncations sit ON
// integer coordinates for the identity operation and for integer rises.  This evaluates both forms on the HOST for every
// sample of every ray of every symmetry operation of one candidate (same source, same operation order, no device needed)
// and counts the samples whose (X, Y, Z) differ in any bit.  out = {samples, mismatches, ray and sample of the first}.
int hh_pab_check_ray_arithmetic(const hh_pa_params* q, int ny, int nx, int device, int64_t out[8]) try {
  if (!q || !out) return pab_fail(nullptr, HH_ERR_ARG, "hh_pab_check_ray_arithmetic: NULL argument");
  const int d2 = q->reconstruct_diameter_2d_pixel > 0 ? q->reconstruct_diameter_2d_pixel : ny;
  const int l2 = q->reconstruct_length_2d_pixel > 0 ? q->reconstruct_length_2d_pixel : nx;
  const int l3 = q->reconstruct_length_3d_pixel > 0 ? q->reconstruct_length_3d_pixel : l2;
  if (q->tilt_degree != 0 || q->psi_degree != 0 || !(q->rise_pixel > 0) || q->csym < 1)
    return pab_fail(nullptr, HH_ERR_ARG, "hh_pab_check_ray_arithmetic: tilt = psi = 0, rise > 0, csym >= 1");
  PaGeom g{};
  g.linear = 1;
  g.L2 = l2; g.D2 = d2; g.mz = l3; g.my = d2; g.mx = d2;
  g.scale = q->scale2d_to_3d;
  g.dy = q->dy_pixel;
  pa_euler1('y', 90.0, g.m_y90);
  double qy[4], qx[4], qq[4];
  pa_quat_axis('y', q->tilt_degree, qy);
  pa_quat_axis('x', q->psi_degree, qx);
  pa_quat_mul(qx, qy, qq);
  pa_quat_matrix(qq, g.m_yx);
  const int hmax = std::max(1, (int)(std::ceil((double)(l3 + l2)) / 2 / q->rise_pixel));
  out[0] = out[1] = 0; out[2] = out[3] = -1; out[4] = out[5] = out[6] = out[7] = -1;
  std::vector<PaOp> all_ops;
  for (int h = -hmax; h <= hmax; ++h)
    for (int cc = 0; cc < q->csym; ++cc) {
      PaOp op;
      pa_euler1('z', q->twist_degree * h + 360.0 * cc / q->csym, op.m_z);
      op.shift = h * q->rise_pixel;
      all_ops.push_back(op);
      for (int k = 0; k < l2; ++k)
        for (int j = 0; j < d2; ++j) {
          const PablRay pr = pabl_ray(g, op, k, j);
          for (int i = 0; i < d2; ++i) {
            double X, Y, Z, X2, Y2, Z2;
            pa_coords(g, op, k, j, i, X, Y, Z);
            pabl_at(pr, i, X2, Y2, Z2);
            ++out[0];
            if (std::memcmp(&X, &X2, 8) || std::memcmp(&Y, &Y2, 8) || std::memcmp(&Z, &Z2, 8)) {
              // (+0 against -0 is not a difference any truncation or fraction can see)
              if (X == X2 && Y == Y2 && Z == Z2) continue;
              if (out[1]++ == 0) { out[2] = ((int64_t)(h + hmax) * l2 + k) * d2 + j; out[3] = i; }
            }
          }
        }
    }
  if (device >= 0) {   // the same comparison by the device's own arithmetic
    PAB_HIP(nullptr, hipSetDevice(device));
    DevArena tmp;
    PaOp* d_ops = tmp.get<PaOp>(all_ops.size());
    unsigned long long* d_counts = tmp.get<unsigned long long>(4);
    if (int rc = pab_arena_ok(nullptr, tmp)) return rc;
    hipError_t e = hipMemcpy(d_ops, all_ops.data(), all_ops.size() * sizeof(PaOp), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_counts, 0, 4 * sizeof(unsigned long long));
    unsigned long long h_counts[4] = {0, 0, 0, 0};
    if (e == hipSuccess) {
      const size_t rays = (size_t)l2 * d2 * all_ops.size();
      hipLaunchKernelGGL(k_pabl_check, dim3((unsigned)((rays + 255) / 256)), dim3(256), 0, 0, g, d_ops, (int)all_ops.size(), d_counts);
      e = hipMemcpy(h_counts, d_counts, sizeof(h_counts), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return pab_fail(nullptr, HH_ERR_HIP, std::string("hh_pab_check_ray_arithmetic: ") + hipGetErrorString(e));
    out[4] = (int64_t)h_counts[0]; out[5] = (int64_t)h_counts[1]; out[6] = (int64_t)h_counts[2];
  }
  return HH_OK;
} HH_CATCH_PAB(nullptr, "hh_pab_check_ray_arithmetic")

// y = A_c x and g = A_c^T y through the SAME product kernels the solve uses (A_c = [A_data; A_hsym] of candidate c, rows in the
// reference's order for the caller): what the parity tests hold against the single-candidate projector and the oracle's
// matrices.  x: [unknowns], y: [data rows + symmetry rows] host float64.  Not to be called while a solve is running.
int hh_pab_matvec(hh_pab* p, int c, const double* x, double* y) try {
  if (!p || !x || !y || c < 0 || c >= p->K) return pab_fail(p, HH_ERR_ARG, "hh_pab_matvec: bad argument");
  PAB_HIP(p, hipSetDevice(p->device));
  pab_cover(p, nullptr, 0);
  int rc = pab_to_device(p, p->d_st, p->st.data(), p->st.size() * sizeof(PabState));
  if (rc) return rc;
  PAB_HIP(p, hipMemsetAsync(p->d_ctl, 0, (size_t)p->K * sizeof(unsigned), p->stream));
  PabView w = pab_view(p);
  if ((rc = pab_to_device(p, w.nv + ((size_t)NV_XF * p->K + c) * p->N, x, (size_t)p->n * sizeof(double)))) return rc;
  auto all = [] __device__(const auto&) { return true; };
  pab_matvec<0>(p, NV_XF, -1, -1, MV_T1, all);
  PAB_HIP(p, hipGetLastError());
  const PabState& s = p->st[(size_t)c];
  std::vector<double> dev((size_t)(s.m_data + s.m_sym));
  if ((rc = pab_to_host(p, dev.data(), w.mv + ((size_t)MV_T1 * p->K + c) * p->MA, dev.size() * sizeof(double)))) return rc;
  // data rows: device (slice-major) order -> the reference's (operation, k, j) order, through the rays
  std::vector<int> ray_dev((size_t)s.m_data);
  if ((rc = pab_to_host(p, ray_dev.data(), p->d_ray_of_row + s.row0, ray_dev.size() * sizeof(int)))) return rc;
  std::vector<std::pair<int, int>> order((size_t)s.m_data);
  for (int64_t r = 0; r < s.m_data; ++r) order[(size_t)r] = {ray_dev[(size_t)r], (int)r};
  std::sort(order.begin(), order.end());
  for (int64_t r = 0; r < s.m_data; ++r) y[r] = dev[(size_t)order[(size_t)r].second];
  for (int64_t r = 0; r < s.m_sym; ++r) y[s.m_data + r] = dev[(size_t)(s.m_data + r)];
  return HH_OK;
} HH_CATCH_PAB(p, "hh_pab_matvec")

int hh_pab_rmatvec(hh_pab* p, int c, const double* y, double* g) try {
  if (!p || !y || !g || c < 0 || c >= p->K) return pab_fail(p, HH_ERR_ARG, "hh_pab_rmatvec: bad argument");
  PAB_HIP(p, hipSetDevice(p->device));
  pab_cover(p, nullptr, 0);
  PabState& s = p->st[(size_t)c];
  double ymax = 0;
  for (int64_t r = 0; r < s.m_data + s.m_sym; ++r) ymax = std::max(ymax, std::fabs(y[r]));
  if (!std::isfinite(ymax)) return pab_fail(p, HH_ERR_ARG, "hh_pab_rmatvec: y is not finite");
  if (p->sliced) pab_fx_scale(s.colsum, ymax, s.fx_scale_r, s.fx_inv_r);
  int rc = pab_to_device(p, p->d_st, p->st.data(), p->st.size() * sizeof(PabState));
  if (rc) return rc;
  PAB_HIP(p, hipMemsetAsync(p->d_ctl, 0, (size_t)p->K * sizeof(unsigned), p->stream));
  PabView w = pab_view(p);
  std::vector<int> ray_dev((size_t)s.m_data);
  if ((rc = pab_to_host(p, ray_dev.data(), p->d_ray_of_row + s.row0, ray_dev.size() * sizeof(int)))) return rc;
  std::vector<std::pair<int, int>> order((size_t)s.m_data);
  for (int64_t r = 0; r < s.m_data; ++r) order[(size_t)r] = {ray_dev[(size_t)r], (int)r};
  std::sort(order.begin(), order.end());
  std::vector<double> dev((size_t)(s.m_data + s.m_sym));
  for (int64_t r = 0; r < s.m_data; ++r) dev[(size_t)order[(size_t)r].second] = y[r];
  for (int64_t r = 0; r < s.m_sym; ++r) dev[(size_t)(s.m_data + r)] = y[s.m_data + r];
  if ((rc = pab_to_device(p, w.mv + ((size_t)MV_T1 * p->K + c) * p->MA, dev.data(), dev.size() * sizeof(double)))) return rc;
  auto all = [] __device__(const auto&) { return true; };
  pab_rmatvec<0>(p, MV_T1, -1, -1, NV_G, all);
  PAB_HIP(p, hipGetLastError());
  return pab_to_host(p, g, w.nv + ((size_t)NV_G * p->K + c) * p->N, (size_t)p->n * sizeof(double));
} HH_CATCH_PAB(p, "hh_pab_rmatvec")

// ---- the scikit-learn models of solve_equations (solver_linear_regression.py:270-342) ------------------------------------------------
// ElasticNet / Lasso (coordinate descent, selection = "random": run-to-run different in the reference), Ridge (L-BFGS-B under
// the positivity rule) and LinearRegression (dense NNLS under it) all minimise, with fit_intercept = True,
//     (1 / 2m) || (b - mean b) - (A - 1 mu^T) w ||^2 + alpha rho |w|_1 + alpha (1 - rho) / 2 |w|^2,     w >= 0 where positive
// (mu = the column means of A; m = rows; Ridge: alpha / m, rho = 0; LinearRegression: alpha = 0) and return w (coef_; the
// intercept is dropped, solver:330).  For rho < 1 or a full-rank A the minimiser is unique whatever the order the reference's
// solver visits the coordinates in, so it is what this computes — FISTA (Beck & Teboulle 2009) with gradient restart
// (O'Donoghue & Candes 2015) on the implicit operator, every vector on the device, every candidate of the batch in the same
// launches; float64 (the reference's solvers run in float32 on its float32 matrix: its results sit 1e-4 from the
// minimiser and scatter by 1e-5 from run to run; the fixtures G14 record both).  The step 1 / L comes from 40 power
// iterations on the centred operator.  A candidate stops when max |w_new - w| <= tol max |w_new|, or when the prox-gradient
// mapping at the momentum point v, L max |v - w_new|, is at most 20 tol lambda_max (lambda_max = max |grad| at w = 0, its
// positive part under positivity), or after max_iter.
// alpha: [K] (the caller repeats all-zero solutions with alpha / 10 like solver:333-338); ridge_form: alpha is divided by m.
// info: [K][3] = {iterations, converged, non-zero coefficients}; objective: [K] value of the function above at w (may be NULL).
int hh_pab_solve_prox(hh_pab* p, const int32_t* positive, const int32_t* clip, const double* alpha, double l1_ratio, int ridge_form,
                      double tol, int max_iter, float* x_out, double* scores, int32_t* info, double* objective) try {
  if (!p || !scores || !alpha) return pab_fail(p, HH_ERR_ARG, "hh_pab_solve_prox: NULL argument");
  if (!(tol > 0) || max_iter < 1 || !(l1_ratio >= 0 && l1_ratio <= 1)) return pab_fail(p, HH_ERR_ARG, "hh_pab_solve_prox: tol > 0, max_iter >= 1, 0 <= l1_ratio <= 1");
  // (the general nearest-neighbour products gather A^T y in float64 along the transposed pattern: the fixed-point scales the
  // steps below update are not read there)
  if (!p->sliced && !p->flat) return pab_fail(p, HH_ERR_ARG, "hh_pab_solve_prox: needs tilt = psi = 0");
  PAB_HIP(p, hipSetDevice(p->device));
  p->launches = p->syncs = p->ticks = p->inconsistent = 0;
  PAB_HIP(p, hipMemsetAsync(p->d_flags, 0, PAB_FLAG_WORDS * sizeof(int), p->stream));
  pab_cover(p, nullptr, 0);
  for (int c = 0; c < p->K; ++c) {
    PabState& s = p->st[(size_t)c];
    if (!(alpha[c] >= 0)) return pab_fail(p, HH_ERR_ARG, "hh_pab_solve_prox: alpha must not be negative");
    const double m = (double)(s.m_data + s.m_sym);
    s.bounded = positive && positive[c] ? 1 : 0;
    s.clip = clip && clip[c] ? 1 : 0;
    s.phase = PH_PRE; s.aug = 0; s.start = 0; s.l_on = 0; s.l_skip = 0; s.pend = 0; s.t_on = 0; s.inb = 0; s.rsu_pos = 0; s.bt_on = 0; s.bt_fix = 0;
    s.p_alpha = ridge_form ? alpha[c] / m : alpha[c];
    s.p_rho = l1_ratio;
    s.p_it = 0; s.p_conv = 0; s.p_nnz = 0; s.p_t = 1.0; s.p_beta = 0; s.p_L = 1; s.p_lam = 0; s.p_obj = 0; s.p_lam0 = 0;
    s.fx_scale_r = s.fx_scale; s.fx_inv_r = s.fx_inv;   // |y| <= 1 for the first transposed product below (a vector of ones)
    s.score = 0;
  }
  int rc = pab_to_device(p, p->d_st, p->st.data(), p->st.size() * sizeof(PabState));
  if (rc) return rc;
  {
    std::vector<unsigned> ctl((size_t)p->K, (unsigned)PH_PRE);
    if ((rc = pab_to_device(p, p->d_ctl, ctl.data(), ctl.size() * sizeof(unsigned)))) return rc;
  }
  auto run = [] __device__(const auto& s) { return s.phase == PH_PRE; };
  auto all = [] __device__(const auto&) { return true; };
  // mu = A^T 1 / m (NV_RH), mean b (p_ybar); w = 0 (NV_X), momentum point (NV_P) = the power iteration's start
  pab_vec<1>(p, CNT_M, pab_red<1>({RED_SUM}, {0}, p->nb_m), all, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
    w.mvec(MV_T2, c)[i] = 1.0;
    acc[0] += w.mvec(MV_B, c)[i];
  });
  pab_scalar<1>(p, pab_red<1>({RED_SUM}, {0}, p->nb_m), all, [] __device__(const PabView&, int, PabState& s, const double* v) {
    s.p_ybar = v[0] / (double)(s.m_data + s.m_sym);
  });
  pab_rmatvec<0>(p, MV_T2, -1, -1, NV_RH, all);
  pab_vec<0>(p, CNT_N, PabRed<0>{}, all, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
#pragma clang fp contract(off)
    w.nvec(NV_RH, c)[i] = w.nvec(NV_RH, c)[i] / (double)(s.m_data + s.m_sym);
    w.nvec(NV_X, c)[i] = 0.0;
    w.nvec(NV_P, c)[i] = 1.0 / sqrt((double)w.n);
  });
  // z = (A - 1 mu^T) src [- (b - mean b) when `residual`] -> MV_R, with sum z, max |z| (the next A^T z's fixed-point scale) and |z|^2
  auto centred_forward = [&](int src, bool residual) {
    pab_vec<1>(p, CNT_N, pab_red<1>({RED_SUM}, {0}, p->nb_n), run, [src] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
      acc[0] += w.nvec(NV_RH, c)[i] * w.nvec(src, c)[i];
    });
    pab_scalar<1>(p, pab_red<1>({RED_SUM}, {0}, p->nb_n), run, [] __device__(const PabView&, int, PabState& s, const double* v) { s.p_mu_w = v[0]; });
    pab_matvec<0>(p, src, -1, -1, MV_T1, run);
    pab_vec<3>(p, CNT_M, pab_red<3>({RED_SUM, RED_MAX, RED_SUM}, {0, 1, 2}, p->nb_m), run,
               [residual] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
                 double z = w.mvec(MV_T1, c)[i] - s.p_mu_w;
                 if (residual) z = z - (w.mvec(MV_B, c)[i] - s.p_ybar);
                 w.mvec(MV_R, c)[i] = z;
                 acc[0] += z; acc[1] = fmax(acc[1], fabs(z)); acc[2] += z * z;
               });
    pab_scalar<3>(p, pab_red<3>({RED_SUM, RED_MAX, RED_SUM}, {0, 1, 2}, p->nb_m), run, [] __device__(const PabView&, int, PabState& s, const double* v) {
      s.p_sum = v[0]; s.rmax = v[1]; s.p_rn2 = v[2];
      pab_fx_scale(s.colsum, s.rmax, s.fx_scale_r, s.fx_inv_r);
    });
  };
  // NV_G = (A - 1 mu^T)^T MV_R
  auto centred_backward = [&] {
    pab_rmatvec<0>(p, MV_R, -1, -1, NV_G, run);
    pab_vec<0>(p, CNT_N, PabRed<0>{}, run, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
#pragma clang fp contract(off)
      w.nvec(NV_G, c)[i] = w.nvec(NV_G, c)[i] - w.nvec(NV_RH, c)[i] * s.p_sum;
    });
  };
  // ---- largest eigenvalue of the centred normal operator: 40 power iterations --------------------------------------------------------
  for (int k = 0; k < 40; ++k) {
    centred_forward(NV_P, false);
    centred_backward();
    pab_vec<1>(p, CNT_N, pab_red<1>({RED_SUM}, {0}, p->nb_n), run, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
      const double g = w.nvec(NV_G, c)[i];
      acc[0] += g * g;
    });
    pab_scalar<1>(p, pab_red<1>({RED_SUM}, {0}, p->nb_n), run, [] __device__(const PabView&, int, PabState& s, const double* v) { s.p_lam = sqrt(v[0]); });
    pab_vec<0>(p, CNT_N, PabRed<0>{}, run, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
      w.nvec(NV_P, c)[i] = s.p_lam > 0 ? w.nvec(NV_G, c)[i] / s.p_lam : 0.0;
    });
  }
  pab_scalar<0>(p, PabRed<0>{}, run, [] __device__(const PabView&, int, PabState& s, const double*) {
    const double m = (double)(s.m_data + s.m_sym);
    s.p_L = 1.02 * s.p_lam / m + s.p_alpha * (1 - s.p_rho);
    if (!(s.p_L > 0)) s.p_L = 1.0;
  });
  pab_vec<0>(p, CNT_N, PabRed<0>{}, run, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double*) { w.nvec(NV_P, c)[i] = 0.0; });
  // ---- FISTA -------------------------------------------------------------------------------------------------------------------------
  int cnt[PAB_FLAG_WORDS] = {0};
  cnt[10] = p->K;
  int it = 0;
  const int per_poll = 16;
  while (it < max_iter) {
    if (it > 0) pab_cover(p, p->d_lists, cnt[10]);
    for (int k = 0; k < per_poll && it < max_iter; ++k, ++it) {
      centred_forward(NV_P, true);
      centred_backward();
      pab_vec<6>(p, CNT_N, pab_red<6>({RED_MAX, RED_MAX, RED_SUM, RED_SUM, RED_MAX, RED_MAX}, {0, 1, 2, 3, 4, 5}, p->nb_n), run,
                 [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
                   const double v = w.nvec(NV_P, c)[i], wo = w.nvec(NV_X, c)[i];
                   const double m = (double)(s.m_data + s.m_sym);
                   const double g = w.nvec(NV_G, c)[i] / m + (s.p_alpha * (1 - s.p_rho)) * v;
                   const double z = v - g / s.p_L, th = s.p_alpha * s.p_rho / s.p_L;
                   double wn;
                   if (s.bounded) wn = fmax(0.0, z - th);
                   else wn = z > th ? z - th : z < -th ? z + th : 0.0;
                   w.nvec(NV_XN, c)[i] = wn;
                   acc[0] = fmax(acc[0], fabs(wn - wo));
                   acc[1] = fmax(acc[1], fabs(wn));
                   acc[2] += (v - wn) * (wn - wo);
                   acc[3] += wn != 0.0 ? 1.0 : 0.0;
                   acc[4] = fmax(acc[4], fabs(v - wn));                       // the prox-gradient mapping, / L
                   acc[5] = fmax(acc[5], s.bounded ? fmax(-g, 0.0) : fabs(g));   // lambda_max at the first step (v = 0)
                 });
      pab_scalar<6>(p, pab_red<6>({RED_MAX, RED_MAX, RED_SUM, RED_SUM, RED_MAX, RED_MAX}, {0, 1, 2, 3, 4, 5}, p->nb_n), run,
                    [tol, max_iter] __device__(const PabView&, int, PabState& s, const double* v) {
        s.p_dw = v[0]; s.p_wmax = v[1]; s.p_nnz = (int)v[3];
        if (s.p_it == 0) s.p_lam0 = v[5];
        double t = s.p_t;
        if (v[2] > 0) t = 1.0;                                  // gradient restart: the momentum points uphill
        const double tn = (1 + sqrt(1 + 4 * t * t)) / 2;
        s.p_beta = (t - 1) / tn;
        s.p_t = tn;
        ++s.p_it;
        // stop on a small relative step, or on optimality: the subgradient residual at w_new, L |v - w_new| up to the
        // change of the gradient between v and w_new, at most 20 tol of lambda_max (the case of ill-conditioned fits
        // without a penalty, whose steps stay large: lreg on the trilinear products)
        const bool done = s.p_dw <= tol * s.p_wmax || s.p_L * v[4] <= 20 * tol * s.p_lam0;
        if (done || s.p_it >= max_iter) s.p_conv = done ? 1 : 2;
      });
      pab_vec<0>(p, CNT_N, PabRed<0>{}, run, [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double*) {
#pragma clang fp contract(off)
        const double wn = w.nvec(NV_XN, c)[i], wo = w.nvec(NV_X, c)[i];
        w.nvec(NV_P, c)[i] = wn + s.p_beta * (wn - wo);
        w.nvec(NV_X, c)[i] = wn;
      });
      pab_scalar<0>(p, PabRed<0>{}, run, [] __device__(const PabView&, int, PabState& s, const double*) { if (s.p_conv) s.phase = PH_DONE; });
    }
    pab_cover(p, nullptr, 0);
    hipLaunchKernelGGL(k_pab_lists, dim3(1), dim3(1024), 0, p->stream, pab_view(p), p->d_lists);
    if ((rc = pab_poll(p, cnt))) return rc;
    if (cnt[PH_DONE] == p->K) break;
  }
  pab_cover(p, nullptr, 0);
  // the objective at w (for the caller's comparison with the reference's own): residual at w, |w|_1, |w|^2
  pab_scalar<0>(p, PabRed<0>{}, all, [] __device__(const PabView&, int, PabState& s, const double*) { s.phase = PH_PRE; });
  centred_forward(NV_X, true);
  pab_vec<2>(p, CNT_N, pab_red<2>({RED_SUM, RED_SUM}, {0, 1}, p->nb_n), all, [] __device__(const PabView& w, int c, int64_t i, const PabState&, double* acc) {
    const double x = w.nvec(NV_X, c)[i];
    acc[0] += fabs(x); acc[1] += x * x;
  });
  pab_scalar<2>(p, pab_red<2>({RED_SUM, RED_SUM}, {0, 1}, p->nb_n), all, [] __device__(const PabView&, int, PabState& s, const double* v) {
    const double m = (double)(s.m_data + s.m_sym);
    s.p_obj = s.p_rn2 / (2 * m) + s.p_alpha * s.p_rho * v[0] + 0.5 * s.p_alpha * (1 - s.p_rho) * v[1];
    s.phase = PH_DONE;
  });
  // x -> float32, prediction, cosine score (solver:484-530)
  {
    float* const xf = p->d_xf;
    const int64_t n = p->N;
    pab_vec<0>(p, CNT_N, PabRed<0>{}, all, [xf, n] __device__(const PabView& w, int c, int64_t i, const PabState&, double*) {
      const float f = (float)w.nvec(NV_X, c)[i];
      xf[(size_t)c * n + i] = f;
      w.nvec(NV_XF, c)[i] = (double)f;
    });
    pab_matvec<0>(p, NV_XF, -1, -1, MV_T1, all);
    pab_vec<3>(p, CNT_MDATA, pab_red<3>({RED_SUM, RED_SUM, RED_SUM}, {0, 1, 2}, p->nb_m), all,
               [] __device__(const PabView& w, int c, int64_t i, const PabState& s, double* acc) {
#pragma clang fp contract(off)
                 double pr = w.mvec(MV_T1, c)[i];
                 if (s.clip && pr < 0) pr = 0;
                 const double b = w.mvec(MV_B, c)[i];
                 acc[0] += pr * b; acc[1] += pr * pr; acc[2] += b * b;
               });
    pab_scalar<3>(p, pab_red<3>({RED_SUM, RED_SUM, RED_SUM}, {0, 1, 2}, p->nb_m), all, [] __device__(const PabView&, int, PabState& s, const double* v) {
      const double norm = sqrt(v[1]) * sqrt(v[2]);
      s.score = norm == 0 ? 0.0 : v[0] / norm;
    });
  }
  PAB_HIP(p, hipGetLastError());
  std::vector<PabState> back((size_t)p->K);
  if ((rc = pab_to_host(p, back.data(), p->d_st, back.size() * sizeof(PabState)))) return rc;
  for (int c = 0; c < p->K; ++c) {
    scores[c] = back[(size_t)c].score;
    if (objective) objective[c] = back[(size_t)c].p_obj;
    if (info) { info[3 * c] = back[(size_t)c].p_it; info[3 * c + 1] = back[(size_t)c].p_conv == 1; info[3 * c + 2] = back[(size_t)c].p_nnz; }
  }
  if (x_out) {
    if ((rc = pab_stage(p, (size_t)p->K * p->N * sizeof(float)))) return rc;
    PAB_HIP(p, hipMemcpyAsync(p->h_stage, p->d_xf, (size_t)p->K * p->N * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    PAB_HIP(p, hipStreamSynchronize(p->stream));
    for (int c = 0; c < p->K; ++c)
      std::memcpy(x_out + (size_t)c * p->n, static_cast<const float*>(p->h_stage) + (size_t)c * p->N, (size_t)p->n * sizeof(float));
  }
  return HH_OK;
} HH_CATCH_PAB(p, "hh_pab_solve_prox")

// the form of the products in use: HH_PAB_FORM_* (include/helicon_hip.h)
int hh_pab_product_form(const hh_pab* p) try {
  if (!p) return HH_ERR_ARG;
  if (!p->linear) return p->sliced ? HH_PAB_FORM_SLICED : HH_PAB_FORM_GENERAL;
  return p->band_T ? HH_PAB_FORM_BANDED : p->fac_G ? HH_PAB_FORM_FACTORED : HH_PAB_FORM_LDS;
} HH_CATCH_PAB(p, "hh_pab_product_form")

// counters of the last hh_pab_solve: {kernel launches, host synchronisations, LSMR iterations queued, self-check failures}
int hh_pab_counters(const hh_pab* p, int64_t out[4]) try {
  if (!p || !out) return HH_ERR_ARG;
  out[0] = p->launches; out[1] = p->syncs; out[2] = p->ticks; out[3] = p->inconsistent;
  return HH_OK;
} HH_CATCH_PAB(p, "hh_pab_counters")

}  // extern "C"
