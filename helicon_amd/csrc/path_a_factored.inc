// path_a_factored.inc — the trilinear projector of the batched Path-A solver in SEPARABLE form (round 4; included by
// path_a_batch.inc after path_a_linear.inc, whose direct kernels remain for lists too long for it: d2 > 128).
//
// Reference: webApps/denovo3D/solver_linear_regression.py:1414-1503 (build_A_data_matrix, "linear").
//
// With tilt = psi = 0 the row of A_data for the ray (operation o, image column k, image row j) is
//     A[(o, k, j), (z, v)] = cz0(o, k) R_o[j][v]   for z = H(o, k),      cz0 = 1 - zf
//                          = cz1(o, k) R_o[j][v]   for z = H(o, k) + 1,  cz1 = zf
// because the in-plane coordinates (X, Y) of a ray's samples depend on (o, j, i) only and the axial coordinate Z on (o, k)
// only: R_o[j] = the bilinear in-plane footprint of image row j under operation o, the SAME for all L2 image columns.
// (Z carries the ~1e-16 rounding noise of scipy's Ry(90) per sample; the factored form uses the noise-free Z of the
// middle sample for zf — a 1e-15 relative change of a weight the reference itself rounds to float32 — and keeps the
// reference's per-sample decision WHICH samples are valid: an (o, k) whose samples are not all valid along z, Z within
// noise of -1 or of mz - 1, gets its own footprint list with just those samples.)
//
// So the direct kernels' 150 vector instructions per (sample, row) — 60 of them float64 coordinate arithmetic, repeated for
// every image column and in both products — shrink to a table look-up: at create, k_pabf_entries writes for every (list,
// j) the valid samples' cell index and in-plane fractions (exact: pa_coords itself); in the products a workgroup owns a
// GROUP of G consecutive home layers (G + 1 planes of x, or of the fixed-point accumulator, in LDS: 5 x 24 KB at D = 64),
// and a "column" (list, j) of the group is walked once for all its <= 8 rows (the image columns k whose home lies in the
// group): per sample 4 in-plane weights, per plane 2 ds_read2_b64 + 8 float64 operations, then the rows are
//     y[(o, k, j)] = cz0 S[H - base] + cz1 S[H + 1 - base],     S[p] = sum over samples of w . x[plane base + p]
// and in the transposed product T[p] = sum over the column's rows of cz . y first, then 4 LDS integer atomics per sample
// and plane.  About 16 instructions per (sample, row) instead of 150, and the footprint lists (3 MB per candidate) are
// read once per group instead of the geometry being recomputed per row.

constexpr int PABF_KMAX = 8;   // rows of a column (= lanes per column)

struct PabfEntry {        // one valid sample of a footprint list
  double xf, yf;
  unsigned idx;           // in-plane index of (y, x) | of (y + 1, x) << 16; (y, x + 1) and (y + 1, x + 1) are the next voxels
  unsigned pad;
};
struct PabfRowRef {       // one (operation, image column) of a column group
  int rowbase;            // first row (candidate-relative, device order) of the (o, k) rays; -1: none
  int hp;                 // home layer - first layer of the group
  unsigned long long jmask[2];   // image rows j that have a ray
  double cz0, cz1;
};
struct PabfGroupList {    // the rows of one footprint list inside one group of home layers
  int list, nk;
  PabfRowRef e[PABF_KMAX];
};
struct PabfZinfo {        // per (operation, image column): k_pabf_zinfo
  int home;               // as k_pabl_has files the rays
  int pad;
  double cz0, cz1;
  unsigned long long zmask[2];   // samples i valid along z
};

// ---- set-up ------------------------------------------------------------------------------------------------------------------
// axial data of every (candidate slot, operation, image column)
__global__ __launch_bounds__(128) void k_pabf_zinfo(PabGeomRef gr, int K, int max_ops, const int* __restrict__ n_used, PabfZinfo* __restrict__ out) {
#pragma clang fp contract(off)
  const int c = blockIdx.z, o = blockIdx.y, k = blockIdx.x * 128 + threadIdx.x;
  if (c >= K) return;
  const PaGeom g = gr.geom[c];
  if (k >= g.L2 || o >= n_used[c]) return;
  const PaOp op = gr.ops[gr.op0[c] + o];
  PabfZinfo z{};
  double X, Y, Z;
  pa_coords(g, op, k, 0, g.D2 / 2, X, Y, Z);
  z.home = max(0, (int)floor(Z - 1e-9));
  // the fraction relative to the home layer: 1 when the noise-free Z is the next integer itself (its samples truncate to
  // home with zf ~ 1 or to home + 1 with zf ~ 0: all weight on plane home + 1), negative for Z in [-1, 0) (int() truncates
  // those to layer 0: weights 1 - Z and Z, the reference's own)
  const int zl = (int)floor(Z);
  const double zf = zl == z.home + 1 ? 1.0 : Z - (double)z.home;
  z.cz0 = 1 - zf;
  z.cz1 = zf;
  for (int i = 0; i < g.D2; ++i) {
    pa_coords(g, op, k, 0, i, X, Y, Z);
    const long long zi = (long long)Z;
    if (zi >= 0 && zi + 1 <= g.mz - 1) z.zmask[i >> 6] |= 1ull << (i & 63);
  }
  out[((size_t)c * max_ops + o) * g.L2 + k] = z;
}
// The in-plane coordinates DO depend on the image column at the 1e-14 level: scipy's Ry(90) has c^2 - s^2 = 2.2e-16 where a
// zero belongs, so X carries (k - L2 / 2) 2.2e-16.  Irrelevant for the weights — but where X or Y sits ON an integer (the
// identity operation, quarter turns) it decides the int() truncation, i.e. WHICH cell a sample uses and, at the rim of the
// cylinder, whether it is valid: columns left and right of the image centre then differ.  Two image columns may share a
// footprint list only if every sample makes the same cell decision; this hashes the decisions of (candidate, operation,
// column): sum over (j, i) of a mix of (sample, cell, validity) — commutative, so the threads need no order.
__device__ __forceinline__ unsigned long long pabf_mix(unsigned long long v) {
  v ^= v >> 33; v *= 0xff51afd7ed558ccdull; v ^= v >> 33; v *= 0xc4ceb9fe1a85ec53ull; v ^= v >> 33;
  return v;
}
__global__ __launch_bounds__(128) void k_pabf_cellhash(PabGeomRef gr, int K, int max_ops, const int* __restrict__ n_used,
                                                       const unsigned* __restrict__ sidx2, unsigned long long* __restrict__ hash) {
#pragma clang fp contract(off)
  const int c = blockIdx.z, o = blockIdx.y, k = blockIdx.x;
  if (c >= K) return;
  const PaGeom g = gr.geom[c];
  if (k >= g.L2 || o >= n_used[c]) return;
  const PaOp op = gr.ops[gr.op0[c] + o];
  unsigned long long h = 0;
  for (int j = threadIdx.x; j < g.D2; j += 128)
    for (int i = 0; i < g.D2; ++i) {
      double X, Y, Z;
      pa_coords(g, op, k, j, i, X, Y, Z);
      const long long yi = (long long)Y, xi = (long long)X;
      unsigned long long cell = ~0ull;   // not valid in the plane
      if (!(yi < 0 || yi + 1 > g.my - 1 || xi < 0 || xi + 1 > g.mx - 1)) {
        const unsigned lo = sidx2[(int)yi * g.mx + (int)xi], hi = sidx2[((int)yi + 1) * g.mx + (int)xi];
        if (!((lo & 0xffffu) == 0xffffu || (lo >> 16) == 0xffffu || (hi & 0xffffu) == 0xffffu || (hi >> 16) == 0xffffu))
          cell = ((unsigned long long)yi << 20) | (unsigned long long)xi;
      }
      h += pabf_mix((((unsigned long long)(j * g.D2 + i)) << 40) ^ cell);
    }
  for (int off = 32; off > 0; off >>= 1) h += __shfl_down(h, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&hash[((size_t)c * max_ops + o) * g.L2 + k], h);
}
// first row and image-row mask of every (operation, image column) that has rays: one thread per data row
__global__ __launch_bounds__(256) void k_pabf_rowbase(PabView w, int max_ops, int* __restrict__ rowbase, unsigned long long* __restrict__ jmask) {
  const int c = PAB_CAND, bx = PAB_BLOCK;
  if (c < 0) return;
  const PabState& s = w.st[c];
  const int64_t r = (int64_t)bx * 256 + threadIdx.x;
  if (r >= s.m_data) return;
  const PaGeom& g = w.lin_geom[c];
  const int ray = w.ray_of_row[s.row0 + r];
  const int j = ray % g.D2, k = (ray / g.D2) % g.L2, o = ray / (g.D2 * g.L2);
  const size_t at = ((size_t)c * max_ops + o) * g.L2 + k;
  atomicMin(&rowbase[at], (int)r);
  atomicOr(&jmask[2 * at + (j >> 6)], 1ull << (j & 63));
}
// the footprint lists: entries[((c * max_lists + list) * D2 + j) * D2 + s], count[(c * max_lists + list) * D2 + j]
struct PabfListRef {
  int op;
  int k;                  // the image column whose arithmetic the list's cells and fractions are taken from
  unsigned long long zmask[2];
};
__global__ __launch_bounds__(64) void k_pabf_entries(PabGeomRef gr, int K, int max_lists, const int* __restrict__ n_lists,
                                                     const PabfListRef* __restrict__ lists, const unsigned* __restrict__ sidx2,
                                                     PabfEntry* __restrict__ entries, unsigned char* __restrict__ count) {
#pragma clang fp contract(off)
  const int c = blockIdx.z, li = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
  if (c >= K || li >= n_lists[c]) return;
  const PaGeom g = gr.geom[c];
  if (j >= g.D2) return;
  const PabfListRef lr = lists[(size_t)c * max_lists + li];
  const PaOp op = gr.ops[gr.op0[c] + lr.op];
  PabfEntry* out = entries + (((size_t)c * max_lists + li) * g.D2 + j) * g.D2;
  int n = 0;
  for (int i = 0; i < g.D2; ++i) {
    if (!((lr.zmask[i >> 6] >> (i & 63)) & 1ull)) continue;
    double X, Y, Z;
    pa_coords(g, op, lr.k, j, i, X, Y, Z);
    const long long yi = (long long)Y, xi = (long long)X;
    if (yi < 0 || yi + 1 > g.my - 1 || xi < 0 || xi + 1 > g.mx - 1) continue;
    const unsigned lo = sidx2[(int)yi * g.mx + (int)xi], hi = sidx2[((int)yi + 1) * g.mx + (int)xi];
    if ((lo & 0xffffu) == 0xffffu || (lo >> 16) == 0xffffu || (hi & 0xffffu) == 0xffffu || (hi >> 16) == 0xffffu) continue;
    PabfEntry e;
    e.xf = X - (double)xi;
    e.yf = Y - (double)yi;
    e.idx = (lo & 0xffffu) | ((hi & 0xffffu) << 16);   // (y, x + 1) = (y, x) + 1: the voxels of a disc row are ranked consecutively
    e.pad = 0;
    out[n++] = e;
  }
  count[((size_t)c * max_lists + li) * g.D2 + j] = (unsigned char)n;
}

// in-plane weights of one sample, order (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)
__device__ __forceinline__ void pabf_weights(const PabfEntry& e, double w[4]) {
#pragma clang fp contract(off)
  const double ax = 1 - e.xf, ay = 1 - e.yf;
  w[0] = ay * ax; w[1] = ay * e.xf; w[2] = e.yf * ax; w[3] = e.yf * e.xf;
}

// ---- A x ---------------------------------------------------------------------------------------------------------------------------
// dynamic LDS: [G + 1][nslice] doubles.  Blocks [0, ng): groups of home layers.  The symmetry / augmented rows are
// k_pabf_tail's (its own launch: they need no LDS, and inside this kernel every workgroup — theirs too — would hold the
// 120 KB of planes, one workgroup per compute unit, while all they do is wait for gathers from L2).  MODE as in k_pabl_matvec.
template <int MODE, int G, class P>
__global__ __launch_bounds__(PABS_THREADS) void k_pabf_matvec(PabView w, int src, int dsc, int rootv, int dst, P pred) {
#pragma clang fp contract(off)
  const int c = PAB_CAND, bx = PAB_BLOCK;
  if (c < 0) return;
  if (!pred(pab_ctl_load(w.ctl, c))) return;
  __shared__ PabState s_lds;
  pab_state_load(&s_lds, &w.st[c]);
  const PabState& s = s_lds;
  extern __shared__ double fac_lds[];
  __shared__ double lds16[PABS_THREADS / 64];
  const bool op_aug = MODE != 1 || s.aug;
  const double* __restrict__ x = w.nvec(src, c);
  const double* __restrict__ d = dsc >= 0 && op_aug ? w.nvec(dsc, c) : nullptr;
  const double* __restrict__ root = rootv >= 0 && op_aug ? w.nvec(rootv, c) : nullptr;
  double* __restrict__ y = w.mvec(dst, c);
  double sq = 0, sqx = 0, mx = 0;
  {
    // block = (group of home layers, part): a group's columns are dealt to fac_split workgroups, each staging the group's
    // planes — a quarter of the work per workgroup, four times the workgroups: with few candidates left in a solve (a
    // launch then is ONE round of workgroups, and its duration theirs) a launch takes a quarter of the time
    const int grp = bx / w.fac_split, part = bx % w.fac_split;
    const int base_z = grp * G;
    const int np = min(G + 1, w.mz - base_z);                  // planes of this group
    const int own = part ? 0 : grp == w.fac_ng - 1 ? np : min(G, np);   // planes whose deferred update is this block's (every plane once)
    // (element by element; four elements per thread asked for together — built as pab_stage_plane and compared back to back on
    // one box — was 1 % slower at 512 candidates and 7 % slower for a single candidate's product)
    for (int p = 0; p < np; ++p) {
      const int64_t pb = (int64_t)(base_z + p) * w.nslice;
      for (int v = threadIdx.x; v < w.nslice; v += PABS_THREADS) {
        const int64_t gi = pb + v;
        double xv = x[gi];
        if (MODE == 1) {
          xv = xv * s.inv_alpha;
          if (s.pend && p < own) {
            const double xn = pab_deferred_update(w, c, gi, s, xv);
            sqx += xn * xn;
          }
        }
        fac_lds[(size_t)p * w.nslice + v] = d ? xv * d[gi] : xv;
      }
    }
    const int d2 = w.d2;
    const int l = threadIdx.x & (PABF_KMAX - 1), colslot = threadIdx.x / PABF_KMAX;
    constexpr int COLS = PABS_THREADS / PABF_KMAX;   // columns per pass
    const int n_gl = w.fac_ngl[(size_t)c * w.fac_ng + grp];
    // the group's list table into LDS: a pass then waits for ONE trip to memory (the samples), not for three in a row
    // (table entry -> sample count -> samples: with 26 passes per workgroup that chain was four fifths of the kernel's time)
    PabfGroupList* const gls = reinterpret_cast<PabfGroupList*>(fac_lds + (size_t)(G + 1) * w.nslice);
    {
      const int* __restrict__ src_ = reinterpret_cast<const int*>(w.fac_gl + ((size_t)c * w.fac_ng + grp) * w.fac_max_gl);
      int* dst_ = reinterpret_cast<int*>(gls);
      for (int t = threadIdx.x; t < n_gl * (int)(sizeof(PabfGroupList) / 4); t += PABS_THREADS) dst_[t] = src_[t];
    }
    __syncthreads();
    const int ncol_all = n_gl * d2;
    const int per_part = ((ncol_all + w.fac_split - 1) / w.fac_split + COLS - 1) / COLS * COLS;
    const int col0 = part * per_part, ncol = min(ncol_all, col0 + per_part);
    for (int cb = col0; cb < ncol; cb += COLS) {
      const int col = cb + colslot;
      const bool live = col < ncol;
      const int gi_ = live ? col / d2 : 0, j = live ? col % d2 : 0;
      const PabfGroupList& gl = gls[gi_];
      const int nk = live ? gl.nk : 0;
      PabfRowRef rr{};
      if (l < nk) rr = gl.e[l];
      // lane l's row of the column, and (LSMR) its old value: asked for now, used after the column's sums
      int r = -1;
      double yold = 0, bold = 0;
      if (l < nk) {
        const unsigned long long jm = (j >> 6) ? rr.jmask[1] : rr.jmask[0];   // (no run-time index into the struct: scratch)
        if ((jm >> (j & 63)) & 1ull) {
          r = rr.rowbase + __popcll(jm & ((1ull << (j & 63)) - 1ull)) + ((j >> 6) ? __popcll(rr.jmask[0]) : 0);
          if (MODE == 1) yold = y[r];
          if (MODE == 2) bold = w.mvec(MV_B, c)[r];
        }
      }
      double S[G + 1];
#pragma unroll
      for (int p = 0; p <= G; ++p) S[p] = 0;
      if (live) {
        const size_t lj = ((size_t)c * w.fac_max_lists + gl.list) * d2 + j;
        const PabfEntry* __restrict__ en = w.fac_entries + lj * d2;
        // a lane's samples of the column, eight at a time, and the column's count beside them: every load of the pass is in
        // flight at once (a list has d2 slots per image row, so the loads need not wait for the count; slots past it are
        // not used)
        const int d2r = (d2 + PABF_KMAX - 1) / PABF_KMAX * PABF_KMAX;
        int n = 0;
        for (int t0 = l; t0 < d2r; t0 += 8 * PABF_KMAX) {
          PabfEntry e[8];
#pragma unroll
          for (int q = 0; q < 8; ++q)
            if (t0 + q * PABF_KMAX < d2) e[q] = en[t0 + q * PABF_KMAX];
          if (t0 == l) n = w.fac_count[lj];
          if (t0 >= n) break;
#pragma unroll
          for (int q = 0; q < 8; ++q)
            if (t0 + q * PABF_KMAX < n) {
              double wt[4];
              pabf_weights(e[q], wt);
              const int i0 = (int)(e[q].idx & 0xffffu), i1 = (int)(e[q].idx >> 16);
#pragma unroll
              for (int p = 0; p <= G; ++p)
                if (p < np) {
                  const double* __restrict__ xp = fac_lds + (size_t)p * w.nslice;
                  double a = wt[0] * xp[i0];
                  const double b1 = xp[i0 + 1], b2 = xp[i1], b3 = xp[i1 + 1];
                  a += wt[1] * b1;
                  a += wt[2] * b2;
                  a += wt[3] * b3;
                  S[p] += a;
                }
            }
        }
      }
      // the column's 8 lanes: butterfly, so that every lane holds the sums (same order on every lane)
#pragma unroll
      for (int p = 0; p <= G; ++p) {
#pragma unroll
        for (int off = 1; off < PABF_KMAX; off <<= 1) S[p] += __shfl_xor(S[p], off, PABF_KMAX);
      }
      if (r >= 0) {   // lane l: the column's row of (operation, image column) entry l
        {
          double lo_ = 0, hi_ = 0;
#pragma unroll
          for (int p = 0; p <= G; ++p) {   // (a register array indexed by a run-time plane would go to scratch)
            if (p == rr.hp) lo_ = S[p];
            if (p == rr.hp + 1) hi_ = S[p];
          }
          double val = rr.cz0 * lo_ + rr.cz1 * hi_;
          if (MODE == 1) val = (yold * s.inv_beta) * s.neg_alpha + val;
          if (MODE == 2) val = val - bold;
          y[r] = val;
          sq += val * val;
          mx = fmax(mx, fabs(val));
        }
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
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 3)[bx], s.pend ? 1.0 : 0.0);   // self-check, see scalar 1
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 4)[bx], (double)s.itn);
  }
  if (MODE == 2) {
    const double v = pabs_block_reduce(RED_MAX, mx, lds16);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 1)[bx], v);
  }
}

// ---- A^T y, scatter half (then k_pabl_finish) ------------------------------------------------------------------------------------------
// dynamic LDS: [G + 1][nslice] long long.  MODE / ABS as in k_pabl_scatter.
template <int MODE, bool ABS, int G, class P>
__global__ __launch_bounds__(PABS_THREADS) void k_pabf_scatter(PabView w, int src, P pred) {
#pragma clang fp contract(off)
  const int c = PAB_CAND, bx = PAB_BLOCK;
  if (c < 0) return;
  if (!pred(pab_ctl_load(w.ctl, c))) return;
  __shared__ PabState s_lds;
  pab_state_load(&s_lds, &w.st[c]);
  const PabState& s = s_lds;
  extern __shared__ double fac_lds[];
  long long* const acc = reinterpret_cast<long long*>(fac_lds);
  const int grp = bx / w.fac_split, part = bx % w.fac_split;
  const int base_z = grp * G;
  const int np = min(G + 1, w.mz - base_z);
  const int n_gl = w.fac_ngl[(size_t)c * w.fac_ng + grp];
  constexpr int COLS = PABS_THREADS / PABF_KMAX;
  const int ncol_all = n_gl * w.d2;
  const int per_part = ((ncol_all + w.fac_split - 1) / w.fac_split + COLS - 1) / COLS * COLS;
  const int col0 = part * per_part, ncol = min(ncol_all, col0 + per_part);
  if (col0 >= ncol) return;
  for (int v = threadIdx.x; v < np * w.nslice; v += PABS_THREADS) acc[v] = 0;
  __syncthreads();
  const double* __restrict__ y = ABS ? nullptr : w.mvec(src, c);
  const double sc = MODE == 1 ? s.inv_beta : 1.0;
  const double scale = ABS ? 1048576.0 : MODE == 1 ? s.fx_scale : s.fx_scale_r;
  const int d2 = w.d2;
  const int l = threadIdx.x & (PABF_KMAX - 1), colslot = threadIdx.x / PABF_KMAX;
  PabfGroupList* const gls = reinterpret_cast<PabfGroupList*>(fac_lds + (size_t)(G + 1) * w.nslice);
  {
    const int* __restrict__ src_ = reinterpret_cast<const int*>(w.fac_gl + ((size_t)c * w.fac_ng + grp) * w.fac_max_gl);
    int* dst_ = reinterpret_cast<int*>(gls);
    for (int t = threadIdx.x; t < n_gl * (int)(sizeof(PabfGroupList) / 4); t += PABS_THREADS) dst_[t] = src_[t];
  }
  __syncthreads();
  for (int cb = col0; cb < ncol; cb += COLS) {
    const int col = cb + colslot;
    const bool live = col < ncol;
    const int gi_ = live ? col / d2 : 0, j = live ? col % d2 : 0;
    const PabfGroupList& gl = gls[gi_];
    // lane l: its row's value times the two axial weights
    double a0 = 0, a1 = 0;
    int hp = -2;
    if (live && l < gl.nk) {
      const PabfRowRef rr = gl.e[l];
      const unsigned long long jm = (j >> 6) ? rr.jmask[1] : rr.jmask[0];
      if ((jm >> (j & 63)) & 1ull) {
        const unsigned long long below = jm & ((1ull << (j & 63)) - 1ull);
        const int r = rr.rowbase + __popcll(below) + ((j >> 6) ? __popcll(rr.jmask[0]) : 0);
        const double v = (ABS ? 1.0 : (MODE == 1 ? y[r] * sc : y[r])) * scale;
        a0 = (ABS ? fabs(rr.cz0) : rr.cz0) * v;
        a1 = (ABS ? fabs(rr.cz1) : rr.cz1) * v;
        hp = rr.hp;
      }
    }
    // T[p] = sum over the column's rows, in entry order, the same on every lane
    double T[G + 1];
#pragma unroll
    for (int p = 0; p <= G; ++p) T[p] = 0;
#pragma unroll
    for (int e = 0; e < PABF_KMAX; ++e) {
      const int hpe = __shfl(hp, e, PABF_KMAX);
      const double b0 = __shfl(a0, e, PABF_KMAX), b1 = __shfl(a1, e, PABF_KMAX);
#pragma unroll
      for (int p = 0; p <= G; ++p) {
        if (p == hpe) T[p] += b0;
        if (p == hpe + 1) T[p] += b1;
      }
    }
    if (live) {
      const size_t lj = ((size_t)c * w.fac_max_lists + gl.list) * d2 + j;
      const PabfEntry* __restrict__ en = w.fac_entries + lj * d2;
      const int d2r = (d2 + PABF_KMAX - 1) / PABF_KMAX * PABF_KMAX;
      int n = 0;
      for (int t0 = l; t0 < d2r; t0 += 8 * PABF_KMAX) {
        PabfEntry eb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (t0 + u * PABF_KMAX < d2) eb[u] = en[t0 + u * PABF_KMAX];
        if (t0 == l) n = w.fac_count[lj];
        if (t0 >= n) break;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (t0 + u * PABF_KMAX < n) {
            double wt[4];
            pabf_weights(eb[u], wt);
            const int i0 = (int)(eb[u].idx & 0xffffu), i1 = (int)(eb[u].idx >> 16);
            const int at[4] = {i0, i0 + 1, i1, i1 + 1};
#pragma unroll
            for (int p = 0; p <= G; ++p)
              if (p < np && T[p] != 0.0) {
                long long* __restrict__ ap = acc + (size_t)p * w.nslice;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const double wv = ABS ? fabs(wt[q]) : wt[q];
                  if (wv != 0.0) atomicAdd(reinterpret_cast<unsigned long long*>(ap + at[q]), (unsigned long long)__double2ll_rn(wv * T[p]));
                }
              }
          }
      }
    }
  }
  __syncthreads();
  // to the candidate's accumulator: the group's first and last plane also receive from the neighbouring groups
  unsigned long long* const Gm = reinterpret_cast<unsigned long long*>(w.acc64 + (size_t)c * w.N + (size_t)base_z * w.nslice);
  for (int v = threadIdx.x; v < np * w.nslice; v += PABS_THREADS) {
    const long long t = acc[v];
    if (t != 0) atomicAdd(Gm + v, (unsigned long long)t);
  }
}

// ---- A x, symmetry rows (16 entries each, gathered from L2) and the augmented rows root[v] x[v] ---------------------------------------
// 256 threads, PABF_TAIL_ROWS rows per thread; block b of this launch is partial-sum block fac_ng + b of the forward product.
constexpr int PABF_TAIL_ROWS = 4;   // (2 -> 4: 4.06 -> 3.98-4.02 s for 512 candidates, back to back; 1: no change)
template <int MODE, class P>
__global__ __launch_bounds__(256) void k_pabf_tail(PabView w, int src, int dsc, int rootv, int dst, P pred) {
#pragma clang fp contract(off)
  const int c = PAB_CAND, bx = PAB_BLOCK;
  if (c < 0) return;
  if (!pred(pab_ctl_load(w.ctl, c))) return;
  __shared__ PabState s_lds;
  pab_state_load(&s_lds, &w.st[c]);
  const PabState& s = s_lds;
  __shared__ double lds4[4];
  const bool op_aug = MODE != 1 || s.aug;
  const double* __restrict__ x = w.nvec(src, c);
  const double* __restrict__ d = dsc >= 0 && op_aug ? w.nvec(dsc, c) : nullptr;
  const double* __restrict__ root = rootv >= 0 && op_aug ? w.nvec(rootv, c) : nullptr;
  double* __restrict__ y = w.mvec(dst, c);
  double sq = 0, mx = 0;
#pragma unroll
  for (int u = 0; u < PABF_TAIL_ROWS; ++u) {
    const int64_t qi = s.m_data + (((int64_t)bx * PABF_TAIL_ROWS + u) * 256 + threadIdx.x);
    int64_t r = -1;
    double val = 0;
    if (qi < s.m_data + s.m_sym) {
      const PaEll16 e = w.sym16[s.sym0 + (qi - s.m_data)];
      double xv[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) xv[t] = x[e.idx[t]];          // sixteen independent gathers in flight
      double dv[16];
      if (d) {
#pragma unroll
        for (int t = 0; t < 16; ++t) dv[t] = d[e.idx[t]];
      }
      double acc = 0;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const double xa = MODE == 1 ? xv[t] * s.inv_alpha : xv[t];
        acc += (double)e.w[t] * (d ? xa * dv[t] : xa);
      }
      r = qi; val = acc;
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
  const int pb = w.fac_ng * w.fac_split + bx;
  if (MODE != 0) {
    const double v = pab_block_reduce(RED_SUM, sq, lds4);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 0)[pb], v);
  }
  if (MODE == 1 && threadIdx.x == 0) {
    pab_store_partial(&w.redp(c, 2)[pb], 0.0);
    pab_store_partial(&w.redp(c, 3)[pb], 0.0);
    pab_store_partial(&w.redp(c, 4)[pb], (double)s.itn);
  }
  if (MODE == 2) {
    const double v = pab_block_reduce(RED_MAX, mx, lds4);
    if (threadIdx.x == 0) pab_store_partial(&w.redp(c, 1)[pb], v);
  }
}
