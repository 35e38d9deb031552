// mfma_tile.inc — what the tile products on the exact-f32 MFMA (v_mfma_f32_32x32x2f32: f32 in, f32 accumulate, an fmaf
// chain) share: the accumulator type, a lane's place in a workgroup tile made of 32 x 32 wavefront sub-tiles, the
// accumulator's row mapping, the two staging loops of a K slice through LDS, the single-accumulator K-slice step and the
// float64 block reduction of an epilogue's sums.  Included inside helicon_hip.hip's unnamed namespace, ahead of
// k_segment_corr.  Users: k_segment_corr (read-out), k_circ_gemm and k_axis_gemm (axis_pass.inc), k_filter_xpass, k_zoom_sweep / k_phase_sweep,
// k_fc_xpass / k_tfsc_xpass (fc_pair_product), k_tfsc_c2r.
//
// The LDS layout every user keeps: A as as[rows][K + 1] ("rows along K"), B as bs[K][columns + 1]; the MFMA takes two k per
// step, lane (r, h) supplying A[row r][kk + h] and B[kk + h][column r].

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TILE_THREADS = 256;   // the workgroup of a Tile64; stage_rows / stage_cols stride by it (k_zoom_sweep's 512 threads stage their own)

// A lane of a TILE_THREADS workgroup that owns a 64 x 64 tile as 2 x 2 wavefront sub-tiles: sub-tile origin (wm, wp),
// r = lane & 31 (the operand row / column this lane supplies, and its accumulator COLUMN), h = lane >> 5 (which of the
// step's two k, and the accumulator's row offset 4 h).
struct Tile64 {
  int tid, lane, wave, r, h, wm, wp;
};
__device__ __forceinline__ Tile64 tile64() {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  return {tid, lane, wave, lane & 31, lane >> 5, (wave >> 1) * 32, (wave & 1) * 32};
}

// C/D layout of the 32 x 32 MFMA: register i of lane (r, h) holds column r of this row.
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// Stage as[mm][kk] = src[row0 + mm][k0 + kk] (row stride ld; zero outside rows x kn): lanes along k, contiguous in memory.
template <int T, int KP>   // KP = K + 1, the padded row
__device__ __forceinline__ void stage_rows(float (&as)[T][KP], const float* __restrict__ src, int64_t ld, int row0, int rows, int k0,
                                           int kn, int tid) {
  constexpr int K = KP - 1;
  for (int e = tid; e < T * K; e += TILE_THREADS) {
    const int mm = e / K, kk = e % K, row = row0 + mm, k = k0 + kk;
    as[mm][kk] = (row < rows && k < kn) ? src[(int64_t)row * ld + k] : 0.f;
  }
}

// Stage bs[q][kk][cc] = src[q][k0 + kk][col0 + cc] for NQ tables of one shape (row stride ld; zero outside kn x cols): lanes
// along the column, contiguous; the tables share the index and the loop, so their loads are in flight together.
template <int NQ, int K, int TP>   // TP = T + 1
__device__ __forceinline__ void stage_cols(float (&bs)[NQ][K][TP], const float* const (&src)[NQ], int64_t ld, int k0, int kn, int col0,
                                           int cols, int tid) {
  constexpr int T = TP - 1;
  for (int e = tid; e < K * T; e += TILE_THREADS) {
    const int kk = e / T, cc = e % T, k = k0 + kk, col = col0 + cc;
    const bool in = k < kn && col < cols;
#pragma unroll
    for (int q = 0; q < NQ; ++q) bs[q][kk][cc] = in ? src[q][(int64_t)k * ld + col] : 0.f;
  }
}

// One staged K slice into one accumulator.  TR swaps the operands: the accumulator's column then runs along A's rows.
template <bool TR, int T, int KP, int K, int TP>
__device__ __forceinline__ void tile_mac(f32x16& acc, const float (&as)[T][KP], const float (&bs)[K][TP], const Tile64& t) {
  static_assert(T == 64 && TP == T + 1 && KP == K + 1 && K % 2 == 0, "a padded 64 x K slice of each operand");
#pragma unroll
  for (int kk = 0; kk < K; kk += 2) {
    const float av = as[t.wm + t.r][kk + t.h], bv = bs[kk + t.h][t.wp + t.r];
    acc = TR ? __builtin_amdgcn_mfma_f32_32x32x2f32(bv, av, acc, 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
  }
}

// NSUM sums of a workgroup of WAVES wavefronts, in float64 and in a fixed order: a __shfl_down tree inside the wavefront,
// then red[0] + red[1] + ... over the wavefronts, left to right; thread e < NSUM writes out[e].  (Starting that sum from 0
// gives the same bits unless every term is -0, and x + y is -0 in round-to-nearest only when both are: every lane's fmaf
// chain, each started from +0, would have to underflow to -0.)  Ends with a barrier: red may be reused at once.
template <int NSUM, int WAVES>
__device__ __forceinline__ void block_sums(double (&sum)[NSUM], double (&red)[WAVES][NSUM], int tid, double* __restrict__ out) {
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int e = 0; e < NSUM; ++e) sum[e] += __shfl_down(sum[e], o, 64);
  if ((tid & 63) == 0)
#pragma unroll
    for (int e = 0; e < NSUM; ++e) red[tid >> 6][e] = sum[e];
  __syncthreads();
  if (tid < NSUM) {
    double tot = red[0][tid];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) tot += red[w][tid];
    out[tid] = tot;
  }
  __syncthreads();
}
