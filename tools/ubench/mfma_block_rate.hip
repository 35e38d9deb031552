// mfma_block_rate.hip — what does v_mfma_f32_4x4x1_16b_f32 cost a SIMD of gfx950 whose vector pipe is busy?  (A
// measurement tool, not part of the library.)
//   hipcc --offload-arch=gfx950 -O3 -o mfma_block_rate mfma_block_rate.hip && timeout 120 ./mfma_block_rate
// For 1, 2 and 4 wavefronts per SIMD (one workgroup of 256, 512, 1024 threads per CU; 96 KiB of LDS per workgroup keep a
// second one off the CU) it times, by the wall clock with every CU busy:
//   fma        16 independent v_fma_f32 chains                                    -> f, ns per FMA and SIMD
//   mfma       the MFMA alone on 8 independent accumulators
//   mix        8 x (1 MFMA + 13 v_fma_f32): the pair walk's mix with its build on the matrix pipe
//   mix8       8 MFMAs, then 104 v_fma_f32: the same mix, the MFMAs in one cluster as a table row issues them
//   swap       v_permlane32_swap_b32 / v_permlane16_swap_b32 alternating, 8 independent register pairs -> s
//   swapmix    8 x (1 swap + 13 v_fma_f32)
// x = (time of mix per round - 104 f) / 8 is what one MFMA adds to a vector stream, s likewise from swapmix.
// Before the timing it checks the operand and result layout of the MFMA against a host loop (A from lane 4 b + i, B from
// lane 4 b + j, D_b[i][j] in register i of lane 4 b + j, sixteen blocks b, K = 1) on a three-step accumulation from a zero C,
// bit for bit against fmaf, and exits with status 1 if it differs.  Denormal products are reported, not judged.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define ITER 8192
#define REP8(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define FMA(r) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(v[r]) : "v"(b), "v"(c));
#define MFMA(r) asm volatile("v_mfma_f32_4x4x1_16b_f32 %0, %1, %2, %0" : "+v"(acc[r]) : "v"(b), "v"(c));
#define SWAP32(r) asm volatile("v_permlane32_swap_b32 %0, %1" : "+v"(v[2 * (r)]), "+v"(v[2 * (r) + 1]));
#define SWAP16(r) asm volatile("v_permlane16_swap_b32 %0, %1" : "+v"(v[2 * (r)]), "+v"(v[2 * (r) + 1]));
// 13 FMAs on chains s .. s + 12 (mod 16): a chain is touched again 16 instructions later at the earliest
#define FMA13(s) FMA((s) & 15) FMA((s + 1) & 15) FMA((s + 2) & 15) FMA((s + 3) & 15) FMA((s + 4) & 15) FMA((s + 5) & 15) \
  FMA((s + 6) & 15) FMA((s + 7) & 15) FMA((s + 8) & 15) FMA((s + 9) & 15) FMA((s + 10) & 15) FMA((s + 11) & 15) FMA((s + 12) & 15)

enum { K_FMA, K_MFMA, K_MIX, K_MIX8, K_SWAP, K_SWAPMIX };

template <int KIND>
__global__ __launch_bounds__(1024) void k_rate(float* out) {
  __shared__ float pad[24576];   // 96 KiB: one workgroup per CU
  float v[16];
  f32x4 acc[8];
  const float b = 1.0001f + threadIdx.x * 1e-7f, c = 1e-6f;
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = (float)i + threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = (f32x4){(float)i, 1.f, 2.f, 3.f};
#pragma unroll 1
  for (int it = 0; it < ITER; ++it) {
    if constexpr (KIND == K_FMA) {
#define X(i) FMA(i) FMA(i + 8)
      REP8(X) REP8(X) REP8(X) REP8(X) REP8(X) REP8(X) REP8(X)   // 112
#undef X
    } else if constexpr (KIND == K_MFMA) {
      REP8(MFMA) REP8(MFMA)
    } else if constexpr (KIND == K_MIX) {
#define X(i) MFMA(i) FMA13(13 * i)
      REP8(X)
#undef X
    } else if constexpr (KIND == K_MIX8) {
      REP8(MFMA)
#define X(i) FMA13(13 * i)
      REP8(X)
#undef X
    } else if constexpr (KIND == K_SWAP) {
#define X(i) SWAP32(i)
      REP8(X)
#undef X
#define X(i) SWAP16(i)
      REP8(X)
#undef X
    } else {
      // (the swap takes two of the three chains its group's FMAs leave out: written 13 and 15 instructions earlier)
#define X(i) FMA13(13 * i + 1) asm volatile("v_permlane32_swap_b32 %0, %1" : "+v"(v[(13 * i) & 15]), "+v"(v[(13 * i + 15) & 15]));
      REP8(X)
#undef X
    }
  }
  asm volatile("s_nop 15\n\ts_nop 15");   // the last MFMA's result, before ordinary code reads it
  float s = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += v[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) s += acc[i].x + acc[i].y + acc[i].z + acc[i].w;
  pad[threadIdx.x] = s;
  __syncthreads();
  out[blockIdx.x * blockDim.x + threadIdx.x] = pad[threadIdx.x ^ 1];
}

// three K = 1 steps from a zero C; a[k], bb[k]: 64 floats each, d: [4][64]
__global__ void k_layout(const float* a, const float* bb, float* d) {
  const int l = threadIdx.x;
  f32x4 acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a[l], bb[l], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a[64 + l], bb[64 + l], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a[128 + l], bb[128 + l], acc, 0, 0, 0);
  for (int r = 0; r < 4; ++r) d[r * 64 + l] = acc[r];
}

static bool ok(hipError_t e, const char* what) {
  if (e != hipSuccess) std::printf("%s: %s\n", what, hipGetErrorString(e));
  return e == hipSuccess;
}

// fills a, bb (3 x 64); returns the count of result words that differ from the host's fmaf chain
static int layout_case(bool denormal, float* da, float* db, float* dd) {
  std::vector<float> a(192), bb(192), d(256);
  unsigned s = denormal ? 77u : 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xFFFF) / 65536.f * 2.f - 1.f; };
  for (int i = 0; i < 192; ++i) {
    a[i] = rnd() * (denormal ? 1e-25f : 3.f);
    bb[i] = rnd() * (denormal ? 1e-15f : 1.f);
  }
  if (!denormal) a[5] = -0.f, bb[70] = 0.f;   // signed zero products
  if (!ok(hipMemcpy(da, a.data(), 192 * 4, hipMemcpyHostToDevice), "copy") ||
      !ok(hipMemcpy(db, bb.data(), 192 * 4, hipMemcpyHostToDevice), "copy"))
    return -1;
  k_layout<<<1, 64>>>(da, db, dd);
  if (!ok(hipDeviceSynchronize(), "layout kernel") || !ok(hipMemcpy(d.data(), dd, 256 * 4, hipMemcpyDeviceToHost), "copy")) return -1;
  int bad = 0;
  for (int blk = 0; blk < 16; ++blk)
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        float want = 0.f;
        for (int k = 0; k < 3; ++k) want = std::fmaf(a[64 * k + 4 * blk + i], bb[64 * k + 4 * blk + j], want);
        const float got = d[i * 64 + 4 * blk + j];
        if (std::memcmp(&want, &got, 4) != 0) {
          if (bad < 4) std::printf("  block %d i %d j %d: host %a device %a\n", blk, i, j, want, got);
          ++bad;
        }
      }
  return bad;
}

template <int KIND>
static double run(const char* name, int per_round, int wps, int cus, float* out) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  for (int w = 0; w < 2; ++w) hipLaunchKernelGGL(k_rate<KIND>, dim3(cus), dim3(256 * wps), 0, 0, out);
  (void)hipEventRecord(e0);
  for (int w = 0; w < 4; ++w) hipLaunchKernelGGL(k_rate<KIND>, dim3(cus), dim3(256 * wps), 0, 0, out);
  (void)hipEventRecord(e1);
  if (!ok(hipDeviceSynchronize(), name)) return -1;
  float ms;
  (void)hipEventElapsedTime(&ms, e0, e1);
  ms /= 4;
  const double round_ns = ms * 1e6 / ((double)wps * ITER);   // SIMD time per round of one wavefront
  std::printf("%-8s waves/SIMD %d: %.3f ms, %8.2f ns per round and SIMD, %.3f ns per instruction and SIMD\n", name, wps, ms, round_ns,
              round_ns / per_round);
  return round_ns;
}

int main() {
  hipDeviceProp_t p;
  if (!ok(hipGetDeviceProperties(&p, 0), "device")) return 2;
  const int cus = p.multiProcessorCount;
  std::printf("%s, %d CUs\n", p.gcnArchName, cus);
  float *out, *da, *db, *dd;
  if (!ok(hipMalloc(&out, (size_t)cus * 1024 * sizeof(float)), "alloc") || !ok(hipMalloc(&da, 192 * 4), "alloc") ||
      !ok(hipMalloc(&db, 192 * 4), "alloc") || !ok(hipMalloc(&dd, 256 * 4), "alloc"))
    return 2;
  const int bad = layout_case(false, da, db, dd);
  if (bad < 0) return 2;
  std::printf("layout and fmaf chain, normal operands: %d of 256 words differ\n", bad);
  const int badd = layout_case(true, da, db, dd);
  if (badd < 0) return 2;
  std::printf("denormal products and sums: %d of 256 words differ from fmaf with denormals kept\n", badd);
  if (bad) return 1;
  for (int wps : {1, 2, 4}) {
    const double f = run<K_FMA>("fma", 112, wps, cus, out) / 112;
    const double m = run<K_MFMA>("mfma", 16, wps, cus, out) / 16;
    const double mix = run<K_MIX>("mix", 112, wps, cus, out);
    const double mix8 = run<K_MIX8>("mix8", 112, wps, cus, out);
    const double sw = run<K_SWAP>("swap", 16, wps, cus, out) / 16;
    const double swm = run<K_SWAPMIX>("swapmix", 112, wps, cus, out);
    if (f < 0 || m < 0 || mix < 0 || mix8 < 0 || sw < 0 || swm < 0) return 2;
    std::printf("waves/SIMD %d: f %.3f ns, MFMA alone %.3f ns (%.2f f), x %.3f ns (%.2f f) spread / %.3f ns (%.2f f) clustered, "
                "s %.3f ns (%.2f f) alone / %.3f ns (%.2f f) among FMAs\n",
                wps, f, m, m / f, (mix - 104 * f) / 8, (mix - 104 * f) / 8 / f, (mix8 - 104 * f) / 8, (mix8 - 104 * f) / 8 / f, sw, sw / f,
                (swm - 104 * f) / 8, (swm - 104 * f) / 8 / f);
  }
  return 0;
}
