// wave_sum_rate.hip — what do the packed pair walk's epilogue instructions that are not arithmetic on the spectrum cost a SIMD
// of gfx950, alone and inside a busy vector stream?  (A measurement tool, not part of the library.)
//   hipcc --offload-arch=gfx950 -O3 -o wave_sum_rate wave_sum_rate.hip && timeout 120 ./wave_sum_rate
// In the manner of mfma_block_rate.hip: one workgroup of 1024 threads per CU (4 wavefronts per SIMD; 96 KiB of LDS keep a
// second one off the CU), every CU busy, wall clock, ns per wave-instruction and SIMD.  Each subject is timed ALONE and as
// `mix`: once (the blocks) or eight times (the single instructions) among 104 v_fma_f32 of 16 independent chains; what it
// adds to the stream is (mix round - 104 f) / count, f the time of one FMA in the bare stream.
//   sqrt, log   v_sqrt_f32, v_log_f32 (the epilogue has 16 of each per pair)
//   cvt         v_cvt_f64_f32
//   dpp3        group_sum3's 18-instruction block as the kernel has it: 12 v_add_f32_dpp inside the 16-lane rows, s_nop 1,
//               3 row_bcast:15 and 3 row_bcast:31 adds; three sums to lane 63
//   lds6        six sums at once through the wavefront's 4 KB of LDS: 3 ds_write2st64_b32 ([s][lane]), 2 ds_read_b128 (lane L
//               reads floats 8 L .. 8 L + 7, lanes 16-31 and 48-63 the upper half first), 7 adds, 3 DPP adds in the group
//               of eight; sum s to lane 8 s.  In the mix the writes, the reads and the adds stand a third of the FMAs apart.
//   lds6same    the same with every lane reading its lower half first: one address, two lanes of a 16-lane group on every
//               bank slot they touch
// Before the timing lds6's totals are held bit for bit to a host sum in the same association,
//   p_c = ((x[8c] + x[8c+1]) + x[8c+2]) + x[8c+3]  +  ((x[8c+4] + x[8c+5]) + x[8c+6]) + x[8c+7],
//   total = ((p0 + p1) + (p2 + p3)) + ((p7 + p6) + (p5 + p4)),
// and the program exits with status 1 if they differ (lds6same must give the same bits: the two halves' sums commute).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#define ITER 8192
#define REP8(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define FMA(r) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(v[r]) : "v"(b), "v"(c));
#define FMA13(s) FMA((s) & 15) FMA((s + 1) & 15) FMA((s + 2) & 15) FMA((s + 3) & 15) FMA((s + 4) & 15) FMA((s + 5) & 15) \
  FMA((s + 6) & 15) FMA((s + 7) & 15) FMA((s + 8) & 15) FMA((s + 9) & 15) FMA((s + 10) & 15) FMA((s + 11) & 15) FMA((s + 12) & 15)
#define FMA104 FMA13(0) FMA13(13) FMA13(26) FMA13(39) FMA13(52) FMA13(65) FMA13(78) FMA13(91)
#define SQRT(r) asm volatile("v_sqrt_f32 %0, %1" : "=v"(u[r]) : "v"(v[r]));
#define LOG(r) asm volatile("v_log_f32 %0, %1" : "=v"(u[r]) : "v"(v[r]));
#define CVT(r) asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[r]) : "v"(v[r]));

// group_sum3 of helicon_hip.hip, instruction for instruction
__device__ __forceinline__ void dpp3(float& a, float& b, float& c) {
  asm volatile(
      "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %1, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %1, %1, %1 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "v_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
      "v_add_f32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 row_bcast:31 row_mask:0xc bank_mask:0xf"
      : "+v"(a), "+v"(b), "+v"(c));
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
// The three steps of lds6.  wa: byte address of the lane's float in row 0 of the wavefront's buffer; r0, r1: byte addresses
// of its first and second 16-byte read.
__device__ __forceinline__ void lds6_write(unsigned wa, float s0, float s1, float s2, float s3, float s4, float s5) {
  asm volatile(
      "ds_write2st64_b32 %0, %1, %2 offset1:1\n\t"
      "ds_write2st64_b32 %0, %3, %4 offset0:2 offset1:3\n\t"
      "ds_write2st64_b32 %0, %5, %6 offset0:4 offset1:5"
      :: "v"(wa), "v"(s0), "v"(s1), "v"(s2), "v"(s3), "v"(s4), "v"(s5) : "memory");
}
__device__ __forceinline__ void lds6_read(unsigned r0, unsigned r1, f32x4& e0, f32x4& e1) {
  asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3" : "=&v"(e0), "=&v"(e1) : "v"(r0), "v"(r1) : "memory");
}
__device__ __forceinline__ float lds6_sum(const f32x4& e0, const f32x4& e1) {
  float tot, hi;
  asm volatile(
      "s_waitcnt lgkmcnt(0)\n\t"
      "v_add_f32 %0, %2, %3\n\t"
      "v_add_f32 %1, %6, %7\n\t"
      "v_add_f32 %0, %0, %4\n\t"
      "v_add_f32 %1, %1, %8\n\t"
      "v_add_f32 %0, %0, %5\n\t"
      "v_add_f32 %1, %1, %9\n\t"
      "v_add_f32 %0, %0, %1\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf"
      : "=&v"(tot), "=&v"(hi) : "v"(e0.x), "v"(e0.y), "v"(e0.z), "v"(e0.w), "v"(e1.x), "v"(e1.y), "v"(e1.z), "v"(e1.w));
  return tot;
}

typedef __attribute__((address_space(3))) void* lptr_t;
__device__ __forceinline__ unsigned lds_offset_of(const void* p) { return (unsigned)(size_t)(lptr_t)(const_cast<void*>(p)); }

enum { K_FMA, K_SQRT, K_SQRTMIX, K_LOG, K_LOGMIX, K_CVT, K_CVTMIX, K_DPP, K_DPPMIX, K_LDS, K_LDSMIX, K_LDSSAME, K_LDSSAMEMIX };

template <int KIND>
__global__ __launch_bounds__(1024) void k_rate(float* out) {
  __shared__ __attribute__((aligned(16))) float pad[24576];   // 96 KiB: one workgroup per CU; a wavefront's 4 KB at 1024 x wave
  float v[16], u[8];
  double d[8];
  const float b = 1.0001f + threadIdx.x * 1e-7f, c = 1e-6f;
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = (float)i + threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; ++i) u[i] = 0.f, d[i] = 0.;
  const unsigned lane = threadIdx.x & 63, wbase = lds_offset_of(pad + (threadIdx.x >> 6) * 1024);
  const unsigned wa = wbase + 4 * lane;
  const unsigned fh = (KIND == K_LDSSAME || KIND == K_LDSSAMEMIX) ? 0 : (lane >> 4) & 1;
  const unsigned r0 = wbase + 32 * lane + 16 * fh, r1 = wbase + 32 * lane + 16 * (fh ^ 1);
  float sink = 0.f;
#pragma unroll 1
  for (int it = 0; it < ITER; ++it) {
    if constexpr (KIND == K_FMA) {
#define X(i) FMA(i) FMA(i + 8)
      REP8(X) REP8(X) REP8(X) REP8(X) REP8(X) REP8(X) REP8(X)   // 112
#undef X
    } else if constexpr (KIND == K_SQRT) {
      REP8(SQRT) REP8(SQRT)
    } else if constexpr (KIND == K_LOG) {
      REP8(LOG) REP8(LOG)
    } else if constexpr (KIND == K_CVT) {
      REP8(CVT) REP8(CVT)
    } else if constexpr (KIND == K_SQRTMIX) {
#define X(i) SQRT(i) FMA13(13 * i)
      REP8(X)
#undef X
    } else if constexpr (KIND == K_LOGMIX) {
#define X(i) LOG(i) FMA13(13 * i)
      REP8(X)
#undef X
    } else if constexpr (KIND == K_CVTMIX) {
#define X(i) CVT(i) FMA13(13 * i)
      REP8(X)
#undef X
    } else if constexpr (KIND == K_DPP) {
      dpp3(v[0], v[1], v[2]);
    } else if constexpr (KIND == K_DPPMIX) {
      dpp3(v[13], v[14], v[15]);   // (chains the last FMAs of the round before left 3 to 1 instructions ago; the kernel's sums are as fresh)
      FMA104
    } else if constexpr (KIND == K_LDS || KIND == K_LDSSAME) {
      f32x4 e0, e1;
      lds6_write(wa, v[0], v[1], v[2], v[3], v[4], v[5]);
      lds6_read(r0, r1, e0, e1);
      sink += lds6_sum(e0, e1);
    } else {
      f32x4 e0, e1;
      lds6_write(wa, v[0], v[1], v[2], v[3], v[4], v[5]);
      FMA13(0) FMA13(13) FMA13(26)
      lds6_read(r0, r1, e0, e1);
      FMA13(39) FMA13(52) FMA13(65)
      sink += lds6_sum(e0, e1);
      FMA13(78) FMA13(91)
    }
  }
  float s = sink;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += v[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) s += u[i] + (float)d[i];
  __syncthreads();
  pad[threadIdx.x] = s;
  __syncthreads();
  out[blockIdx.x * blockDim.x + threadIdx.x] = pad[threadIdx.x ^ 1];
}

// one wavefront: x[6][64] -> tot[64] (lane 8 s holds sum s)
template <bool SAME>
__global__ void k_check(const float* x, float* tot) {
  __shared__ __attribute__((aligned(16))) float buf[1024];
  const unsigned lane = threadIdx.x, wbase = lds_offset_of(buf);
  buf[384 + lane] = 0.f;   // (what lanes 48-63 read)
  buf[448 + lane] = 0.f;
  __syncthreads();
  const unsigned fh = SAME ? 0 : (lane >> 4) & 1;
  f32x4 e0, e1;
  lds6_write(wbase + 4 * lane, x[lane], x[64 + lane], x[128 + lane], x[192 + lane], x[256 + lane], x[320 + lane]);
  lds6_read(wbase + 32 * lane + 16 * fh, wbase + 32 * lane + 16 * (fh ^ 1), e0, e1);
  tot[lane] = lds6_sum(e0, e1);
}

static bool ok(hipError_t e, const char* what) {
  if (e != hipSuccess) std::printf("%s: %s\n", what, hipGetErrorString(e));
  return e == hipSuccess;
}

// returns the count of the six totals (of either form) that differ from the host's
static int check_sums() {
  std::vector<float> x(384), got(64);
  unsigned s = 2024u;
  for (auto& e : x) {
    s = s * 1664525u + 1013904223u;
    e = std::ldexp((float)((s >> 8) & 0xFFFF) / 65536.f * 2.f - 1.f, (int)(s >> 28) - 8);   // mixed magnitudes: the order shows
  }
  float *dx, *dt;
  if (!ok(hipMalloc(&dx, 384 * 4), "alloc") || !ok(hipMalloc(&dt, 64 * 4), "alloc") ||
      !ok(hipMemcpy(dx, x.data(), 384 * 4, hipMemcpyHostToDevice), "copy"))
    return -1;
  int bad = 0;
  for (int same = 0; same < 2; ++same) {
    if (same) k_check<true><<<1, 64>>>(dx, dt);
    else k_check<false><<<1, 64>>>(dx, dt);
    if (!ok(hipDeviceSynchronize(), "check kernel") || !ok(hipMemcpy(got.data(), dt, 64 * 4, hipMemcpyDeviceToHost), "copy")) return -1;
    for (int sum = 0; sum < 6; ++sum) {
      float p[8];
      for (int c = 0; c < 8; ++c) {
        const float* e = &x[64 * sum + 8 * c];
        volatile float lo = ((e[0] + e[1]) + e[2]) + e[3], hi = ((e[4] + e[5]) + e[6]) + e[7];
        p[c] = lo + hi;
      }
      volatile float l = (p[0] + p[1]) + (p[2] + p[3]), r = (p[7] + p[6]) + (p[5] + p[4]);
      const float want = l + r;
      if (std::memcmp(&want, &got[8 * sum], 4) != 0) {
        std::printf("  sum %d (%s): host %a device %a\n", sum, same ? "lds6same" : "lds6", want, got[8 * sum]);
        ++bad;
      }
    }
  }
  (void)hipFree(dx);
  (void)hipFree(dt);
  return bad;
}

template <int KIND>
static double run(const char* name, int per_round, int cus, float* out) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  for (int w = 0; w < 2; ++w) hipLaunchKernelGGL(k_rate<KIND>, dim3(cus), dim3(1024), 0, 0, out);
  (void)hipEventRecord(e0);
  for (int w = 0; w < 4; ++w) hipLaunchKernelGGL(k_rate<KIND>, dim3(cus), dim3(1024), 0, 0, out);
  (void)hipEventRecord(e1);
  if (!ok(hipDeviceSynchronize(), name)) return -1;
  float ms;
  (void)hipEventElapsedTime(&ms, e0, e1);
  ms /= 4;
  const double round_ns = ms * 1e6 / (4.0 * ITER);   // SIMD time per round of one wavefront
  std::printf("%-12s %.3f ms, %8.2f ns per round and SIMD, %.3f ns per instruction and SIMD\n", name, ms, round_ns, round_ns / per_round);
  return round_ns;
}

int main() {
  hipDeviceProp_t p;
  if (!ok(hipGetDeviceProperties(&p, 0), "device")) return 2;
  const int cus = p.multiProcessorCount;
  std::printf("%s, %d CUs, 4 wavefronts per SIMD\n", p.gcnArchName, cus);
  const int bad = check_sums();
  if (bad < 0) return 2;
  std::printf("lds6 and lds6same against the host sum in the same association: %d of 12 totals differ\n", bad);
  if (bad) return 1;
  float* out;
  if (!ok(hipMalloc(&out, (size_t)cus * 1024 * sizeof(float)), "alloc")) return 2;
  const double f = run<K_FMA>("fma", 112, cus, out) / 112;
  const double sq = run<K_SQRT>("sqrt", 16, cus, out) / 16, sqm = run<K_SQRTMIX>("sqrtmix", 112, cus, out);
  const double lg = run<K_LOG>("log", 16, cus, out) / 16, lgm = run<K_LOGMIX>("logmix", 112, cus, out);
  const double cv = run<K_CVT>("cvt", 16, cus, out) / 16, cvm = run<K_CVTMIX>("cvtmix", 112, cus, out);
  const double dp = run<K_DPP>("dpp3", 18, cus, out), dpm = run<K_DPPMIX>("dpp3mix", 122, cus, out);
  const double ld = run<K_LDS>("lds6", 15, cus, out), ldm = run<K_LDSMIX>("lds6mix", 119, cus, out);
  const double ls = run<K_LDSSAME>("lds6same", 15, cus, out), lsm = run<K_LDSSAMEMIX>("lds6samemix", 119, cus, out);
  if (f < 0 || sq < 0 || sqm < 0 || lg < 0 || lgm < 0 || cv < 0 || cvm < 0 || dp < 0 || dpm < 0 || ld < 0 || ldm < 0 || ls < 0 || lsm < 0) return 2;
  std::printf("f = %.3f ns per FMA and SIMD\n", f);
  std::printf("v_sqrt_f32     alone %.3f ns (%.2f f), among FMAs %.3f ns (%.2f f)\n", sq, sq / f, (sqm - 104 * f) / 8, (sqm - 104 * f) / 8 / f);
  std::printf("v_log_f32      alone %.3f ns (%.2f f), among FMAs %.3f ns (%.2f f)\n", lg, lg / f, (lgm - 104 * f) / 8, (lgm - 104 * f) / 8 / f);
  std::printf("v_cvt_f64_f32  alone %.3f ns (%.2f f), among FMAs %.3f ns (%.2f f)\n", cv, cv / f, (cvm - 104 * f) / 8, (cvm - 104 * f) / 8 / f);
  std::printf("dpp3 block     alone %.2f ns (%.1f f), among FMAs %.2f ns (%.1f f)\n", dp, dp / f, dpm - 104 * f, (dpm - 104 * f) / f);
  std::printf("lds6 block     alone %.2f ns (%.1f f), among FMAs %.2f ns (%.1f f)\n", ld, ld / f, ldm - 104 * f, (ldm - 104 * f) / f);
  std::printf("lds6same block alone %.2f ns (%.1f f), among FMAs %.2f ns (%.1f f)\n", ls, ls / f, lsm - 104 * f, (lsm - 104 * f) / f);
  std::printf("per pair: 2 dpp3 + 5 cvt - lds6 = %.2f ns among FMAs\n", 2 * (dpm - 104 * f) + 5 * (cvm - 104 * f) / 8 - (ldm - 104 * f));
  return 0;
}
