/*
 * lora_kernels.hip -- LoRA adapters merged into the weights: ONE launch over a descriptor table of every
 * touched tensor of a model.
 *
 *   k_lora_merge   for a weight viewed as a dense row-major [N, K] matrix in its physical memory order,
 *
 *                      W[n, k] = rn_dtype( f32(base[n, k]) + s ),   s = sum_j c_j * ( sum_q up_j[n, q] * down_j[q, k] )
 *
 *                  both sums fp32 fmaf chains from +0 in a fixed order (q ascending inside an adapter, adapters in table order),
 *                  one fp32 add to the pristine base, one rounding to the weight's type.  A tensor without adapters is a plain
 *                  copy of its base (bits, not arithmetic: -0 and NaN payloads survive).
 *
 *                  A workgroup owns one TM x TN tile of one tensor; it finds (tensor, tile row, tile column) by a binary search
 *                  of its block index in the table's prefix sum of tile counts.  The contraction is short (r = 1 .. ~128) and
 *                  the output large, so the kernel is an SGEMM-shaped VALU tile loop: up[tile rows, q chunk] and down[q chunk, tile
 *                  columns] are staged through LDS QC values of q at a time (zero-filled outside the matrix), every thread keeps
 *                  a 4 x 8 micro-tile of the inner sum and of s in registers.  The f32-input MFMA has the same numerics (an fmaf
 *                  chain) and the same peak rate as the f32 VALU on gfx950; the VALU form takes any r without a k-step tail and
 *                  was chosen for that.  Base reads and destination writes run along K: 4 consecutive
 *                  elements per access when the tensor's rows allow it (K % 4 == 0 and both pointers aligned to 4 elements), one
 *                  element per access otherwise -- the same bits either way.
 */
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "elastic_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int TM = 64;            // tile rows (N); 16 thread rows of 4
constexpr int TN = 128;           // tile columns (K); two groups of 16 threads x 4 consecutive columns
constexpr int QC = 16;            // q values staged per LDS round
constexpr int UP_PITCH = TM + 4;  // floats per q row of the staged up tile: keeps the float4 reads aligned, spreads the transposing writes
constexpr int MAX_RANK = 1 << 16;

// table words (int64), see elastic_hip.h
constexpr int T_WORDS = ED_LORA_TENSOR_WORDS, A_WORDS = ED_LORA_ADAPTER_WORDS;
enum { T_BASE = 0, T_DST, T_N, T_K, T_DTYPE, T_A0, T_A1, T_TILE0 };
enum { A_UP = 0, A_DOWN, A_R, A_C };

__device__ __forceinline__ uint32_t bf16_bits(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even, like torch
  return u >> 16;
}

__device__ __forceinline__ float ld1(const void* p, int64_t i, int dtype) {
  if (dtype == ED_F32) return ((const float*)p)[i];
  if (dtype == ED_F16) return __half2float(((const __half*)p)[i]);
  return __uint_as_float(((uint32_t)((const uint16_t*)p)[i]) << 16);
}

__device__ __forceinline__ void st1(void* p, int64_t i, float v, int dtype) {
  if (dtype == ED_F32) ((float*)p)[i] = v;
  else if (dtype == ED_F16) ((__half*)p)[i] = __float2half_rn(v);
  else ((uint16_t*)p)[i] = (uint16_t)bf16_bits(v);
}

__device__ __forceinline__ float4 ld4(const void* p, int64_t i, int dtype) {
  if (dtype == ED_F32) return *reinterpret_cast<const float4*>((const float*)p + i);
  const uint2 pk = *reinterpret_cast<const uint2*>((const uint16_t*)p + i);
  if (dtype == ED_F16)
    return make_float4(__half2float(__ushort_as_half((uint16_t)(pk.x & 0xffffu))), __half2float(__ushort_as_half((uint16_t)(pk.x >> 16))),
                       __half2float(__ushort_as_half((uint16_t)(pk.y & 0xffffu))), __half2float(__ushort_as_half((uint16_t)(pk.y >> 16))));
  return make_float4(__uint_as_float(pk.x << 16), __uint_as_float(pk.x & 0xffff0000u), __uint_as_float(pk.y << 16),
                     __uint_as_float(pk.y & 0xffff0000u));
}

__device__ __forceinline__ void st4(void* p, int64_t i, float4 v, int dtype) {
  if (dtype == ED_F32) {
    *reinterpret_cast<float4*>((float*)p + i) = v;
    return;
  }
  uint2 pk;
  if (dtype == ED_F16) {
    pk.x = (uint32_t)__half_as_ushort(__float2half_rn(v.x)) | ((uint32_t)__half_as_ushort(__float2half_rn(v.y)) << 16);
    pk.y = (uint32_t)__half_as_ushort(__float2half_rn(v.z)) | ((uint32_t)__half_as_ushort(__float2half_rn(v.w)) << 16);
  } else {
    pk.x = bf16_bits(v.x) | (bf16_bits(v.y) << 16);
    pk.y = bf16_bits(v.z) | (bf16_bits(v.w) << 16);
  }
  *reinterpret_cast<uint2*>((uint16_t*)p + i) = pk;
}

// plain copy of 4 consecutive elements / of one element (a tensor with no active adapter)
__device__ __forceinline__ void cp4(const void* s, void* d, int64_t i, int dtype) {
  if (dtype == ED_F32) *reinterpret_cast<uint4*>((uint32_t*)d + i) = *reinterpret_cast<const uint4*>((const uint32_t*)s + i);
  else *reinterpret_cast<uint2*>((uint16_t*)d + i) = *reinterpret_cast<const uint2*>((const uint16_t*)s + i);
}
__device__ __forceinline__ void cp1(const void* s, void* d, int64_t i, int dtype) {
  if (dtype == ED_F32) ((uint32_t*)d)[i] = ((const uint32_t*)s)[i];
  else ((uint16_t*)d)[i] = ((const uint16_t*)s)[i];
}

__global__ void __launch_bounds__(THREADS)
k_lora_merge(const int64_t* __restrict__ table, int n_tensors) {
  __shared__ __attribute__((aligned(16))) float s_up[QC][UP_PITCH];
  __shared__ __attribute__((aligned(16))) float s_down[QC][TN];

  // the last tensor whose first tile is <= this block (tile0 is ascending, tensor 0 starts at 0).  Uniform over the workgroup, and
  // the table stays cache-resident: a cooperative lookup (every thread testing its share of the records, an LDS atomicMax) was
  // measured and is slower (4.7 against 4.05 ms on the 700-tensor SDXL table at r = 16).
  const int64_t blk = blockIdx.x;
  int lo = 0, hi = n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[(int64_t)mid * T_WORDS + T_TILE0] <= blk) lo = mid;
    else hi = mid - 1;
  }
  const int64_t* T = table + (int64_t)lo * T_WORDS;
  const void* base = reinterpret_cast<const void*>(T[T_BASE]);
  void* dst = reinterpret_cast<void*>(T[T_DST]);
  const int N = (int)T[T_N], K = (int)T[T_K], dtype = (int)T[T_DTYPE];
  const int a0 = (int)T[T_A0], a1 = (int)T[T_A1];
  const int tiles_k = (K + TN - 1) / TN;
  const int local = (int)(blk - T[T_TILE0]);
  const int n0 = (local / tiles_k) * TM, k0 = (local % tiles_k) * TN;

  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int esz = dtype == ED_F32 ? 4 : 2;
  const bool wide = (K & 3) == 0 && ((T[T_BASE] | T[T_DST]) & (int64_t)(4 * esz - 1)) == 0;

  float s[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) s[i][j] = 0.0f;

  const int64_t* A = table + (int64_t)n_tensors * T_WORDS;
  for (int a = a0; a < a1; ++a) {
    const float* __restrict__ up = reinterpret_cast<const float*>(A[(int64_t)a * A_WORDS + A_UP]);
    const float* __restrict__ down = reinterpret_cast<const float*>(A[(int64_t)a * A_WORDS + A_DOWN]);
    const int r = (int)A[(int64_t)a * A_WORDS + A_R];
    const float c = __uint_as_float((uint32_t)A[(int64_t)a * A_WORDS + A_C]);
    float acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = 0.0f;

    for (int q0 = 0; q0 < r; q0 += QC) {
      const int qn = min(QC, r - q0);
      __syncthreads();  // the previous round's reads are done
      // up[n0 .. n0 + TM, q0 .. q0 + QC] -> s_up[q][n] (TM * QC = 1024 values, 4 per thread; consecutive lanes along q)
#pragma unroll
      for (int e = tid; e < TM * QC; e += THREADS) {
        const int nl = e / QC, q = e % QC;
        const int n = n0 + nl;
        s_up[q][nl] = (n < N && q < qn) ? up[(int64_t)n * r + q0 + q] : 0.0f;
      }
      // down[q0 .. q0 + QC, k0 .. k0 + TN] -> s_down[q][k] (consecutive lanes along k)
#pragma unroll
      for (int e = tid; e < QC * TN; e += THREADS) {
        const int q = e / TN, kl = e % TN;
        const int k = k0 + kl;
        s_down[q][kl] = (k < K && q < qn) ? down[(int64_t)(q0 + q) * K + k] : 0.0f;
      }
      __syncthreads();
      for (int q = 0; q < qn; ++q) {
        const float4 u = *reinterpret_cast<const float4*>(&s_up[q][ty * 4]);
        const float4 d0 = *reinterpret_cast<const float4*>(&s_down[q][tx * 4]);
        const float4 d1 = *reinterpret_cast<const float4*>(&s_down[q][64 + tx * 4]);
        const float uu[4] = {u.x, u.y, u.z, u.w};
        const float dd[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(uu[i], dd[j], acc[i][j]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) s[i][j] = fmaf(c, acc[i][j], s[i][j]);
  }

  const bool copy = a0 == a1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + ty * 4 + i;
    if (n >= N) continue;
    const int64_t row = (int64_t)n * K;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int k = k0 + g * 64 + tx * 4;
      if (k >= K) continue;
      if (wide) {  // K % 4 == 0 and k % 4 == 0: the group of 4 is inside the row, and row + k is a multiple of 4 elements
        if (copy) {
          cp4(base, dst, row + k, dtype);
        } else {
          const float4 b = ld4(base, row + k, dtype);
          st4(dst, row + k, make_float4(__fadd_rn(b.x, s[i][4 * g]), __fadd_rn(b.y, s[i][4 * g + 1]),
                                        __fadd_rn(b.z, s[i][4 * g + 2]), __fadd_rn(b.w, s[i][4 * g + 3])), dtype);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (k + j >= K) break;
          if (copy) cp1(base, dst, row + k + j, dtype);
          else st1(dst, row + k + j, __fadd_rn(ld1(base, row + k + j, dtype), s[i][4 * g + j]), dtype);
        }
      }
    }
  }
}

inline int64_t tiles_of(int64_t N, int64_t K) { return ((N + TM - 1) / TM) * ((K + TN - 1) / TN); }

}  // namespace

extern "C" {

int ed_lora_merge(const int64_t* table_host, const int64_t* table_dev, int n_tensors, int n_adapters, int64_t n_tiles,
                  void* stream) {
  if (!table_host || !table_dev || n_tensors < 1 || n_adapters < 0 || n_tiles < 1 || n_tiles > INT32_MAX ||
      (((uintptr_t)table_dev) & 7u) != 0)
    return (int)hipErrorInvalidValue;
  const int64_t* A = table_host + (int64_t)n_tensors * T_WORDS;
  int64_t tile = 0, next_adapter = 0;
  for (int t = 0; t < n_tensors; ++t) {
    const int64_t* T = table_host + (int64_t)t * T_WORDS;
    const int64_t N = T[T_N], K = T[T_K], dtype = T[T_DTYPE];
    if (dtype != ED_F32 && dtype != ED_F16 && dtype != ED_BF16) return (int)hipErrorInvalidValue;
    const int64_t esz = dtype == ED_F32 ? 4 : 2;
    if (!T[T_BASE] || !T[T_DST] || T[T_BASE] == T[T_DST] || ((T[T_BASE] | T[T_DST]) & (esz - 1)) != 0)
      return (int)hipErrorInvalidValue;
    if (N < 1 || K < 1 || N > INT32_MAX || K > INT32_MAX || N * K > INT32_MAX) return (int)hipErrorInvalidValue;
    // adapters of consecutive tensors are consecutive ranges: every adapter record belongs to exactly one tensor
    if (T[T_A0] != next_adapter || T[T_A1] < T[T_A0] || T[T_A1] > n_adapters) return (int)hipErrorInvalidValue;
    next_adapter = T[T_A1];
    if (T[T_TILE0] != tile) return (int)hipErrorInvalidValue;
    tile += tiles_of(N, K);
    for (int64_t a = T[T_A0]; a < T[T_A1]; ++a) {
      const int64_t* R = A + a * A_WORDS;
      if (!R[A_UP] || !R[A_DOWN] || ((R[A_UP] | R[A_DOWN]) & 3) != 0 || R[A_R] < 1 || R[A_R] > MAX_RANK ||
          (R[A_C] >> 32) != 0)
        return (int)hipErrorInvalidValue;
      const uint32_t bits = (uint32_t)R[A_C];
      float c;
      memcpy(&c, &bits, sizeof c);
      if (!isfinite(c)) return (int)hipErrorInvalidValue;
    }
  }
  if (next_adapter != n_adapters || tile != n_tiles) return (int)hipErrorInvalidValue;
  k_lora_merge<<<(unsigned)n_tiles, THREADS, 0, (hipStream_t)stream>>>(table_dev, n_tensors);
  return (int)hipGetLastError();
}

}  // extern "C"
