// vae_kernels.hip -- the fp32 VAE's ResnetBlock convolutions on the 16-bit MFMA pipe WITHOUT giving up fp32 accuracy (round 5).
//
// The reference keeps the VAE in fp32 on purpose (elastic_diffusion.py:328 encodes the pad strips outside autocast; :267-310 decodes
// in fp32), and the parity gates hold this repo to that (latents 1e-4 / images 1e-3 against the reference's goldens).  Rounds 1-4 left
// every VAE convolution to MIOpen's fp32 kernels: ~100 TFLOP/s on a chip whose fp32 matrix peak is 157 and whose 16-bit MFMA peak is
// 2500 -- 8 % of the headline image (100 pad-strip encodes) and a quarter of the tiled 2048 x 2048 decode.
//
// Operand splitting: an fp32 value v is carried as two fp16 numbers, hi = fp16(v) and lo = fp16(v - hi): hi + lo = v to 2^-22 |v|
// (11 + 11 significand bits).  With x = xh + xl and w = wh + wl,
//     x . w = xh.wh + xl.wh + xh.wl  (+ xl.wl, 2^-22 relative: dropped)
// and the three kept products, accumulated in fp32 by the MFMA, are ONE 16-bit convolution over 3 Cin channels:
//     x'' = [xh | xl | xh]  (per pixel),  w'' = [wh | wh | wl]  (per tap)        =>  conv(x'', w'') = conv(x, w) to ~3e-7 relative.
// So the existing implicit-GEMM main loop (gemm_kernels.hip, `ed_conv3x3_nhwc`) runs unchanged on channel-concatenated operands;
// what is new is (a) this file: GroupNorm + SiLU over an fp32 NHWC activation that WRITES the split 3C-channel fp16 operand (the
// activation after GroupNorm + SiLU is bounded by the affine parameters, so fp16's range is safe there -- which is why only the
// ResnetBlock convolutions take this path and the stream-fed up / down-sampling convolutions stay with the library), and (b) an
// fp32-output epilogue of the GEMM kernel (fp32 bias, fp32 residual, a power-of-two scale that undoes the weight pre-scaling which
// keeps wl out of fp16's subnormal range): `ed_conv3x3_nhwc_f32out`.  Three MFMA passes at ~1 PFLOP/s are ~3.5 x the fp32 pipe.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "elastic_hip.h"

namespace {

#define GV_THREADS 256
#define GV_UNROLL 4
#define GV_MAXG 256

__device__ __forceinline__ float silu32(float x) { return x / (1.0f + expf(-x)); }
// fp16(clamp(v, +-65504)): identical to (_Float16)v inside fp16's range (NaN stays NaN: both comparisons are false)
__device__ __forceinline__ _Float16 sat16(float v) { return (_Float16)(v > 65504.f ? 65504.f : (v < -65504.f ? -65504.f : v)); }
// the per-tensor power of two of the raw-stream split: e = max(0, exponent(absmax) - 14), so that |2^-e v| < 2^15 for every |v| <= absmax
// (gemm_kernels.hip holds the same three lines for the convolution's 2^e)
__device__ __forceinline__ int split_exponent(float absmax) {
  const int E = (int)((__builtin_bit_cast(uint32_t, absmax) >> 23) & 0xffu) - 127;
  return E > 14 ? E - 14 : 0;
}

// ---- statistics: every thread owns one 4-channel column (cpg % 4 == 0: the column lies inside ONE group) and walks rows ----------
// x [N, HW, C] fp32 (channels-last memory of a [N, C, H, W] tensor); partial [N, nchunks, G, 2] (sum, sum of squares) of x - K, where K
// is the group's first element (pixel 0, channel g * cpg), read by every block of the sample and again by the apply pass: shifted by a
// sample of the data the sums are a few standard deviations in size, so the fp32 partials and var = qq/n - (ss/n)^2 keep their digits
// whatever the group's mean.  Fixed summation order: bit-reproducible.
// WEIGHTED: pixel (y, x) counts wy[y] * wx[x] times (either vector may be NULL = all ones) -- the narrowed constant-image encode, where
// one row / column stands for a run of identical ones.  Both sums carry the weight; the apply pass divides by the
// weighted element count.  The weighted sums are kept in two parts: every pixel ONCE, by the unweighted code (same order, same fp32
// partials: all-ones weights give the unweighted bits), and the EXCESS (w - 1) of the few heavy pixels in double, in double partials
// [N, nchunks, G, 2] behind the fp32 ones (three times the workspace) -- a handful of heavy terms can dominate a sum, and their rounding
// errors would not average out as they do over thousands of equal terms.  The unweighted instantiation is the code it always was.
template <bool WEIGHTED>
__global__ void __launch_bounds__(GV_THREADS)
k_gn32_nhwc_partial(const float* __restrict__ x, float* __restrict__ partial, int C, int HW, int G, int rows_per_block,
                    const float* __restrict__ wx, const float* __restrict__ wy, int W) {
  extern __shared__ double sh_raw[];
  float* sh = reinterpret_cast<float*>(sh_raw);          // [row lanes][VC][2]
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int VC = C >> 2, cpg = C / G;
  const int ncol = (VC + GV_THREADS - 1) / GV_THREADS;        // columns per thread (1 for C <= 1024)
  const int R = ncol == 1 ? GV_THREADS / VC : 1;              // row lanes
  const int my_r = ncol == 1 ? threadIdx.x / VC : 0;
  const int my_c = ncol == 1 ? threadIdx.x % VC : threadIdx.x;
  const bool active = ncol == 1 ? (int)threadIdx.x < R * VC : true;
  const int r0 = chunk * rows_per_block, r1 = min(HW, r0 + rows_per_block);
  const float* base = x + (int64_t)n * HW * C;
  if (active) {
    for (int j = 0; j < ncol; ++j) {
      const int vc = my_c + j * GV_THREADS;
      if (vc >= VC) break;
      float s = 0.f, q = 0.f;
      double es = 0.0, eq = 0.0;  // (WEIGHTED) the excess weight's share
      const float K = base[((vc << 2) / cpg) * cpg];
      auto add = [&](float4 v, int pix) {
        v.x -= K, v.y -= K, v.z -= K, v.w -= K;
        s += (v.x + v.y) + (v.z + v.w);
        q += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        if (WEIGHTED) {
          const int py = pix / W;
          const double w = (double)(wy ? wy[py] : 1.0f) * (double)(wx ? wx[pix - py * W] : 1.0f) - 1.0;
          if (w != 0.0) {
            const double a = v.x, b = v.y, c = v.z, d = v.w;
            es += w * ((a + b) + (c + d));
            eq += w * ((a * a + b * b) + (c * c + d * d));
          }
        }
      };
      const float* col = base + (vc << 2);
      const int64_t step = (int64_t)R * C;
      int row = r0 + my_r;
      for (; row + (GV_UNROLL - 1) * R < r1; row += GV_UNROLL * R) {
        const float* p0 = col + (int64_t)row * C;
        float4 v[GV_UNROLL];
#pragma unroll
        for (int u = 0; u < GV_UNROLL; ++u) v[u] = *reinterpret_cast<const float4*>(p0 + u * step);
#pragma unroll
        for (int u = 0; u < GV_UNROLL; ++u) add(v[u], row + u * R);
      }
      for (; row < r1; row += R) add(*reinterpret_cast<const float4*>(col + (int64_t)row * C), row);
      float* slot = sh + ((int64_t)my_r * VC + vc) * 2;
      slot[0] = s, slot[1] = q;
      if (WEIGHTED) {  // the double slots lie behind the R * VC float pairs
        double* eslot = sh_raw + (int64_t)R * VC + ((int64_t)my_r * VC + vc) * 2;
        eslot[0] = es, eslot[1] = eq;
      }
    }
  }
  __syncthreads();
  float* dst = partial + ((int64_t)n * gridDim.x + chunk) * 2 * G;
  const int cols_per_group = cpg >> 2;
  for (int g = threadIdx.x; g < G; g += GV_THREADS) {
    double s = 0.0, q = 0.0;
    for (int vc = g * cols_per_group; vc < (g + 1) * cols_per_group; ++vc)
      for (int r = 0; r < R; ++r) {
        const float* slot = sh + ((int64_t)r * VC + vc) * 2;
        s += (double)slot[0];
        q += (double)slot[1];
      }
    dst[2 * g] = (float)s;
    dst[2 * g + 1] = (float)q;
    if (WEIGHTED) {
      double es = 0.0, eq = 0.0;
      for (int vc = g * cols_per_group; vc < (g + 1) * cols_per_group; ++vc)
        for (int r = 0; r < R; ++r) {
          const double* eslot = sh_raw + (int64_t)R * VC + ((int64_t)r * VC + vc) * 2;
          es += eslot[0];
          eq += eslot[1];
        }
      // [N, nchunks, G, 2] doubles behind the [gridDim.y, nchunks, G, 2] floats
      double* edst = reinterpret_cast<double*>(partial + (int64_t)gridDim.y * gridDim.x * 2 * G) + ((int64_t)n * gridDim.x + chunk) * 2 * G;
      edst[2 * g] = es;
      edst[2 * g + 1] = eq;
    }
  }
}

// ---- apply: y = [silu]((x - mean) rstd gamma + beta) in fp32, written as
//   SPLIT = false: fp32 [N, HW, C]
//   SPLIT = true : fp16 [N, HW, 3 C] = [hi | lo | hi] with hi = fp16(y), lo = fp16(y - hi)     (the A operand of ed_conv3x3_nhwc_f32out)
template <bool ACT, bool SPLIT>
__global__ void __launch_bounds__(GV_THREADS)
k_gn32_nhwc_apply(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                  const float* __restrict__ partial, void* __restrict__ out, int C, int HW, int G, int rows_per_block, double count,
                  float eps, const float* __restrict__ wx, const float* __restrict__ wy, int W) {
  __shared__ double red[2 * GV_THREADS];
  __shared__ float stats[2 * GV_MAXG];
  // (walked back to front, like the 16-bit kernel's apply pass: what the statistics pass read last is what the last-level cache still holds)
  const int n = gridDim.y - 1 - blockIdx.y, chunk = gridDim.x - 1 - blockIdx.x, nchunks = gridDim.x;
  {
    const int parts = GV_THREADS / G > 0 ? GV_THREADS / G : 1;
    const int g = threadIdx.x % G, part = threadIdx.x / G;
    double s = 0.0, q = 0.0;
    if (part < parts) {
      const float* p = partial + (int64_t)n * nchunks * 2 * G + 2 * g;
      for (int c = part; c < nchunks; c += parts) {
        s += (double)p[(int64_t)c * 2 * G];
        q += (double)p[(int64_t)c * 2 * G + 1];
      }
    }
    red[2 * threadIdx.x] = s, red[2 * threadIdx.x + 1] = q;
    __syncthreads();
    if ((int)threadIdx.x < G) {
      double ss = 0.0, qq = 0.0;
      for (int k = 0; k < parts; ++k) {
        ss += red[2 * (k * G + threadIdx.x)];
        qq += red[2 * (k * G + threadIdx.x) + 1];
      }
      if (wx || wy) {  // weighted statistics: the excess weights' sums (double partials behind the fp32 ones; nothing to add when all
                       // weights are 1), and the element count (C / G) sum(wy) sum(wx) (integers held in fp32: the sums are exact)
        const double* e = reinterpret_cast<const double*>(partial + (int64_t)gridDim.y * nchunks * 2 * G) + (int64_t)n * nchunks * 2 * G +
                          2 * threadIdx.x;
        double es = 0.0, eq = 0.0;
        for (int c = 0; c < nchunks; ++c) {
          es += e[(int64_t)c * 2 * G];
          eq += e[(int64_t)c * 2 * G + 1];
        }
        if (es != 0.0) ss += es;
        if (eq != 0.0) qq += eq;
        double sx = W, sy = HW / W;
        if (wx) {
          sx = 0.0;
          for (int i = 0; i < W; ++i) sx += (double)wx[i];
        }
        if (wy) {
          sy = 0.0;
          for (int i = 0; i < HW / W; ++i) sy += (double)wy[i];
        }
        count = sx * sy * (double)(C / G);
      }
      const double dmean = ss / count;  // of x - K (k_gn32_nhwc_partial)
      double var = qq / count - dmean * dmean;
      if (var < 0.0) var = 0.0;
      const double mean = (double)x[(int64_t)n * HW * C + (int64_t)threadIdx.x * (C / G)] + dmean;
      stats[2 * threadIdx.x] = (float)mean;
      stats[2 * threadIdx.x + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
  }
  const int VC = C >> 2, cpg = C / G;
  const int ncol = (VC + GV_THREADS - 1) / GV_THREADS;
  const int R = ncol == 1 ? GV_THREADS / VC : 1;
  const int my_r = ncol == 1 ? threadIdx.x / VC : 0;
  const int my_c = ncol == 1 ? threadIdx.x % VC : threadIdx.x;
  if (ncol == 1 && (int)threadIdx.x >= R * VC) return;
  const int r0 = chunk * rows_per_block, r1 = min(HW, r0 + rows_per_block);
  const float* xb = x + (int64_t)n * HW * C;
  for (int j = 0; j < ncol; ++j) {
    const int vc = my_c + j * GV_THREADS;
    if (vc >= VC) break;
    const int c0 = vc << 2, g = c0 / cpg;
    const float mean = stats[2 * g], rstd = stats[2 * g + 1];
    const float4 gm = *reinterpret_cast<const float4*>(gamma + c0), bt = *reinterpret_cast<const float4*>(beta + c0);
    const float a0 = rstd * gm.x, a1 = rstd * gm.y, a2 = rstd * gm.z, a3 = rstd * gm.w;
    const float b0 = fmaf(-a0, mean, bt.x), b1 = fmaf(-a1, mean, bt.y), b2 = fmaf(-a2, mean, bt.z), b3 = fmaf(-a3, mean, bt.w);
    auto norm = [&](const float4& v) {
      float4 o;
      o.x = fmaf(a0, v.x, b0), o.y = fmaf(a1, v.y, b1), o.z = fmaf(a2, v.z, b2), o.w = fmaf(a3, v.w, b3);
      if (ACT) o.x = silu32(o.x), o.y = silu32(o.y), o.z = silu32(o.z), o.w = silu32(o.w);
      return o;
    };
    auto store = [&](int64_t row, const float4& y) {
      if (SPLIT) {
        uint16_t* ob = reinterpret_cast<uint16_t*>(out) + ((int64_t)n * HW + row) * (3 * (int64_t)C) + c0;
        // saturating (round 6): a value beyond fp16's range gives a finite clamped operand, never hi = inf, lo = -inf
        const _Float16 h0 = sat16(y.x), h1 = sat16(y.y), h2 = sat16(y.z), h3 = sat16(y.w);
        const _Float16 l0 = sat16(y.x - (float)h0), l1 = sat16(y.y - (float)h1), l2 = sat16(y.z - (float)h2), l3 = sat16(y.w - (float)h3);
        uint2 hi, lo;
        hi.x = (uint32_t)__builtin_bit_cast(uint16_t, h0) | ((uint32_t)__builtin_bit_cast(uint16_t, h1) << 16);
        hi.y = (uint32_t)__builtin_bit_cast(uint16_t, h2) | ((uint32_t)__builtin_bit_cast(uint16_t, h3) << 16);
        lo.x = (uint32_t)__builtin_bit_cast(uint16_t, l0) | ((uint32_t)__builtin_bit_cast(uint16_t, l1) << 16);
        lo.y = (uint32_t)__builtin_bit_cast(uint16_t, l2) | ((uint32_t)__builtin_bit_cast(uint16_t, l3) << 16);
        *reinterpret_cast<uint2*>(ob) = hi;
        *reinterpret_cast<uint2*>(ob + C) = lo;
        *reinterpret_cast<uint2*>(ob + 2 * C) = hi;
      } else {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + ((int64_t)n * HW + row) * C + c0) = y;
      }
    };
    const int64_t step = (int64_t)R * C;
    int row = r0 + my_r;
    for (; row + (GV_UNROLL - 1) * R < r1; row += GV_UNROLL * R) {
      const float* p0 = xb + (int64_t)row * C + c0;
      float4 v[GV_UNROLL];
#pragma unroll
      for (int u = 0; u < GV_UNROLL; ++u) v[u] = *reinterpret_cast<const float4*>(p0 + u * step);
#pragma unroll
      for (int u = 0; u < GV_UNROLL; ++u) store(row + u * R, norm(v[u]));
    }
    for (; row < r1; row += R) store(row, norm(*reinterpret_cast<const float4*>(xb + (int64_t)row * C + c0)));
  }
}

// ---- split of a raw fp32 channels-last activation (no normalisation in front of it: the decoder's upsampler convolutions) -----------
// x fp32 [N, H, W, C] -> out fp16 [N, U H, U W, 3 C] = [hi | lo | hi], U = 1 or 2 (nearest-neighbour 2x upsampling folded into the write:
// every input pixel lands on its U x U output pixels).  The stream is not bounded by an affine map (the real SDXL decoder stream leaves
// fp16's range), so the tensor is scaled by 2^-e, e from its absolute maximum (k_absmax32 below; exact), before the split, and the
// convolution multiplies by 2^e: exact over the whole fp32 range (round 6; round 5 clamped hi only: 11 bits in (65504, 1.3e5], inf - inf
// beyond).  Without an absmax (NULL) hi and lo both saturate: finite everywhere, exact up to 65504.
template <int U>
__global__ void __launch_bounds__(256)
k_split32_nhwc(const float* __restrict__ x, uint16_t* __restrict__ out, int C, int H, int W, int64_t n_vec, const float* __restrict__ absmax) {
  const int VC = C >> 2;
  const float sc = absmax ? __builtin_bit_cast(float, (uint32_t)(127 - split_exponent(*absmax)) << 23) : 1.0f;   // 2^-e
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pix = i / VC;
    const int c0 = (int)(i - pix * VC) << 2;
    const float4 v = *reinterpret_cast<const float4*>(x + pix * C + c0);
    const float f[4] = {v.x * sc, v.y * sc, v.z * sc, v.w * sc};
    uint32_t hw[2], lw[2];
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      uint16_t hb[2], lb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const _Float16 h = sat16(f[e + j]);
        const _Float16 l = sat16(f[e + j] - (float)h);
        hb[j] = __builtin_bit_cast(uint16_t, h), lb[j] = __builtin_bit_cast(uint16_t, l);
      }
      hw[e >> 1] = (uint32_t)hb[0] | ((uint32_t)hb[1] << 16);
      lw[e >> 1] = (uint32_t)lb[0] | ((uint32_t)lb[1] << 16);
    }
    const uint2 hi = {hw[0], hw[1]}, lo = {lw[0], lw[1]};
    const int64_t n = pix / ((int64_t)H * W), rem = pix - n * (int64_t)H * W;
    const int y = (int)(rem / W), xx = (int)(rem - (int64_t)y * W);
#pragma unroll
    for (int dy = 0; dy < U; ++dy)
#pragma unroll
      for (int dx = 0; dx < U; ++dx) {
        uint16_t* ob = out + ((n * (U * H) + (U * y + dy)) * (int64_t)(U * W) + (U * xx + dx)) * (3 * (int64_t)C) + c0;
        *reinterpret_cast<uint2*>(ob) = hi;
        *reinterpret_cast<uint2*>(ob + C) = lo;
        *reinterpret_cast<uint2*>(ob + 2 * C) = hi;
      }
  }
}

// ---- max |x| of an fp32 tensor as a bit pattern (non-negative floats order like unsigned integers; NaN patterns sort above Inf) ------
__global__ void __launch_bounds__(256)
k_absmax32(const float* __restrict__ x, uint32_t* __restrict__ out, int64_t n) {
  uint32_t m = 0;
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const uint4 v = *reinterpret_cast<const uint4*>(x + 4 * i);
    const uint32_t a = max(v.x & 0x7fffffffu, v.y & 0x7fffffffu), b = max(v.z & 0x7fffffffu, v.w & 0x7fffffffu);
    m = max(m, max(a, b));
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < n - 4 * n4) m = max(m, __builtin_bit_cast(uint32_t, x[4 * n4 + threadIdx.x]) & 0x7fffffffu);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

inline int done() { return (int)hipGetLastError(); }

inline int gv_chunks(int C, int HW, int* rows_per_block) {
  // ~64 K elements per block, at most 256 chunks per sample (every apply block re-reads its sample's [nchunks, G, 2] partial sums)
  int rpb = (65536 + C - 1) / C;
  if ((HW + rpb - 1) / rpb > 256) rpb = (HW + 255) / 256;
  if (rpb < 1) rpb = 1;
  *rows_per_block = rpb;
  return (HW + rpb - 1) / rpb;
}

// both GroupNorm entry points: wx [W] / wy [HW / W] are the optional pixel multiplicities (NULL, NULL: W is not looked at)
int gn32_nhwc_launch(const void* x, const void* gamma, const void* beta, void* out, float* workspace, int N, int C, int HW, int W, int G,
                     float eps, int act_silu, int split16, const float* wx, const float* wy, void* stream) {
  if (N == 0) return 0;
  if (N < 0 || HW <= 0 || W <= 0 || HW % W != 0 || (((uintptr_t)wx | (uintptr_t)wy) & 3u) || G <= 0 || G > GV_MAXG || C % G != 0 ||
      (C / G) % 4 != 0 || C > 4 * GV_THREADS * 4 || N > 65535 ||
      (((uintptr_t)x | (uintptr_t)out | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)workspace) & 15u))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  int rpb;
  const int nchunks = gv_chunks(C, HW, &rpb);
  dim3 grid(nchunks, N);
  const int VC = C / 4;
  const size_t lds = sizeof(float) * 2 * (size_t)VC * (VC <= GV_THREADS ? GV_THREADS / VC : 1);
  if (wx || wy) k_gn32_nhwc_partial<true><<<grid, GV_THREADS, 3 * lds, s>>>((const float*)x, workspace, C, HW, G, rpb, wx, wy, W);
  else k_gn32_nhwc_partial<false><<<grid, GV_THREADS, lds, s>>>((const float*)x, workspace, C, HW, G, rpb, nullptr, nullptr, W);
  const double count = (double)HW * (C / G);
#define GV_APPLY(ACT, SPLIT)                                                                                                      \
  k_gn32_nhwc_apply<ACT, SPLIT><<<grid, GV_THREADS, 0, s>>>((const float*)x, (const float*)gamma, (const float*)beta, workspace, \
                                                            out, C, HW, G, rpb, count, eps, wx, wy, W)
  if (act_silu && split16) GV_APPLY(true, true);
  else if (act_silu) GV_APPLY(true, false);
  else if (split16) GV_APPLY(false, true);
  else GV_APPLY(false, false);
#undef GV_APPLY
  return done();
}

}  // namespace

extern "C" {

int64_t ed_groupnorm_nhwc_f32_workspace(int N, int C, int HW, int G) {
  if (G <= 0 || C <= 0 || HW <= 0) return 0;
  int rpb;
  const int nchunks = gv_chunks(C, HW, &rpb);
  return (int64_t)N * nchunks * G * 2 * (int64_t)sizeof(float);
}

int ed_groupnorm_nhwc_f32(const void* x, const void* gamma, const void* beta, void* out, float* workspace, int N, int C, int HW, int G,
                          float eps, int act_silu, int split16, void* stream) {
  return gn32_nhwc_launch(x, gamma, beta, out, workspace, N, C, HW, HW, G, eps, act_silu, split16, nullptr, nullptr, stream);
}

int ed_groupnorm_nhwc_f32_weighted(const void* x, const void* gamma, const void* beta, void* out, float* workspace, int N, int C, int H,
                                   int W, int G, float eps, int act_silu, int split16, const float* wx, const float* wy, void* stream) {
  if (H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffffll) return (int)hipErrorInvalidValue;
  return gn32_nhwc_launch(x, gamma, beta, out, workspace, N, C, H * W, W, G, eps, act_silu, split16, wx, wy, stream);
}

int ed_absmax_f32(const void* x, int64_t n, float* out, void* stream) {
  if (n < 0 || !out || ((uintptr_t)x & 15u) || ((uintptr_t)out & 3u)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(out, 0, sizeof(float), s);
  if (e != hipSuccess) return (int)e;
  if (n == 0) return 0;
  int64_t blocks = ((n >> 2) + 256 * 8 - 1) / (256 * 8);      // 8 16-byte loads per thread
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  k_absmax32<<<(unsigned)blocks, 256, 0, s>>>((const float*)x, reinterpret_cast<uint32_t*>(out), n);
  return done();
}

int ed_split_f32_nhwc(const void* x, void* out, int N, int C, int H, int W, int upsample2x, const float* absmax, void* stream) {
  if (N == 0) return 0;
  if (N < 0 || C <= 0 || C % 4 != 0 || H <= 0 || W <= 0 || (((uintptr_t)x | (uintptr_t)out) & 15u) || ((3 * C * 2) % 8) != 0 ||
      ((uintptr_t)absmax & 3u))
    return (int)hipErrorInvalidValue;
  const int64_t n_vec = (int64_t)N * H * W * (C / 4);
  int64_t blocks = (n_vec + 255) / 256;
  if (blocks > 65536 * 16) blocks = 65536 * 16;
  hipStream_t s = (hipStream_t)stream;
  if (upsample2x) k_split32_nhwc<2><<<(unsigned)blocks, 256, 0, s>>>((const float*)x, (uint16_t*)out, C, H, W, n_vec, absmax);
  else k_split32_nhwc<1><<<(unsigned)blocks, 256, 0, s>>>((const float*)x, (uint16_t*)out, C, H, W, n_vec, absmax);
  return done();
}

}  // extern "C"
