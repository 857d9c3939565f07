// elastic_kernels.hip -- gfx950 (MI355X, CDNA4) kernels + C ABI for the ElasticDiffusion hot path.
//
// Every kernel here is HBM/latency bound latent-space glue (gather / scatter / select / a few fp32 flops per
// element); tensors are 64 KiB - 12 MiB, so the design rules are: one launch per logical phase, x-fastest
// coalesced addressing (64 lanes x 4 B or 16 B contiguous), 16-byte vector access on the pure streaming kernels,
// no atomics, no read-modify-write, no host sync.  MFMA is deliberately not used: nothing here is a contraction.
//
// fp32 arithmetic is written with explicit __fmul_rn/__fadd_rn/__fsub_rn/__fdiv_rn and the file is compiled with
// -ffp-contract=off so no FMA is formed: results are bit-identical to the reference's torch-CPU op sequence.
//
// Interface documentation (and the reference file:line each entry replaces) lives in include/elastic_hip.h.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "elastic_hip.h"

#define ED_ABI_VERSION 13
#define ED_BLOCK 256

namespace {

// ---- element type adapters (model-boundary tensors may be f32 / f16 / bf16) -----------------------
struct F32 { using type = float; };
struct F16 { using type = __half; };
struct BF16 { using type = uint16_t; };

template <typename Tag> __device__ __forceinline__ float ld(const void* p, int64_t i);
template <> __device__ __forceinline__ float ld<F32>(const void* p, int64_t i) { return ((const float*)p)[i]; }
template <> __device__ __forceinline__ float ld<F16>(const void* p, int64_t i) { return __half2float(((const __half*)p)[i]); }
template <> __device__ __forceinline__ float ld<BF16>(const void* p, int64_t i) {
  return __uint_as_float(((uint32_t)((const uint16_t*)p)[i]) << 16);
}

template <typename Tag> __device__ __forceinline__ void st(void* p, int64_t i, float v);
template <> __device__ __forceinline__ void st<F32>(void* p, int64_t i, float v) { ((float*)p)[i] = v; }
template <> __device__ __forceinline__ void st<F16>(void* p, int64_t i, float v) { ((__half*)p)[i] = __float2half_rn(v); }
template <> __device__ __forceinline__ void st<BF16>(void* p, int64_t i, float v) {
  uint32_t u = __float_as_uint(v);
  uint16_t r;
  if ((u & 0x7fffffffu) > 0x7f800000u) {
    r = 0x7fc0;  // NaN
  } else {
    u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even, like torch
    r = (uint16_t)(u >> 16);
  }
  ((uint16_t*)p)[i] = r;
}

// 4 consecutive elements: 16-byte (f32) or 8-byte (16-bit) vector access; callers guarantee alignment
template <typename Tag> __device__ __forceinline__ void st4(void* p, int64_t i, float a, float b, float c, float d);
template <> __device__ __forceinline__ void st4<F32>(void* p, int64_t i, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>((float*)p + i) = make_float4(a, b, c, d);
}
template <> __device__ __forceinline__ void st4<F16>(void* p, int64_t i, float a, float b, float c, float d) {
  uint2 pk;
  pk.x = (uint32_t)__half_as_ushort(__float2half_rn(a)) | ((uint32_t)__half_as_ushort(__float2half_rn(b)) << 16);
  pk.y = (uint32_t)__half_as_ushort(__float2half_rn(c)) | ((uint32_t)__half_as_ushort(__float2half_rn(d)) << 16);
  *reinterpret_cast<uint2*>((uint16_t*)p + i) = pk;
}
__device__ __forceinline__ uint32_t bf16_bits(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
template <> __device__ __forceinline__ void st4<BF16>(void* p, int64_t i, float a, float b, float c, float d) {
  uint2 pk;
  pk.x = bf16_bits(a) | (bf16_bits(b) << 16);
  pk.y = bf16_bits(c) | (bf16_bits(d) << 16);
  *reinterpret_cast<uint2*>((uint16_t*)p + i) = pk;
}
template <typename Tag> __device__ __forceinline__ float4 ld4(const void* p, int64_t i);
template <> __device__ __forceinline__ float4 ld4<F32>(const void* p, int64_t i) {
  return *reinterpret_cast<const float4*>((const float*)p + i);
}
template <> __device__ __forceinline__ float4 ld4<F16>(const void* p, int64_t i) {
  uint2 pk = *reinterpret_cast<const uint2*>((const uint16_t*)p + i);
  return make_float4(__half2float(__ushort_as_half((uint16_t)(pk.x & 0xffffu))), __half2float(__ushort_as_half((uint16_t)(pk.x >> 16))),
                     __half2float(__ushort_as_half((uint16_t)(pk.y & 0xffffu))), __half2float(__ushort_as_half((uint16_t)(pk.y >> 16))));
}
template <> __device__ __forceinline__ float4 ld4<BF16>(const void* p, int64_t i) {
  uint2 pk = *reinterpret_cast<const uint2*>((const uint16_t*)p + i);
  return make_float4(__uint_as_float(pk.x << 16), __uint_as_float(pk.x & 0xffff0000u), __uint_as_float(pk.y << 16),
                     __uint_as_float(pk.y & 0xffff0000u));
}

inline int grid_for(int64_t n, int per_thread = 1) {
  int64_t t = (n + per_thread - 1) / per_thread;
  int64_t g = (t + ED_BLOCK - 1) / ED_BLOCK;
  return (int)(g < 1 ? 1 : g);
}

inline int done() { return (int)hipGetLastError(); }

// ---- ed_gather_views / ed_tile_gather_pad ----------------------------------------------------------
// X (ed_assemble_rows_x): rows carry C + E channels; channel c >= C is the same gather applied to plane c - C of `extra`
// ([B,E,H,W]), with the constant pad_value[c - C] wherever a latent channel reads the frame.  X = false is the code as it was.
template <typename Tag, bool X = false>
__device__ __forceinline__ void gather_windows_body(int64_t t, const float* __restrict__ latent, void* __restrict__ out, int B, int C, int H, int W,
                 const int32_t* __restrict__ wy0, const int32_t* __restrict__ wx0, int V, int Sh, int Sw,
                 int PH, int PW, int off_y, int off_x, const float* __restrict__ frame, float divisor, int use_div,
                 const float* __restrict__ extra = nullptr, int E = 0, const float* __restrict__ pad_value = nullptr) {
  const int CT = X ? C + E : C;
  int64_t n = (int64_t)V * B * CT * PH * PW;
  if (t >= n) return;
  int x = (int)(t % PW);
  int64_t r = t / PW;
  int y = (int)(r % PH);
  r /= PH;
  int c = (int)(r % CT);
  r /= CT;  // row = v*B + b
  int b = (int)(r % B);
  int v = (int)(r / B);
  const bool ex = X && c >= C;
  int yy = y - off_y, xx = x - off_x;
  float val;
  if (yy >= 0 && yy < Sh && xx >= 0 && xx < Sw) {
    int sy = wy0[v] + yy, sx = wx0[v] + xx;
    if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
      val = ex ? extra[(((int64_t)b * E + (c - C)) * H + sy) * W + sx] : latent[(((int64_t)b * C + c) * H + sy) * W + sx];
      if (use_div) val = __fdiv_rn(val, divisor);
    } else {
      val = 0.0f;
    }
  } else if (ex) {
    val = pad_value[c - C];
  } else {
    val = frame ? frame[((int64_t)c * PH + y) * PW + x] : 0.0f;
  }
  st<Tag>(out, t, val);
}

template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_gather_windows(const float* __restrict__ latent, void* __restrict__ out, int B, int C, int H, int W,
                 const int32_t* __restrict__ wy0, const int32_t* __restrict__ wx0, int V, int Sh, int Sw,
                 int PH, int PW, int off_y, int off_x, const float* __restrict__ frame, float divisor, int use_div) {
  gather_windows_body<Tag>((int64_t)blockIdx.x * ED_BLOCK + threadIdx.x, latent, out, B, C, H, W, wy0, wx0, V, Sh, Sw, PH, PW, off_y, off_x, frame, divisor, use_div);
}

// 4 consecutive x per thread; requires PW, Sw, off_x multiples of 4 (a group is entirely inside or outside the window)
template <typename Tag, bool X = false>
__device__ __forceinline__ void gather_windows_x4_body(int64_t t, const float* __restrict__ latent, void* __restrict__ out, int B, int C, int H, int W,
                    const int32_t* __restrict__ wy0, const int32_t* __restrict__ wx0, int V, int Sh, int Sw,
                    int PH, int PW, int off_y, int off_x, const float* __restrict__ frame, float divisor, int use_div,
                    const float* __restrict__ extra = nullptr, int E = 0, const float* __restrict__ pad_value = nullptr) {
  const int CT = X ? C + E : C;
  int PW4 = PW >> 2;
  int64_t n = (int64_t)V * B * CT * PH * PW4;
  if (t >= n) return;
  int x = (int)(t % PW4) << 2;
  int64_t r = t / PW4;
  int y = (int)(r % PH);
  r /= PH;
  int c = (int)(r % CT);
  r /= CT;
  int b = (int)(r % B);
  int v = (int)(r / B);
  const bool ex = X && c >= C;
  int yy = y - off_y, xx = x - off_x;
  float val[4];
  if (yy >= 0 && yy < Sh && xx >= 0 && xx < Sw) {
    int sy = wy0[v] + yy, sx0 = wx0[v] + xx;
    const float* src = ex ? extra + (((int64_t)b * E + (c - C)) * H + sy) * W : latent + (((int64_t)b * C + c) * H + sy) * W;
    bool row_ok = sy >= 0 && sy < H;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int sx = sx0 + e;
      float f = (row_ok && sx >= 0 && sx < W) ? src[sx] : 0.0f;
      val[e] = (use_div && row_ok && sx >= 0 && sx < W) ? __fdiv_rn(f, divisor) : f;
    }
  } else if (ex) {
    val[0] = val[1] = val[2] = val[3] = pad_value[c - C];
  } else if (frame) {
    float4 f = *reinterpret_cast<const float4*>(frame + ((int64_t)c * PH + y) * PW + x);
    val[0] = f.x; val[1] = f.y; val[2] = f.z; val[3] = f.w;
  } else {
    val[0] = val[1] = val[2] = val[3] = 0.0f;
  }
  st4<Tag>(out, t << 2, val[0], val[1], val[2], val[3]);
}

template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_gather_windows_x4(const float* __restrict__ latent, void* __restrict__ out, int B, int C, int H, int W,
                    const int32_t* __restrict__ wy0, const int32_t* __restrict__ wx0, int V, int Sh, int Sw,
                    int PH, int PW, int off_y, int off_x, const float* __restrict__ frame, float divisor, int use_div) {
  gather_windows_x4_body<Tag>((int64_t)blockIdx.x * ED_BLOCK + threadIdx.x, latent, out, B, C, H, W, wy0, wx0, V, Sh, Sw, PH, PW, off_y, off_x, frame, divisor, use_div);
}

// ---- ed_scatter_centres ----------------------------------------------------------------------------
template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_scatter_centres(const void* __restrict__ pred, float* __restrict__ local, int B, int C, int H, int W,
                  int PH, int PW, int ncb, const int32_t* __restrict__ row_blk, const int32_t* __restrict__ row_src,
                  const int32_t* __restrict__ col_blk, const int32_t* __restrict__ col_src) {
  int64_t n = (int64_t)B * C * H * W;
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  int X = (int)(t % W);
  int64_t r = t / W;
  int Y = (int)(r % H);
  r /= H;
  int c = (int)(r % C);
  int b = (int)(r / C);
  float cur = 0.0f;
  bool settled = false;
#pragma unroll
  for (int kr = 0; kr < 2; ++kr) {
    int rb = row_blk[Y * 2 + kr];
    if (rb < 0 || settled) continue;
    int sy = row_src[Y * 2 + kr];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      int cb = col_blk[X * 2 + kc];
      if (cb < 0 || settled) continue;
      int sx = col_src[X * 2 + kc];
      int64_t row = (int64_t)(rb * ncb + cb) * B + b;
      cur = ld<Tag>(pred, ((row * C + c) * PH + sy) * PW + sx);
      if (cur != 0.0f) settled = true;  // NaN != 0 is true, as in torch
    }
  }
  local[t] = cur;
}

// ---- ed_pick_assemble ------------------------------------------------------------------------------
template <typename Tag, bool X = false>
__device__ __forceinline__ void pick_assemble_body(int64_t t, const float* __restrict__ latent, const uint8_t* __restrict__ idx,
                const int32_t* __restrict__ src_row, const int32_t* __restrict__ src_col,
                const float* __restrict__ frame, void* __restrict__ out, float* __restrict__ low,
                int K, int B, int C, int H, int W, int h, int w, int PH, int PW, int off_y, int off_x,
                const float* __restrict__ extra = nullptr, int E = 0, const float* __restrict__ pad_value = nullptr,
                const int copies = 2) {  // rows written per step and sample: uncond + cond, or uncond + P cond (ed_assemble_rows_n)
  const int CT = X ? C + E : C;  // X: see gather_windows_body; `low` keeps the C latent channels
  int64_t n = (int64_t)K * B * CT * PH * PW;
  if (t >= n) return;
  int x = (int)(t % PW);
  int64_t r = t / PW;
  int y = (int)(r % PH);
  r /= PH;
  int c = (int)(r % CT);
  r /= CT;
  int b = (int)(r % B);
  int k = (int)(r / B);
  const bool ex = X && c >= C;
  int i = y - off_y, j = x - off_x;
  float val;
  if (i >= 0 && i < h && j >= 0 && j < w) {
    int q = idx[(int64_t)k * h * w + (int64_t)i * w + j];
    int sy = src_row[2 * i + (q >> 1)];
    int sx = src_col[2 * j + (q & 1)];
    if (ex) {
      val = extra[(((int64_t)b * E + (c - C)) * H + sy) * W + sx];
    } else {
      val = latent[(((int64_t)b * C + c) * H + sy) * W + sx];
      if (low) low[((((int64_t)k * B + b) * C + c) * h + i) * w + j] = val;
    }
  } else if (ex) {
    val = pad_value[c - C];
  } else {
    val = frame ? frame[((int64_t)c * PH + y) * PW + x] : 0.0f;
  }
  int64_t plane = (int64_t)PH * PW;
  int64_t e = ((int64_t)c * PH + y) * PW + x;
  for (int q = 0; q < copies; ++q) st<Tag>(out, (((int64_t)k * copies + q) * B + b) * CT * plane + e, val);
}

template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_pick_assemble(const float* __restrict__ latent, const uint8_t* __restrict__ idx,
                const int32_t* __restrict__ src_row, const int32_t* __restrict__ src_col,
                const float* __restrict__ frame, void* __restrict__ out, float* __restrict__ low,
                int K, int B, int C, int H, int W, int h, int w, int PH, int PW, int off_y, int off_x) {
  pick_assemble_body<Tag>((int64_t)blockIdx.x * ED_BLOCK + threadIdx.x, latent, idx, src_row, src_col, frame, out, low, K, B, C, H, W, h, w, PH, PW, off_y, off_x);
}

// 4 consecutive x per thread; requires PW, w, off_x multiples of 4
template <typename Tag, bool X = false>
__device__ __forceinline__ void pick_assemble_x4_body(int64_t t, const float* __restrict__ latent, const uint8_t* __restrict__ idx,
                   const int32_t* __restrict__ src_row, const int32_t* __restrict__ src_col,
                   const float* __restrict__ frame, void* __restrict__ out, float* __restrict__ low,
                   int K, int B, int C, int H, int W, int h, int w, int PH, int PW, int off_y, int off_x,
                   const float* __restrict__ extra = nullptr, int E = 0, const float* __restrict__ pad_value = nullptr,
                   const int copies = 2) {
  const int CT = X ? C + E : C;
  int PW4 = PW >> 2;
  int64_t n = (int64_t)K * B * CT * PH * PW4;
  if (t >= n) return;
  int x = (int)(t % PW4) << 2;
  int64_t r = t / PW4;
  int y = (int)(r % PH);
  r /= PH;
  int c = (int)(r % CT);
  r /= CT;
  int b = (int)(r % B);
  int k = (int)(r / B);
  const bool ex = X && c >= C;
  int i = y - off_y, j = x - off_x;
  float val[4];
  if (i >= 0 && i < h && j >= 0 && j < w) {
    uint32_t q4 = *reinterpret_cast<const uint32_t*>(idx + (int64_t)k * h * w + (int64_t)i * w + j);
    const float* plane = ex ? extra + ((int64_t)b * E + (c - C)) * H * W : latent + ((int64_t)b * C + c) * H * W;
    int r0 = src_row[2 * i], r1 = src_row[2 * i + 1];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int q = (q4 >> (8 * e)) & 0xff;
      int sy = (q >> 1) ? r1 : r0;
      int sx = src_col[2 * (j + e) + (q & 1)];
      val[e] = plane[(int64_t)sy * W + sx];
    }
    if (low && !ex)
      *reinterpret_cast<float4*>(low + ((((int64_t)k * B + b) * C + c) * h + i) * w + j) =
          make_float4(val[0], val[1], val[2], val[3]);
  } else if (ex) {
    val[0] = val[1] = val[2] = val[3] = pad_value[c - C];
  } else if (frame) {
    float4 f = *reinterpret_cast<const float4*>(frame + ((int64_t)c * PH + y) * PW + x);
    val[0] = f.x; val[1] = f.y; val[2] = f.z; val[3] = f.w;
  } else {
    val[0] = val[1] = val[2] = val[3] = 0.0f;
  }
  int64_t plane_sz = (int64_t)PH * PW;
  int64_t e0 = ((int64_t)c * PH + y) * PW + x;
  for (int q = 0; q < copies; ++q)
    st4<Tag>(out, (((int64_t)k * copies + q) * B + b) * CT * plane_sz + e0, val[0], val[1], val[2], val[3]);
}

template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_pick_assemble_x4(const float* __restrict__ latent, const uint8_t* __restrict__ idx,
                   const int32_t* __restrict__ src_row, const int32_t* __restrict__ src_col,
                   const float* __restrict__ frame, void* __restrict__ out, float* __restrict__ low,
                   int K, int B, int C, int H, int W, int h, int w, int PH, int PW, int off_y, int off_x) {
  pick_assemble_x4_body<Tag>((int64_t)blockIdx.x * ED_BLOCK + threadIdx.x, latent, idx, src_row, src_col, frame, out, low, K, B, C, H, W, h, w, PH, PW, off_y, off_x);
}

// ---- ed_unpad_direction ----------------------------------------------------------------------------
template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_unpad_direction(const void* __restrict__ uo, float* __restrict__ dirs, float* __restrict__ uncond_last,
                  int K, int B, int C, int h, int w, int PH, int PW, int off_y, int off_x) {
  int64_t n = (int64_t)K * B * C * h * w;
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  int j = (int)(t % w);
  int64_t r = t / w;
  int i = (int)(r % h);
  r /= h;
  int c = (int)(r % C);
  r /= C;
  int b = (int)(r % B);
  int k = (int)(r / B);
  int64_t plane = (int64_t)PH * PW;
  int64_t e = ((int64_t)c * PH + (i + off_y)) * PW + (j + off_x);
  float u = ld<Tag>(uo, (((int64_t)k * 2 + 0) * B + b) * C * plane + e);
  float cd = ld<Tag>(uo, (((int64_t)k * 2 + 1) * B + b) * C * plane + e);
  dirs[t] = __fsub_rn(cd, u);
  if (uncond_last && k == K - 1) uncond_last[(((int64_t)b * C + c) * h + i) * w + j] = u;
}

// 4 consecutive j per thread; requires w, PW, off_x multiples of 4
template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_unpad_direction_x4(const void* __restrict__ uo, float* __restrict__ dirs, float* __restrict__ uncond_last,
                     int K, int B, int C, int h, int w, int PH, int PW, int off_y, int off_x) {
  int w4 = w >> 2;
  int64_t n = (int64_t)K * B * C * h * w4;
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  int j = (int)(t % w4) << 2;
  int64_t r = t / w4;
  int i = (int)(r % h);
  r /= h;
  int c = (int)(r % C);
  r /= C;
  int b = (int)(r % B);
  int k = (int)(r / B);
  int64_t plane = (int64_t)PH * PW;
  int64_t e = ((int64_t)c * PH + (i + off_y)) * PW + (j + off_x);
  float4 u = ld4<Tag>(uo, (((int64_t)k * 2 + 0) * B + b) * C * plane + e);
  float4 cd = ld4<Tag>(uo, (((int64_t)k * 2 + 1) * B + b) * C * plane + e);
  float4 d = make_float4(__fsub_rn(cd.x, u.x), __fsub_rn(cd.y, u.y), __fsub_rn(cd.z, u.z), __fsub_rn(cd.w, u.w));
  *reinterpret_cast<float4*>(dirs + (t << 2)) = d;
  if (uncond_last && k == K - 1)
    *reinterpret_cast<float4*>(uncond_last + (((int64_t)b * C + c) * h + i) * w + j) = u;
}

// ---- ed_fill_directions ----------------------------------------------------------------------------
// stamp[n*4 + q] = last resampling step whose pick at reduced pixel n was q (int8, -1 = never); built on the host next
// to the draws.  A full-res pixel is covered by step k iff one of its (<= 2 x 2) pick-grid cells (rr,cc) was picked.
__device__ __forceinline__ int last_covering_step(const int8_t* __restrict__ stamp, const int32_t* __restrict__ inv_row,
                                                  const int32_t* __restrict__ inv_col, int K, int w, int Y, int X) {
  int r0 = inv_row[Y * 2], r1 = inv_row[Y * 2 + 1];
  int c0 = inv_col[X * 2], c1 = inv_col[X * 2 + 1];
  int best = -1;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    int rr = a ? r1 : r0;
    if (rr < 0) continue;
#pragma unroll
    for (int bq = 0; bq < 2; ++bq) {
      int cc = bq ? c1 : c0;
      if (cc < 0) continue;
      int k = stamp[((int64_t)(rr >> 1) * w + (cc >> 1)) * 4 + ((rr & 1) * 2 + (cc & 1))];
      best = k > best ? k : best;
    }
  }
  return best < 0 ? K - 1 : best;  // fill_all: what no pick reached takes the last step's upsample (ED:643-644)
}

__global__ void __launch_bounds__(ED_BLOCK)
k_fill_directions(const float* __restrict__ dirs, const int8_t* __restrict__ stamp,
                  const int32_t* __restrict__ inv_row, const int32_t* __restrict__ inv_col,
                  const int32_t* __restrict__ up_row, const int32_t* __restrict__ up_col,
                  const int32_t* __restrict__ down_row, const int32_t* __restrict__ down_col,
                  float* __restrict__ target, float* __restrict__ low_dir,
                  int K, int B, int C, int H, int W, int h, int w) {
  int64_t nfull = (int64_t)H * W;
  int64_t nlow = low_dir ? (int64_t)h * w : 0;
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= nfull + nlow) return;
  int Y, X;
  float* dst;
  int64_t dplane, doff;
  if (t < nfull) {
    Y = (int)(t / W);
    X = (int)(t % W);
    dst = target;
    dplane = nfull;
    doff = t;
  } else {
    int64_t u = t - nfull;
    int i = (int)(u / w), j = (int)(u % w);
    Y = down_row[i];
    X = down_col[j];
    dst = low_dir;
    dplane = (int64_t)h * w;
    doff = u;
  }
  int k = last_covering_step(stamp, inv_row, inv_col, K, w, Y, X);
  int64_t lplane = (int64_t)h * w;
  int64_t src = (int64_t)up_row[Y] * w + up_col[X];
  int BC = B * C;
  for (int bc = 0; bc < BC; ++bc)
    dst[(int64_t)bc * dplane + doff] = dirs[((int64_t)k * BC + bc) * lplane + src];
}

// ---- ed_cfg_ddim_step ------------------------------------------------------------------------------
// VP = the scheduler's prediction_type is "v_prediction": the guided model output m = l + g*d (formed in model-output
// space either way, ED:1031) is a velocity, x0 = sa*x - sb*m and eps = sa*m + sb*x (every product rounded on its own, in
// diffusers' order); otherwise m is the noise and x0 = (x - sb*m) / sa.  A compile-time variant: the epsilon
// instantiations are the code they were before the variant existed.
template <bool VP>
__device__ __forceinline__ float pred_x0(float m, float xv, float sb, float sa) {
  if (VP) return __fsub_rn(__fmul_rn(sa, xv), __fmul_rn(sb, m));
  return __fdiv_rn(__fsub_rn(xv, __fmul_rn(sb, m)), sa);
}

// Guidance rescale (arXiv 2305.08891 section 3.4, the reference's rescale_noise_cfg ED:800-811) on a guided model output m
// of sample b: m <- gr * (m * ratio[b]) + omgr * m, ratio[b] = std(m at g = 1) / std(m) over the sample (k_guidance_moments /
// k_phase_moments below), gr / omgr = float32(guidance_rescale) / float32(1 - guidance_rescale) from the host; every product
// and sum rounded on its own, in the reference's order.  GR is a compile-time variant: the <.., false> instantiations are the
// code they were before it existed and never read `rs`.
struct Rescale {
  const float* ratio;  // [B] on the device
  float gr, omgr;
  int64_t per;         // elements per sample of the flat kernels (k_cfg_ddim_*)
};

template <bool GR>
__device__ __forceinline__ float rescaled(float m, float r, float gr, float omgr) {
  if (!GR) return m;
  return __fadd_rn(__fmul_rn(gr, __fmul_rn(m, r)), __fmul_rn(omgr, m));
}

// The step variant (compile-time): ST_DDIM is the eta = 0 DDIM update and the code it was before the variant
// existed.  ST_MS1 / ST_MS2 are DPM-Solver++(2M), midpoint form, first / second order: x0 is the same pred_x0 of the same guided
// output, and with the host's scalars c_x = sigma_prev / sigma_t (in `sp`), b = alpha_prev * (exp(-h) - 1) (in `sd`), hb = 0.5 * b and
// r_inv = h / h0:   prev = (c_x * x - b * x0) - hb * (r_inv * (x0 - x0_hist)),   left to right, every product rounded on its own; the
// first-order form stops after the first bracket and never reads the history.  Which of the two runs is the host's choice per launch.
enum { ST_DDIM = 0, ST_MS1 = 1, ST_MS2 = 2 };

struct Multistep {
  const float* x0_hist;  // the previous timestep's x0 at the output element's index (ST_MS2 only)
  float hb, r_inv;
};

// The noise variant (compile-time, orthogonal to ST): the stochastic samplers -- DDIM with eta > 0, SDE-DPM-Solver++
// (2M), LCM -- are the deterministic update with other host scalars plus c_n * noise, `noise` one more fp32 operand at the output
// element's index (drawn on the host in the reference's order):   prev = prev + c_n * noise,   the product rounded on its own.  The
// <.., false> instantiations are the code they were before the variant existed; their argument blocks keep their types.
struct MultistepNZ : Multistep {
  const float* noise;
  float c_n;
};
template <bool NZ> struct MultistepOf { typedef Multistep type; };
template <> struct MultistepOf<true> { typedef MultistepNZ type; };

template <bool VP, bool GR = false, int ST = ST_DDIM, bool NZ = false>
__device__ __forceinline__ void ddim_one(float l, float d, float xv, float g, float sb, float sa, float sp, float sd,
                                         float& prev, float& x0, float r = 0.0f, float gr = 0.0f, float omgr = 0.0f,
                                         float x0h = 0.0f, float hb = 0.0f, float r_inv = 0.0f, float c_n = 0.0f,
                                         float nz = 0.0f) {
  float m = rescaled<GR>(__fadd_rn(l, __fmul_rn(g, d)), r, gr, omgr);
  x0 = pred_x0<VP>(m, xv, sb, sa);
  if (ST != ST_DDIM) {
    prev = __fsub_rn(__fmul_rn(sp, xv), __fmul_rn(sd, x0));
    if (ST == ST_MS2) prev = __fsub_rn(prev, __fmul_rn(hb, __fmul_rn(r_inv, __fsub_rn(x0, x0h))));
    if (NZ) prev = __fadd_rn(prev, __fmul_rn(c_n, nz));
    return;
  }
  float eps = VP ? __fadd_rn(__fmul_rn(sa, m), __fmul_rn(sb, xv)) : m;
  prev = __fadd_rn(__fmul_rn(sp, x0), __fmul_rn(sd, eps));
  if (NZ) prev = __fadd_rn(prev, __fmul_rn(c_n, nz));
}

// The <VP, true> instantiation is only launched with rs.per % 4 == 0 (cfg_ddim_x4), so the 4 elements of a thread belong to
// one sample; <VP, false> never reads rs.
template <bool VP, bool GR = false, int ST = ST_DDIM, bool NZ = false>
__global__ void __launch_bounds__(ED_BLOCK)
k_cfg_ddim_v4(const float4* __restrict__ local, const float4* __restrict__ dir, const float4* __restrict__ x,
              float4* __restrict__ prev, float4* __restrict__ x0, float g, float sb, float sa, float sp, float sd,
              int64_t n4, const Rescale rs, const typename MultistepOf<NZ>::type ms) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n4) return;
  float4 l = local[t], d = dir[t], xv = x[t], p, o;
  const float r = GR ? rs.ratio[(t << 2) / rs.per] : 0.0f;
  float4 hx = {0.0f, 0.0f, 0.0f, 0.0f};
  if (ST == ST_MS2) hx = ((const float4*)ms.x0_hist)[t];
  if constexpr (NZ) {
    const float4 nz = ((const float4*)ms.noise)[t];
    ddim_one<VP, GR, ST, true>(l.x, d.x, xv.x, g, sb, sa, sp, sd, p.x, o.x, r, rs.gr, rs.omgr, hx.x, ms.hb, ms.r_inv, ms.c_n, nz.x);
    ddim_one<VP, GR, ST, true>(l.y, d.y, xv.y, g, sb, sa, sp, sd, p.y, o.y, r, rs.gr, rs.omgr, hx.y, ms.hb, ms.r_inv, ms.c_n, nz.y);
    ddim_one<VP, GR, ST, true>(l.z, d.z, xv.z, g, sb, sa, sp, sd, p.z, o.z, r, rs.gr, rs.omgr, hx.z, ms.hb, ms.r_inv, ms.c_n, nz.z);
    ddim_one<VP, GR, ST, true>(l.w, d.w, xv.w, g, sb, sa, sp, sd, p.w, o.w, r, rs.gr, rs.omgr, hx.w, ms.hb, ms.r_inv, ms.c_n, nz.w);
  } else {
    ddim_one<VP, GR, ST>(l.x, d.x, xv.x, g, sb, sa, sp, sd, p.x, o.x, r, rs.gr, rs.omgr, hx.x, ms.hb, ms.r_inv);
    ddim_one<VP, GR, ST>(l.y, d.y, xv.y, g, sb, sa, sp, sd, p.y, o.y, r, rs.gr, rs.omgr, hx.y, ms.hb, ms.r_inv);
    ddim_one<VP, GR, ST>(l.z, d.z, xv.z, g, sb, sa, sp, sd, p.z, o.z, r, rs.gr, rs.omgr, hx.z, ms.hb, ms.r_inv);
    ddim_one<VP, GR, ST>(l.w, d.w, xv.w, g, sb, sa, sp, sd, p.w, o.w, r, rs.gr, rs.omgr, hx.w, ms.hb, ms.r_inv);
  }
  prev[t] = p;
  x0[t] = o;
}

template <bool VP, bool GR = false, int ST = ST_DDIM, bool NZ = false>
__global__ void __launch_bounds__(ED_BLOCK)
k_cfg_ddim_s(const float* __restrict__ local, const float* __restrict__ dir, const float* __restrict__ x,
             float* __restrict__ prev, float* __restrict__ x0, float g, float sb, float sa, float sp, float sd,
             int64_t n, const Rescale rs, const typename MultistepOf<NZ>::type ms) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  float p, o;
  if constexpr (NZ) {
    ddim_one<VP, GR, ST, true>(local[t], dir[t], x[t], g, sb, sa, sp, sd, p, o, GR ? rs.ratio[t / rs.per] : 0.0f, rs.gr, rs.omgr,
                               ST == ST_MS2 ? ms.x0_hist[t] : 0.0f, ms.hb, ms.r_inv, ms.c_n, ms.noise[t]);
  } else {
    ddim_one<VP, GR, ST>(local[t], dir[t], x[t], g, sb, sa, sp, sd, p, o, GR ? rs.ratio[t / rs.per] : 0.0f, rs.gr, rs.omgr,
                         ST == ST_MS2 ? ms.x0_hist[t] : 0.0f, ms.hb, ms.r_inv);
  }
  prev[t] = p;
  x0[t] = o;
}

// ---- ed_assemble_rows: ed_pick_assemble + ed_gather_views in ONE launch ----------------------------
// The first `pick_blocks` workgroups assemble the K CFG pairs, the rest gather the V context crops; both write rows of
// the same fused model batch.  PX4 / GX4: the 4-wide variants (host checks the alignment conditions per part).
struct AssembleArgs {
  const float* latent;
  int B, C, H, W;
  // global (pick) part
  const uint8_t* idx;
  const int32_t *src_row, *src_col;
  const float* gframe;
  void* g_out;
  float* low;
  int K, h, w, gPH, gPW, g_off_y, g_off_x;
  // view part
  const int32_t *win_y0, *win_x0;
  const float* vframe;
  void* v_out;
  int V, Sh, Sw, vPH, vPW, v_off_y, v_off_x;
  int pick_blocks;
};

template <typename Tag, bool PX4, bool GX4>
__global__ void __launch_bounds__(ED_BLOCK)
k_assemble_rows(const AssembleArgs a) {
  if ((int)blockIdx.x < a.pick_blocks) {
    int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (PX4)
      pick_assemble_x4_body<Tag>(t, a.latent, a.idx, a.src_row, a.src_col, a.gframe, a.g_out, a.low, a.K, a.B, a.C, a.H, a.W,
                                 a.h, a.w, a.gPH, a.gPW, a.g_off_y, a.g_off_x);
    else
      pick_assemble_body<Tag>(t, a.latent, a.idx, a.src_row, a.src_col, a.gframe, a.g_out, a.low, a.K, a.B, a.C, a.H, a.W,
                              a.h, a.w, a.gPH, a.gPW, a.g_off_y, a.g_off_x);
  } else {
    int64_t t = (int64_t)((int)blockIdx.x - a.pick_blocks) * ED_BLOCK + threadIdx.x;
    if (GX4)
      gather_windows_x4_body<Tag>(t, a.latent, a.v_out, a.B, a.C, a.H, a.W, a.win_y0, a.win_x0, a.V, a.Sh, a.Sw, a.vPH, a.vPW,
                                  a.v_off_y, a.v_off_x, a.vframe, 1.0f, 0);
    else
      gather_windows_body<Tag>(t, a.latent, a.v_out, a.B, a.C, a.H, a.W, a.win_y0, a.win_x0, a.V, a.Sh, a.Sw, a.vPH, a.vPW,
                               a.v_off_y, a.v_off_x, a.vframe, 1.0f, 0);
  }
}

// ---- ed_assemble_rows_x: ed_assemble_rows on rows of C + E channels (9-channel inpainting UNets) --------
// The same two bodies with the channel loop over C + E: channels C.. gather `extra` through the index map of the row's latent.
struct AssembleArgsX : AssembleArgs {
  const float* extra;      // [B,E,H,W]
  const float* pad_value;  // [E]
  int E;
};

template <typename Tag, bool PX4, bool GX4>
__global__ void __launch_bounds__(ED_BLOCK)
k_assemble_rows_x(const AssembleArgsX a) {
  if ((int)blockIdx.x < a.pick_blocks) {
    int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (PX4)
      pick_assemble_x4_body<Tag, true>(t, a.latent, a.idx, a.src_row, a.src_col, a.gframe, a.g_out, a.low, a.K, a.B, a.C, a.H,
                                       a.W, a.h, a.w, a.gPH, a.gPW, a.g_off_y, a.g_off_x, a.extra, a.E, a.pad_value);
    else
      pick_assemble_body<Tag, true>(t, a.latent, a.idx, a.src_row, a.src_col, a.gframe, a.g_out, a.low, a.K, a.B, a.C, a.H, a.W,
                                    a.h, a.w, a.gPH, a.gPW, a.g_off_y, a.g_off_x, a.extra, a.E, a.pad_value);
  } else {
    int64_t t = (int64_t)((int)blockIdx.x - a.pick_blocks) * ED_BLOCK + threadIdx.x;
    if (GX4)
      gather_windows_x4_body<Tag, true>(t, a.latent, a.v_out, a.B, a.C, a.H, a.W, a.win_y0, a.win_x0, a.V, a.Sh, a.Sw, a.vPH,
                                        a.vPW, a.v_off_y, a.v_off_x, a.vframe, 1.0f, 0, a.extra, a.E, a.pad_value);
    else
      gather_windows_body<Tag, true>(t, a.latent, a.v_out, a.B, a.C, a.H, a.W, a.win_y0, a.win_x0, a.V, a.Sh, a.Sw, a.vPH, a.vPW,
                                     a.v_off_y, a.v_off_x, a.vframe, 1.0f, 0, a.extra, a.E, a.pad_value);
  }
}

// ---- ed_assemble_rows_n: ed_assemble_rows_x with `copies` rows per resampling step and sample (regional prompts, section 28) -----
// The picked vector is gathered once and stored `copies` times; E = 0 (extra NULL) is the 4-channel case.
struct AssembleArgsN : AssembleArgsX {
  int copies;
};

template <typename Tag, bool PX4, bool GX4>
__global__ void __launch_bounds__(ED_BLOCK)
k_assemble_rows_n(const AssembleArgsN a) {
  if ((int)blockIdx.x < a.pick_blocks) {
    int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (PX4)
      pick_assemble_x4_body<Tag, true>(t, a.latent, a.idx, a.src_row, a.src_col, a.gframe, a.g_out, a.low, a.K, a.B, a.C, a.H,
                                       a.W, a.h, a.w, a.gPH, a.gPW, a.g_off_y, a.g_off_x, a.extra, a.E, a.pad_value, a.copies);
    else
      pick_assemble_body<Tag, true>(t, a.latent, a.idx, a.src_row, a.src_col, a.gframe, a.g_out, a.low, a.K, a.B, a.C, a.H, a.W,
                                    a.h, a.w, a.gPH, a.gPW, a.g_off_y, a.g_off_x, a.extra, a.E, a.pad_value, a.copies);
  } else {
    int64_t t = (int64_t)((int)blockIdx.x - a.pick_blocks) * ED_BLOCK + threadIdx.x;
    if (GX4)
      gather_windows_x4_body<Tag, true>(t, a.latent, a.v_out, a.B, a.C, a.H, a.W, a.win_y0, a.win_x0, a.V, a.Sh, a.Sw, a.vPH,
                                        a.vPW, a.v_off_y, a.v_off_x, a.vframe, 1.0f, 0, a.extra, a.E, a.pad_value);
    else
      gather_windows_body<Tag, true>(t, a.latent, a.v_out, a.B, a.C, a.H, a.W, a.win_y0, a.win_x0, a.V, a.Sh, a.Sw, a.vPH, a.vPW,
                                     a.v_off_y, a.v_off_x, a.vframe, 1.0f, 0, a.extra, a.E, a.pad_value);
  }
}

// ---- ed_ip_mask_rows: per-row IP-Adapter attention masks, four pyramid levels in ONE launch ----------
// A workgroup of one wave owns an 8 x 8 patch of level 0 of one (step or view, sample, adapter) plane: lane (ty, tx) gathers its
// pixel exactly as the extra channels of ed_assemble_rows_n are gathered with pad_value = 0, the patch goes to LDS, and 16 / 4 / 1
// lanes form its 4 x 4 / 2 x 2 / 1 pixels of levels 1 / 2 / 3 as 0.25f * ((a + b) + (c + d)), each operation rounded on its own.
// A step's plane is stored `copies` times (the rows of one step share their frame), a view's once.
struct IpMaskArgs {
  const float* masks;  // [B,A,H,W]
  int B, A, H, W;
  const uint8_t* idx;
  const int32_t *src_row, *src_col;
  int K, h, w, g_off_y, g_off_x;
  const int32_t *win_y0, *win_x0;
  int V, Sh, Sw, v_off_y, v_off_x;
  int PH, PW, copies;
  float* m;            // [(K*copies + V)*B, A, S]
  int S, pick_blocks;  // S = sum over the four levels; pick_blocks = K*B*A*(PH/8)*(PW/8)
};

__global__ void __launch_bounds__(64)
k_ip_mask_rows(const IpMaskArgs a) {
  __shared__ float l0[64], l1[16], l2[4];
  const int tid = threadIdx.x, ty = tid >> 3, tx = tid & 7;
  const bool pick = (int)blockIdx.x < a.pick_blocks;
  int r = pick ? (int)blockIdx.x : (int)blockIdx.x - a.pick_blocks;
  const int npx = a.PW >> 3, npy = a.PH >> 3;
  const int px = r % npx;
  r /= npx;
  const int py = r % npy;
  r /= npy;
  const int ad = r % a.A;
  r /= a.A;
  const int b = r % a.B, kv = r / a.B;  // kv: the resampling step or the view
  const int y = 8 * py + ty, x = 8 * px + tx;
  const float* plane = a.masks + ((int64_t)b * a.A + ad) * a.H * a.W;
  float val = 0.0f;
  int sy = -1, sx = -1;
  if (pick) {
    const int i = y - a.g_off_y, j = x - a.g_off_x;
    if (i >= 0 && i < a.h && j >= 0 && j < a.w) {
      const int q = a.idx[(int64_t)kv * a.h * a.w + (int64_t)i * a.w + j];
      sy = a.src_row[2 * i + ((q >> 1) & 1)];
      sx = a.src_col[2 * j + (q & 1)];
    }
  } else {
    const int yy = y - a.v_off_y, xx = x - a.v_off_x;
    if (yy >= 0 && yy < a.Sh && xx >= 0 && xx < a.Sw) sy = a.win_y0[kv] + yy, sx = a.win_x0[kv] + xx;
  }
  if (sy >= 0 && sy < a.H && sx >= 0 && sx < a.W) val = plane[(int64_t)sy * a.W + sx];
  l0[tid] = val;
  __syncthreads();
  float v1 = 0.0f, v2 = 0.0f, v3 = 0.0f;
  if (tid < 16) {
    const int yy = tid >> 2, xx = tid & 3;
    v1 = __fmul_rn(0.25f, __fadd_rn(__fadd_rn(l0[16 * yy + 2 * xx], l0[16 * yy + 2 * xx + 1]),
                                    __fadd_rn(l0[16 * yy + 8 + 2 * xx], l0[16 * yy + 8 + 2 * xx + 1])));
    l1[tid] = v1;
  }
  __syncthreads();
  if (tid < 4) {
    const int yy = tid >> 1, xx = tid & 1;
    v2 = __fmul_rn(0.25f, __fadd_rn(__fadd_rn(l1[8 * yy + 2 * xx], l1[8 * yy + 2 * xx + 1]),
                                    __fadd_rn(l1[8 * yy + 4 + 2 * xx], l1[8 * yy + 4 + 2 * xx + 1])));
    l2[tid] = v2;
  }
  __syncthreads();
  if (tid == 0) v3 = __fmul_rn(0.25f, __fadd_rn(__fadd_rn(l2[0], l2[1]), __fadd_rn(l2[2], l2[3])));
  // level L at offset sum_{l<L} (PH>>l)(PW>>l) of the row's [S] floats
  const int o1 = a.PH * a.PW, o2 = o1 + (o1 >> 2), o3 = o2 + (o1 >> 4);
  const int e0 = y * a.PW + x;
  const int e1 = o1 + (4 * py + (tid >> 2)) * (a.PW >> 1) + 4 * px + (tid & 3);
  const int e2 = o2 + (2 * py + (tid >> 1)) * (a.PW >> 2) + 2 * px + (tid & 1);
  const int e3 = o3 + py * (a.PW >> 3) + px;
  const int n = pick ? a.copies : 1;
  for (int q = 0; q < n; ++q) {
    const int64_t row = pick ? ((int64_t)kv * a.copies + q) * a.B + b : ((int64_t)a.K * a.copies + kv) * a.B + b;
    float* out = a.m + (row * a.A + ad) * a.S;
    out[e0] = val;
    if (tid < 16) out[e1] = v1;
    if (tid < 4) out[e2] = v2;
    if (tid == 0) out[e3] = v3;
  }
}

// ---- ed_phase_epilogue: unpad + fill + scatter + CFG/DDIM (+ RRG) in ONE launch ---------------------
// Everything downstream of the model call is a per-output-pixel gather: which resampling step covers the pixel (stamp
// table) -> cond - uncond of that step's rows; the first non-zero covering view centre; the DDIM update; optionally the
// reduced-resolution-guidance term of ED:886-940 / ED:1078.  Same fp32 operation order as the separate kernels
// (__f*_rn, no contraction): results are bit-identical to ed_unpad_direction -> ed_fill_directions ->
// ed_scatter_centres -> ed_cfg_ddim_step [-> ed_rrg_update].
struct EpilogueArgs {
  const void *g_out, *v_out;
  const float* x;
  const int8_t* stamp;
  const int32_t *inv_row, *inv_col, *up_row, *up_col, *down_row, *down_col;
  const int32_t *row_blk, *row_src, *col_blk, *col_src;
  const float* low_latent;                       // [B,C,h,w] last picked reduced latent (RRG) or NULL
  float *prev, *x0, *x_next, *low_dir, *uncond_last, *direction, *local;  // x_next/direction/local optional
  int K, B, C, H, W, h, w, gPH, gPW, g_off_y, g_off_x, vPH, vPW, ncb;
  float g, sb, sa, sp, sd, rrg_norm, rrg_weight;
  const float *ratio, *ratio_low;  // guidance rescale (GR variants only): [B] each, ratio_low for the fused RRG term
  float gr, omgr;
};

// The argument block of the multistep variants (sp / sd then hold c_x / b).  A type of its own: EpilogueArgs, which the DDIM
// instantiations and k_phase_moments take, keeps its size, so their kernel-argument offsets are what they were.
struct EpilogueArgsMS : EpilogueArgs {
  const float* x0_hist;
  float hb, r_inv;
};
// ... and of the noise variants (section 29), for every ST: again a type of its own.
struct EpilogueArgsNZ : EpilogueArgsMS {
  const float* noise;  // [B,C,H,W]
  float c_n;
};
template <int ST, bool NZ = false> struct EpilogueArgsOf { typedef EpilogueArgsMS type; };
template <> struct EpilogueArgsOf<ST_DDIM, false> { typedef EpilogueArgs type; };
template <int ST> struct EpilogueArgsOf<ST, true> { typedef EpilogueArgsNZ type; };

template <typename Tag>
__device__ __forceinline__ float direction_at(const EpilogueArgs& a, int b, int c, int Y, int X) {
  int k = last_covering_step(a.stamp, a.inv_row, a.inv_col, a.K, a.w, Y, X);
  int64_t plane = (int64_t)a.gPH * a.gPW;
  int64_t e = ((int64_t)c * a.gPH + (a.up_row[Y] + a.g_off_y)) * a.gPW + (a.up_col[X] + a.g_off_x);
  float u = ld<Tag>(a.g_out, (((int64_t)k * 2 + 0) * a.B + b) * a.C * plane + e);
  float cd = ld<Tag>(a.g_out, (((int64_t)k * 2 + 1) * a.B + b) * a.C * plane + e);
  return __fsub_rn(cd, u);
}

// local unconditional score: first covering view whose centre value is non-zero (ED:852-861)
template <typename Tag>
__device__ __forceinline__ float local_at(const EpilogueArgs& a, int b, int c, int Y, int X) {
  float loc = 0.0f;
  bool settled = false;
#pragma unroll
  for (int kr = 0; kr < 2; ++kr) {
    int rb = a.row_blk[Y * 2 + kr];
    if (rb < 0 || settled) continue;
    int sy = a.row_src[Y * 2 + kr];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      int cb = a.col_blk[X * 2 + kc];
      if (cb < 0 || settled) continue;
      int sx = a.col_src[X * 2 + kc];
      int64_t row = (int64_t)(rb * a.ncb + cb) * a.B + b;
      loc = ld<Tag>(a.v_out, ((row * a.C + c) * a.vPH + sy) * a.vPW + sx);
      if (loc != 0.0f) settled = true;
    }
  }
  return loc;
}

// the last resampling step's unconditional output at reduced pixel (i, j) (ed_unpad_direction's uncond_last)
template <typename Tag>
__device__ __forceinline__ float uncond_last_at(const EpilogueArgs& a, int b, int c, int i, int j) {
  int64_t plane = (int64_t)a.gPH * a.gPW;
  int64_t e = ((int64_t)c * a.gPH + (i + a.g_off_y)) * a.gPW + (j + a.g_off_x);
  return ld<Tag>(a.g_out, (((int64_t)(a.K - 1) * 2 + 0) * a.B + b) * a.C * plane + e);
}

template <typename Tag, bool VP, bool GR = false, int ST = ST_DDIM, bool NZ = false>
__global__ void __launch_bounds__(ED_BLOCK)
k_phase_epilogue(const typename EpilogueArgsOf<ST, NZ>::type a) {
  const int64_t nfull = (int64_t)a.B * a.C * a.H * a.W;
  const int64_t nlow = (int64_t)a.B * a.C * a.h * a.w;
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= nfull + nlow) return;
  if (t >= nfull) {  // reduced-resolution by-products for RRG / the caller: direction sampled at the nearest-downsample points
    int64_t u = t - nfull;
    int j = (int)(u % a.w);
    int64_t r = u / a.w;
    int i = (int)(r % a.h);
    r /= a.h;
    int c = (int)(r % a.C);
    int b = (int)(r / a.C);
    if (a.low_dir) a.low_dir[u] = direction_at<Tag>(a, b, c, a.down_row[i], a.down_col[j]);
    if (a.uncond_last) a.uncond_last[u] = uncond_last_at<Tag>(a, b, c, i, j);
    return;
  }
  int X = (int)(t % a.W);
  int64_t r = t / a.W;
  int Y = (int)(r % a.H);
  r /= a.H;
  int c = (int)(r % a.C);
  int b = (int)(r / a.C);
  float loc = local_at<Tag>(a, b, c, Y, X);
  float d = direction_at<Tag>(a, b, c, Y, X);
  float pv, z0;
  if constexpr (NZ) {  // x_next below is formed from the prev that carries the noise
    float x0h = 0.0f;
    if constexpr (ST == ST_MS2) x0h = a.x0_hist[t];
    ddim_one<VP, GR, ST, true>(loc, d, a.x[t], a.g, a.sb, a.sa, a.sp, a.sd, pv, z0, GR ? a.ratio[b] : 0.0f, a.gr, a.omgr, x0h, a.hb,
                               a.r_inv, a.c_n, a.noise[t]);
  } else if constexpr (ST == ST_DDIM) {
    ddim_one<VP, GR>(loc, d, a.x[t], a.g, a.sb, a.sa, a.sp, a.sd, pv, z0, GR ? a.ratio[b] : 0.0f, a.gr, a.omgr);
  } else {
    float x0h = 0.0f;
    if constexpr (ST == ST_MS2) x0h = a.x0_hist[t];
    ddim_one<VP, GR, ST>(loc, d, a.x[t], a.g, a.sb, a.sa, a.sp, a.sd, pv, z0, GR ? a.ratio[b] : 0.0f, a.gr, a.omgr, x0h, a.hb,
                         a.r_inv);
  }
  a.prev[t] = pv;
  a.x0[t] = z0;
  if (a.direction) a.direction[t] = d;
  if (a.local) a.local[t] = loc;
  if (a.x_next) {  // ED:886-940 closed form + ED:1078, as k_rrg_update
    int i = a.up_row[Y], j = a.up_col[X];
    float lu = uncond_last_at<Tag>(a, b, c, i, j);
    float ldir = direction_at<Tag>(a, b, c, a.down_row[i], a.down_col[j]);
    float m = rescaled<GR>(__fadd_rn(lu, __fmul_rn(a.g, ldir)), GR ? a.ratio_low[b] : 0.0f, a.gr, a.omgr);
    float up = pred_x0<VP>(m, a.low_latent[(((int64_t)b * a.C + c) * a.h + i) * a.w + j], a.sb, a.sa);
    float grad = __fmul_rn(__fmul_rn(a.rrg_norm, __fsub_rn(z0, up)), a.rrg_weight);
    a.x_next[t] = __fadd_rn(pv, -grad);
  }
}

// ---- ed_guidance_moments / ed_phase_moments: the per-sample std ratio of the guidance rescale -------------------
// ratio[b] = std(m_text[b]) / std(m_cfg[b]) over all elements of sample b (unbiased, torch.std's default), m_cfg = l + g*d
// and m_text = l + d as fp32 values.  Deterministic two-step reduction, no atomics: a fixed number of blocks per sample
// (moments_blocks(n)) each write ONE partial -- Welford triples (count, mean, M2) of both quantities, 6 doubles -- into the
// caller's workspace; k_moments_finalise merges a sample's partials in a fixed order.  Accumulation is in fp64 and
// shifted: each thread sums x - K and (x - K)^2 with K its own first element, so nothing is lost to cancellation however
// large the mean is next to the spread (the GroupNorm kernels' idiom, unet_kernels.hip), and the triples are merged with
// Chan's formula like merge() there.
#define ED_MOM_MAX_BLOCKS 256
#define ED_MOM_PER_THREAD 4

struct WelfordD {
  double n, mean, m2;
};
__device__ __forceinline__ WelfordD merge_d(WelfordD a, WelfordD b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  double n = a.n + b.n;
  double d = b.mean - a.mean;
  WelfordD r;
  r.n = n;
  r.mean = a.mean + d * (b.n / n);
  r.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / n);
  return r;
}
__device__ __forceinline__ WelfordD shfl_down_d(WelfordD w, int off) {
  WelfordD o;
  o.n = __shfl_down(w.n, off, 64);
  o.mean = __shfl_down(w.mean, off, 64);
  o.m2 = __shfl_down(w.m2, off, 64);
  return o;
}

struct PairAcc {  // one thread's shifted sums of m_cfg (c) and m_text (t)
  double n = 0.0, kc = 0.0, kt = 0.0, sc = 0.0, ssc = 0.0, st = 0.0, sst = 0.0;
  __device__ __forceinline__ void add(float l, float d, float g) { add_pair(__fadd_rn(l, __fmul_rn(g, d)), __fadd_rn(l, d)); }
  __device__ __forceinline__ void add_pair(float mc, float mt) {
    if (n == 0.0) kc = (double)mc, kt = (double)mt;
    double a = (double)mc - kc, b = (double)mt - kt;
    sc += a, ssc += a * a, st += b, sst += b * b, n += 1.0;
  }
  __device__ __forceinline__ WelfordD get(bool cfg) const {
    WelfordD w = {n, 0.0, 0.0};
    if (n > 0.0) {
      double s = cfg ? sc : st, ss = cfg ? ssc : sst, mu = s / n;
      w.mean = (cfg ? kc : kt) + mu;
      w.m2 = fmax(ss - s * mu, 0.0);
    }
    return w;
  }
};

// block-wide merge (wave shuffles, then the 4 wave results in order); thread 0 writes the block's partial
__device__ __forceinline__ void moments_block_store(const PairAcc& acc, double* __restrict__ partial) {
  WelfordD wc = acc.get(true), wt = acc.get(false);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    wc = merge_d(wc, shfl_down_d(wc, off));
    wt = merge_d(wt, shfl_down_d(wt, off));
  }
  __shared__ WelfordD part[2][ED_BLOCK / 64];
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[0][wave] = wc, part[1][wave] = wt;
  __syncthreads();
  if (threadIdx.x == 0) {
    wc = part[0][0], wt = part[1][0];
    for (int k = 1; k < ED_BLOCK / 64; ++k) wc = merge_d(wc, part[0][k]), wt = merge_d(wt, part[1][k]);
    partial[0] = wc.n, partial[1] = wc.mean, partial[2] = wc.m2;
    partial[3] = wt.n, partial[4] = wt.mean, partial[5] = wt.m2;
  }
}

// grid = B * nblk: block (b, k) strides over sample b's n elements.  text (optional): m_text given as a tensor (plain CFG,
// where it is the conditional prediction itself) instead of local + direction.
__global__ void __launch_bounds__(ED_BLOCK)
k_guidance_moments(const float* __restrict__ local, const float* __restrict__ dir, const float* __restrict__ text, float g,
                   int64_t n, int nblk, double* __restrict__ partials) {
  const int b = blockIdx.x / nblk, k = blockIdx.x % nblk;
  const float* l = local + (int64_t)b * n;
  const float* d = dir + (int64_t)b * n;
  PairAcc acc;
  for (int64_t i = (int64_t)k * ED_BLOCK + threadIdx.x; i < n; i += (int64_t)nblk * ED_BLOCK) {
    if (text) acc.add_pair(__fadd_rn(l[i], __fmul_rn(g, d[i])), text[(int64_t)b * n + i]);
    else acc.add(l[i], d[i], g);
  }
  moments_block_store(acc, partials + (int64_t)blockIdx.x * 6);
}

// The same statistics over the gathers of k_phase_epilogue (direction / local never exist in memory): the first B * nblk_full
// blocks reduce local + g * direction over (C,H,W), the next B * nblk_low blocks (present when ratio_low is wanted) the
// reduced-resolution pair uncond_last + g * low_dir of the fused RRG term over (C,h,w).
template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_phase_moments(const EpilogueArgs a, int nblk_full, int nblk_low, double* __restrict__ partials) {
  PairAcc acc;
  const int full_blocks = a.B * nblk_full;
  if ((int)blockIdx.x < full_blocks) {
    const int b = blockIdx.x / nblk_full, k = blockIdx.x % nblk_full;
    const int64_t n = (int64_t)a.C * a.H * a.W;
    for (int64_t i = (int64_t)k * ED_BLOCK + threadIdx.x; i < n; i += (int64_t)nblk_full * ED_BLOCK) {
      int X = (int)(i % a.W);
      int64_t r = i / a.W;
      int Y = (int)(r % a.H), c = (int)(r / a.H);
      acc.add(local_at<Tag>(a, b, c, Y, X), direction_at<Tag>(a, b, c, Y, X), a.g);
    }
  } else {
    const int q = (int)blockIdx.x - full_blocks;
    const int b = q / nblk_low, k = q % nblk_low;
    const int64_t n = (int64_t)a.C * a.h * a.w;
    for (int64_t i = (int64_t)k * ED_BLOCK + threadIdx.x; i < n; i += (int64_t)nblk_low * ED_BLOCK) {
      int j = (int)(i % a.w);
      int64_t r = i / a.w;
      int ii = (int)(r % a.h), c = (int)(r / a.h);
      acc.add(uncond_last_at<Tag>(a, b, c, ii, j), direction_at<Tag>(a, b, c, a.down_row[ii], a.down_col[j]), a.g);
    }
  }
  moments_block_store(acc, partials + (int64_t)blockIdx.x * 6);
}

// grid = B (+ B for the reduced-resolution pair), one wave each: lane l merges partials l, l + 64, ... in order, then a
// shuffle tree; ratio = fp32(std_text) / fp32(std_cfg), one fp32 division.
__global__ void __launch_bounds__(64)
k_moments_finalise(const double* __restrict__ partials, int B, int nblk_full, int nblk_low, float* __restrict__ ratio,
                   float* __restrict__ ratio_low) {
  const bool low = (int)blockIdx.x >= B;
  const int b = low ? (int)blockIdx.x - B : (int)blockIdx.x;
  const int nblk = low ? nblk_low : nblk_full;
  const double* p = partials + ((low ? (int64_t)B * nblk_full : 0) + (int64_t)b * nblk) * 6;
  WelfordD wc = {0.0, 0.0, 0.0}, wt = {0.0, 0.0, 0.0};
  for (int k = threadIdx.x; k < nblk; k += 64) {
    wc = merge_d(wc, WelfordD{p[k * 6 + 0], p[k * 6 + 1], p[k * 6 + 2]});
    wt = merge_d(wt, WelfordD{p[k * 6 + 3], p[k * 6 + 4], p[k * 6 + 5]});
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    wc = merge_d(wc, shfl_down_d(wc, off));
    wt = merge_d(wt, shfl_down_d(wt, off));
  }
  if (threadIdx.x == 0) {
    float std_cfg = (float)sqrt(wc.m2 / (wc.n - 1.0)), std_text = (float)sqrt(wt.m2 / (wt.n - 1.0));
    (low ? ratio_low : ratio)[b] = __fdiv_rn(std_text, std_cfg);
  }
}

inline int moments_blocks(int64_t n) {
  int64_t g = (n + (int64_t)ED_BLOCK * ED_MOM_PER_THREAD - 1) / ((int64_t)ED_BLOCK * ED_MOM_PER_THREAD);
  return (int)(g < 1 ? 1 : (g > ED_MOM_MAX_BLOCKS ? ED_MOM_MAX_BLOCKS : g));
}

// ---- regional prompts ------------------------------------------------------------------
// A step of the model batch holds 1 + P rows per sample, uncond first and then the P cond rows (base prompt, regions); the class
// direction of a pixel is the weighted sum of the P directions cond_p - uncond with the per-pixel weights region_w [P,H,W] of
// k_region_weights.  A term whose weight is 0 is skipped -- its row is not read -- and the first term that is not starts the sum, so
// one-hot weights give the bits of that region's own direction.  Everything downstream is k_phase_epilogue's.  The argument block
// is a type of its own (as EpilogueArgsMS): the blocks of the non-regional instantiations keep their sizes.
#define ED_MAX_REGION_ROWS 8

struct EpilogueArgsRG : EpilogueArgsMS {
  const float* region_w;  // [P,H,W]
  int P;
};

template <typename Tag>
__device__ __forceinline__ float direction_rg_at(const EpilogueArgsRG& a, int b, int c, int Y, int X) {
  int k = last_covering_step(a.stamp, a.inv_row, a.inv_col, a.K, a.w, Y, X);
  int64_t plane = (int64_t)a.gPH * a.gPW, wplane = (int64_t)a.H * a.W;
  int64_t e = ((int64_t)c * a.gPH + (a.up_row[Y] + a.g_off_y)) * a.gPW + (a.up_col[X] + a.g_off_x);
  const int64_t row0 = (int64_t)k * (1 + a.P);
  const float* wp = a.region_w + (int64_t)Y * a.W + X;
  float u = 0.0f, d = 0.0f;
  bool any = false;
  for (int p = 0; p < a.P; ++p) {
    float wv = wp[p * wplane];
    if (wv == 0.0f) continue;
    if (!any) u = ld<Tag>(a.g_out, ((row0 + 0) * a.B + b) * a.C * plane + e);
    float cd = ld<Tag>(a.g_out, ((row0 + 1 + p) * a.B + b) * a.C * plane + e);
    float term = __fmul_rn(wv, __fsub_rn(cd, u));
    d = any ? __fadd_rn(d, term) : term;
    any = true;
  }
  return d;
}

template <typename Tag>
__device__ __forceinline__ float uncond_last_rg_at(const EpilogueArgsRG& a, int b, int c, int i, int j) {
  int64_t plane = (int64_t)a.gPH * a.gPW;
  int64_t e = ((int64_t)c * a.gPH + (i + a.g_off_y)) * a.gPW + (j + a.g_off_x);
  return ld<Tag>(a.g_out, (((int64_t)(a.K - 1) * (1 + a.P) + 0) * a.B + b) * a.C * plane + e);
}

// k_phase_epilogue with the regional direction: same thread mapping, same operation order after `d`
template <typename Tag, bool VP, bool GR, int ST>
__global__ void __launch_bounds__(ED_BLOCK)
k_phase_epilogue_rg(const EpilogueArgsRG a) {
  const int64_t nfull = (int64_t)a.B * a.C * a.H * a.W;
  const int64_t nlow = (int64_t)a.B * a.C * a.h * a.w;
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= nfull + nlow) return;
  if (t >= nfull) {
    int64_t u = t - nfull;
    int j = (int)(u % a.w);
    int64_t r = u / a.w;
    int i = (int)(r % a.h);
    r /= a.h;
    int c = (int)(r % a.C);
    int b = (int)(r / a.C);
    if (a.low_dir) a.low_dir[u] = direction_rg_at<Tag>(a, b, c, a.down_row[i], a.down_col[j]);
    if (a.uncond_last) a.uncond_last[u] = uncond_last_rg_at<Tag>(a, b, c, i, j);
    return;
  }
  int X = (int)(t % a.W);
  int64_t r = t / a.W;
  int Y = (int)(r % a.H);
  r /= a.H;
  int c = (int)(r % a.C);
  int b = (int)(r / a.C);
  float loc = local_at<Tag>(a, b, c, Y, X);
  float d = direction_rg_at<Tag>(a, b, c, Y, X);
  float pv, z0, x0h = 0.0f;
  if constexpr (ST == ST_MS2) x0h = a.x0_hist[t];
  ddim_one<VP, GR, ST>(loc, d, a.x[t], a.g, a.sb, a.sa, a.sp, a.sd, pv, z0, GR ? a.ratio[b] : 0.0f, a.gr, a.omgr, x0h, a.hb, a.r_inv);
  a.prev[t] = pv;
  a.x0[t] = z0;
  if (a.direction) a.direction[t] = d;
  if (a.local) a.local[t] = loc;
  if (a.x_next) {
    int i = a.up_row[Y], j = a.up_col[X];
    float lu = uncond_last_rg_at<Tag>(a, b, c, i, j);
    float ldir = direction_rg_at<Tag>(a, b, c, a.down_row[i], a.down_col[j]);
    float m = rescaled<GR>(__fadd_rn(lu, __fmul_rn(a.g, ldir)), GR ? a.ratio_low[b] : 0.0f, a.gr, a.omgr);
    float up = pred_x0<VP>(m, a.low_latent[(((int64_t)b * a.C + c) * a.h + i) * a.w + j], a.sb, a.sa);
    float grad = __fmul_rn(__fmul_rn(a.rrg_norm, __fsub_rn(z0, up)), a.rrg_weight);
    a.x_next[t] = __fadd_rn(pv, -grad);
  }
}

// k_phase_moments over the regional direction
template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_phase_moments_rg(const EpilogueArgsRG a, int nblk_full, int nblk_low, double* __restrict__ partials) {
  PairAcc acc;
  const int full_blocks = a.B * nblk_full;
  if ((int)blockIdx.x < full_blocks) {
    const int b = blockIdx.x / nblk_full, k = blockIdx.x % nblk_full;
    const int64_t n = (int64_t)a.C * a.H * a.W;
    for (int64_t i = (int64_t)k * ED_BLOCK + threadIdx.x; i < n; i += (int64_t)nblk_full * ED_BLOCK) {
      int X = (int)(i % a.W);
      int64_t r = i / a.W;
      int Y = (int)(r % a.H), c = (int)(r / a.H);
      acc.add(local_at<Tag>(a, b, c, Y, X), direction_rg_at<Tag>(a, b, c, Y, X), a.g);
    }
  } else {
    const int q = (int)blockIdx.x - full_blocks;
    const int b = q / nblk_low, k = q % nblk_low;
    const int64_t n = (int64_t)a.C * a.h * a.w;
    for (int64_t i = (int64_t)k * ED_BLOCK + threadIdx.x; i < n; i += (int64_t)nblk_low * ED_BLOCK) {
      int j = (int)(i % a.w);
      int64_t r = i / a.w;
      int ii = (int)(r % a.h), c = (int)(r / a.h);
      acc.add(uncond_last_rg_at<Tag>(a, b, c, ii, j), direction_rg_at<Tag>(a, b, c, a.down_row[ii], a.down_col[j]), a.g);
    }
  }
  moments_block_store(acc, partials + (int64_t)blockIdx.x * 6);
}

// ed_region_weights: n masks u8 [n,HW] and their weights -> w f32 [n + 1,HW], plane 0 the base prompt's.  r_p = weight_p * (m_p / 255),
// s = r_1 + .. + r_n in order, r_0 = max(0, 1 - s), tot = r_0 + s (>= 1 up to rounding, never 0), w_p = r_p / tot.
struct RegionWeightArgs {
  float weight[ED_MAX_REGION_ROWS - 1];
};

__device__ __forceinline__ void region_weights_one(const uint32_t* m, const RegionWeightArgs& rw, int n, float* out) {
  float r[ED_MAX_REGION_ROWS - 1];
  float s = 0.0f;
#pragma unroll
  for (int p = 0; p < ED_MAX_REGION_ROWS - 1; ++p) {
    if (p < n) {
      r[p] = __fmul_rn(rw.weight[p], __fdiv_rn((float)m[p], 255.0f));
      s = p ? __fadd_rn(s, r[p]) : r[p];
    }
  }
  float r0 = fmaxf(0.0f, __fsub_rn(1.0f, s));
  float tot = __fadd_rn(r0, s);
  out[0] = __fdiv_rn(r0, tot);
#pragma unroll
  for (int p = 0; p < ED_MAX_REGION_ROWS - 1; ++p)
    if (p < n) out[1 + p] = __fdiv_rn(r[p], tot);
}

__global__ void __launch_bounds__(ED_BLOCK)
k_region_weights(const uint8_t* __restrict__ masks, const RegionWeightArgs rw, int n, int64_t HW, float* __restrict__ w) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= HW) return;
  uint32_t m[ED_MAX_REGION_ROWS - 1];
  float out[ED_MAX_REGION_ROWS];
#pragma unroll
  for (int p = 0; p < ED_MAX_REGION_ROWS - 1; ++p) m[p] = p < n ? masks[p * HW + t] : 0u;
  region_weights_one(m, rw, n, out);
#pragma unroll
  for (int p = 0; p < ED_MAX_REGION_ROWS; ++p)
    if (p <= n) w[p * HW + t] = out[p];
}

// 4 consecutive pixels per thread: one 4-byte load per mask, one 16-byte store per plane; requires HW % 4 == 0
__global__ void __launch_bounds__(ED_BLOCK)
k_region_weights_x4(const uint32_t* __restrict__ masks, const RegionWeightArgs rw, int n, int64_t HW4, float4* __restrict__ w) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= HW4) return;
  uint32_t pk[ED_MAX_REGION_ROWS - 1];
#pragma unroll
  for (int p = 0; p < ED_MAX_REGION_ROWS - 1; ++p) pk[p] = p < n ? masks[p * HW4 + t] : 0u;
  float out[4][ED_MAX_REGION_ROWS];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    uint32_t m[ED_MAX_REGION_ROWS - 1];
#pragma unroll
    for (int p = 0; p < ED_MAX_REGION_ROWS - 1; ++p) m[p] = (pk[p] >> (8 * e)) & 0xffu;
    region_weights_one(m, rw, n, out[e]);
  }
#pragma unroll
  for (int p = 0; p < ED_MAX_REGION_ROWS; ++p)
    if (p <= n) w[p * HW4 + t] = make_float4(out[0][p], out[1][p], out[2][p], out[3][p]);
}

// ed_region_blend (the un-fused path): out[bc, i] = sum_p w[p, i] * dirs[p, bc, i] with direction_rg_at's skip rule and order
__device__ __forceinline__ float region_blend_one(const float* __restrict__ dirs, const float* __restrict__ w, int P, int64_t dstride,
                                                   int64_t wstride, int64_t di, int64_t wi) {
  float d = 0.0f;
  bool any = false;
  for (int p = 0; p < P; ++p) {
    float wv = w[p * wstride + wi];
    if (wv == 0.0f) continue;
    float term = __fmul_rn(wv, dirs[p * dstride + di]);
    d = any ? __fadd_rn(d, term) : term;
    any = true;
  }
  return d;
}

__global__ void __launch_bounds__(ED_BLOCK)
k_region_blend(const float* __restrict__ dirs, const float* __restrict__ w, float* __restrict__ out, int P, int64_t n, int64_t HW) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  out[t] = region_blend_one(dirs, w, P, n, HW, t, t % HW);
}

// 4 consecutive elements per thread; requires HW % 4 == 0 (a group lies in one plane) and 16-byte aligned buffers
__global__ void __launch_bounds__(ED_BLOCK)
k_region_blend_v4(const float4* __restrict__ dirs, const float4* __restrict__ w, float4* __restrict__ out, int P, int64_t n4,
                  int64_t HW4) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n4) return;
  int64_t wi = t % HW4;
  float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  bool any[4] = {false, false, false, false};
  for (int p = 0; p < P; ++p) {
    float4 wv4 = w[p * HW4 + wi];
    if (wv4.x == 0.0f && wv4.y == 0.0f && wv4.z == 0.0f && wv4.w == 0.0f) continue;
    float4 dv4 = dirs[p * n4 + t];
    float wv[4] = {wv4.x, wv4.y, wv4.z, wv4.w}, dv[4] = {dv4.x, dv4.y, dv4.z, dv4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (wv[e] == 0.0f) continue;
      float term = __fmul_rn(wv[e], dv[e]);
      d[e] = any[e] ? __fadd_rn(d[e], term) : term;
      any[e] = true;
    }
  }
  out[t] = make_float4(d[0], d[1], d[2], d[3]);
}

// ---- ed_undo_step ----------------------------------------------------------------------------------
// n_sub independent 16-byte loads per lane are issued before the dependent chain -> deep memory-level parallelism.
__global__ void __launch_bounds__(ED_BLOCK)
k_undo_v4(const float4* __restrict__ x_in, const float4* __restrict__ noise, const float2* __restrict__ coef,
          float4* __restrict__ x_out, int n_sub, int64_t n4) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n4) return;
  float4 xv = x_in[t];
  int k = 0;
  for (; k + 4 <= n_sub; k += 4) {
    float4 z0 = noise[(int64_t)(k + 0) * n4 + t];
    float4 z1 = noise[(int64_t)(k + 1) * n4 + t];
    float4 z2 = noise[(int64_t)(k + 2) * n4 + t];
    float4 z3 = noise[(int64_t)(k + 3) * n4 + t];
    float2 c0 = coef[k], c1 = coef[k + 1], c2 = coef[k + 2], c3 = coef[k + 3];
#define ED_UNDO(NZ, CF)                                             \
  xv.x = __fadd_rn(__fmul_rn(CF.x, xv.x), __fmul_rn(CF.y, NZ.x)); \
  xv.y = __fadd_rn(__fmul_rn(CF.x, xv.y), __fmul_rn(CF.y, NZ.y)); \
  xv.z = __fadd_rn(__fmul_rn(CF.x, xv.z), __fmul_rn(CF.y, NZ.z)); \
  xv.w = __fadd_rn(__fmul_rn(CF.x, xv.w), __fmul_rn(CF.y, NZ.w));
    ED_UNDO(z0, c0) ED_UNDO(z1, c1) ED_UNDO(z2, c2) ED_UNDO(z3, c3)
  }
  for (; k < n_sub; ++k) {
    float4 z = noise[(int64_t)k * n4 + t];
    float2 c = coef[k];
    ED_UNDO(z, c)
  }
#undef ED_UNDO
  x_out[t] = xv;
}

__global__ void __launch_bounds__(ED_BLOCK)
k_undo_s(const float* __restrict__ x_in, const float* __restrict__ noise, const float2* __restrict__ coef,
         float* __restrict__ x_out, int n_sub, int64_t n) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  float xv = x_in[t];
  for (int k = 0; k < n_sub; ++k) {
    float2 c = coef[k];
    xv = __fadd_rn(__fmul_rn(c.x, xv), __fmul_rn(c.y, noise[(int64_t)k * n + t]));
  }
  x_out[t] = xv;
}

// ---- ed_rrg_update ---------------------------------------------------------------------------------
template <bool VP, bool GR = false>
__global__ void __launch_bounds__(ED_BLOCK)
k_rrg_update(const float* __restrict__ prev, const float* __restrict__ x0, const float* __restrict__ low_latent,
             const float* __restrict__ low_uncond, const float* __restrict__ low_dir,
             const int32_t* __restrict__ up_row, const int32_t* __restrict__ up_col, float* __restrict__ out,
             float g, float sb, float sa, float norm, float weight, int B, int C, int H, int W, int h, int w,
             const Rescale rs) {
  int64_t n = (int64_t)B * C * H * W;
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  int X = (int)(t % W);
  int64_t r = t / W;
  int Y = (int)(r % H);
  int64_t bc = r / H;
  int64_t s = (bc * h + up_row[Y]) * w + up_col[X];
  float m = rescaled<GR>(__fadd_rn(low_uncond[s], __fmul_rn(g, low_dir[s])), GR ? rs.ratio[bc / C] : 0.0f, rs.gr, rs.omgr);
  float up = pred_x0<VP>(m, low_latent[s], sb, sa);
  float grad = __fmul_rn(__fmul_rn(norm, __fsub_rn(x0[t], up)), weight);  // d/dx0 of weight*mse(up, x0)
  out[t] = __fadd_rn(prev[t], -grad);
}

template <bool VP, bool GR = false>
__global__ void __launch_bounds__(ED_BLOCK)
k_rrg_update_x4(const float* __restrict__ prev, const float* __restrict__ x0, const float* __restrict__ low_latent,
                const float* __restrict__ low_uncond, const float* __restrict__ low_dir,
                const int32_t* __restrict__ up_row, const int32_t* __restrict__ up_col, float* __restrict__ out,
                float g, float sb, float sa, float norm, float weight, int B, int C, int H, int W, int h, int w,
                const Rescale rs) {
  int W4 = W >> 2;
  int64_t n = (int64_t)B * C * H * W4;
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  int X = (int)(t % W4) << 2;
  int64_t r = t / W4;
  int Y = (int)(r % H);
  int64_t bc = r / H;
  int64_t base = (bc * h + up_row[Y]) * w;
  float4 p = *reinterpret_cast<const float4*>(prev + (t << 2));
  float4 z = *reinterpret_cast<const float4*>(x0 + (t << 2));
  float pv[4] = {p.x, p.y, p.z, p.w}, zv[4] = {z.x, z.y, z.z, z.w}, o[4];
  const float rt = GR ? rs.ratio[bc / C] : 0.0f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    int64_t s = base + up_col[X + e];
    float m = rescaled<GR>(__fadd_rn(low_uncond[s], __fmul_rn(g, low_dir[s])), rt, rs.gr, rs.omgr);
    float up = pred_x0<VP>(m, low_latent[s], sb, sa);
    float grad = __fmul_rn(__fmul_rn(norm, __fsub_rn(zv[e], up)), weight);
    o[e] = __fadd_rn(pv[e], -grad);
  }
  *reinterpret_cast<float4*>(out + (t << 2)) = make_float4(o[0], o[1], o[2], o[3]);
}

// ---- ed_gather2d -----------------------------------------------------------------------------------
template <typename TI, typename TO>
__global__ void __launch_bounds__(ED_BLOCK)
k_gather2d(const void* __restrict__ in, void* __restrict__ out, int C, int H, int W,
           const int32_t* __restrict__ src_n, const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
           int N, int oh, int ow) {
  int64_t n = (int64_t)N * C * oh * ow;
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  int j = (int)(t % ow);
  int64_t r = t / ow;
  int i = (int)(r % oh);
  r /= oh;
  int c = (int)(r % C);
  int m = (int)(r / C);
  int sy = rows[(int64_t)m * oh + i], sx = cols[(int64_t)m * ow + j];
  float v = 0.0f;
  if (sy >= 0 && sx >= 0) v = ld<TI>(in, (((int64_t)src_n[m] * C + c) * H + sy) * W + sx);
  st<TO>(out, t, v);
}

// ---- ed_tile_accumulate_normalise ------------------------------------------------------------------
template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_tile_accumulate(const void* __restrict__ dec, float* __restrict__ image, int B, int Cimg, int HP, int WP, int TP,
                  int nct, const int32_t* __restrict__ row_tile, const int32_t* __restrict__ row_src,
                  const int32_t* __restrict__ col_tile, const int32_t* __restrict__ col_src) {
  int64_t n = (int64_t)B * Cimg * HP * WP;
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  int X = (int)(t % WP);
  int64_t r = t / WP;
  int Y = (int)(r % HP);
  r /= HP;
  int c = (int)(r % Cimg);
  int b = (int)(r / Cimg);
  float sum = 0.0f, cnt = 0.0f;
  for (int kr = 0; kr < ED_TILE_MAXC; ++kr) {
    int rb = row_tile[Y * ED_TILE_MAXC + kr];
    if (rb < 0) break;
    int sy = row_src[Y * ED_TILE_MAXC + kr];
    for (int kc = 0; kc < ED_TILE_MAXC; ++kc) {
      int cb = col_tile[X * ED_TILE_MAXC + kc];
      if (cb < 0) break;
      int sx = col_src[X * ED_TILE_MAXC + kc];
      int64_t row = (int64_t)(rb * nct + cb) * B + b;
      float v = ld<Tag>(dec, ((row * Cimg + c) * TP + sy) * TP + sx);
      v = __fadd_rn(__fdiv_rn(v, 2.0f), 0.5f);
      v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);  // clamp(0,1); NaN stays NaN like torch.clamp
      sum = __fadd_rn(sum, v);
      cnt = __fadd_rn(cnt, 1.0f);
    }
  }
  image[t] = __fdiv_rn(sum, cnt);
}

// ---- img2img / inpainting glue ------------------------------------------------
// Four pure streaming kernels that run once per image (the first three) or once per phase (the blend), on 12 MB of pixels at
// most and 64 KiB - 1 MiB latents: one thread per 4 elements with 16-byte accesses where the extents and pointers allow it, a
// scalar kernel otherwise; both evaluate the same expression per element, so they give the same bits.

// ed_u8_to_vae_input: v -> 2 * (v / 255) - 1, each operation rounded on its own (np.float32(v) / 255, then 2 * x - 1)
__device__ __forceinline__ float vae_input_of(uint32_t v) {
  return __fsub_rn(__fmul_rn(2.0f, __fdiv_rn((float)v, 255.0f)), 1.0f);
}

// 4 pixels per thread: 12 interleaved bytes as three aligned dwords in, one 4-element vector store per colour plane out
template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_u8_to_vae_input_x4(const uint32_t* __restrict__ img, void* __restrict__ out, int64_t HW) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= (HW >> 2)) return;
  uint32_t w0 = img[3 * t], w1 = img[3 * t + 1], w2 = img[3 * t + 2];  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
  int64_t p = t << 2;
  st4<Tag>(out, p, vae_input_of(w0 & 255u), vae_input_of(w0 >> 24), vae_input_of((w1 >> 16) & 255u),
           vae_input_of((w2 >> 8) & 255u));
  st4<Tag>(out, HW + p, vae_input_of((w0 >> 8) & 255u), vae_input_of(w1 & 255u), vae_input_of(w1 >> 24),
           vae_input_of((w2 >> 16) & 255u));
  st4<Tag>(out, 2 * HW + p, vae_input_of((w0 >> 16) & 255u), vae_input_of((w1 >> 8) & 255u), vae_input_of(w2 & 255u),
           vae_input_of(w2 >> 24));
}

template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_u8_to_vae_input(const uint8_t* __restrict__ img, void* __restrict__ out, int64_t HW) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= 3 * HW) return;
  int64_t c = t / HW, p = t - c * HW;
  st<Tag>(out, t, vae_input_of(img[3 * p + c]));
}

// ed_u8_to_clip_input: centre crop + CLIPImageProcessor's rescale and normalise of an already resized picture.
// One thread per output element; x = float(double(v) * (1 / 255)) -- the processor rescales in fp64 and rounds once to fp32 -- then
// (x - mean_c) / std_c in fp32, each operation rounded on its own.  256 possible x values per channel: nothing worth vectorising at
// 3 x 224 x 224 elements once per image.
__global__ void __launch_bounds__(ED_BLOCK)
k_u8_to_clip_input(const uint8_t* __restrict__ img, int W, int y0, int x0, int S, float* __restrict__ out, float m0, float m1, float m2,
                   float s0, float s1, float s2) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  const int64_t SS = (int64_t)S * S;
  if (t >= 3 * SS) return;
  const int c = (int)(t / SS);
  const int64_t p = t - c * SS;
  const int y = (int)(p / S), x = (int)(p - (int64_t)y * S);
  const uint32_t v = img[((int64_t)(y0 + y) * W + (x0 + x)) * 3 + c];
  const float r = (float)((double)v * (1.0 / 255.0));
  const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
  out[t] = __fdiv_rn(__fsub_rn(r, mean), sd);
}

// ed_u8_to_vae_input_masked: the same value, or +0.0 where the pixel's mask byte is >= threshold (a select, so the zero has no sign
// to inherit: DESIGN.md section 22.3).  4 pixels per thread: the 4 mask bytes as one aligned dword.
__device__ __forceinline__ float vae_input_masked_of(uint32_t v, uint32_t m, uint32_t thr) {
  return m >= thr ? 0.0f : vae_input_of(v);
}

template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_u8_to_vae_input_masked_x4(const uint32_t* __restrict__ img, const uint32_t* __restrict__ mask, uint32_t thr, void* __restrict__ out,
                            int64_t HW) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= (HW >> 2)) return;
  uint32_t w0 = img[3 * t], w1 = img[3 * t + 1], w2 = img[3 * t + 2];  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
  uint32_t m4 = mask[t];
  uint32_t m0 = m4 & 255u, m1 = (m4 >> 8) & 255u, m2 = (m4 >> 16) & 255u, m3 = m4 >> 24;
  int64_t p = t << 2;
  st4<Tag>(out, p, vae_input_masked_of(w0 & 255u, m0, thr), vae_input_masked_of(w0 >> 24, m1, thr),
           vae_input_masked_of((w1 >> 16) & 255u, m2, thr), vae_input_masked_of((w2 >> 8) & 255u, m3, thr));
  st4<Tag>(out, HW + p, vae_input_masked_of((w0 >> 8) & 255u, m0, thr), vae_input_masked_of(w1 & 255u, m1, thr),
           vae_input_masked_of(w1 >> 24, m2, thr), vae_input_masked_of((w2 >> 16) & 255u, m3, thr));
  st4<Tag>(out, 2 * HW + p, vae_input_masked_of((w0 >> 16) & 255u, m0, thr), vae_input_masked_of((w1 >> 8) & 255u, m1, thr),
           vae_input_masked_of(w2 & 255u, m2, thr), vae_input_masked_of(w2 >> 24, m3, thr));
}

template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_u8_to_vae_input_masked(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, uint32_t thr, void* __restrict__ out,
                         int64_t HW) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= 3 * HW) return;
  int64_t c = t / HW, p = t - c * HW;
  st<Tag>(out, t, vae_input_masked_of(img[3 * p + c], mask[p], thr));
}

// ed_img2img_init: z0 = (mean + std * eps) * sf, x = a * z0 + b * noise
__device__ __forceinline__ void img2img_one(float m, float s, float e, float nz, float sf, float a, float b, float& z, float& x) {
  z = __fmul_rn(__fadd_rn(m, __fmul_rn(s, e)), sf);
  x = __fadd_rn(__fmul_rn(a, z), __fmul_rn(b, nz));
}

template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_img2img_init_v4(const void* __restrict__ mean, const void* __restrict__ stdv, const float4* __restrict__ eps,
                  const float4* __restrict__ noise, float sf, float a, float b, float4* __restrict__ z0,
                  float4* __restrict__ x, int64_t n4) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n4) return;
  float4 m = ld4<Tag>(mean, t << 2), s = ld4<Tag>(stdv, t << 2), e = eps[t], nz = noise[t], z, o;
  img2img_one(m.x, s.x, e.x, nz.x, sf, a, b, z.x, o.x);
  img2img_one(m.y, s.y, e.y, nz.y, sf, a, b, z.y, o.y);
  img2img_one(m.z, s.z, e.z, nz.z, sf, a, b, z.z, o.z);
  img2img_one(m.w, s.w, e.w, nz.w, sf, a, b, z.w, o.w);
  z0[t] = z;
  x[t] = o;
}

template <typename Tag>
__global__ void __launch_bounds__(ED_BLOCK)
k_img2img_init_s(const void* __restrict__ mean, const void* __restrict__ stdv, const float* __restrict__ eps,
                 const float* __restrict__ noise, float sf, float a, float b, float* __restrict__ z0,
                 float* __restrict__ x, int64_t n) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  float z, o;
  img2img_one(ld<Tag>(mean, t), ld<Tag>(stdv, t), eps[t], noise[t], sf, a, b, z, o);
  z0[t] = z;
  x[t] = o;
}

// ed_mask_to_latent: m[y, x] = src[scale * y, scale * x] >= threshold.  A strided byte gather into at most 64 KiB: every sample
// sits in a sector of its own, so there is nothing to widen; one thread per output byte.
__global__ void __launch_bounds__(ED_BLOCK)
k_mask_to_latent(const uint8_t* __restrict__ src, int W, int scale, int threshold, uint8_t* __restrict__ m, int Hl, int Wl) {
  int t = blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= Hl * Wl) return;
  int y = t / Wl, x = t - y * Wl;
  m[t] = (int)src[(int64_t)y * scale * W + (int64_t)x * scale] >= threshold ? 1 : 0;
}

// ed_inpaint_blend: out = m ? x : known, known = CLEAN ? z0 : a * z0 + b * noise; a select, so the kept side never sees x and the
// repainted side never sees z0 / noise (NaN / inf on the side not taken do not leak).  out may be x (every thread reads its own
// elements before it writes them): x and out are not __restrict__.
template <bool CLEAN>
__device__ __forceinline__ float blend_one(uint32_t m, float xv, float z, float nz, float a, float b) {
  if (m) return xv;
  return CLEAN ? z : __fadd_rn(__fmul_rn(a, z), __fmul_rn(b, nz));
}

template <bool CLEAN>
__global__ void __launch_bounds__(ED_BLOCK)
k_inpaint_blend_v4(const float4* x, const uint32_t* __restrict__ mask, const float4* __restrict__ z0,
                   const float4* __restrict__ noise, float a, float b, float4* out, int64_t n4, int64_t HW4) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n4) return;
  uint32_t m = mask[t % HW4];
  float4 xv = x[t], z = z0[t], nz = CLEAN ? z : noise[t], o;
  o.x = blend_one<CLEAN>(m & 255u, xv.x, z.x, nz.x, a, b);
  o.y = blend_one<CLEAN>((m >> 8) & 255u, xv.y, z.y, nz.y, a, b);
  o.z = blend_one<CLEAN>((m >> 16) & 255u, xv.z, z.z, nz.z, a, b);
  o.w = blend_one<CLEAN>(m >> 24, xv.w, z.w, nz.w, a, b);
  out[t] = o;
}

template <bool CLEAN>
__global__ void __launch_bounds__(ED_BLOCK)
k_inpaint_blend_s(const float* x, const uint8_t* __restrict__ mask, const float* __restrict__ z0,
                  const float* __restrict__ noise, float a, float b, float* out, int64_t n, int64_t HW) {
  int64_t t = (int64_t)blockIdx.x * ED_BLOCK + threadIdx.x;
  if (t >= n) return;
  float z = z0[t];
  out[t] = blend_one<CLEAN>(mask[t % HW], x[t], z, CLEAN ? z : noise[t], a, b);
}

}  // namespace

// ====================================================================================================
// C ABI
// ====================================================================================================
#define ED_LAUNCH_T(dtype, KERNEL, n, ...)                                                       \
  switch (dtype) {                                                                               \
    case ED_F32: KERNEL<F32><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__); break;   \
    case ED_F16: KERNEL<F16><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__); break;   \
    case ED_BF16: KERNEL<BF16><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__); break; \
    default: return (int)hipErrorInvalidValue;                                                   \
  }
#define ED_LAUNCH(KERNEL, n, ...) KERNEL<<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__)
// prediction-type variants: <false> = epsilon, <true> = v_prediction
#define ED_LAUNCH_VP(vp, KERNEL, n, ...)                                               \
  do {                                                                                 \
    if (vp) KERNEL<true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);   \
    else KERNEL<false><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);     \
  } while (0)

// ... x guidance-rescale variants: <vp, true> when a ratio buffer is given
#define ED_LAUNCH_VP_GR(vp, gr, KERNEL, n, ...)                                               \
  do {                                                                                        \
    if (!(gr)) ED_LAUNCH_VP(vp, KERNEL, n, __VA_ARGS__);                                      \
    else if (vp) KERNEL<true, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);  \
    else KERNEL<false, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);         \
  } while (0)

static const Rescale NO_RESCALE = {nullptr, 0.0f, 0.0f, 1};

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

extern "C" {

int ed_version(void) { return ED_ABI_VERSION; }

const char* ed_error_string(int err) { return hipGetErrorString((hipError_t)err); }

int ed_gather_views(const float* latent, void* out, int dtype, int B, int C, int H, int W, const int32_t* win_y0,
                    const int32_t* win_x0, int V, int Sh, int Sw, int PH, int PW, int off_y, int off_x,
                    const float* frame, float divisor, void* stream) {
  int64_t n = (int64_t)V * B * C * PH * PW;
  if (n == 0) return 0;
  int use_div = divisor != 1.0f;
  if ((PW & 3) == 0 && (Sw & 3) == 0 && (off_x & 3) == 0 && aligned16(out) && (!frame || aligned16(frame))) {
    n >>= 2;
    ED_LAUNCH_T(dtype, k_gather_windows_x4, n, latent, out, B, C, H, W, win_y0, win_x0, V, Sh, Sw, PH, PW, off_y, off_x,
                frame, divisor, use_div);
    return done();
  }
  ED_LAUNCH_T(dtype, k_gather_windows, n, latent, out, B, C, H, W, win_y0, win_x0, V, Sh, Sw, PH, PW, off_y, off_x,
                                         frame, divisor, use_div);
  return done();
}

int ed_tile_gather_pad(const float* latent, void* tiles, int dtype, int B, int C, int H, int W, const int32_t* tile_y0,
                       const int32_t* tile_x0, int T_, int Ts, float scaling_factor, void* stream) {
  return ed_gather_views(latent, tiles, dtype, B, C, H, W, tile_y0, tile_x0, T_, Ts, Ts, Ts, Ts, 0, 0, nullptr,
                         scaling_factor, stream);
}

int ed_scatter_centres(const void* pred, int dtype, float* local, int B, int C, int H, int W, int PH, int PW,
                       int n_col_blocks, const int32_t* row_blk, const int32_t* row_src, const int32_t* col_blk,
                       const int32_t* col_src, void* stream) {
  int64_t n = (int64_t)B * C * H * W;
  if (n == 0) return 0;
  ED_LAUNCH_T(dtype, k_scatter_centres, n, pred, local, B, C, H, W, PH, PW, n_col_blocks, row_blk, row_src, col_blk,
                                         col_src);
  return done();
}

int ed_pick_assemble(const float* latent, const uint8_t* idx, const int32_t* src_row, const int32_t* src_col,
                     const float* frame, void* out, int dtype, float* low, int K, int B, int C, int H, int W, int h,
                     int w, int PH, int PW, int off_y, int off_x, void* stream) {
  int64_t n = (int64_t)K * B * C * PH * PW;
  if (n == 0) return 0;
  if ((PW & 3) == 0 && (w & 3) == 0 && (off_x & 3) == 0 && aligned16(out) && aligned16(idx) &&
      (!frame || aligned16(frame)) && (!low || aligned16(low))) {
    n >>= 2;
    ED_LAUNCH_T(dtype, k_pick_assemble_x4, n, latent, idx, src_row, src_col, frame, out, low, K, B, C, H, W, h, w, PH,
                PW, off_y, off_x);
    return done();
  }
  ED_LAUNCH_T(dtype, k_pick_assemble, n, latent, idx, src_row, src_col, frame, out, low, K, B, C, H, W, h, w, PH, PW,
                                         off_y, off_x);
  return done();
}

int ed_assemble_rows(const float* latent, int B, int C, int H, int W, const uint8_t* idx, const int32_t* src_row,
                     const int32_t* src_col, const float* gframe, void* g_rows, float* low, int K, int h, int w, int gPH,
                     int gPW, int g_off_y, int g_off_x, const int32_t* win_y0, const int32_t* win_x0,
                     const float* vframe, void* v_rows, int V, int Sh, int Sw, int vPH, int vPW, int v_off_y, int v_off_x,
                     int dtype, void* stream) {
  int64_t n_g = (int64_t)K * B * C * gPH * gPW, n_v = (int64_t)V * B * C * vPH * vPW;
  if (n_g + n_v == 0) return 0;
  bool px4 = (gPW & 3) == 0 && (w & 3) == 0 && (g_off_x & 3) == 0 && aligned16(g_rows) && aligned16(idx) &&
             (!gframe || aligned16(gframe)) && (!low || aligned16(low));
  bool gx4 = (vPW & 3) == 0 && (Sw & 3) == 0 && (v_off_x & 3) == 0 && aligned16(v_rows) && (!vframe || aligned16(vframe));
  AssembleArgs a;
  a.latent = latent, a.B = B, a.C = C, a.H = H, a.W = W;
  a.idx = idx, a.src_row = src_row, a.src_col = src_col, a.gframe = gframe, a.g_out = g_rows, a.low = low;
  a.K = K, a.h = h, a.w = w, a.gPH = gPH, a.gPW = gPW, a.g_off_y = g_off_y, a.g_off_x = g_off_x;
  a.win_y0 = win_y0, a.win_x0 = win_x0, a.vframe = vframe, a.v_out = v_rows;
  a.V = V, a.Sh = Sh, a.Sw = Sw, a.vPH = vPH, a.vPW = vPW, a.v_off_y = v_off_y, a.v_off_x = v_off_x;
  a.pick_blocks = n_g ? grid_for(px4 ? n_g >> 2 : n_g) : 0;
  int view_blocks = n_v ? grid_for(gx4 ? n_v >> 2 : n_v) : 0;
  dim3 grid(a.pick_blocks + view_blocks), block(ED_BLOCK);
  hipStream_t st_ = (hipStream_t)stream;
#define ED_ASM(T)                                                              \
  if (px4 && gx4) k_assemble_rows<T, true, true><<<grid, block, 0, st_>>>(a);  \
  else if (px4) k_assemble_rows<T, true, false><<<grid, block, 0, st_>>>(a);   \
  else if (gx4) k_assemble_rows<T, false, true><<<grid, block, 0, st_>>>(a);   \
  else k_assemble_rows<T, false, false><<<grid, block, 0, st_>>>(a);
  switch (dtype) {
    case ED_F32: ED_ASM(F32) break;
    case ED_F16: ED_ASM(F16) break;
    case ED_BF16: ED_ASM(BF16) break;
    default: return (int)hipErrorInvalidValue;
  }
#undef ED_ASM
  return done();
}

int ed_assemble_rows_x(const float* latent, int B, int C, int H, int W, const uint8_t* idx, const int32_t* src_row,
                       const int32_t* src_col, const float* gframe, void* g_rows, float* low, int K, int h, int w, int gPH,
                       int gPW, int g_off_y, int g_off_x, const int32_t* win_y0, const int32_t* win_x0,
                       const float* vframe, void* v_rows, int V, int Sh, int Sw, int vPH, int vPW, int v_off_y, int v_off_x,
                       int dtype, const float* extra, int E, const float* pad_value, void* stream) {
  if (!extra || !pad_value || E < 1 || C < 1 || B < 0 || K < 0 || V < 0 || H < 1 || W < 1 || h < 0 || w < 0 || Sh < 0 || Sw < 0 ||
      g_off_y < 0 || g_off_x < 0 || g_off_y + h > gPH || g_off_x + w > gPW || v_off_y < 0 || v_off_x < 0 || v_off_y + Sh > vPH ||
      v_off_x + Sw > vPW)
    return (int)hipErrorInvalidValue;
  int64_t n_g = (int64_t)K * B * (C + E) * gPH * gPW, n_v = (int64_t)V * B * (C + E) * vPH * vPW;
  if (n_g + n_v == 0) return 0;
  // the extras are read one element at a time in both forms, so `extra` carries no alignment condition
  bool px4 = (gPW & 3) == 0 && (w & 3) == 0 && (g_off_x & 3) == 0 && aligned16(g_rows) && aligned16(idx) &&
             (!gframe || aligned16(gframe)) && (!low || aligned16(low));
  bool gx4 = (vPW & 3) == 0 && (Sw & 3) == 0 && (v_off_x & 3) == 0 && aligned16(v_rows) && (!vframe || aligned16(vframe));
  AssembleArgsX a;
  a.latent = latent, a.B = B, a.C = C, a.H = H, a.W = W;
  a.idx = idx, a.src_row = src_row, a.src_col = src_col, a.gframe = gframe, a.g_out = g_rows, a.low = low;
  a.K = K, a.h = h, a.w = w, a.gPH = gPH, a.gPW = gPW, a.g_off_y = g_off_y, a.g_off_x = g_off_x;
  a.win_y0 = win_y0, a.win_x0 = win_x0, a.vframe = vframe, a.v_out = v_rows;
  a.V = V, a.Sh = Sh, a.Sw = Sw, a.vPH = vPH, a.vPW = vPW, a.v_off_y = v_off_y, a.v_off_x = v_off_x;
  a.extra = extra, a.pad_value = pad_value, a.E = E;
  a.pick_blocks = n_g ? grid_for(px4 ? n_g >> 2 : n_g) : 0;
  int view_blocks = n_v ? grid_for(gx4 ? n_v >> 2 : n_v) : 0;
  dim3 grid(a.pick_blocks + view_blocks), block(ED_BLOCK);
  hipStream_t st_ = (hipStream_t)stream;
#define ED_ASM_X(T)                                                              \
  if (px4 && gx4) k_assemble_rows_x<T, true, true><<<grid, block, 0, st_>>>(a);  \
  else if (px4) k_assemble_rows_x<T, true, false><<<grid, block, 0, st_>>>(a);   \
  else if (gx4) k_assemble_rows_x<T, false, true><<<grid, block, 0, st_>>>(a);   \
  else k_assemble_rows_x<T, false, false><<<grid, block, 0, st_>>>(a);
  switch (dtype) {
    case ED_F32: ED_ASM_X(F32) break;
    case ED_F16: ED_ASM_X(F16) break;
    case ED_BF16: ED_ASM_X(BF16) break;
    default: return (int)hipErrorInvalidValue;
  }
#undef ED_ASM_X
  return done();
}

int ed_assemble_rows_n(const float* latent, int B, int C, int H, int W, const uint8_t* idx, const int32_t* src_row,
                       const int32_t* src_col, const float* gframe, void* g_rows, float* low, int K, int h, int w, int gPH,
                       int gPW, int g_off_y, int g_off_x, const int32_t* win_y0, const int32_t* win_x0,
                       const float* vframe, void* v_rows, int V, int Sh, int Sw, int vPH, int vPW, int v_off_y, int v_off_x,
                       int dtype, const float* extra, int E, const float* pad_value, int copies, void* stream) {
  if (copies < 2 || copies > 1 + ED_MAX_REGION_ROWS || E < 0 || (E > 0 && (!extra || !pad_value)) || (E == 0 && extra) || !latent ||
      C < 1 || B < 0 || K < 0 || V < 0 || H < 1 || W < 1 || h < 0 || w < 0 || Sh < 0 || Sw < 0 || g_off_y < 0 || g_off_x < 0 ||
      g_off_y + h > gPH || g_off_x + w > gPW || v_off_y < 0 || v_off_x < 0 || v_off_y + Sh > vPH || v_off_x + Sw > vPW)
    return (int)hipErrorInvalidValue;
  int64_t n_g = (int64_t)K * B * (C + E) * gPH * gPW, n_v = (int64_t)V * B * (C + E) * vPH * vPW;
  if (n_g + n_v == 0) return 0;
  if ((n_g && (!g_rows || !idx || !src_row || !src_col)) || (n_v && (!v_rows || !win_y0 || !win_x0))) return (int)hipErrorInvalidValue;
  bool px4 = (gPW & 3) == 0 && (w & 3) == 0 && (g_off_x & 3) == 0 && aligned16(g_rows) && aligned16(idx) &&
             (!gframe || aligned16(gframe)) && (!low || aligned16(low));
  bool gx4 = (vPW & 3) == 0 && (Sw & 3) == 0 && (v_off_x & 3) == 0 && aligned16(v_rows) && (!vframe || aligned16(vframe));
  AssembleArgsN a;
  a.latent = latent, a.B = B, a.C = C, a.H = H, a.W = W;
  a.idx = idx, a.src_row = src_row, a.src_col = src_col, a.gframe = gframe, a.g_out = g_rows, a.low = low;
  a.K = K, a.h = h, a.w = w, a.gPH = gPH, a.gPW = gPW, a.g_off_y = g_off_y, a.g_off_x = g_off_x;
  a.win_y0 = win_y0, a.win_x0 = win_x0, a.vframe = vframe, a.v_out = v_rows;
  a.V = V, a.Sh = Sh, a.Sw = Sw, a.vPH = vPH, a.vPW = vPW, a.v_off_y = v_off_y, a.v_off_x = v_off_x;
  a.extra = extra, a.pad_value = pad_value, a.E = E, a.copies = copies;
  a.pick_blocks = n_g ? grid_for(px4 ? n_g >> 2 : n_g) : 0;
  int view_blocks = n_v ? grid_for(gx4 ? n_v >> 2 : n_v) : 0;
  dim3 grid(a.pick_blocks + view_blocks), block(ED_BLOCK);
  hipStream_t st_ = (hipStream_t)stream;
#define ED_ASM_N(T)                                                              \
  if (px4 && gx4) k_assemble_rows_n<T, true, true><<<grid, block, 0, st_>>>(a);  \
  else if (px4) k_assemble_rows_n<T, true, false><<<grid, block, 0, st_>>>(a);   \
  else if (gx4) k_assemble_rows_n<T, false, true><<<grid, block, 0, st_>>>(a);   \
  else k_assemble_rows_n<T, false, false><<<grid, block, 0, st_>>>(a);
  switch (dtype) {
    case ED_F32: ED_ASM_N(F32) break;
    case ED_F16: ED_ASM_N(F16) break;
    case ED_BF16: ED_ASM_N(BF16) break;
    default: return (int)hipErrorInvalidValue;
  }
#undef ED_ASM_N
  return done();
}

int ed_ip_mask_rows(const float* masks, int B, int A, int H, int W, const uint8_t* idx, const int32_t* src_row,
                    const int32_t* src_col, int K, int h, int w, int g_off_y, int g_off_x, const int32_t* win_y0,
                    const int32_t* win_x0, int V, int Sh, int Sw, int v_off_y, int v_off_x, int PH, int PW, int copies, float* m,
                    void* stream) {
  if (!masks || !m || A < 1 || A > 4 || copies < 2 || copies > 1 + ED_MAX_REGION_ROWS || B < 0 || K < 0 || V < 0 || H < 1 || W < 1 ||
      h < 0 || w < 0 || Sh < 0 || Sw < 0 || PH < 8 || PW < 8 || (PH & 7) || (PW & 7) || PH > 4096 || PW > 4096 || g_off_y < 0 ||
      g_off_x < 0 || g_off_y + h > PH || g_off_x + w > PW || v_off_y < 0 || v_off_x < 0 || v_off_y + Sh > PH || v_off_x + Sw > PW)
    return (int)hipErrorInvalidValue;
  if ((int64_t)(K + V) * B == 0) return 0;
  if ((K && (!idx || !src_row || !src_col)) || (V && (!win_y0 || !win_x0))) return (int)hipErrorInvalidValue;
  const int64_t patches = (int64_t)B * A * (PH >> 3) * (PW >> 3);
  if (patches * ((int64_t)K + V) > 0x7fffffff) return (int)hipErrorInvalidValue;
  IpMaskArgs a;
  a.masks = masks, a.B = B, a.A = A, a.H = H, a.W = W;
  a.idx = idx, a.src_row = src_row, a.src_col = src_col, a.K = K, a.h = h, a.w = w, a.g_off_y = g_off_y, a.g_off_x = g_off_x;
  a.win_y0 = win_y0, a.win_x0 = win_x0, a.V = V, a.Sh = Sh, a.Sw = Sw, a.v_off_y = v_off_y, a.v_off_x = v_off_x;
  a.PH = PH, a.PW = PW, a.copies = copies, a.m = m;
  a.S = PH * PW + (PH >> 1) * (PW >> 1) + (PH >> 2) * (PW >> 2) + (PH >> 3) * (PW >> 3);
  a.pick_blocks = (int)(patches * K);
  dim3 grid((unsigned)(patches * ((int64_t)K + V))), block(64);
  k_ip_mask_rows<<<grid, block, 0, (hipStream_t)stream>>>(a);
  return done();
}

// does the history [x0_hist, x0_hist + n) share an element with one of the two outputs of the step?  (they are written while the
// history of other elements is still being read)
static inline bool hist_overlaps(const float* x0_hist, const float* prev, const float* x0, int64_t n) {
  if (!x0_hist) return false;
  uintptr_t h = (uintptr_t)x0_hist, bytes = (uintptr_t)n * sizeof(float);
  uintptr_t p = (uintptr_t)prev, o = (uintptr_t)x0;
  return (h < p + bytes && p < h + bytes) || (h < o + bytes && o < h + bytes);
}

// The noise operand of the stochastic samplers (section 29) and its scalar, as the *_sde entry points take them.
struct Noise {
  const float* noise;
  float c_n;
};

// does the noise [noise, noise + n) share an element with an output of the step (x_next may be NULL)?
static inline bool noise_overlaps(const float* noise, const float* prev, const float* x0, const float* x_next, int64_t n) {
  return hist_overlaps(noise, prev, x0, n) || (x_next && hist_overlaps(noise, x_next, x_next, n));
}

static int phase_epilogue_launch(bool vp, const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                      const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                      const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                      const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                      float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                      int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                      int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev,
                      float sqrt_1m_alpha_prev, float rrg_norm, float rrg_weight, void* stream,
                      const float* ratio = nullptr, const float* ratio_low = nullptr, float gr = 0.0f, float omgr = 0.0f,
                      const Multistep* ms = nullptr, const Noise* nz = nullptr) {
  int64_t n = (int64_t)B * C * H * W + (int64_t)B * C * h * w;
  if ((int64_t)B * C * H * W == 0) return 0;
  if (x_next && !low_latent) return (int)hipErrorInvalidValue;
  if (ratio && x_next && !ratio_low) return (int)hipErrorInvalidValue;
  if (ms && hist_overlaps(ms->x0_hist, prev, x0, (int64_t)B * C * H * W)) return (int)hipErrorInvalidValue;
  if (nz && noise_overlaps(nz->noise, prev, x0, x_next, (int64_t)B * C * H * W)) return (int)hipErrorInvalidValue;
  EpilogueArgsNZ a;  // launched as its EpilogueArgsMS base without `nz`, as its EpilogueArgs base without `ms` either
  a.noise = nz ? nz->noise : nullptr, a.c_n = nz ? nz->c_n : 0.0f;
  a.ratio = ratio, a.ratio_low = ratio_low, a.gr = gr, a.omgr = omgr;
  a.x0_hist = ms ? ms->x0_hist : nullptr, a.hb = ms ? ms->hb : 0.0f, a.r_inv = ms ? ms->r_inv : 0.0f;
  a.g_out = g_out, a.v_out = v_out, a.x = x, a.stamp = stamp;
  a.inv_row = inv_row, a.inv_col = inv_col, a.up_row = up_row, a.up_col = up_col, a.down_row = down_row, a.down_col = down_col;
  a.row_blk = row_blk, a.row_src = row_src, a.col_blk = col_blk, a.col_src = col_src;
  a.low_latent = low_latent, a.prev = prev, a.x0 = x0, a.x_next = x_next, a.low_dir = low_dir, a.uncond_last = uncond_last;
  a.direction = direction, a.local = local;
  a.K = K, a.B = B, a.C = C, a.H = H, a.W = W, a.h = h, a.w = w, a.gPH = gPH, a.gPW = gPW, a.g_off_y = g_off_y;
  a.g_off_x = g_off_x, a.vPH = vPH, a.vPW = vPW, a.ncb = n_col_blocks;
  a.g = g, a.sb = sqrt_beta_t, a.sa = sqrt_alpha_t, a.sp = sqrt_alpha_prev, a.sd = sqrt_1m_alpha_prev;
  a.rrg_norm = rrg_norm, a.rrg_weight = rrg_weight;
  // the noise variants (section 29): the same choice of ST, <.., true>; without `nz` nothing below changed
#define ED_EPI_NZ(T, ST)                                                                                            \
  if (ratio && vp) k_phase_epilogue<T, true, true, ST, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);  \
  else if (ratio) k_phase_epilogue<T, false, true, ST, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);  \
  else if (vp) k_phase_epilogue<T, true, false, ST, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);     \
  else k_phase_epilogue<T, false, false, ST, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);
#define ED_EPI_NZ_T(ST)                        \
  switch (dtype) {                             \
    case ED_F32: ED_EPI_NZ(F32, ST) break;     \
    case ED_F16: ED_EPI_NZ(F16, ST) break;     \
    case ED_BF16: ED_EPI_NZ(BF16, ST) break;   \
    default: return (int)hipErrorInvalidValue; \
  }
  if (nz) {
    if (!ms) { ED_EPI_NZ_T(ST_DDIM) } else if (ms->x0_hist) { ED_EPI_NZ_T(ST_MS2) } else { ED_EPI_NZ_T(ST_MS1) }
    return done();
  }
#undef ED_EPI_NZ_T
#undef ED_EPI_NZ
  // the multistep variants: <.., ST_MS2> when a history is given, <.., ST_MS1> otherwise (sqrt_alpha_prev / sqrt_1m_alpha_prev
  // carry c_x / b); without `ms` the launches below are the ones there always were
#define ED_EPI_MS(T, ST)                                                                                       \
  if (ratio && vp) k_phase_epilogue<T, true, true, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);   \
  else if (ratio) k_phase_epilogue<T, false, true, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);   \
  else if (vp) k_phase_epilogue<T, true, false, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);      \
  else k_phase_epilogue<T, false, false, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);
#define ED_EPI_MS_T(ST)                        \
  switch (dtype) {                             \
    case ED_F32: ED_EPI_MS(F32, ST) break;     \
    case ED_F16: ED_EPI_MS(F16, ST) break;     \
    case ED_BF16: ED_EPI_MS(BF16, ST) break;   \
    default: return (int)hipErrorInvalidValue; \
  }
  if (ms) {
    if (ms->x0_hist) { ED_EPI_MS_T(ST_MS2) } else { ED_EPI_MS_T(ST_MS1) }
    return done();
  }
#undef ED_EPI_MS_T
#undef ED_EPI_MS
#define ED_EPI(T)                                                                                        \
  if (ratio && vp) k_phase_epilogue<T, true, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);  \
  else if (ratio) k_phase_epilogue<T, false, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);  \
  else if (vp) k_phase_epilogue<T, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);            \
  else k_phase_epilogue<T, false><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);
  switch (dtype) {
    case ED_F32: ED_EPI(F32) break;
    case ED_F16: ED_EPI(F16) break;
    case ED_BF16: ED_EPI(BF16) break;
    default: return (int)hipErrorInvalidValue;
  }
#undef ED_EPI
  return done();
}

static inline bool bad_prediction_type(int pt) { return pt != ED_PRED_EPSILON && pt != ED_PRED_V; }

int ed_phase_epilogue(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                      const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                      const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                      const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                      float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                      int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                      int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev,
                      float sqrt_1m_alpha_prev, float rrg_norm, float rrg_weight, void* stream) {
  return phase_epilogue_launch(false, g_out, v_out, dtype, x, stamp, inv_row, inv_col, up_row, up_col, down_row, down_col,
                               row_blk, row_src, col_blk, col_src, low_latent, prev, x0, x_next, low_dir, uncond_last,
                               direction, local, K, B, C, H, W, h, w, gPH, gPW, g_off_y, g_off_x, vPH, vPW, n_col_blocks, g,
                               sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_1m_alpha_prev, rrg_norm, rrg_weight, stream);
}

int ed_phase_epilogue_pt(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                         const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                         const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                         const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                         float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                         int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                         int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev,
                         float sqrt_1m_alpha_prev, float rrg_norm, float rrg_weight, int prediction_type, void* stream) {
  if (bad_prediction_type(prediction_type)) return (int)hipErrorInvalidValue;
  return phase_epilogue_launch(prediction_type == ED_PRED_V, g_out, v_out, dtype, x, stamp, inv_row, inv_col, up_row, up_col,
                               down_row, down_col, row_blk, row_src, col_blk, col_src, low_latent, prev, x0, x_next, low_dir,
                               uncond_last, direction, local, K, B, C, H, W, h, w, gPH, gPW, g_off_y, g_off_x, vPH, vPW,
                               n_col_blocks, g, sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_1m_alpha_prev, rrg_norm,
                               rrg_weight, stream);
}

int ed_unpad_direction(const void* unet_out, int dtype, float* dirs, float* uncond_last, int K, int B, int C, int h,
                       int w, int PH, int PW, int off_y, int off_x, void* stream) {
  int64_t n = (int64_t)K * B * C * h * w;
  if (n == 0) return 0;
  if ((PW & 3) == 0 && (w & 3) == 0 && (off_x & 3) == 0 && aligned16(unet_out) && aligned16(dirs) &&
      (!uncond_last || aligned16(uncond_last))) {
    n >>= 2;
    ED_LAUNCH_T(dtype, k_unpad_direction_x4, n, unet_out, dirs, uncond_last, K, B, C, h, w, PH, PW, off_y, off_x);
    return done();
  }
  ED_LAUNCH_T(dtype, k_unpad_direction, n, unet_out, dirs, uncond_last, K, B, C, h, w, PH, PW, off_y, off_x);
  return done();
}

int ed_fill_directions(const float* dirs, const int8_t* stamp, const int32_t* inv_row, const int32_t* inv_col,
                       const int32_t* up_row, const int32_t* up_col, const int32_t* down_row, const int32_t* down_col,
                       float* target, float* low_dir, int K, int B, int C, int H, int W, int h, int w, void* stream) {
  int64_t n = (int64_t)H * W + (low_dir ? (int64_t)h * w : 0);
  if (n == 0 || K <= 0) return K <= 0 ? (int)hipErrorInvalidValue : 0;
  ED_LAUNCH(k_fill_directions, n, dirs, stamp, inv_row,
                     inv_col, up_row, up_col, down_row, down_col, target, low_dir, K, B, C, H, W, h, w);
  return done();
}

// The 16-byte kernels (k_cfg_ddim_v4) take every call whose element count and buffers allow it; a ratio adds ONE condition,
// that a sample is a whole number of float4s.  Without a ratio rs.per plays no part: the plain entry points choose as they
// always did.
static inline bool cfg_ddim_x4(const float* local, const float* direction, const float* x, const float* prev, const float* x0,
                               int64_t n, const Rescale& rs) {
  return (n & 3) == 0 && (!rs.ratio || (rs.per & 3) == 0) && aligned16(local) && aligned16(direction) && aligned16(x) &&
         aligned16(prev) && aligned16(x0);
}

static const Multistep NO_MULTISTEP = {nullptr, 0.0f, 0.0f};

static int cfg_ddim_launch(bool vp, const float* local, const float* direction, const float* x, float* prev, float* x0, float g,
                           float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev, float sqrt_one_minus_alpha_prev,
                           int64_t n, void* stream, const Rescale rs = NO_RESCALE) {
  if (n == 0) return 0;
  if (cfg_ddim_x4(local, direction, x, prev, x0, n, rs)) {
    ED_LAUNCH_VP_GR(vp, rs.ratio, k_cfg_ddim_v4, n / 4, (const float4*)local, (const float4*)direction, (const float4*)x,
                    (float4*)prev, (float4*)x0, g, sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_one_minus_alpha_prev,
                    n / 4, rs, NO_MULTISTEP);
  } else {
    ED_LAUNCH_VP_GR(vp, rs.ratio, k_cfg_ddim_s, n, local, direction, x, prev, x0, g, sqrt_beta_t, sqrt_alpha_t,
                    sqrt_alpha_prev, sqrt_one_minus_alpha_prev, n, rs, NO_MULTISTEP);
  }
  return done();
}

// The multistep launch: the 16-byte form under cfg_ddim_x4's conditions and, with a history, an aligned history; the scalar form
// otherwise.  <.., ST_MS2> with a history, <.., ST_MS1> without.
static inline bool cfg_ms_x4(const float* local, const float* direction, const float* x, const float* prev, const float* x0,
                             int64_t n, const Rescale& rs, const float* x0_hist) {
  return cfg_ddim_x4(local, direction, x, prev, x0, n, rs) && (!x0_hist || aligned16(x0_hist));
}

#define ED_LAUNCH_MS(vp, gr, ST, KERNEL, n, ...)                                                               \
  do {                                                                                                         \
    if ((gr) && (vp)) KERNEL<true, true, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);   \
    else if (gr) KERNEL<false, true, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);       \
    else if (vp) KERNEL<true, false, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);       \
    else KERNEL<false, false, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);              \
  } while (0)

static int cfg_ms_launch(bool vp, const float* local, const float* direction, const float* x, float* prev, float* x0, float g,
                         float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, int64_t n, void* stream, const Rescale rs,
                         const Multistep ms) {
  if (n == 0) return 0;
  if (hist_overlaps(ms.x0_hist, prev, x0, n)) return (int)hipErrorInvalidValue;
  if (cfg_ms_x4(local, direction, x, prev, x0, n, rs, ms.x0_hist)) {
#define ED_MS_V4(ST)                                                                                                       \
  ED_LAUNCH_MS(vp, rs.ratio, ST, k_cfg_ddim_v4, n / 4, (const float4*)local, (const float4*)direction, (const float4*)x, \
               (float4*)prev, (float4*)x0, g, sqrt_beta_t, sqrt_alpha_t, c_x, b, n / 4, rs, ms)
    if (ms.x0_hist) ED_MS_V4(ST_MS2); else ED_MS_V4(ST_MS1);
#undef ED_MS_V4
  } else {
#define ED_MS_S(ST) \
  ED_LAUNCH_MS(vp, rs.ratio, ST, k_cfg_ddim_s, n, local, direction, x, prev, x0, g, sqrt_beta_t, sqrt_alpha_t, c_x, b, n, rs, ms)
    if (ms.x0_hist) ED_MS_S(ST_MS2); else ED_MS_S(ST_MS1);
#undef ED_MS_S
  }
  return done();
}

// The noise launch (section 29): `st` is ST_DDIM (sp / sd = sqrt(abar_prev) / sd_eta) or ST_MS1 / ST_MS2 as cfg_ms_launch chooses them.
// The 16-byte form under cfg_ms_x4's conditions and an aligned noise; the scalar form otherwise.
#define ED_LAUNCH_NZ(vp, gr, ST, KERNEL, n, ...)                                                                     \
  do {                                                                                                               \
    if ((gr) && (vp)) KERNEL<true, true, ST, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);   \
    else if (gr) KERNEL<false, true, ST, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);       \
    else if (vp) KERNEL<true, false, ST, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);       \
    else KERNEL<false, false, ST, true><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(__VA_ARGS__);              \
  } while (0)

static int cfg_nz_launch(bool vp, int st, const float* local, const float* direction, const float* x, float* prev, float* x0,
                         float g, float sqrt_beta_t, float sqrt_alpha_t, float sp, float sd, int64_t n, void* stream,
                         const Rescale rs, const Multistep ms, const Noise nz) {
  if (n == 0) return 0;
  if (hist_overlaps(ms.x0_hist, prev, x0, n) || noise_overlaps(nz.noise, prev, x0, nullptr, n)) return (int)hipErrorInvalidValue;
  MultistepNZ a;
  a.x0_hist = ms.x0_hist, a.hb = ms.hb, a.r_inv = ms.r_inv, a.noise = nz.noise, a.c_n = nz.c_n;
  if (cfg_ms_x4(local, direction, x, prev, x0, n, rs, ms.x0_hist) && aligned16(nz.noise)) {
#define ED_NZ_V4(ST)                                                                                                       \
  ED_LAUNCH_NZ(vp, rs.ratio, ST, k_cfg_ddim_v4, n / 4, (const float4*)local, (const float4*)direction, (const float4*)x, \
               (float4*)prev, (float4*)x0, g, sqrt_beta_t, sqrt_alpha_t, sp, sd, n / 4, rs, a)
    if (st == ST_DDIM) ED_NZ_V4(ST_DDIM); else if (st == ST_MS2) ED_NZ_V4(ST_MS2); else ED_NZ_V4(ST_MS1);
#undef ED_NZ_V4
  } else {
#define ED_NZ_S(ST) \
  ED_LAUNCH_NZ(vp, rs.ratio, ST, k_cfg_ddim_s, n, local, direction, x, prev, x0, g, sqrt_beta_t, sqrt_alpha_t, sp, sd, n, rs, a)
    if (st == ST_DDIM) ED_NZ_S(ST_DDIM); else if (st == ST_MS2) ED_NZ_S(ST_MS2); else ED_NZ_S(ST_MS1);
#undef ED_NZ_S
  }
  return done();
}

int ed_cfg_ddim_step(const float* local, const float* direction, const float* x, float* prev, float* x0, float g,
                     float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev, float sqrt_one_minus_alpha_prev,
                     int64_t n, void* stream) {
  return cfg_ddim_launch(false, local, direction, x, prev, x0, g, sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev,
                         sqrt_one_minus_alpha_prev, n, stream);
}

int ed_cfg_ddim_step_pt(const float* local, const float* direction, const float* x, float* prev, float* x0, float g,
                        float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev, float sqrt_one_minus_alpha_prev,
                        int64_t n, int prediction_type, void* stream) {
  if (bad_prediction_type(prediction_type)) return (int)hipErrorInvalidValue;
  return cfg_ddim_launch(prediction_type == ED_PRED_V, local, direction, x, prev, x0, g, sqrt_beta_t, sqrt_alpha_t,
                         sqrt_alpha_prev, sqrt_one_minus_alpha_prev, n, stream);
}

int ed_undo_step(const float* x_in, const float* noise, const float* coef, float* x_out, int n_sub, int64_t n,
                 void* stream) {
  if (n == 0) return 0;
  if ((n & 3) == 0 && aligned16(x_in) && aligned16(noise) && aligned16(x_out)) {
    ED_LAUNCH(k_undo_v4, n / 4, (const float4*)x_in,
                       (const float4*)noise, (const float2*)coef, (float4*)x_out, n_sub, n / 4);
  } else {
    ED_LAUNCH(k_undo_s, n, x_in, noise,
                       (const float2*)coef, x_out, n_sub, n);
  }
  return done();
}

static int rrg_update_launch(bool vp, const float* prev, const float* x0, const float* low_latent, const float* low_uncond,
                             const float* low_dir, const int32_t* up_row, const int32_t* up_col, float* out, float g,
                             float sqrt_beta_t, float sqrt_alpha_t, float norm, float weight, int B, int C, int H, int W,
                             int h, int w, void* stream, const Rescale rs = NO_RESCALE) {
  int64_t n = (int64_t)B * C * H * W;
  if (n == 0) return 0;
  if ((W & 3) == 0 && aligned16(prev) && aligned16(x0) && aligned16(out)) {
    n >>= 2;
    ED_LAUNCH_VP_GR(vp, rs.ratio, k_rrg_update_x4, n, prev, x0, low_latent, low_uncond, low_dir, up_row, up_col, out, g,
                    sqrt_beta_t, sqrt_alpha_t, norm, weight, B, C, H, W, h, w, rs);
    return done();
  }
  ED_LAUNCH_VP_GR(vp, rs.ratio, k_rrg_update, n, prev, x0, low_latent, low_uncond, low_dir, up_row, up_col, out, g,
                  sqrt_beta_t, sqrt_alpha_t, norm, weight, B, C, H, W, h, w, rs);
  return done();
}

int ed_rrg_update(const float* prev, const float* x0, const float* low_latent, const float* low_uncond,
                  const float* low_dir, const int32_t* up_row, const int32_t* up_col, float* out, float g,
                  float sqrt_beta_t, float sqrt_alpha_t, float norm, float weight, int B, int C, int H, int W, int h,
                  int w, void* stream) {
  return rrg_update_launch(false, prev, x0, low_latent, low_uncond, low_dir, up_row, up_col, out, g, sqrt_beta_t,
                           sqrt_alpha_t, norm, weight, B, C, H, W, h, w, stream);
}

int ed_rrg_update_pt(const float* prev, const float* x0, const float* low_latent, const float* low_uncond,
                     const float* low_dir, const int32_t* up_row, const int32_t* up_col, float* out, float g,
                     float sqrt_beta_t, float sqrt_alpha_t, float norm, float weight, int B, int C, int H, int W, int h,
                     int w, int prediction_type, void* stream) {
  if (bad_prediction_type(prediction_type)) return (int)hipErrorInvalidValue;
  return rrg_update_launch(prediction_type == ED_PRED_V, prev, x0, low_latent, low_uncond, low_dir, up_row, up_col, out, g,
                           sqrt_beta_t, sqrt_alpha_t, norm, weight, B, C, H, W, h, w, stream);
}

int ed_gather2d(const void* in, int in_dtype, void* out, int out_dtype, int C, int H, int W, const int32_t* src_n,
                const int32_t* rows, const int32_t* cols, int N, int oh, int ow, void* stream) {
  int64_t n = (int64_t)N * C * oh * ow;
  if (n == 0) return 0;
#define ED_G2D(TI, TO) \
  k_gather2d<TI, TO><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(in, out, C, H, W, src_n, rows, cols, N, oh, ow)
  int key = in_dtype * 3 + out_dtype;
  switch (key) {
    case 0: ED_G2D(F32, F32); break;
    case 1: ED_G2D(F32, F16); break;
    case 2: ED_G2D(F32, BF16); break;
    case 3: ED_G2D(F16, F32); break;
    case 4: ED_G2D(F16, F16); break;
    case 5: ED_G2D(F16, BF16); break;
    case 6: ED_G2D(BF16, F32); break;
    case 7: ED_G2D(BF16, F16); break;
    case 8: ED_G2D(BF16, BF16); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef ED_G2D
  return done();
}

int ed_tile_accumulate_normalise(const void* decoded, int dtype, float* image, int B, int Cimg, int HP, int WP, int TP,
                                 int n_col_tiles, const int32_t* row_tile, const int32_t* row_src,
                                 const int32_t* col_tile, const int32_t* col_src, void* stream) {
  int64_t n = (int64_t)B * Cimg * HP * WP;
  if (n == 0) return 0;
  ED_LAUNCH_T(dtype, k_tile_accumulate, n, decoded, image, B, Cimg, HP, WP, TP, n_col_tiles, row_tile, row_src, col_tile,
                                         col_src);
  return done();
}

// ---- guidance rescale ------------------------------------------------------------------------------
int64_t ed_guidance_moments_workspace(int B, int64_t n_full, int64_t n_low) {
  if (B <= 0 || n_full < 0 || n_low < 0) return 0;
  int64_t blocks = (int64_t)B * ((n_full ? moments_blocks(n_full) : 0) + (n_low ? moments_blocks(n_low) : 0));
  return blocks * 6 * (int64_t)sizeof(double);
}

static inline bool bad_workspace(const void* ws) { return !ws || (((uintptr_t)ws) & 7u) != 0; }

int ed_guidance_moments(const float* local, const float* direction, const float* text, float g, int B, int64_t n,
                        float* ratio, void* workspace, void* stream) {
  if (B <= 0 || n <= 0) return B < 0 || n < 0 ? (int)hipErrorInvalidValue : 0;
  if (bad_workspace(workspace) || !ratio) return (int)hipErrorInvalidValue;
  int nblk = moments_blocks(n);
  k_guidance_moments<<<B * nblk, ED_BLOCK, 0, (hipStream_t)stream>>>(local, direction, text, g, n, nblk,
                                                                     (double*)workspace);
  k_moments_finalise<<<B, 64, 0, (hipStream_t)stream>>>((const double*)workspace, B, nblk, 0, ratio, nullptr);
  return done();
}

int ed_phase_moments(const void* g_out, const void* v_out, int dtype, const int8_t* stamp, const int32_t* inv_row,
                     const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col, const int32_t* down_row,
                     const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src, const int32_t* col_blk,
                     const int32_t* col_src, float* ratio, float* ratio_low, void* workspace, int K, int B, int C, int H,
                     int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW, int n_col_blocks,
                     float g, void* stream) {
  int64_t n_full = (int64_t)C * H * W, n_low = (int64_t)C * h * w;
  if (B <= 0 || n_full <= 0) return B < 0 || n_full < 0 ? (int)hipErrorInvalidValue : 0;
  if (bad_workspace(workspace) || !ratio || K <= 0 || (ratio_low && n_low <= 0)) return (int)hipErrorInvalidValue;
  EpilogueArgs a = {};
  a.g_out = g_out, a.v_out = v_out, a.stamp = stamp;
  a.inv_row = inv_row, a.inv_col = inv_col, a.up_row = up_row, a.up_col = up_col, a.down_row = down_row, a.down_col = down_col;
  a.row_blk = row_blk, a.row_src = row_src, a.col_blk = col_blk, a.col_src = col_src;
  a.K = K, a.B = B, a.C = C, a.H = H, a.W = W, a.h = h, a.w = w, a.gPH = gPH, a.gPW = gPW, a.g_off_y = g_off_y;
  a.g_off_x = g_off_x, a.vPH = vPH, a.vPW = vPW, a.ncb = n_col_blocks, a.g = g;
  int nblk_full = moments_blocks(n_full), nblk_low = ratio_low ? moments_blocks(n_low) : 0;
  dim3 grid(B * (nblk_full + nblk_low)), block(ED_BLOCK);
  hipStream_t st_ = (hipStream_t)stream;
  switch (dtype) {
    case ED_F32: k_phase_moments<F32><<<grid, block, 0, st_>>>(a, nblk_full, nblk_low, (double*)workspace); break;
    case ED_F16: k_phase_moments<F16><<<grid, block, 0, st_>>>(a, nblk_full, nblk_low, (double*)workspace); break;
    case ED_BF16: k_phase_moments<BF16><<<grid, block, 0, st_>>>(a, nblk_full, nblk_low, (double*)workspace); break;
    default: return (int)hipErrorInvalidValue;
  }
  k_moments_finalise<<<ratio_low ? 2 * B : B, 64, 0, st_>>>((const double*)workspace, B, nblk_full, nblk_low, ratio, ratio_low);
  return done();
}

int ed_cfg_ddim_step_gr(const float* local, const float* direction, const float* x, float* prev, float* x0, float g,
                        float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev, float sqrt_one_minus_alpha_prev,
                        int64_t n, int prediction_type, const float* ratio, float gr, float omgr, int B, void* stream) {
  if (bad_prediction_type(prediction_type)) return (int)hipErrorInvalidValue;
  Rescale rs = NO_RESCALE;
  if (ratio) {
    if (B <= 0 || n % B) return (int)hipErrorInvalidValue;
    rs.ratio = ratio, rs.gr = gr, rs.omgr = omgr, rs.per = n / B;
    if (rs.per == 0) return 0;
  }
  return cfg_ddim_launch(prediction_type == ED_PRED_V, local, direction, x, prev, x0, g, sqrt_beta_t, sqrt_alpha_t,
                         sqrt_alpha_prev, sqrt_one_minus_alpha_prev, n, stream, rs);
}

int ed_cfg_ddim_step_width(const float* local, const float* direction, const float* x, const float* prev, const float* x0,
                           int64_t n, const float* ratio, int B) {
  Rescale rs = NO_RESCALE;
  if (ratio) {
    if (B <= 0 || n % B) return 0;
    rs.ratio = ratio, rs.per = n / B;
  }
  return cfg_ddim_x4(local, direction, x, prev, x0, n, rs) ? 4 : 1;
}

int ed_rrg_update_gr(const float* prev, const float* x0, const float* low_latent, const float* low_uncond,
                     const float* low_dir, const int32_t* up_row, const int32_t* up_col, float* out, float g,
                     float sqrt_beta_t, float sqrt_alpha_t, float norm, float weight, int B, int C, int H, int W, int h,
                     int w, int prediction_type, const float* ratio_low, float gr, float omgr, void* stream) {
  if (bad_prediction_type(prediction_type)) return (int)hipErrorInvalidValue;
  Rescale rs = NO_RESCALE;
  if (ratio_low) rs.ratio = ratio_low, rs.gr = gr, rs.omgr = omgr;
  return rrg_update_launch(prediction_type == ED_PRED_V, prev, x0, low_latent, low_uncond, low_dir, up_row, up_col, out, g,
                           sqrt_beta_t, sqrt_alpha_t, norm, weight, B, C, H, W, h, w, stream, rs);
}

int ed_phase_epilogue_gr(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                         const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                         const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                         const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                         float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                         int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                         int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev,
                         float sqrt_1m_alpha_prev, float rrg_norm, float rrg_weight, int prediction_type,
                         const float* ratio, const float* ratio_low, float gr, float omgr, void* stream) {
  if (bad_prediction_type(prediction_type)) return (int)hipErrorInvalidValue;
  return phase_epilogue_launch(prediction_type == ED_PRED_V, g_out, v_out, dtype, x, stamp, inv_row, inv_col, up_row, up_col,
                               down_row, down_col, row_blk, row_src, col_blk, col_src, low_latent, prev, x0, x_next, low_dir,
                               uncond_last, direction, local, K, B, C, H, W, h, w, gPH, gPW, g_off_y, g_off_x, vPH, vPW,
                               n_col_blocks, g, sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_1m_alpha_prev, rrg_norm,
                               rrg_weight, stream, ratio, ratio_low, gr, omgr);
}

// ---- DPM-Solver++(2M) ------------------------------------------------------------
int ed_cfg_ddim_step_ms(const float* local, const float* direction, const float* x, float* prev, float* x0, float g,
                        float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, float half_b, float r_inv, int64_t n,
                        int prediction_type, const float* ratio, float gr, float omgr, int B, const float* x0_hist,
                        void* stream) {
  if (bad_prediction_type(prediction_type)) return (int)hipErrorInvalidValue;
  Rescale rs = NO_RESCALE;
  if (ratio) {
    if (B <= 0 || n % B) return (int)hipErrorInvalidValue;
    rs.ratio = ratio, rs.gr = gr, rs.omgr = omgr, rs.per = n / B;
    if (rs.per == 0) return 0;
  }
  Multistep ms = {x0_hist, half_b, r_inv};
  return cfg_ms_launch(prediction_type == ED_PRED_V, local, direction, x, prev, x0, g, sqrt_beta_t, sqrt_alpha_t, c_x, b, n,
                       stream, rs, ms);
}

int ed_phase_epilogue_ms(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                         const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                         const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                         const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                         float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                         int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                         int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, float half_b,
                         float r_inv, float rrg_norm, float rrg_weight, int prediction_type, const float* ratio,
                         const float* ratio_low, float gr, float omgr, const float* x0_hist, void* stream) {
  if (bad_prediction_type(prediction_type)) return (int)hipErrorInvalidValue;
  Multistep ms = {x0_hist, half_b, r_inv};
  return phase_epilogue_launch(prediction_type == ED_PRED_V, g_out, v_out, dtype, x, stamp, inv_row, inv_col, up_row, up_col,
                               down_row, down_col, row_blk, row_src, col_blk, col_src, low_latent, prev, x0, x_next, low_dir,
                               uncond_last, direction, local, K, B, C, H, W, h, w, gPH, gPW, g_off_y, g_off_x, vPH, vPW,
                               n_col_blocks, g, sqrt_beta_t, sqrt_alpha_t, c_x, b, rrg_norm, rrg_weight, stream, ratio, ratio_low,
                               gr, omgr, &ms);
}

// ---- stochastic samplers: DDIM eta > 0, SDE-DPM-Solver++(2M), LCM ------------------
static inline bool bad_sde_arguments(int form, float c_n, const float* noise, const float* x0_hist, int prediction_type) {
  if (bad_prediction_type(prediction_type) || (form != ED_FORM_DDIM && form != ED_FORM_MULTISTEP)) return true;
  if (!noise || !__builtin_isfinite(c_n)) return true;
  return form == ED_FORM_DDIM && x0_hist != nullptr;
}

int ed_cfg_ddim_step_sde(const float* local, const float* direction, const float* x, float* prev, float* x0, float g,
                         float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, float half_b, float r_inv, int64_t n,
                         int prediction_type, const float* ratio, float gr, float omgr, int B, const float* x0_hist, int form,
                         float c_n, const float* noise, void* stream) {
  if (bad_sde_arguments(form, c_n, noise, x0_hist, prediction_type)) return (int)hipErrorInvalidValue;
  if (noise_overlaps(noise, prev, x0, nullptr, n)) return (int)hipErrorInvalidValue;
  Rescale rs = NO_RESCALE;
  if (ratio) {
    if (B <= 0 || n % B) return (int)hipErrorInvalidValue;
    rs.ratio = ratio, rs.gr = gr, rs.omgr = omgr, rs.per = n / B;
    if (rs.per == 0) return 0;
  }
  const bool vp = prediction_type == ED_PRED_V;
  Multistep ms = {x0_hist, half_b, r_inv};
  if (c_n == 0.0f) {  // not a stochastic step: the deterministic launch, which never reads the noise
    if (form == ED_FORM_DDIM) return cfg_ddim_launch(vp, local, direction, x, prev, x0, g, sqrt_beta_t, sqrt_alpha_t, c_x, b, n, stream, rs);
    return cfg_ms_launch(vp, local, direction, x, prev, x0, g, sqrt_beta_t, sqrt_alpha_t, c_x, b, n, stream, rs, ms);
  }
  Noise nz = {noise, c_n};
  return cfg_nz_launch(vp, form == ED_FORM_DDIM ? ST_DDIM : x0_hist ? ST_MS2 : ST_MS1, local, direction, x, prev, x0, g, sqrt_beta_t,
                       sqrt_alpha_t, c_x, b, n, stream, rs, ms, nz);
}

int ed_phase_epilogue_sde(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                          const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                          const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                          const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                          float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                          int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                          int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, float half_b,
                          float r_inv, float rrg_norm, float rrg_weight, int prediction_type, const float* ratio,
                          const float* ratio_low, float gr, float omgr, const float* x0_hist, int form, float c_n,
                          const float* noise, void* stream) {
  if (bad_sde_arguments(form, c_n, noise, x0_hist, prediction_type)) return (int)hipErrorInvalidValue;
  if (noise_overlaps(noise, prev, x0, x_next, (int64_t)B * C * H * W)) return (int)hipErrorInvalidValue;
  Multistep ms = {x0_hist, half_b, r_inv};
  Noise nz = {noise, c_n};
  return phase_epilogue_launch(prediction_type == ED_PRED_V, g_out, v_out, dtype, x, stamp, inv_row, inv_col, up_row, up_col,
                               down_row, down_col, row_blk, row_src, col_blk, col_src, low_latent, prev, x0, x_next, low_dir,
                               uncond_last, direction, local, K, B, C, H, W, h, w, gPH, gPW, g_off_y, g_off_x, vPH, vPW,
                               n_col_blocks, g, sqrt_beta_t, sqrt_alpha_t, c_x, b, rrg_norm, rrg_weight, stream, ratio, ratio_low,
                               gr, omgr, form == ED_FORM_DDIM ? nullptr : &ms, c_n == 0.0f ? nullptr : &nz);
}

// ---- img2img / inpainting -----------------------------------------------------------------------------
int ed_u8_to_vae_input(const uint8_t* img, int H, int W, void* out, int dtype, void* stream) {
  if (!img || !out || H < 0 || W < 0) return (int)hipErrorInvalidValue;
  int64_t HW = (int64_t)H * W;
  if (HW == 0) return 0;
  if ((HW & 3) == 0 && (((uintptr_t)img) & 3u) == 0 && aligned16(out)) {
    ED_LAUNCH_T(dtype, k_u8_to_vae_input_x4, HW >> 2, (const uint32_t*)img, out, HW);
  } else {
    ED_LAUNCH_T(dtype, k_u8_to_vae_input, 3 * HW, img, out, HW);
  }
  return done();
}

int ed_u8_to_clip_input(const uint8_t* img, int H, int W, int y0, int x0, int S, float* out, float mean0, float mean1, float mean2,
                        float std0, float std1, float std2, void* stream) {
  if (!img || !out || H < 1 || W < 1 || S < 1 || y0 < 0 || x0 < 0) return (int)hipErrorInvalidValue;
  if ((int64_t)y0 + S > H || (int64_t)x0 + S > W) return (int)hipErrorInvalidValue;  // the crop lies inside the picture
  if (!(std0 != 0.0f) || !(std1 != 0.0f) || !(std2 != 0.0f)) return (int)hipErrorInvalidValue;
  ED_LAUNCH(k_u8_to_clip_input, 3 * (int64_t)S * S, img, W, y0, x0, S, out, mean0, mean1, mean2, std0, std1, std2);
  return done();
}

int ed_u8_to_vae_input_masked(const uint8_t* img, const uint8_t* mask, int threshold, int H, int W, void* out, int dtype,
                              void* stream) {
  if (!img || !mask || !out || H < 0 || W < 0 || threshold < 1 || threshold > 255) return (int)hipErrorInvalidValue;
  int64_t HW = (int64_t)H * W;
  if (HW == 0) return 0;
  if ((HW & 3) == 0 && (((uintptr_t)img) & 3u) == 0 && (((uintptr_t)mask) & 3u) == 0 && aligned16(out)) {
    ED_LAUNCH_T(dtype, k_u8_to_vae_input_masked_x4, HW >> 2, (const uint32_t*)img, (const uint32_t*)mask, (uint32_t)threshold, out,
                HW);
  } else {
    ED_LAUNCH_T(dtype, k_u8_to_vae_input_masked, 3 * HW, img, mask, (uint32_t)threshold, out, HW);
  }
  return done();
}

int ed_img2img_init(const void* mean, const void* std, int dtype, const float* eps, const float* noise, float sf, float a,
                    float b, float* z0, float* x, int64_t n, void* stream) {
  if (!mean || !std || !eps || !noise || !z0 || !x || n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if ((n & 3) == 0 && aligned16(mean) && aligned16(std) && aligned16(eps) && aligned16(noise) && aligned16(z0) && aligned16(x)) {
    ED_LAUNCH_T(dtype, k_img2img_init_v4, n / 4, mean, std, (const float4*)eps, (const float4*)noise, sf, a, b, (float4*)z0,
                (float4*)x, n / 4);
  } else {
    ED_LAUNCH_T(dtype, k_img2img_init_s, n, mean, std, eps, noise, sf, a, b, z0, x, n);
  }
  return done();
}

int ed_mask_to_latent(const uint8_t* src, int H, int W, int scale, int threshold, uint8_t* mask, int Hl, int Wl, void* stream) {
  if (!src || !mask || scale < 1 || Hl < 0 || Wl < 0 || (int64_t)Hl * scale != H || (int64_t)Wl * scale != W ||
      (int64_t)Hl * Wl > INT32_MAX)
    return (int)hipErrorInvalidValue;
  if (Hl == 0 || Wl == 0) return 0;
  ED_LAUNCH(k_mask_to_latent, (int64_t)Hl * Wl, src, W, scale, threshold, mask, Hl, Wl);
  return done();
}

int ed_inpaint_blend(const float* x, const uint8_t* mask, const float* z0, const float* noise, float a, float b, int clean,
                     float* out, int planes, int64_t HW, void* stream) {
  if (!x || !mask || !z0 || !out || (!clean && !noise) || planes < 0 || HW < 0) return (int)hipErrorInvalidValue;
  int64_t n = (int64_t)planes * HW;
  if (n == 0) return 0;
  if ((HW & 3) == 0 && aligned16(x) && aligned16(z0) && (clean || aligned16(noise)) && aligned16(out) &&
      (((uintptr_t)mask) & 3u) == 0) {
    if (clean)
      ED_LAUNCH(k_inpaint_blend_v4<true>, n / 4, (const float4*)x, (const uint32_t*)mask, (const float4*)z0,
                (const float4*)noise, a, b, (float4*)out, n / 4, HW / 4);
    else
      ED_LAUNCH(k_inpaint_blend_v4<false>, n / 4, (const float4*)x, (const uint32_t*)mask, (const float4*)z0,
                (const float4*)noise, a, b, (float4*)out, n / 4, HW / 4);
  } else {
    if (clean) ED_LAUNCH(k_inpaint_blend_s<true>, n, x, mask, z0, noise, a, b, out, n, HW);
    else ED_LAUNCH(k_inpaint_blend_s<false>, n, x, mask, z0, noise, a, b, out, n, HW);
  }
  return done();
}

// ---- regional prompts -------------------------------------------------------------------
static inline bool ranges_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  if (!a || !b || abytes <= 0 || bbytes <= 0) return false;
  uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bbytes && y < x + (uintptr_t)abytes;
}

static inline bool bad_region_rows(int P) { return P < 1 || P > ED_MAX_REGION_ROWS; }

int ed_region_weights(const uint8_t* masks, const float* weights, int n, int64_t HW, float* region_w, void* stream) {
  if (bad_region_rows(n + 1) || n < 1 || !masks || !weights || !region_w || HW < 0) return (int)hipErrorInvalidValue;
  for (int p = 0; p < n; ++p)
    if (!(weights[p] > 0.0f) || !(weights[p] <= 3.0e38f)) return (int)hipErrorInvalidValue;
  if (ranges_overlap(masks, (int64_t)n * HW, region_w, (int64_t)(n + 1) * HW * 4)) return (int)hipErrorInvalidValue;
  if (HW == 0) return 0;
  RegionWeightArgs rw = {};
  for (int p = 0; p < n; ++p) rw.weight[p] = weights[p];
  if ((HW & 3) == 0 && (((uintptr_t)masks) & 3u) == 0 && aligned16(region_w))
    ED_LAUNCH(k_region_weights_x4, HW >> 2, (const uint32_t*)masks, rw, n, HW >> 2, (float4*)region_w);
  else
    ED_LAUNCH(k_region_weights, HW, masks, rw, n, HW, region_w);
  return done();
}

int ed_region_blend(const float* dirs, const float* region_w, float* out, int P, int planes, int64_t HW, void* stream) {
  if (bad_region_rows(P) || !dirs || !region_w || !out || planes < 0 || HW < 0) return (int)hipErrorInvalidValue;
  int64_t n = (int64_t)planes * HW;
  if (ranges_overlap(region_w, (int64_t)P * HW * 4, out, n * 4) || ranges_overlap(dirs, (int64_t)P * n * 4, out, n * 4))
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if ((HW & 3) == 0 && aligned16(dirs) && aligned16(region_w) && aligned16(out))
    ED_LAUNCH(k_region_blend_v4, n >> 2, (const float4*)dirs, (const float4*)region_w, (float4*)out, P, n >> 2, HW >> 2);
  else
    ED_LAUNCH(k_region_blend, n, dirs, region_w, out, P, n, HW);
  return done();
}

// region_w must not share memory with anything the launch writes
static bool region_w_overlaps_outputs(const float* region_w, int P, int B, int C, int H, int W, int h, int w, const float* const* full,
                                      int n_full, const float* const* low, int n_low) {
  int64_t wb = (int64_t)P * H * W * 4, fb = (int64_t)B * C * H * W * 4, lb = (int64_t)B * C * h * w * 4;
  for (int i = 0; i < n_full; ++i)
    if (ranges_overlap(region_w, wb, full[i], fb)) return true;
  for (int i = 0; i < n_low; ++i)
    if (ranges_overlap(region_w, wb, low[i], lb)) return true;
  return false;
}

int ed_phase_epilogue_rg(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                         const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                         const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                         const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                         float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                         int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                         int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, float half_b,
                         float r_inv, float rrg_norm, float rrg_weight, int prediction_type, const float* ratio,
                         const float* ratio_low, float gr, float omgr, const float* x0_hist, int multistep,
                         const float* region_w, int P, void* stream) {
  if (bad_prediction_type(prediction_type) || bad_region_rows(P) || (!region_w && P > 1) || (multistep != 0 && multistep != 1) ||
      (!multistep && x0_hist))
    return (int)hipErrorInvalidValue;
  const bool vp = prediction_type == ED_PRED_V;
  Multistep ms = {x0_hist, half_b, r_inv};
  if (!region_w)  // P == 1: the launch of ed_phase_epilogue_ms (multistep) / ed_phase_epilogue_gr
    return phase_epilogue_launch(vp, g_out, v_out, dtype, x, stamp, inv_row, inv_col, up_row, up_col, down_row, down_col, row_blk,
                                 row_src, col_blk, col_src, low_latent, prev, x0, x_next, low_dir, uncond_last, direction, local, K,
                                 B, C, H, W, h, w, gPH, gPW, g_off_y, g_off_x, vPH, vPW, n_col_blocks, g, sqrt_beta_t, sqrt_alpha_t,
                                 c_x, b, rrg_norm, rrg_weight, stream, ratio, ratio_low, gr, omgr, multistep ? &ms : nullptr);
  const float* full[] = {prev, x0, x_next, direction, local};
  const float* low[] = {low_dir, uncond_last};
  if (B < 0 || C < 0 || H < 0 || W < 0 || h < 0 || w < 0 || K <= 0 ||
      region_w_overlaps_outputs(region_w, P, B, C, H, W, h, w, full, 5, low, 2))
    return (int)hipErrorInvalidValue;
  int64_t n = (int64_t)B * C * H * W + (int64_t)B * C * h * w;
  if ((int64_t)B * C * H * W == 0) return 0;
  if (!g_out || !v_out || !x || !prev || !x0) return (int)hipErrorInvalidValue;
  if (x_next && !low_latent) return (int)hipErrorInvalidValue;
  if (ratio && x_next && !ratio_low) return (int)hipErrorInvalidValue;
  if (hist_overlaps(x0_hist, prev, x0, (int64_t)B * C * H * W)) return (int)hipErrorInvalidValue;
  EpilogueArgsRG a;
  a.region_w = region_w, a.P = P;
  a.ratio = ratio, a.ratio_low = ratio_low, a.gr = gr, a.omgr = omgr;
  a.x0_hist = x0_hist, a.hb = half_b, a.r_inv = r_inv;
  a.g_out = g_out, a.v_out = v_out, a.x = x, a.stamp = stamp;
  a.inv_row = inv_row, a.inv_col = inv_col, a.up_row = up_row, a.up_col = up_col, a.down_row = down_row, a.down_col = down_col;
  a.row_blk = row_blk, a.row_src = row_src, a.col_blk = col_blk, a.col_src = col_src;
  a.low_latent = low_latent, a.prev = prev, a.x0 = x0, a.x_next = x_next, a.low_dir = low_dir, a.uncond_last = uncond_last;
  a.direction = direction, a.local = local;
  a.K = K, a.B = B, a.C = C, a.H = H, a.W = W, a.h = h, a.w = w, a.gPH = gPH, a.gPW = gPW, a.g_off_y = g_off_y;
  a.g_off_x = g_off_x, a.vPH = vPH, a.vPW = vPW, a.ncb = n_col_blocks;
  a.g = g, a.sb = sqrt_beta_t, a.sa = sqrt_alpha_t, a.sp = c_x, a.sd = b;
  a.rrg_norm = rrg_norm, a.rrg_weight = rrg_weight;
#define ED_EPI_RG(T, ST)                                                                                          \
  if (ratio && vp) k_phase_epilogue_rg<T, true, true, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);   \
  else if (ratio) k_phase_epilogue_rg<T, false, true, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);   \
  else if (vp) k_phase_epilogue_rg<T, true, false, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);      \
  else k_phase_epilogue_rg<T, false, false, ST><<<grid_for(n), ED_BLOCK, 0, (hipStream_t)stream>>>(a);
#define ED_EPI_RG_T(ST)                        \
  switch (dtype) {                             \
    case ED_F32: ED_EPI_RG(F32, ST) break;     \
    case ED_F16: ED_EPI_RG(F16, ST) break;     \
    case ED_BF16: ED_EPI_RG(BF16, ST) break;   \
    default: return (int)hipErrorInvalidValue; \
  }
  if (!multistep) { ED_EPI_RG_T(ST_DDIM) } else if (x0_hist) { ED_EPI_RG_T(ST_MS2) } else { ED_EPI_RG_T(ST_MS1) }
#undef ED_EPI_RG_T
#undef ED_EPI_RG
  return done();
}

int ed_phase_moments_rg(const void* g_out, const void* v_out, int dtype, const int8_t* stamp, const int32_t* inv_row,
                        const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col, const int32_t* down_row,
                        const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src, const int32_t* col_blk,
                        const int32_t* col_src, float* ratio, float* ratio_low, void* workspace, int K, int B, int C, int H,
                        int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW, int n_col_blocks,
                        float g, const float* region_w, int P, void* stream) {
  if (bad_region_rows(P) || (!region_w && P > 1)) return (int)hipErrorInvalidValue;
  if (!region_w)
    return ed_phase_moments(g_out, v_out, dtype, stamp, inv_row, inv_col, up_row, up_col, down_row, down_col, row_blk, row_src,
                            col_blk, col_src, ratio, ratio_low, workspace, K, B, C, H, W, h, w, gPH, gPW, g_off_y, g_off_x, vPH,
                            vPW, n_col_blocks, g, stream);
  int64_t n_full = (int64_t)C * H * W, n_low = (int64_t)C * h * w;
  if (B <= 0 || n_full <= 0) return B < 0 || n_full < 0 ? (int)hipErrorInvalidValue : 0;
  if (bad_workspace(workspace) || !ratio || K <= 0 || (ratio_low && n_low <= 0)) return (int)hipErrorInvalidValue;
  int nblk_full = moments_blocks(n_full), nblk_low = ratio_low ? moments_blocks(n_low) : 0;
  int64_t wb = (int64_t)P * H * W * 4;
  if (ranges_overlap(region_w, wb, ratio, (int64_t)B * 4) || ranges_overlap(region_w, wb, ratio_low, (int64_t)B * 4) ||
      ranges_overlap(region_w, wb, workspace, (int64_t)B * (nblk_full + nblk_low) * 6 * 8))
    return (int)hipErrorInvalidValue;
  EpilogueArgsRG a = {};
  a.region_w = region_w, a.P = P;
  a.g_out = g_out, a.v_out = v_out, a.stamp = stamp;
  a.inv_row = inv_row, a.inv_col = inv_col, a.up_row = up_row, a.up_col = up_col, a.down_row = down_row, a.down_col = down_col;
  a.row_blk = row_blk, a.row_src = row_src, a.col_blk = col_blk, a.col_src = col_src;
  a.K = K, a.B = B, a.C = C, a.H = H, a.W = W, a.h = h, a.w = w, a.gPH = gPH, a.gPW = gPW, a.g_off_y = g_off_y;
  a.g_off_x = g_off_x, a.vPH = vPH, a.vPW = vPW, a.ncb = n_col_blocks, a.g = g;
  dim3 grid(B * (nblk_full + nblk_low)), block(ED_BLOCK);
  hipStream_t st_ = (hipStream_t)stream;
  switch (dtype) {
    case ED_F32: k_phase_moments_rg<F32><<<grid, block, 0, st_>>>(a, nblk_full, nblk_low, (double*)workspace); break;
    case ED_F16: k_phase_moments_rg<F16><<<grid, block, 0, st_>>>(a, nblk_full, nblk_low, (double*)workspace); break;
    case ED_BF16: k_phase_moments_rg<BF16><<<grid, block, 0, st_>>>(a, nblk_full, nblk_low, (double*)workspace); break;
    default: return (int)hipErrorInvalidValue;
  }
  k_moments_finalise<<<ratio_low ? 2 * B : B, 64, 0, st_>>>((const double*)workspace, B, nblk_full, nblk_low, ratio, ratio_low);
  return done();
}

}  // extern "C"
