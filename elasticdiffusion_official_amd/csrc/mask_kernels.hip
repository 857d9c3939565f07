/*
 * mask_kernels.hip -- soft-edged inpainting: pre- and post-processing of ONE image around the denoising
 * loop, plus the per-phase graded blend.  All integer or select arithmetic; every kernel is bit-exact against tests/soft_inpaint_cpu.py.
 *
 *   k_box3_rows / k_box3_cols   PIL.ImageFilter.GaussianBlur on an 8-bit single-channel image: three box passes per direction,
 *                               each on the previous pass's bytes.  One pass over a line of n bytes, c(i) = clamp(i, 0, n - 1):
 *
 *                                   acc    = sum_{d = -r..r} in[c(x + d)]
 *                                   far    = in[c(x - r - 1)] + in[c(x + r + 1)]
 *                                   out[x] = (acc * ww + far * fw + 2^23) >> 24          uint32, cannot overflow
 *
 *                               A launch does the three passes of its direction on lines staged in LDS (two buffers, ping-pong),
 *                               so the image crosses HBM once per direction.  The row kernel stages one line per workgroup; the
 *                               column kernel a strip of S columns x H rows, read and written as S-byte row segments.  A thread
 *                               owns a run of consecutive outputs of a line: one direct window sum for the first, then
 *                               acc += in[c(x + r + 1)] - in[c(x - r)] for each next one (exact integers either way).
 *   k_mask_levels               the gather of ed_mask_to_latent without the comparison: level[y, x] = src[s * y, s * x].
 *   k_blend_level_v4 / _s       ed_inpaint_blend with keep_known = level[p] <= thr in place of the mask byte.
 *   k_composite_x4 / _s         u = (uint8)(decoded * 255) (fp32 product, truncated), then PIL.Image.composite per channel:
 *                               t = u * m + init * (255 - m) + 128; out = (t + (t >> 8)) >> 8.  Planar float in, interleaved bytes out.
 *   k_canvas_pad                np.pad(img, mode="edge") and the 0 / 255 mask of the new border, one launch.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "elastic_hip.h"

namespace {

constexpr int MASK_MAX_DIM = 8192;                      // ops.RESIZE_MAX_DIM
constexpr int THREADS = 256;
constexpr int COL_LDS_BYTES = 64 * 1024;                // both buffers of a column strip: 2 * H * S <= this, so two workgroups fit a CU

inline bool dim_ok(int v) { return v >= 1 && v <= MASK_MAX_DIM; }
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
inline int blocks_for(int64_t n) { return (int)((n + THREADS - 1) / THREADS); }

// ---- box blur ---------------------------------------------------------------------------------------------------
// One pass over a line held in LDS: element i of the line is in[i * stride]; outputs [x0, x1) are this thread's.
__device__ __forceinline__ void box_pass_run(const uint8_t* in, uint8_t* out, int n, int stride, int x0, int x1, int r, uint32_t ww,
                                             uint32_t fw) {
  if (x0 >= x1) return;
  const int last = n - 1;
  uint32_t acc = 0;
  for (int d = -r; d <= r; ++d) acc += in[min(max(x0 + d, 0), last) * stride];
  for (int x = x0;; ++x) {
    const uint32_t lo = in[min(max(x - r - 1, 0), last) * stride], hi = in[min(x + r + 1, last) * stride];
    out[x * stride] = (uint8_t)((acc * ww + (lo + hi) * fw + (1u << 23)) >> 24);
    if (x + 1 >= x1) break;
    acc += hi - in[min(max(x - r, 0), last) * stride];
  }
}

// rows: one workgroup per line
__global__ void __launch_bounds__(THREADS)
k_box3_rows(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int r, uint32_t ww, uint32_t fw, int wide) {
  __shared__ __attribute__((aligned(16))) uint8_t s_line[2][MASK_MAX_DIM];
  const int tid = threadIdx.x;
  const uint8_t* in = src + (size_t)blockIdx.x * W;
  uint8_t* o = dst + (size_t)blockIdx.x * W;
  if (wide) {                                           // W % 4 == 0 and both images 4-byte aligned: so is every line
    for (int k = tid; k < (W >> 2); k += THREADS) reinterpret_cast<uint32_t*>(s_line[0])[k] = reinterpret_cast<const uint32_t*>(in)[k];
  } else {
    for (int k = tid; k < W; k += THREADS) s_line[0][k] = in[k];
  }
  __syncthreads();
  const int run = (W + THREADS - 1) / THREADS;
  const int x0 = min(tid * run, W), x1 = min(x0 + run, W);
  box_pass_run(s_line[0], s_line[1], W, 1, x0, x1, r, ww, fw);
  __syncthreads();
  box_pass_run(s_line[1], s_line[0], W, 1, x0, x1, r, ww, fw);
  __syncthreads();
  box_pass_run(s_line[0], s_line[1], W, 1, x0, x1, r, ww, fw);
  __syncthreads();
  if (wide) {
    for (int k = tid; k < (W >> 2); k += THREADS) reinterpret_cast<uint32_t*>(o)[k] = reinterpret_cast<const uint32_t*>(s_line[1])[k];
  } else {
    for (int k = tid; k < W; k += THREADS) o[k] = s_line[1][k];
  }
}

// columns: one workgroup per strip of S columns (S a power of two in 4..32, 2 * H * S <= COL_LDS_BYTES); the strip is an [H][S] byte
// image in LDS.  THREADS / S threads share a column, each with a run of rows.
__global__ void __launch_bounds__(THREADS)
k_box3_cols(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int S, int r, uint32_t ww, uint32_t fw,
            int wide) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_strip[];
  uint8_t* b0 = s_strip;
  uint8_t* b1 = s_strip + (size_t)H * S;
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * S;
  const int nc = min(S, W - c0);                        // columns of this strip that exist
  const int sdw = S >> 2;
  if (wide && nc == S) {                                // W % 4 == 0, 4-byte aligned images: aligned dwords of every row segment
    for (int k = tid; k < H * sdw; k += THREADS) {
      const int y = k / sdw, q = k - y * sdw;
      reinterpret_cast<uint32_t*>(b0)[k] = *reinterpret_cast<const uint32_t*>(src + (size_t)y * W + c0 + 4 * q);
    }
  } else {
    for (int k = tid; k < H * S; k += THREADS) {
      const int y = k / S, c = k - y * S;
      b0[k] = c < nc ? src[(size_t)y * W + c0 + c] : (uint8_t)0;
    }
  }
  __syncthreads();
  const int col = tid % S, part = tid / S, parts = THREADS / S;
  const int run = (H + parts - 1) / parts;
  const int y0 = min(part * run, H), y1 = min(y0 + run, H);
  box_pass_run(b0 + col, b1 + col, H, S, y0, y1, r, ww, fw);
  __syncthreads();
  box_pass_run(b1 + col, b0 + col, H, S, y0, y1, r, ww, fw);
  __syncthreads();
  box_pass_run(b0 + col, b1 + col, H, S, y0, y1, r, ww, fw);
  __syncthreads();
  if (wide && nc == S) {
    for (int k = tid; k < H * sdw; k += THREADS) {
      const int y = k / sdw, q = k - y * sdw;
      *reinterpret_cast<uint32_t*>(dst + (size_t)y * W + c0 + 4 * q) = reinterpret_cast<const uint32_t*>(b1)[k];
    }
  } else {
    for (int k = tid; k < H * S; k += THREADS) {
      const int y = k / S, c = k - y * S;
      if (c < nc) dst[(size_t)y * W + c0 + c] = b1[k];
    }
  }
}

// ---- level map -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS)
k_mask_levels(const uint8_t* __restrict__ src, int W, int scale, uint8_t* __restrict__ level, int Hl, int Wl) {
  const int t = blockIdx.x * THREADS + threadIdx.x;
  if (t >= Hl * Wl) return;
  const int y = t / Wl, x = t - y * Wl;
  level[t] = src[(int64_t)y * scale * W + (int64_t)x * scale];
}

// ---- graded blend ----------------------------------------------------------------------------------------------------
// out = level > thr ? x : known, known = CLEAN ? z0 : a * z0 + b * noise; a select (the side not taken is never combined
// arithmetically).  out may be x: every thread reads its own elements before it writes them, so x and out are not __restrict__.
template <bool CLEAN>
__device__ __forceinline__ float blend_one(bool repaint, float xv, float z, float nz, float a, float b) {
  if (repaint) return xv;
  return CLEAN ? z : __fadd_rn(__fmul_rn(a, z), __fmul_rn(b, nz));
}

template <bool CLEAN>
__global__ void __launch_bounds__(THREADS)
k_blend_level_v4(const float4* x, const uint32_t* __restrict__ level, uint32_t thr, const float4* __restrict__ z0,
                 const float4* __restrict__ noise, float a, float b, float4* out, int64_t n4, int64_t HW4) {
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (t >= n4) return;
  const uint32_t m = level[t % HW4];
  const float4 xv = x[t], z = z0[t], nz = CLEAN ? z : noise[t];
  float4 o;
  o.x = blend_one<CLEAN>((m & 255u) > thr, xv.x, z.x, nz.x, a, b);
  o.y = blend_one<CLEAN>(((m >> 8) & 255u) > thr, xv.y, z.y, nz.y, a, b);
  o.z = blend_one<CLEAN>(((m >> 16) & 255u) > thr, xv.z, z.z, nz.z, a, b);
  o.w = blend_one<CLEAN>((m >> 24) > thr, xv.w, z.w, nz.w, a, b);
  out[t] = o;
}

template <bool CLEAN>
__global__ void __launch_bounds__(THREADS)
k_blend_level_s(const float* x, const uint8_t* __restrict__ level, uint32_t thr, const float* __restrict__ z0,
                const float* __restrict__ noise, float a, float b, float* out, int64_t n, int64_t HW) {
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (t >= n) return;
  const float z = z0[t];
  out[t] = blend_one<CLEAN>((uint32_t)level[t % HW] > thr, x[t], z, CLEAN ? z : noise[t], a, b);
}

// ---- composite -------------------------------------------------------------------------------------------------------
// the byte of a decoded value: the fp32 product with 255, truncated; the input is clamped to [0, 1] by the decoder, and the min keeps
// anything else a byte
__device__ __forceinline__ uint32_t byte_of(float d) { return min((uint32_t)__fmul_rn(d, 255.0f), 255u); }

__device__ __forceinline__ uint32_t composite_one(float d, uint32_t init, uint32_t m) {
  const uint32_t t = byte_of(d) * m + init * (255u - m) + 128u;
  return (t + (t >> 8)) >> 8;
}

// 4 pixels per thread: a float4 of every colour plane and the mask's dword in, three dwords of interleaved bytes in and out
__global__ void __launch_bounds__(THREADS)
k_composite_x4(const float4* __restrict__ dec, const uint32_t* __restrict__ init, const uint32_t* __restrict__ mask,
               uint32_t* __restrict__ out, int64_t HW4) {
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (t >= HW4) return;
  const float4 R = dec[t], G = dec[HW4 + t], B = dec[2 * HW4 + t];
  const uint32_t m = mask[t], m0 = m & 255u, m1 = (m >> 8) & 255u, m2 = (m >> 16) & 255u, m3 = m >> 24;
  const uint32_t w0 = init[3 * t], w1 = init[3 * t + 1], w2 = init[3 * t + 2];  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
  out[3 * t] = composite_one(R.x, w0 & 255u, m0) | composite_one(G.x, (w0 >> 8) & 255u, m0) << 8 |
               composite_one(B.x, (w0 >> 16) & 255u, m0) << 16 | composite_one(R.y, w0 >> 24, m1) << 24;
  out[3 * t + 1] = composite_one(G.y, w1 & 255u, m1) | composite_one(B.y, (w1 >> 8) & 255u, m1) << 8 |
                   composite_one(R.z, (w1 >> 16) & 255u, m2) << 16 | composite_one(G.z, w1 >> 24, m2) << 24;
  out[3 * t + 2] = composite_one(B.z, w2 & 255u, m2) | composite_one(R.w, (w2 >> 8) & 255u, m3) << 8 |
                   composite_one(G.w, (w2 >> 16) & 255u, m3) << 16 | composite_one(B.w, w2 >> 24, m3) << 24;
}

__global__ void __launch_bounds__(THREADS)
k_composite_s(const float* __restrict__ dec, const uint8_t* __restrict__ init, const uint8_t* __restrict__ mask,
              uint8_t* __restrict__ out, int64_t HW) {
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (t >= 3 * HW) return;
  const int64_t p = t / 3, c = t - 3 * p;
  out[t] = (uint8_t)composite_one(dec[c * HW + p], init[t], mask[p]);
}

// ---- outpainting canvas ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS)
k_canvas_pad(const uint8_t* __restrict__ img, int H, int W, int left, int top, int Ho, int Wo, uint8_t* __restrict__ canvas,
             uint8_t* __restrict__ mask) {
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (t >= (int64_t)Ho * Wo) return;
  const int y = (int)(t / Wo), x = (int)(t - (int64_t)y * Wo);
  const int sy = y - top, sx = x - left;
  const bool inside = sy >= 0 && sy < H && sx >= 0 && sx < W;
  const uint8_t* s = img + ((size_t)min(max(sy, 0), H - 1) * W + min(max(sx, 0), W - 1)) * 3;
  uint8_t* d = canvas + t * 3;
  d[0] = s[0];
  d[1] = s[1];
  d[2] = s[2];
  mask[t] = inside ? 0 : 255;
}

// what a pass may be given: 0 <= r, and weights that keep the result a byte -- (2r + 1) * ww + 2 * fw <= 2^24
inline bool box_ok(int r, int64_t ww, int64_t fw) {
  return r >= 0 && r <= MASK_MAX_DIM && ww >= 0 && fw >= 0 && (2 * (int64_t)r + 1) * ww + 2 * fw <= (1 << 24);
}

}  // namespace

extern "C" {

int ed_box_blur3_rows_u8(const uint8_t* src, int H, int W, int r, int ww, int fw, uint8_t* dst, void* stream) {
  if (!src || !dst || !dim_ok(H) || !dim_ok(W) || !box_ok(r, ww, fw)) return (int)hipErrorInvalidValue;
  const int wide = (W & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3u) == 0;
  k_box3_rows<<<H, THREADS, 0, (hipStream_t)stream>>>(src, dst, W, r, (uint32_t)ww, (uint32_t)fw, wide);
  return (int)hipGetLastError();
}

int ed_box_blur3_cols_strip(int H, int W) {
  if (!dim_ok(H) || !dim_ok(W)) return 0;
  int S = 32;                                                        // 32-byte row segments: one sector per row of a strip
  while (S > 4 && 2 * (int64_t)H * S > COL_LDS_BYTES) S >>= 1;       // H = 8192 -> 4: 2 * 8192 * 4 = 64 KiB
  while (S > 8 && (W + S - 1) / S < 256) S >>= 1;                    // narrower strips until there is a workgroup per CU
  return S;
}

int ed_box_blur3_cols_u8(const uint8_t* src, int H, int W, int r, int ww, int fw, uint8_t* dst, void* stream) {
  if (!src || !dst || !dim_ok(H) || !dim_ok(W) || !box_ok(r, ww, fw)) return (int)hipErrorInvalidValue;
  const int S = ed_box_blur3_cols_strip(H, W);
  const size_t lds = 2 * (size_t)H * S;
  if (S < 4 || lds > (size_t)COL_LDS_BYTES) return (int)hipErrorInvalidValue;
  const int wide = (W & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3u) == 0;
  k_box3_cols<<<(W + S - 1) / S, THREADS, lds, (hipStream_t)stream>>>(src, dst, H, W, S, r, (uint32_t)ww, (uint32_t)fw, wide);
  return (int)hipGetLastError();
}

int ed_mask_levels_to_latent(const uint8_t* src, int H, int W, int scale, uint8_t* level, int Hl, int Wl, void* stream) {
  if (!src || !level || scale < 1 || Hl < 0 || Wl < 0 || (int64_t)Hl * scale != H || (int64_t)Wl * scale != W ||
      (int64_t)Hl * Wl > INT32_MAX)
    return (int)hipErrorInvalidValue;
  if (Hl == 0 || Wl == 0) return 0;
  k_mask_levels<<<blocks_for((int64_t)Hl * Wl), THREADS, 0, (hipStream_t)stream>>>(src, W, scale, level, Hl, Wl);
  return (int)hipGetLastError();
}

int ed_inpaint_blend_level(const float* x, const uint8_t* level, int thr, const float* z0, const float* noise, float a, float b,
                           int clean, float* out, int planes, int64_t HW, void* stream) {
  if (!x || !level || !z0 || !out || (!clean && !noise) || planes < 0 || HW < 0 || thr < 0 || thr > 255)
    return (int)hipErrorInvalidValue;
  const int64_t n = (int64_t)planes * HW;
  if (n == 0) return 0;
  if (n > (int64_t)INT32_MAX * THREADS) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if ((HW & 3) == 0 && aligned16(x) && aligned16(z0) && (clean || aligned16(noise)) && aligned16(out) &&
      (((uintptr_t)level) & 3u) == 0) {
    if (clean)
      k_blend_level_v4<true><<<blocks_for(n / 4), THREADS, 0, s>>>((const float4*)x, (const uint32_t*)level, (uint32_t)thr,
                                                                   (const float4*)z0, (const float4*)noise, a, b, (float4*)out, n / 4, HW / 4);
    else
      k_blend_level_v4<false><<<blocks_for(n / 4), THREADS, 0, s>>>((const float4*)x, (const uint32_t*)level, (uint32_t)thr,
                                                                    (const float4*)z0, (const float4*)noise, a, b, (float4*)out, n / 4, HW / 4);
  } else {
    if (clean) k_blend_level_s<true><<<blocks_for(n), THREADS, 0, s>>>(x, level, (uint32_t)thr, z0, noise, a, b, out, n, HW);
    else k_blend_level_s<false><<<blocks_for(n), THREADS, 0, s>>>(x, level, (uint32_t)thr, z0, noise, a, b, out, n, HW);
  }
  return (int)hipGetLastError();
}

int ed_composite_u8(const float* decoded, const uint8_t* init, const uint8_t* mask, uint8_t* out, int H, int W, void* stream) {
  if (!decoded || !init || !mask || !out || !dim_ok(H) || !dim_ok(W)) return (int)hipErrorInvalidValue;
  const int64_t HW = (int64_t)H * W;
  if ((W & 3) == 0 && aligned16(decoded) && (((uintptr_t)init | (uintptr_t)mask | (uintptr_t)out) & 3u) == 0)
    k_composite_x4<<<blocks_for(HW / 4), THREADS, 0, (hipStream_t)stream>>>((const float4*)decoded, (const uint32_t*)init,
                                                                            (const uint32_t*)mask, (uint32_t*)out, HW / 4);
  else
    k_composite_s<<<blocks_for(3 * HW), THREADS, 0, (hipStream_t)stream>>>(decoded, init, mask, out, HW);
  return (int)hipGetLastError();
}

int ed_canvas_pad_u8(const uint8_t* img, int H, int W, int left, int top, int right, int bottom, uint8_t* canvas, uint8_t* mask,
                     void* stream) {
  if (!img || !canvas || !mask || !dim_ok(H) || !dim_ok(W) || left < 0 || top < 0 || right < 0 || bottom < 0)
    return (int)hipErrorInvalidValue;
  const int64_t Ho = (int64_t)H + top + bottom, Wo = (int64_t)W + left + right;
  if (Ho > MASK_MAX_DIM || Wo > MASK_MAX_DIM) return (int)hipErrorInvalidValue;
  k_canvas_pad<<<blocks_for(Ho * Wo), THREADS, 0, (hipStream_t)stream>>>(img, H, W, left, top, (int)Ho, (int)Wo, canvas, mask);
  return (int)hipGetLastError();
}

}  // extern "C"
