/*
 * resize_kernels.hip -- Pillow's 8-bit antialiased resize (Image.resize with BICUBIC / LANCZOS on L / RGB images) for the
 * condition image of the ControlNet variant (EDC:1392 resizes the photo with PIL's default filter, EDC:173-175, 1017 resize a
 * wrong-sized condition with Lanczos).  Pre-processing of ONE image before the denoising loop starts.
 *
 * The arithmetic is Pillow's, restated in DESIGN.md ("Pillow-exact resize") and tests/resize_cpu.py: the host computes int32
 * fixed-point coefficients (22 fraction bits) and (first tap, taps) per output index (resample.py); a pass is
 *
 *     out = clamp((2^21 + sum_{x < n} in[xmin + x] * k[x]) >> 22, 0, 255)        int32, arithmetic shift
 *
 * per byte.  255 * sum |k| < 2^31, so every partial sum is exact and the taps may be summed in any order and by any number of
 * lanes.  A two-dimensional resize is the horizontal pass into a uint8 intermediate, then the vertical pass.
 *
 *   k_resize_rows   horizontal pass.  One workgroup owns a tile of 64 outputs x up to 16 rows: it stages the source span of the
 *                   tile into LDS through the aligned dwords that cover it (a row of an H x W x 3 byte image starts at any byte
 *                   alignment), accumulates from LDS with G lanes per output byte (G = 1 for short filters; up to 64 lanes split
 *                   the taps of a long one and reduce with wave shuffles), and writes the tile as dwords into a destination whose
 *                   pitch is a multiple of 4.
 *   k_resize_cols   vertical pass.  One thread owns four consecutive bytes of an output row and walks the taps down the source
 *                   rows with one dword load per tap; no LDS.  Writes the uint8 image and / or the fp32 (1,3,H,W) condition
 *                   tensor (byte / 255, correctly rounded; C = 1 replicated to the three planes).
 *
 * Neither kernel trusts the tables for memory safety: first taps and tap counts are clamped to the source extent and to ksize.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "elastic_hip.h"

namespace {

constexpr int RESIZE_MAX_DIM = 8192;
constexpr int THREADS = 256;
constexpr int PB = 22;                                  // fraction bits of a coefficient
constexpr int ROUND = 1 << (PB - 1);

constexpr int TW = 64;                                  // outputs per tile (a multiple of 4: a tile starts on a dword of dst)
constexpr int MAX_TR = 16;                              // rows per tile, at most
constexpr int SRC_DW = 8192;                            // 32 KB of staged source: one row of 8192 RGB pixels is 6145 dwords
constexpr int TAPS_PER_LANE = 32;                       // the launcher splits an output's taps over lanes beyond this

__device__ inline uint8_t clip8(int acc) { return (uint8_t)min(max((acc + ROUND) >> PB, 0), 255); }

// dword at the 4-aligned address a; the bytes outside the buffer [lo, hi) read as 0 and are never touched
__device__ inline uint32_t load_dword_in(uintptr_t a, uintptr_t lo, uintptr_t hi) {
  if (a >= lo && a + 4 <= hi) return *reinterpret_cast<const uint32_t*>(a);
  uint32_t v = 0;
  for (int j = 0; j < 4; ++j)
    if (a + j >= lo && a + j < hi) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(a + j) << (8 * j);
  return v;
}

// ---- k_resize_rows ----------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(THREADS) void k_resize_rows(const uint8_t* __restrict__ src, int H, int W, int src_pitch,
                                                         const int32_t* __restrict__ coeff, const int32_t* __restrict__ bounds,
                                                         int ksize, int W_out, uint8_t* __restrict__ dst, int dst_pitch, int TR,
                                                         int G) {
  constexpr int OUT_ROW_DW = TW * C / 4;                // dwords of one tile row of results
  __shared__ uint32_t s_src[SRC_DW];                    // staged rows, ndw dwords each, from the aligned dword that holds the span's first byte
  __shared__ uint32_t s_out[MAX_TR * OUT_ROW_DW];
  __shared__ int s_span[2];
  const int tid = threadIdx.x;
  const int o0 = blockIdx.x * TW, nout = min(TW, W_out - o0);
  const int y0 = blockIdx.y * TR, nrows = min(TR, H - y0);

  // source span [xs, xe) of the tile: the union of its outputs' taps
  if (tid == 0) {
    s_span[0] = W;
    s_span[1] = 0;
  }
  for (int i = tid; i < MAX_TR * OUT_ROW_DW; i += THREADS) s_out[i] = 0;
  __syncthreads();
  if (tid < nout) {
    const int xmin = min(max(bounds[2 * (o0 + tid)], 0), W);
    const int n = min(max(bounds[2 * (o0 + tid) + 1], 0), min(ksize, W - xmin));
    if (n > 0) {
      atomicMin(&s_span[0], xmin);
      atomicMax(&s_span[1], xmin + n);
    }
  }
  __syncthreads();
  const int xs = s_span[0], xe = max(s_span[1], xs);
  const int span_b = (xe - xs) * C;                     // <= 8192 * 3 bytes
  const int ndw = (span_b + 3) / 4 + 1;                 // dwords that cover span_b bytes at any alignment: <= 6145
  const int rows_fit = min(SRC_DW / ndw, MAX_TR);       // >= 1
  const uintptr_t lo = (uintptr_t)src, hi = lo + (size_t)(H - 1) * src_pitch + (size_t)W * C;
  const int groups = THREADS / G, g = tid % G, slot = tid / G;

  for (int r0 = 0; r0 < nrows; r0 += rows_fit) {
    const int nr = min(rows_fit, nrows - r0);
    for (int idx = tid; idx < nr * ndw; idx += THREADS) {
      const int r = idx / ndw, k = idx - r * ndw;
      const uintptr_t p = lo + (size_t)(y0 + r0 + r) * src_pitch + (size_t)xs * C;     // first byte of the span in this row
      const uintptr_t a = (p & ~(uintptr_t)3) + 4 * (uintptr_t)k;
      if (a < p + span_b) s_src[idx] = load_dword_in(a, lo, hi);
    }
    __syncthreads();

    // item = (row, output, channel), channel fastest; every lane runs the same number of rounds so that the shuffles are uniform
    const int items = nr * nout * C;
    const int rounds = (items + groups - 1) / groups;
    for (int j = 0; j < rounds; ++j) {
      const int it = slot + j * groups;
      const bool valid = it < items;
      int acc = 0, r = 0, ol = 0, c = 0;
      if (valid) {
        c = it % C;
        const int t = it / C;
        ol = t % nout;
        r = t / nout;
        const int xmin = min(max(bounds[2 * (o0 + ol)], 0), W);
        const int n = min(max(bounds[2 * (o0 + ol) + 1], 0), min(ksize, W - xmin));
        const uintptr_t p = lo + (size_t)(y0 + r0 + r) * src_pitch + (size_t)xs * C;
        const uint8_t* s = reinterpret_cast<const uint8_t*>(s_src) + (size_t)r * ndw * 4 + (p & 3) + (xmin - xs) * C + c;
        const int32_t* k = coeff + (size_t)(o0 + ol) * ksize;
        for (int x = g; x < n; x += G) acc += (int)s[x * C] * k[x];
      }
      for (int m = G >> 1; m; m >>= 1) acc += __shfl_xor(acc, m);
      if (valid && g == 0) reinterpret_cast<uint8_t*>(s_out)[(r0 + r) * (OUT_ROW_DW * 4) + ol * C + c] = clip8(acc);
    }
    __syncthreads();
  }

  // dst and dst_pitch are multiples of 4 and the pitch covers the last dword of a row: whole dwords, padding bytes are written as 0
  const int out_dw = (nout * C + 3) / 4;
  for (int idx = tid; idx < nrows * out_dw; idx += THREADS) {
    const int r = idx / out_dw, k = idx - r * out_dw;
    *reinterpret_cast<uint32_t*>(dst + (size_t)(y0 + r) * dst_pitch + (size_t)o0 * C + 4 * k) = s_out[r * OUT_ROW_DW + k];
  }
}

// ---- k_resize_cols ----------------------------------------------------------------------------------------------
// four bytes at any alignment as one dword access (gfx950 global memory takes unaligned dwords)
__device__ inline uint32_t load4(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
__device__ inline void store4(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

template <int C>
__global__ __launch_bounds__(THREADS) void k_resize_cols(const uint8_t* __restrict__ src, int H, int WCb, int src_pitch,
                                                         const int32_t* __restrict__ coeff, const int32_t* __restrict__ bounds,
                                                         int ksize, int H_out, uint8_t* __restrict__ dst_u8,
                                                         float* __restrict__ dst_cond) {
  const int b = (blockIdx.x * THREADS + threadIdx.x) * 4;             // first of this thread's bytes in the row
  if (b >= WCb) return;
  const int o = blockIdx.y;
  const int ymin = min(max(bounds[2 * o], 0), H);
  const int n = min(max(bounds[2 * o + 1], 0), min(ksize, H - ymin));
  const int nb = min(4, WCb - b);                                     // < 4 only for the last thread of a row
  const int32_t* k = coeff + (size_t)o * ksize;
  const uint8_t* p = src + (size_t)ymin * src_pitch + b;
  int acc[4] = {0, 0, 0, 0};
  if (nb == 4) {
#pragma unroll 4
    for (int x = 0; x < n; ++x, p += src_pitch) {
      const uint32_t v = load4(p);
      const int kx = k[x];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += (int)((v >> (8 * j)) & 0xffu) * kx;
    }
  } else {
    for (int x = 0; x < n; ++x, p += src_pitch) {
      const int kx = k[x];
      for (int j = 0; j < nb; ++j) acc[j] += (int)p[j] * kx;
    }
  }
  uint8_t v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = clip8(acc[j]);
  if (dst_u8) {
    uint8_t* d = dst_u8 + (size_t)o * WCb + b;
    if (nb == 4) {
      store4(d, (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24);
    } else {
      for (int j = 0; j < nb; ++j) d[j] = v[j];
    }
  }
  if (dst_cond) {
    const int W = WCb / C;
    const size_t plane = (size_t)H_out * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= nb) break;
      const float f = __fdiv_rn((float)v[j], 255.0f);                 // a multiply by 1 / 255 differs from the division on some bytes
      if (C == 1) {
        float* d = dst_cond + (size_t)o * W + b + j;
        d[0] = d[plane] = d[2 * plane] = f;
      } else {
        const int x = (b + j) / C, c = (b + j) - x * C;
        dst_cond[c * plane + (size_t)o * W + x] = f;
      }
    }
  }
}

inline bool dim_ok(int v) { return v >= 1 && v <= RESIZE_MAX_DIM; }

}  // namespace

extern "C" {

int ed_resize_rows_u8(const uint8_t* src, int H, int W, int C, int src_pitch, const int32_t* coeff, const int32_t* bounds, int ksize,
                      int W_out, uint8_t* dst, int dst_pitch, void* stream) {
  if (!src || !coeff || !bounds || !dst || (C != 1 && C != 3) || !dim_ok(H) || !dim_ok(W) || !dim_ok(W_out) || ksize < 1)
    return (int)hipErrorInvalidValue;
  if (src_pitch < W * C || (dst_pitch & 3) || dst_pitch < ((W_out * C + 3) & ~3) || ((uintptr_t)dst & 3)) return (int)hipErrorInvalidValue;
  // lanes per output byte: the smallest power of two that leaves each lane at most TAPS_PER_LANE taps, one wavefront at the most
  int G = 1;
  while (G < 64 && (int64_t)G * TAPS_PER_LANE < ksize) G *= 2;
  // rows per tile: as many as the tile's expected span (64 outputs at this scale, plus one filter width) lets into the staging buffer;
  // the kernel works through its rows in as many LDS fills as the real span needs, so this only shapes the grid
  const int nout = W_out < TW ? W_out : TW;
  int64_t span = ((int64_t)nout * W + W_out - 1) / W_out + ksize + 1;
  if (span > W) span = W;
  const int ndw = (int)((span * C + 3) / 4 + 1);
  int TR = SRC_DW / ndw;
  TR = TR < 1 ? 1 : TR > MAX_TR ? MAX_TR : TR;
  const dim3 grid((W_out + TW - 1) / TW, (H + TR - 1) / TR);
  if (C == 1)
    k_resize_rows<1><<<grid, THREADS, 0, (hipStream_t)stream>>>(src, H, W, src_pitch, coeff, bounds, ksize, W_out, dst, dst_pitch, TR, G);
  else
    k_resize_rows<3><<<grid, THREADS, 0, (hipStream_t)stream>>>(src, H, W, src_pitch, coeff, bounds, ksize, W_out, dst, dst_pitch, TR, G);
  return (int)hipGetLastError();
}

int ed_resize_cols_u8(const uint8_t* src, int H, int WC_bytes, int src_pitch, const int32_t* coeff, const int32_t* bounds, int ksize,
                      int H_out, int C, uint8_t* dst_u8, float* dst_cond, void* stream) {
  if (!src || !coeff || !bounds || (!dst_u8 && !dst_cond) || (C != 1 && C != 3) || !dim_ok(H) || !dim_ok(H_out) || ksize < 1)
    return (int)hipErrorInvalidValue;
  if (WC_bytes < 1 || WC_bytes % C != 0 || !dim_ok(WC_bytes / C) || src_pitch < WC_bytes) return (int)hipErrorInvalidValue;
  const dim3 grid((WC_bytes + 4 * THREADS - 1) / (4 * THREADS), H_out);
  if (C == 1)
    k_resize_cols<1><<<grid, THREADS, 0, (hipStream_t)stream>>>(src, H, WC_bytes, src_pitch, coeff, bounds, ksize, H_out, dst_u8, dst_cond);
  else
    k_resize_cols<3><<<grid, THREADS, 0, (hipStream_t)stream>>>(src, H, WC_bytes, src_pitch, coeff, bounds, ksize, H_out, dst_u8, dst_cond);
  return (int)hipGetLastError();
}

}  // extern "C"
