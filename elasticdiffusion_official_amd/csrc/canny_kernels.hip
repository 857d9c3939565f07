/*
 * canny_kernels.hip -- the Canny edge detector behind ElasticDiffusionControlNet.process_condition_image('canny')
 * (EDC:1102-1110: cv2.Canny(img, 100, 200) replicated to three channels).  Pre-processing of ONE image before the
 * denoising loop starts: three kernels, no gradient / magnitude image in HBM.
 *
 * The algorithm is OpenCV 4.x cv::Canny(src, edges, t1, t2, apertureSize = 3, L2gradient = false) for 8-bit input,
 * restated in DESIGN.md ("Canny condition extraction") and in tests/canny_cpu.py.  All arithmetic is integer: the
 * result is exact and independent of the order of evaluation.
 *
 *   k_canny_map         uint8 HWC image -> uint8 map (1 = not an edge, 0 = candidate, 2 = strong): Sobel 3x3 with a
 *                       replicated border, L1 magnitude, channel of the largest magnitude, non-maximum suppression,
 *                       thresholds.  One workgroup per 64 x 16 tile.
 *   k_canny_hysteresis  one pass of the hysteresis flood: per 64 x 32 tile, flood inside LDS until the tile is stable.
 *                       The host relaunches until a pass promotes nothing.
 *   k_canny_edges       map -> uint8 H x W x 3 edge image (255 / 0) and / or the fp32 (1,3,H,W) condition (1.0 / 0.0).
 *
 * Global memory is read as dwords and unpacked (a row of an H x W x 3 byte image starts at any byte alignment, so
 * every staging loop works on the aligned dwords that cover its byte range and keeps the bytes inside the range).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "elastic_hip.h"

namespace {

constexpr int CANNY_MAX_DIM = 8192;
constexpr int THREADS = 256;

// ---- k_canny_map ------------------------------------------------------------------------------------------------
constexpr int MAP_TW = 64, MAP_TH = 16;                 // output tile
constexpr int IN_W = MAP_TW + 4, IN_H = MAP_TH + 4;     // staged input: tile + 2-pixel halo
constexpr int G_W = MAP_TW + 2, G_H = MAP_TH + 2;       // magnitude: tile + 1-pixel ring

// dword at byte offset a (a % 4 == 0) of a buffer of `total` bytes; the last, partial dword is assembled from bytes
__device__ inline uint32_t load_dword(const uint8_t* base, size_t a, size_t total) {
  if (a + 4 <= total) return *reinterpret_cast<const uint32_t*>(base + a);
  uint32_t v = 0;
  for (int j = 0; j < 4; ++j)
    if (a + j < total) v |= (uint32_t)base[a + j] << (8 * j);
  return v;
}

template <int C>
__global__ __launch_bounds__(THREADS) void k_canny_map(const uint8_t* __restrict__ img, int H, int W, int low, int high,
                                                       uint8_t* __restrict__ map) {
  constexpr int NDW = (IN_W * C + 3) / 4 + 1;           // dwords that cover one staged row at any byte alignment
  constexpr int ROWB = NDW * 4;                         // LDS row stride in bytes
  __shared__ uint8_t s_in[IN_H * ROWB];                 // s_in[r][(x - (x0 - 2)) * C + c], r <-> y = clamp(y0 - 2 + r)
  __shared__ uint16_t s_m[G_H * G_W];                   // magnitude (<= 2040), 0 outside the image
  __shared__ uint32_t s_g[MAP_TH * MAP_TW];             // (dx & 0xffff) | (dy << 16) of the selected channel
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * MAP_TW, y0 = blockIdx.y * MAP_TH;
  const int xs = max(x0 - 2, 0), xe = min(x0 + MAP_TW + 2, W);        // staged columns [xs, xe), all inside the image
  const size_t total = (size_t)H * W * C;

  for (int idx = tid; idx < IN_H * NDW; idx += THREADS) {
    const int r = idx / NDW, k = idx - r * NDW;
    const int y = min(max(y0 - 2 + r, 0), H - 1);
    const size_t gb0 = ((size_t)y * W + xs) * C, gb1 = ((size_t)y * W + xe) * C;   // byte range of this row
    const size_t a = (gb0 & ~(size_t)3) + 4 * (size_t)k;
    if (a >= gb1) continue;
    const uint32_t v = load_dword(img, a, total);
    uint8_t* dst = s_in + r * ROWB + (xs - (x0 - 2)) * C;                           // where byte gb0 lands
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t b = a + j;
      if (b >= gb0 && b < gb1) dst[b - gb0] = (uint8_t)(v >> (8 * j));
    }
  }
  __syncthreads();

  // gradients of the tile + 1 ring; the replicated border is a clamp of the coordinates (every clamped coordinate is staged)
  for (int p = tid; p < G_H * G_W; p += THREADS) {
    const int gy = p / G_W, gx = p - gy * G_W;
    const int y = y0 - 1 + gy, x = x0 - 1 + gx;
    int m = 0, bdx = 0, bdy = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const uint8_t* r0 = s_in + (max(y - 1, 0) - (y0 - 2)) * ROWB;
      const uint8_t* r1 = s_in + (y - (y0 - 2)) * ROWB;
      const uint8_t* r2 = s_in + (min(y + 1, H - 1) - (y0 - 2)) * ROWB;
      const int c0 = (max(x - 1, 0) - (x0 - 2)) * C, c1 = (x - (x0 - 2)) * C, c2 = (min(x + 1, W - 1) - (x0 - 2)) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int a00 = r0[c0 + c], a01 = r0[c1 + c], a02 = r0[c2 + c];
        const int a10 = r1[c0 + c], a12 = r1[c2 + c];
        const int a20 = r2[c0 + c], a21 = r2[c1 + c], a22 = r2[c2 + c];
        const int dx = (a02 - a00) + 2 * (a12 - a10) + (a22 - a20);
        const int dy = (a20 - a00) + 2 * (a21 - a01) + (a22 - a02);
        const int n = abs(dx) + abs(dy);
        if (c == 0 || n > m) {          // strict >: ties go to the lowest channel
          m = n;
          bdx = dx;
          bdy = dy;
        }
      }
    }
    s_m[p] = (uint16_t)m;
    if (gy >= 1 && gy <= MAP_TH && gx >= 1 && gx <= MAP_TW)
      s_g[(gy - 1) * MAP_TW + gx - 1] = ((uint32_t)bdx & 0xffffu) | ((uint32_t)bdy << 16);
  }
  __syncthreads();

  // non-maximum suppression + thresholds: 4 adjacent pixels per thread, one dword store where the row allows it
  const int ty = tid / (MAP_TW / 4), cx = (tid % (MAP_TW / 4)) * 4;
  const int y = y0 + ty, x = x0 + cx;
  if (y >= H || x >= W) return;
  uint32_t packed = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint16_t* mc = s_m + (ty + 1) * G_W + cx + j + 1;
    const int m = mc[0];
    uint32_t code = 1;
    if (m > low) {
      const uint32_t g = s_g[ty * MAP_TW + cx + j];
      const int dx = (int16_t)(g & 0xffffu), dy = (int32_t)g >> 16;
      const int ax = abs(dx), ay = abs(dy) << 15;
      const int tg22x = ax * 13573, tg67x = tg22x + (ax << 16);
      bool keep;
      if (ay < tg22x) {
        keep = m > mc[-1] && m >= mc[1];
      } else if (ay > tg67x) {
        keep = m > mc[-G_W] && m >= mc[G_W];
      } else {
        const int s = ((dx ^ dy) < 0) ? -1 : 1;
        keep = m > mc[-G_W - s] && m > mc[G_W + s];
      }
      if (keep) code = m > high ? 2 : 0;
    }
    packed |= code << (8 * j);
  }
  uint8_t* dst = map + (size_t)y * W + x;
  if ((W & 3) == 0 && x + 4 <= W) {
    *reinterpret_cast<uint32_t*>(dst) = packed;
  } else {
    for (int j = 0; j < 4 && x + j < W; ++j) dst[j] = (uint8_t)(packed >> (8 * j));
  }
}

// ---- k_canny_hysteresis -----------------------------------------------------------------------------------------
constexpr int HY_TW = 64, HY_TH = 32;                   // tile; each thread owns 8 adjacent pixels of one row
constexpr int HY_LW = HY_TW + 2, HY_LH = HY_TH + 2;     // tile + 1-pixel halo
constexpr int HY_NDW = (HY_LW + 3) / 4 + 1;
constexpr int HY_ROWB = HY_NDW * 4;

/*
 * One global pass.  A candidate (0) becomes strong (2) when one of its 8 neighbours is strong; the tile repeats that inside
 * LDS until nothing in it changes, then writes the promoted bytes and counts itself in *changed.
 *
 * Why concurrent tiles need no ordering: promotion is monotone (a byte only ever goes 0 -> 2, and only the workgroup that
 * owns a pixel writes it).  A halo byte read while the neighbouring tile is still promoting is either the old 0 or the new 2.
 * A stale 0 can only DELAY a promotion that the next pass makes (the neighbour's write is visible by then, and the pass that
 * wrote it raised *changed, so there is a next pass); it can never cause a promotion that the sequential flood would not
 * make, because every 2 in memory is a pixel connected to a strong pixel.  The same holds inside the tile, where threads read
 * LDS bytes that other threads are promoting in the same sweep.  The fixed point (no pass changes anything) is the unique
 * closure, whatever order the tiles ran in.
 */
__global__ __launch_bounds__(THREADS) void k_canny_hysteresis(uint8_t* map, int H, int W, uint32_t* changed) {
  __shared__ __attribute__((aligned(16))) uint8_t s[HY_LH * HY_ROWB];   // filled as dwords
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * HY_TW, y0 = blockIdx.y * HY_TH;
  const int xs = max(x0 - 1, 0), xe = min(x0 + HY_TW + 1, W);
  const size_t total = (size_t)H * W;

  for (int i = tid; i < HY_LH * HY_ROWB / 4; i += THREADS) reinterpret_cast<uint32_t*>(s)[i] = 0x01010101u;   // outside = not an edge
  __syncthreads();
  for (int idx = tid; idx < HY_LH * HY_NDW; idx += THREADS) {
    const int r = idx / HY_NDW, k = idx - r * HY_NDW;
    const int y = y0 - 1 + r;
    if (y < 0 || y >= H) continue;
    const size_t gb0 = (size_t)y * W + xs, gb1 = (size_t)y * W + xe;
    const size_t a = (gb0 & ~(size_t)3) + 4 * (size_t)k;
    if (a >= gb1) continue;
    const uint32_t v = load_dword(map, a, total);
    uint8_t* dst = s + r * HY_ROWB + (xs - (x0 - 1));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t b = a + j;
      if (b >= gb0 && b < gb1) dst[b - gb0] = (uint8_t)(v >> (8 * j));
    }
  }
  __syncthreads();

  const int ty = tid / (HY_TW / 8), cx = (tid % (HY_TW / 8)) * 8;
  uint8_t* own = s + (ty + 1) * HY_ROWB + cx + 1;      // own[j] = pixel (y0 + ty, x0 + cx + j); pixels outside the image hold 1
  uint32_t cand = 0, promoted = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (own[j] == 0) cand |= 1u << j;
  for (;;) {
    int ch = 0;
    for (uint32_t rest = cand; rest; rest &= rest - 1) {
      const int j = __ffs(rest) - 1;
      const uint8_t* c = own + j;
      const bool strong = c[-HY_ROWB - 1] == 2 || c[-HY_ROWB] == 2 || c[-HY_ROWB + 1] == 2 || c[-1] == 2 || c[1] == 2 ||
                          c[HY_ROWB - 1] == 2 || c[HY_ROWB] == 2 || c[HY_ROWB + 1] == 2;
      if (strong) {
        own[j] = 2;
        cand &= ~(1u << j);
        promoted |= 1u << j;
        ch = 1;
      }
    }
    if (!__syncthreads_or(ch)) break;
  }
  for (uint32_t rest = promoted; rest; rest &= rest - 1) {
    const int j = __ffs(rest) - 1;
    map[(size_t)(y0 + ty) * W + x0 + cx + j] = 2;      // only pixels inside the image were ever candidates
  }
  if (__syncthreads_or(promoted != 0) && tid == 0) atomicAdd(changed, 1u);
}

// ---- k_canny_edges ----------------------------------------------------------------------------------------------
// 4 pixels per thread over the flat map: one dword in, three dwords of HWC bytes and / or three float4 (one per plane) out.
__global__ __launch_bounds__(THREADS) void k_canny_edges(const uint8_t* __restrict__ map, size_t n, uint8_t* __restrict__ edges,
                                                         float* __restrict__ cond) {
  const size_t a = ((size_t)blockIdx.x * THREADS + threadIdx.x) * 4;
  if (a >= n) return;
  const uint32_t v = load_dword(map, a, n);
  bool e[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = ((v >> (8 * j)) & 0xffu) == 2u;
  if (a + 4 <= n) {
    if (edges) {
      const uint32_t b0 = e[0] ? 0xffu : 0u, b1 = e[1] ? 0xffu : 0u, b2 = e[2] ? 0xffu : 0u, b3 = e[3] ? 0xffu : 0u;
      uint32_t* d = reinterpret_cast<uint32_t*>(edges + 3 * a);           // 3 a is a multiple of 4
      d[0] = b0 * 0x010101u | b1 << 24;
      d[1] = b1 * 0x0101u | b2 * 0x01010000u;
      d[2] = b2 | b3 * 0x01010100u;
    }
    if (cond) {
      const float4 f = make_float4(e[0] ? 1.f : 0.f, e[1] ? 1.f : 0.f, e[2] ? 1.f : 0.f, e[3] ? 1.f : 0.f);
      if ((n & 3) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(cond + c * n + a) = f;
      } else {
        for (int c = 0; c < 3; ++c) {
          float* d = cond + c * n + a;
          d[0] = f.x, d[1] = f.y, d[2] = f.z, d[3] = f.w;
        }
      }
    }
  } else {
    for (int j = 0; a + j < n; ++j) {
      if (edges) edges[3 * (a + j)] = edges[3 * (a + j) + 1] = edges[3 * (a + j) + 2] = e[j] ? 255 : 0;
      if (cond) cond[a + j] = cond[n + a + j] = cond[2 * n + a + j] = e[j] ? 1.f : 0.f;
    }
  }
}

inline bool dims_ok(int H, int W) { return H >= 1 && H <= CANNY_MAX_DIM && W >= 1 && W <= CANNY_MAX_DIM; }

}  // namespace

extern "C" {

int64_t ed_canny_workspace(int H, int W, int C) {
  if (!dims_ok(H, W) || (C != 1 && C != 3)) return -1;
  return 256;                                           // the "a tile changed" counter of ed_canny_hysteresis
}

int ed_canny_map(const uint8_t* img, int H, int W, int C, int low, int high, uint8_t* map, void* stream) {
  if (!img || !map || !dims_ok(H, W) || (C != 1 && C != 3)) return (int)hipErrorInvalidValue;
  if (low > high) {
    const int t = low;
    low = high;
    high = t;
  }
  const dim3 grid((W + MAP_TW - 1) / MAP_TW, (H + MAP_TH - 1) / MAP_TH);
  if (C == 1)
    k_canny_map<1><<<grid, THREADS, 0, (hipStream_t)stream>>>(img, H, W, low, high, map);
  else
    k_canny_map<3><<<grid, THREADS, 0, (hipStream_t)stream>>>(img, H, W, low, high, map);
  return (int)hipGetLastError();
}

int ed_canny_hysteresis(uint8_t* map, int H, int W, void* workspace, int32_t* passes_out, void* stream) {
  if (!map || !workspace || !passes_out || !dims_ok(H, W)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* changed = (uint32_t*)workspace;
  hipError_t e = hipMemsetAsync(changed, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((W + HY_TW - 1) / HY_TW, (H + HY_TH - 1) / HY_TH);
  // every pass but the last promotes at least one pixel, so H W + 1 passes cannot be exceeded; reaching the cap means the
  // flood is broken and is reported, never returned as a truncated result
  const int64_t cap = (int64_t)H * W + 1;
  uint32_t seen = 0, now = 0;
  int64_t passes = 0;
  *passes_out = 0;
  for (;;) {
    if (passes >= cap) return (int)hipErrorUnknown;
    k_canny_hysteresis<<<grid, THREADS, 0, s>>>(map, H, W, changed);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = hipMemcpyAsync(&now, changed, sizeof(uint32_t), hipMemcpyDeviceToHost, s)) != hipSuccess) return (int)e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return (int)e;
    *passes_out = (int32_t)++passes;
    if (now == seen) return 0;                          // the counter only grows: unchanged = this pass promoted nothing
    seen = now;
  }
}

int ed_canny_edges(const uint8_t* map, int H, int W, uint8_t* edges, float* cond, void* stream) {
  if (!map || (!edges && !cond) || !dims_ok(H, W)) return (int)hipErrorInvalidValue;
  const size_t n = (size_t)H * W;
  const unsigned blocks = (unsigned)((n + 4 * THREADS - 1) / (4 * THREADS));
  k_canny_edges<<<blocks, THREADS, 0, (hipStream_t)stream>>>(map, n, edges, cond);
  return (int)hipGetLastError();
}

}  // extern "C"
