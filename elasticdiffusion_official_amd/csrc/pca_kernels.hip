/*
 * pca_kernels.hip -- the score PCA maps of the reference's diagnostic script (pca_diffusion_scores.py:165-179; DESIGN.md section
 * 26): a 4-channel score [B, 4, H, W] projected onto the first three principal components of each sample's pixels and scaled to
 * bytes [B, H, W, 3], on the device and without a host sync.
 *
 * The rules of elastic_kernels.hip hold here: no atomics, no read-modify-write, deterministic fixed-order merges, and nothing is a
 * contraction worth an MFMA (a 4 x 4 covariance).  The tensors are 8 KiB - 1 MiB, so every launch is latency bound: one pixel per
 * thread per iteration, the four planes read with consecutive lanes on consecutive pixels (4-byte loads: a view that starts at any
 * element of a buffer is accepted).
 *
 *   ed_score_pca_fit
 *     k_pca_extent    (normalize only) grid B * nblk: the minimum and maximum of the block's share of the score, one float pair per
 *                     block.  The reference normalises the class direction, s' = (s - min) / (max - min) * 2 - 1 over the whole
 *                     tensor in fp32, BEFORE the fit; mathematically that moves neither components nor bytes, but its fp32 rounding
 *                     is part of what the reference computes (a score whose channels are almost constant at different levels is
 *                     quantised by it), so every kernel below forms s' per element with the reference's four operations instead of
 *                     transforming the statistics.  Each block merges the B * nblk pairs itself.
 *     k_pca_moments   grid B * nblk (nblk = pca_blocks(n), fixed by the pixel count n = H * W alone): block (b, k) strides over
 *                     sample b and writes ONE partial of 16 doubles: the sums of d_c = x_c - K_c (4), of d_i d_j for i <= j (10),
 *                     the minimum and the maximum of x.  K_c = x_c[pixel 0] of the sample, so the sums stay of the size of the
 *                     spread however large the mean is (the shifted sums of section 16.2).  Wave shuffles, then the 4 waves in order.
 *     k_pca_finalise  one wave per sample: lane l merges partials l, l + 64, ... in order, then a shuffle tree; lane 0 forms mean and
 *                     covariance (/ (n - 1)), diagonalises it with PCA_SWEEPS sweeps of cyclic Jacobi in fp64 (a rotation whose
 *                     off-diagonal is negligible against both diagonal entries is skipped and the entry set to 0), sorts the
 *                     eigenpairs in descending order, turns every kept component so that its entry of largest magnitude is positive
 *                     and writes components / mean / explained variance as fp32.
 *   ed_score_pca_map
 *     k_pca_range     grid B * nblk: r_j = fp32(sum_c (x_c - mean_c) comp[j][c]) per pixel, the sum in fp64 from the fp64 mean and
 *                     components the fit left in the workspace (12 multiply-adds per pixel next to 16 bytes read: free, and it
 *                     makes r the specification's r to the bit -- a score on a lattice of a few fp32 values, such as a class
 *                     direction that is a constant plus rounding noise, puts (r - lo) / (hi - lo) * 255 exactly ON integers, where
 *                     an fp32 contraction would flip half of the bytes); the minimum and maximum over the block's pixels and the
 *                     three components -> one float pair per block.
 *     k_pca_bytes     grid B * ceil(n / 256): every block merges its sample's nblk pairs (one per thread, shuffles, the 4 waves in
 *                     order), recomputes r for its pixels with the same operations and writes
 *                     (uint8)((r - lo) / (hi - lo) * 255) (fp32, truncated; 0 where hi == lo).
 *                     Recomputing costs a second read of 16 bytes per pixel; a projection buffer would cost 12 written + 12 read.
 *   Bytes per pixel and map: 16 read by each of k_pca_moments, k_pca_range and k_pca_bytes, 3 written: 51 (67 with normalize).
 */
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "elastic_hip.h"

namespace {

constexpr int PCA_BLOCK = 256;
constexpr int PCA_PIX_PER_THREAD = 2;   // pixels a thread takes before another block is added ...
constexpr int PCA_MAX_BLOCKS = 256;     // ... up to this many blocks per sample (k_pca_bytes merges one pair per thread)
constexpr int PCA_PART = 16;            // doubles per partial: 4 sums, 10 second moments, min, max
constexpr int PCA_SWEEPS = 10;          // cyclic Jacobi on a 4 x 4 matrix is at rounding level after 5 or 6
constexpr int64_t PCA_MAX_PIXELS = (int64_t)1 << 28;
static_assert(PCA_MAX_BLOCKS <= PCA_BLOCK, "k_pca_bytes reads one partial per thread");

inline int pca_blocks(int64_t n) {
  int64_t g = (n + (int64_t)PCA_BLOCK * PCA_PIX_PER_THREAD - 1) / ((int64_t)PCA_BLOCK * PCA_PIX_PER_THREAD);
  return (int)(g < 1 ? 1 : (g > PCA_MAX_BLOCKS ? PCA_MAX_BLOCKS : g));
}

// workspace: [B * nblk * 16 doubles: moment partials][B * 16 doubles: components (12) and mean (4) in fp64][B * nblk * 2 floats:
// range partials of the projection][B * nblk * 2 floats: extent partials of the score]
inline int64_t ws_basis_offset(int B, int nblk) { return (int64_t)B * nblk * PCA_PART; }            // in doubles
inline int64_t ws_range_offset(int B, int nblk) { return (ws_basis_offset(B, nblk) + (int64_t)B * 16) * 8; }  // in bytes
inline int64_t ws_extent_offset(int B, int nblk) { return ws_range_offset(B, nblk) + (int64_t)B * nblk * 8; }
inline int64_t ws_bytes(int B, int nblk) { return ws_extent_offset(B, nblk) + (int64_t)B * nblk * 8; }

// the reference's normalisation of one element, four fp32 operations; off for a constant tensor (there the reference divides by 0)
struct Affine {
  bool on;
  float lo, span;
  __device__ __forceinline__ float operator()(float x) const {
    return on ? __fsub_rn(__fmul_rn(__fdiv_rn(__fsub_rn(x, lo), span), 2.0f), 1.0f) : x;
  }
};
__device__ __forceinline__ Affine make_affine(float lo, float hi) { return Affine{hi > lo, lo, __fsub_rn(hi, lo)}; }

// block-wide minimum / maximum: shuffles, then the 4 waves in order; every thread returns with the result
__device__ __forceinline__ void block_range(float& lo, float& hi) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_down(lo, off, 64));
    hi = fmaxf(hi, __shfl_down(hi, off, 64));
  }
  __shared__ float part[2][PCA_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[0][wave] = lo, part[1][wave] = hi;
  __syncthreads();
  lo = part[0][0], hi = part[1][0];
#pragma unroll
  for (int w = 1; w < PCA_BLOCK / 64; ++w) lo = fminf(lo, part[0][w]), hi = fmaxf(hi, part[1][w]);
}

__global__ void __launch_bounds__(PCA_BLOCK)
k_pca_extent(const float* __restrict__ score, int64_t n, int nblk, float* __restrict__ extent_partials) {
  const int b = blockIdx.x / nblk, k = blockIdx.x % nblk;
  const float* __restrict__ x = score + (int64_t)b * 4 * n;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = (int64_t)k * PCA_BLOCK + threadIdx.x; i < n; i += (int64_t)nblk * PCA_BLOCK) {
    const float x0 = x[i], x1 = x[n + i], x2 = x[2 * n + i], x3 = x[3 * n + i];
    lo = fminf(fminf(lo, x0), fminf(x1, fminf(x2, x3)));
    hi = fmaxf(fmaxf(hi, x0), fmaxf(x1, fmaxf(x2, x3)));
  }
  block_range(lo, hi);
  if (threadIdx.x == 0) extent_partials[(int64_t)blockIdx.x * 2] = lo, extent_partials[(int64_t)blockIdx.x * 2 + 1] = hi;
}

__global__ void __launch_bounds__(PCA_BLOCK)
k_pca_moments(const float* __restrict__ score, int64_t n, int nblk, const float* __restrict__ extent_partials, int n_extent,
              double* __restrict__ partials) {
  const int b = blockIdx.x / nblk, k = blockIdx.x % nblk;
  const float* __restrict__ x = score + (int64_t)b * 4 * n;
  Affine f = {false, 0.0f, 1.0f};
  if (extent_partials) {  // the whole tensor's extent: every block merges all the pairs, in the same order
    float tlo = INFINITY, thi = -INFINITY;
    for (int q = threadIdx.x; q < n_extent; q += PCA_BLOCK)
      tlo = fminf(tlo, extent_partials[2 * q]), thi = fmaxf(thi, extent_partials[2 * q + 1]);
    block_range(tlo, thi);
    f = make_affine(tlo, thi);
  }
  const double K0 = (double)f(x[0]), K1 = (double)f(x[n]), K2 = (double)f(x[2 * n]), K3 = (double)f(x[3 * n]);
  double v[PCA_PART - 2];
#pragma unroll
  for (int j = 0; j < PCA_PART - 2; ++j) v[j] = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = (int64_t)k * PCA_BLOCK + threadIdx.x; i < n; i += (int64_t)nblk * PCA_BLOCK) {
    const float x0 = x[i], x1 = x[n + i], x2 = x[2 * n + i], x3 = x[3 * n + i];
    lo = fminf(fminf(lo, x0), fminf(x1, fminf(x2, x3)));  // of the score as given
    hi = fmaxf(fmaxf(hi, x0), fmaxf(x1, fmaxf(x2, x3)));
    const double d0 = (double)f(x0) - K0, d1 = (double)f(x1) - K1, d2 = (double)f(x2) - K2, d3 = (double)f(x3) - K3;
    v[0] += d0, v[1] += d1, v[2] += d2, v[3] += d3;
    v[4] += d0 * d0, v[5] += d0 * d1, v[6] += d0 * d2, v[7] += d0 * d3;
    v[8] += d1 * d1, v[9] += d1 * d2, v[10] += d1 * d3;
    v[11] += d2 * d2, v[12] += d2 * d3, v[13] += d3 * d3;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int j = 0; j < PCA_PART - 2; ++j) v[j] += __shfl_down(v[j], off, 64);
    lo = fminf(lo, __shfl_down(lo, off, 64));
    hi = fmaxf(hi, __shfl_down(hi, off, 64));
  }
  __shared__ double part[PCA_BLOCK / 64][PCA_PART];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < PCA_PART - 2; ++j) part[wave][j] = v[j];
    part[wave][PCA_PART - 2] = (double)lo, part[wave][PCA_PART - 1] = (double)hi;
  }
  __syncthreads();
  if (threadIdx.x < PCA_PART) {  // thread j merges value j of the 4 waves in order
    const int j = threadIdx.x;
    double a = part[0][j];
    for (int w = 1; w < PCA_BLOCK / 64; ++w) {
      const double c = part[w][j];
      a = j == PCA_PART - 2 ? fmin(a, c) : (j == PCA_PART - 1 ? fmax(a, c) : a + c);
    }
    partials[(int64_t)blockIdx.x * PCA_PART + j] = a;
  }
}

// one Jacobi rotation of the symmetric A (upper and lower kept equal) in the (P, Q) plane, accumulated into the columns of V
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  const double g = 100.0 * fabs(apq);
  if (fabs(A[P][P]) + g == fabs(A[P][P]) && fabs(A[Q][Q]) + g == fabs(A[Q][Q])) {  // negligible (0 included): theta would overflow
    A[P][Q] = A[Q][P] = 0.0;
    return;
  }
  const double h = A[Q][Q] - A[P][P];
  double t;
  if (fabs(h) + g == fabs(h)) {
    t = apq / h;
  } else {
    const double theta = 0.5 * h / apq;
    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
  }
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  A[P][P] -= t * apq;
  A[Q][Q] += t * apq;
  A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const double arp = A[r][P], arq = A[r][Q];
      A[r][P] = A[P][r] = c * arp - s * arq;
      A[r][Q] = A[Q][r] = s * arp + c * arq;
    }
    const double vrp = V[r][P], vrq = V[r][Q];
    V[r][P] = c * vrp - s * vrq;
    V[r][Q] = s * vrp + c * vrq;
  }
}

template <int I, int J>
__device__ __forceinline__ void order_pair(double (&w)[4], double (&V)[4][4]) {  // the larger eigenvalue (and its column) to I
  if (w[J] > w[I]) {
    const double t = w[I];
    w[I] = w[J], w[J] = t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double u = V[r][I];
      V[r][I] = V[r][J], V[r][J] = u;
    }
  }
}

__global__ void __launch_bounds__(64)
k_pca_finalise(const double* __restrict__ partials, const float* __restrict__ score, int B, int64_t n, int nblk, int normalize,
               float* __restrict__ components, float* __restrict__ mean, float* __restrict__ variance, float* __restrict__ norm,
               double* __restrict__ basis64) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double v[PCA_PART - 2];
#pragma unroll
  for (int j = 0; j < PCA_PART - 2; ++j) v[j] = 0.0;
  const double* p = partials + (int64_t)b * nblk * PCA_PART;
  for (int k = lane; k < nblk; k += 64) {
#pragma unroll
    for (int j = 0; j < PCA_PART - 2; ++j) v[j] += p[k * PCA_PART + j];
  }
  double lo = INFINITY, hi = -INFINITY;  // of the WHOLE tensor: the reference normalises with one minimum and one maximum
  for (int k = lane; k < B * nblk; k += 64) {
    lo = fmin(lo, partials[(int64_t)k * PCA_PART + PCA_PART - 2]);
    hi = fmax(hi, partials[(int64_t)k * PCA_PART + PCA_PART - 1]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int j = 0; j < PCA_PART - 2; ++j) v[j] += __shfl_down(v[j], off, 64);
    lo = fmin(lo, __shfl_down(lo, off, 64));
    hi = fmax(hi, __shfl_down(hi, off, 64));
  }
  if (lane != 0) return;

  const float* x = score + (int64_t)b * 4 * n;
  const Affine f = normalize ? make_affine((float)lo, (float)hi) : Affine{false, 0.0f, 1.0f};  // as k_pca_moments had it
  const double nn = (double)n;
  double mu[4], m[4], A[4][4], V[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    mu[c] = v[c] / nn;
    m[c] = (double)f(x[(int64_t)c * n]) + mu[c];
  }
  {
    int q = 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = i; j < 4; ++j, ++q) A[i][j] = A[j][i] = (v[q] - v[i] * mu[j]) / (nn - 1.0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < PCA_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1>(A, V);
    jacobi_rotate<0, 2>(A, V);
    jacobi_rotate<0, 3>(A, V);
    jacobi_rotate<1, 2>(A, V);
    jacobi_rotate<1, 3>(A, V);
    jacobi_rotate<2, 3>(A, V);
  }
  double w[4] = {A[0][0], A[1][1], A[2][2], A[3][3]};
  order_pair<0, 1>(w, V);  // a sorting network of 5 comparisons: descending
  order_pair<2, 3>(w, V);
  order_pair<0, 2>(w, V);
  order_pair<1, 3>(w, V);
  order_pair<1, 2>(w, V);

#pragma unroll
  for (int j = 0; j < 3; ++j) {
    int best = 0;
#pragma unroll
    for (int c = 1; c < 4; ++c) {
      if (fabs(V[c][j]) > fabs(V[best][j])) best = c;
    }
    const double sign = V[best][j] < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      components[((int64_t)b * 3 + j) * 4 + c] = (float)(sign * V[c][j]);
      basis64[(int64_t)b * 16 + j * 4 + c] = sign * V[c][j];
    }
    variance[(int64_t)b * 3 + j] = (float)fmax(w[j], 0.0);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    mean[(int64_t)b * 4 + c] = (float)m[c];
    basis64[(int64_t)b * 16 + 12 + c] = m[c];
  }
  norm[(int64_t)b * 2] = (float)lo, norm[(int64_t)b * 2 + 1] = (float)hi;
}

struct Basis {  // one sample's components and mean as the fit left them, fp64
  double c[3][4], m[4];
};
__device__ __forceinline__ Basis load_basis(const double* __restrict__ basis64, int b) {
  Basis s;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s.c[j][c] = basis64[(int64_t)b * 16 + j * 4 + c];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) s.m[c] = basis64[(int64_t)b * 16 + 12 + c];
  return s;
}
// r_j = fp32(((d0 c_j0 + d1 c_j1) + d2 c_j2) + d3 c_j3) in fp64 (no contraction: the file is compiled with -ffp-contract=off), the
// same operations in k_pca_range and k_pca_bytes: the same bits
__device__ __forceinline__ void project(const float* __restrict__ x, int64_t n, int64_t i, const Affine& f, const Basis& s,
                                        float (&r)[3]) {
  const double d0 = (double)f(x[i]) - s.m[0], d1 = (double)f(x[n + i]) - s.m[1], d2 = (double)f(x[2 * n + i]) - s.m[2],
               d3 = (double)f(x[3 * n + i]) - s.m[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) r[j] = (float)(((d0 * s.c[j][0] + d1 * s.c[j][1]) + d2 * s.c[j][2]) + d3 * s.c[j][3]);
}

__global__ void __launch_bounds__(PCA_BLOCK)
k_pca_range(const float* __restrict__ score, int64_t n, int nblk, const double* __restrict__ basis64,
            const float* __restrict__ norm, float* __restrict__ range_partials) {
  const int b = blockIdx.x / nblk, k = blockIdx.x % nblk;
  const float* __restrict__ x = score + (int64_t)b * 4 * n;
  const Basis s = load_basis(basis64, b);
  const Affine f = norm ? make_affine(norm[0], norm[1]) : Affine{false, 0.0f, 1.0f};
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = (int64_t)k * PCA_BLOCK + threadIdx.x; i < n; i += (int64_t)nblk * PCA_BLOCK) {
    float r[3];
    project(x, n, i, f, s, r);
    lo = fminf(fminf(lo, r[0]), fminf(r[1], r[2]));
    hi = fmaxf(fmaxf(hi, r[0]), fmaxf(r[1], r[2]));
  }
  block_range(lo, hi);
  if (threadIdx.x == 0) range_partials[(int64_t)blockIdx.x * 2] = lo, range_partials[(int64_t)blockIdx.x * 2 + 1] = hi;
}

__global__ void __launch_bounds__(PCA_BLOCK)
k_pca_bytes(const float* __restrict__ score, int64_t n, int nblk, int blocks_per_sample, const double* __restrict__ basis64,
            const float* __restrict__ norm, const float* __restrict__ range_partials, uint8_t* __restrict__ out) {
  const int b = blockIdx.x / blocks_per_sample, k = blockIdx.x % blocks_per_sample;
  float lo = INFINITY, hi = -INFINITY;
  if ((int)threadIdx.x < nblk) {
    lo = range_partials[((int64_t)b * nblk + threadIdx.x) * 2];
    hi = range_partials[((int64_t)b * nblk + threadIdx.x) * 2 + 1];
  }
  block_range(lo, hi);
  const int64_t i = (int64_t)k * PCA_BLOCK + threadIdx.x;
  if (i >= n) return;
  const Basis s = load_basis(basis64, b);
  const Affine f = norm ? make_affine(norm[0], norm[1]) : Affine{false, 0.0f, 1.0f};
  float r[3];
  project(score + (int64_t)b * 4 * n, n, i, f, s, r);
  const float span = __fsub_rn(hi, lo);
  uint8_t* o = out + ((int64_t)b * n + i) * 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // in [0, 255] by construction; fminf / fmaxf also turn a NaN (a non-finite score) into a byte
    const float q = __fmul_rn(__fdiv_rn(__fsub_rn(r[j], lo), span), 255.0f);
    o[j] = hi > lo ? (uint8_t)(int)fminf(fmaxf(q, 0.0f), 255.0f) : (uint8_t)0;
  }
}

struct Span {
  const void* p;
  int64_t bytes;
};
// every buffer present, aligned to `align[i]`, and no two of them sharing a byte
inline bool spans_ok(const Span* s, const int* align, int count) {
  for (int i = 0; i < count; ++i) {
    if (!s[i].p || s[i].bytes <= 0 || (((uintptr_t)s[i].p) & (uintptr_t)(align[i] - 1)) != 0) return false;
    for (int j = 0; j < i; ++j) {
      const uintptr_t a0 = (uintptr_t)s[i].p, a1 = a0 + (uintptr_t)s[i].bytes, b0 = (uintptr_t)s[j].p, b1 = b0 + (uintptr_t)s[j].bytes;
      if (a0 < b1 && b0 < a1) return false;
    }
  }
  return true;
}
inline bool shape_ok(int B, int C, int H, int W) {
  return B >= 1 && C == 4 && H >= 1 && W >= 1 && (int64_t)H * W >= 4 && (int64_t)H * W <= PCA_MAX_PIXELS &&
         (int64_t)B * (((int64_t)H * W + PCA_BLOCK - 1) / PCA_BLOCK) <= INT_MAX;
}

}  // namespace

extern "C" {

int64_t ed_score_pca_workspace(int B, int64_t n) {
  if (B <= 0 || n < 4 || n > PCA_MAX_PIXELS) return 0;
  return ws_bytes(B, pca_blocks(n));
}

int ed_score_pca_fit(const float* score, int B, int C, int H, int W, int normalize, float* components, float* mean,
                     float* explained_variance, float* norm, void* workspace, void* stream) {
  if (!shape_ok(B, C, H, W)) return (int)hipErrorInvalidValue;
  const int64_t n = (int64_t)H * W;
  const int nblk = pca_blocks(n);
  const Span spans[6] = {{score, (int64_t)B * 4 * n * 4}, {components, (int64_t)B * 48}, {mean, (int64_t)B * 16},
                         {explained_variance, (int64_t)B * 12}, {norm, (int64_t)B * 8}, {workspace, ws_bytes(B, nblk)}};
  const int align[6] = {4, 4, 4, 4, 4, 8};
  if (!spans_ok(spans, align, 6)) return (int)hipErrorInvalidValue;
  double* ws = (double*)workspace;
  float* extent = normalize ? (float*)((char*)workspace + ws_extent_offset(B, nblk)) : nullptr;
  if (normalize) k_pca_extent<<<B * nblk, PCA_BLOCK, 0, (hipStream_t)stream>>>(score, n, nblk, extent);
  k_pca_moments<<<B * nblk, PCA_BLOCK, 0, (hipStream_t)stream>>>(score, n, nblk, extent, B * nblk, ws);
  k_pca_finalise<<<B, 64, 0, (hipStream_t)stream>>>(ws, score, B, n, nblk, normalize, components, mean, explained_variance, norm,
                                                    ws + ws_basis_offset(B, nblk));
  return (int)hipGetLastError();
}

int ed_score_pca_map(const float* score, int B, int C, int H, int W, const float* norm, uint8_t* out, void* workspace,
                     void* stream) {
  if (!shape_ok(B, C, H, W)) return (int)hipErrorInvalidValue;
  const int64_t n = (int64_t)H * W;
  const int nblk = pca_blocks(n);
  // norm is optional: present, it must be a buffer of its own like the others
  const Span spans[4] = {{score, (int64_t)B * 4 * n * 4}, {out, (int64_t)B * n * 3}, {workspace, ws_bytes(B, nblk)},
                         {norm, (int64_t)B * 8}};
  const int align[4] = {4, 1, 8, 4};
  if (!spans_ok(spans, align, norm ? 4 : 3)) return (int)hipErrorInvalidValue;
  const double* basis64 = (const double*)workspace + ws_basis_offset(B, nblk);
  float* range_partials = (float*)((char*)workspace + ws_range_offset(B, nblk));
  const int per_sample = (int)((n + PCA_BLOCK - 1) / PCA_BLOCK);
  k_pca_range<<<B * nblk, PCA_BLOCK, 0, (hipStream_t)stream>>>(score, n, nblk, basis64, norm, range_partials);
  k_pca_bytes<<<B * per_sample, PCA_BLOCK, 0, (hipStream_t)stream>>>(score, n, nblk, per_sample, basis64, norm, range_partials,
                                                                      out);
  return (int)hipGetLastError();
}

}  // extern "C"
