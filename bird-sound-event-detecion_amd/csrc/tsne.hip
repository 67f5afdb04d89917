// Exact t-SNE of an embedding (bsed_tsne_affinities / bsed_tsne_gradient / bsed_tsne_update, ABI 19): the all-pairs
// form of sklearn's TSNE(method="exact") at two components.  The rules -- the perplexity search, the symmetric
// affinities, the gradient of the KL divergence at one degree of freedom, the momentum / gains step -- are stated in
// include/bsed.h; tsne.py drives them.  No atomics, no fence: every sum has an order fixed by its arguments.
//
// Affinities, four launches:
//   d2_tile_kernel          (d2_tile.h, shared with svc.hip; its loop, d2_tile_acc, also with pair_stats.hip) grid
//                           (tiles, tiles), 256 threads: the 64 x 64 squared distances of a tile pair -> P[i][j] =
//                           d2(i, j), symmetric bit for bit, 0 on the diagonal.
//   tsne_search_kernel      one workgroup per row.  The row of d2 stays in LDS while it fits (N <= 32768: 128 KB of the
//                           160 KB; the sums take 128 B); past that the row is re-read from P, which the L2 holds.  Per
//                           step every thread adds exp(-d2 beta) and d2 exp(-d2 beta) of its columns in float64, in
//                           column order; the 256 partials are folded by a fixed tree.  After the last step the row is
//                           overwritten with the conditional probabilities.
//   tsne_symmetrize_kernel  grid (tiles, tiles); the workgroups with tile row <= tile column take a tile and its mirror
//                           image through LDS (rows 65 floats apart) and write p(j|i) + p(i|j) to both; the float32 sum
//                           is commutative, so P is symmetric bit for bit.  Each leaves the float64 sum of what it wrote
//                           as a partial.
//   tsne_total_kernel       one workgroup adds the partials in index order -> sum_p.
// Gradient, three launches (five with want_error):
//   tsne_pairs_kernel       grid (tiles of 64 rows, splits), 256 threads: thread (ty, tx) owns rows 4 ty .. + 3 and,
//                           per tile of 64 columns, columns 4 tx .. + 3 (one 16-byte load of P per row when P allows
//                           it).  P is streamed once; y comes from the cache.  Per pair, in float32: w, P w dy, w^2 dy;
//                           the four columns of a thread are added in float32 in column order, tiles in float64, the
//                           16 threads of a row by the fixed DPP tree of d2_tile.h (d2_row_sum), the column tiles of
//                           a split by its d2_split_range, the split count by d2_auto_splits: pair_stats.hip's rules.
//                           Partials per (split, row):
//                           attraction (2), repulsion (2), sum of w.
//   tsne_rows_kernel        adds the partials of a row in split order.
//   tsne_finish_kernel      one workgroup of 1024: Z in row order, then the gradient, |grad|^2 and the stats.
//   tsne_kl_kernel          (want_error) the same tiling in float64 with Z known: the terms of the KL divergence, one
//                           partial per workgroup;  tsne_kl_finish_kernel adds them in index order.
// Update: one elementwise launch, products unfused (bit for bit what numpy computes in float32).
#include "../../include/bsed.h"
#include "bsed_common.h"
#include "d2_tile.h"
#include <math.h>

#define TSNE_TILE D2_TILE
#define TSNE_THREADS D2_THREADS
#define TSNE_ROW_LDS_MAX 32768           // the longest row of d2 that stays in LDS
#define TSNE_SEARCH_STEPS 100
#define TSNE_EPS 2.220446049250313e-16   // the machine epsilon of float64: sklearn's clamp inside the logarithm

// the sum of v over the workgroup (a multiple of 64 threads, at most 1024), the same value in every thread: a fixed
// tree inside each wave, then the waves in order.  red: 16 doubles of LDS; two barriers
__device__ __forceinline__ double tsne_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  __syncthreads();                                                  // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
  for (int k = 0; k < waves; ++k) s += red[k];
  return s;
}

// ---------------------------------------------------------------------------------------------- affinities
template <bool LDSROW>
__global__ __launch_bounds__(TSNE_THREADS) void tsne_search_kernel(float* __restrict__ P, int N, double log_perplexity,
                                                                   float* __restrict__ beta_out) {
  extern __shared__ __attribute__((aligned(16))) float d2row[];     // N floats when LDSROW
  __shared__ double red[16];
  const int tid = threadIdx.x, i = blockIdx.x;
  float* Pi = P + (size_t)i * N;
  if (LDSROW) {
    for (int j = tid; j < N; j += TSNE_THREADS) d2row[j] = Pi[j];
    __syncthreads();
  }
  double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY, used = 1.0, S = 1.0;
  for (int l = 0; l < TSNE_SEARCH_STEPS; ++l) {
    double s = 0.0, t = 0.0;
    for (int j = tid; j < N; j += TSNE_THREADS)
      if (j != i) {
        const double d = (double)(LDSROW ? d2row[j] : Pi[j]);
        const double e = exp(-d * beta);
        s += e;
        t += d * e;
      }
    S = tsne_block_sum(s, red);
    const double T = tsne_block_sum(t, red);
    if (S == 0.0) S = (double)1e-8f;
    used = beta;
    const double diff = log(S) + beta * (T / S) - log_perplexity;   // the same in every thread: the branches are uniform
    if (fabs(diff) <= (double)1e-5f) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
    }
  }
  // the row keeps the probabilities of the last beta that was EVALUATED (sklearn's P does), not of the step after it
  for (int j = tid; j < N; j += TSNE_THREADS) {
    const double d = (double)(LDSROW ? d2row[j] : Pi[j]);
    Pi[j] = j == i ? 0.f : (float)(exp(-d * used) / S);
  }
  if (tid == 0) beta_out[i] = (float)used;
}

__global__ __launch_bounds__(TSNE_THREADS) void tsne_symmetrize_kernel(float* __restrict__ P, int N,
                                                                       double* __restrict__ partial) {
  __shared__ float A[TSNE_TILE][TSNE_TILE + 1];
  __shared__ float B[TSNE_TILE][TSNE_TILE + 1];
  __shared__ double red[16];
  const int ti = blockIdx.x, tj = blockIdx.y, tiles = gridDim.x;
  if (ti > tj) {                                                    // the mirror image: done by (tj, ti)
    if (threadIdx.x == 0) partial[(size_t)ti * tiles + tj] = 0.0;
    return;
  }
  const int i0 = ti * TSNE_TILE, j0 = tj * TSNE_TILE, c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  for (int r = r0; r < TSNE_TILE; r += 4) {
    A[r][c] = (i0 + r < N && j0 + c < N) ? P[(size_t)(i0 + r) * N + j0 + c] : 0.f;
    B[r][c] = (j0 + r < N && i0 + c < N) ? P[(size_t)(j0 + r) * N + i0 + c] : 0.f;
  }
  __syncthreads();                                                  // every read of P is done before the first write
  double sum = 0.0;
  for (int r = r0; r < TSNE_TILE; r += 4) {
    if (i0 + r < N && j0 + c < N) {
      const float v = A[r][c] + B[c][r];
      P[(size_t)(i0 + r) * N + j0 + c] = v;
      sum += (double)v;
    }
    if (ti != tj && j0 + r < N && i0 + c < N) P[(size_t)(j0 + r) * N + i0 + c] = A[c][r] + B[r][c];
  }
  sum = tsne_block_sum(sum, red);
  if (threadIdx.x == 0) partial[(size_t)ti * tiles + tj] = ti == tj ? sum : 2.0 * sum;
}

__global__ __launch_bounds__(1024) void tsne_total_kernel(const double* __restrict__ partial, size_t n,
                                                          double* __restrict__ out) {
  __shared__ double red[16];
  double s = 0.0;
  for (size_t k = threadIdx.x; k < n; k += 1024) s += partial[k];
  s = tsne_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

// ---------------------------------------------------------------------------------------------- gradient
// the four columns j .. j + 3 of a row of P; zero past N
template <bool VEC>
__device__ __forceinline__ f32x4 tsne_p4(const float* __restrict__ Prow, int j, int N) {
  if (VEC && j + 4 <= N) return *reinterpret_cast<const f32x4*>(Prow + j);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (j < N) v[0] = Prow[j];
  if (j + 1 < N) v[1] = Prow[j + 1];
  if (j + 2 < N) v[2] = Prow[j + 2];
  if (j + 3 < N) v[3] = Prow[j + 3];
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(TSNE_THREADS) void tsne_pairs_kernel(const float* __restrict__ y, const float* __restrict__ P,
                                                                  int N, int splits, double* __restrict__ ws_part) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.x * TSNE_TILE, split = blockIdx.y;
  int t_begin, t_end;
  d2_split_range(N, split, splits, t_begin, t_end);
  float yi[4][2];
  int row[4];
  double acc[4][5];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    row[r] = i0 + ty * 4 + r;
    const int rr = row[r] < N ? row[r] : N - 1;                     // a row past the end: computed, never stored
    yi[r][0] = y[2 * (size_t)rr];
    yi[r][1] = y[2 * (size_t)rr + 1];
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[r][q] = 0.0;
  }
  for (int t = t_begin; t < t_end; ++t) {
    const int j = t * TSNE_TILE + tx * 4;
    float yj[4][2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int jj = j + c < N ? j + c : N - 1;
      yj[c][0] = y[2 * (size_t)jj];
      yj[c][1] = y[2 * (size_t)jj + 1];
    }
    f32x4 p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = row[r] < N ? row[r] : N - 1;
      p[r] = tsne_p4<VEC>(P + (size_t)rr * N, j, N);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, sw = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float dx = yi[r][0] - yj[c][0], dy = yi[r][1] - yj[c][1];
        const float d2 = fmaf(dx, dx, dy * dy);
        const float w = (j + c < N && j + c != row[r]) ? 1.0f / (1.0f + d2) : 0.f;
        const float pw = p[r][c] * w, w2 = w * w;
        ax += pw * dx; ay += pw * dy;
        rx += w2 * dx; ry += w2 * dy;
        sw += w;
      }
      acc[r][0] += (double)ax; acc[r][1] += (double)ay;
      acc[r][2] += (double)rx; acc[r][3] += (double)ry;
      acc[r][4] += (double)sw;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const double v = d2_row_sum(acc[r][q]);
      if (tx == 0 && row[r] < N) ws_part[((size_t)split * N + row[r]) * 5 + q] = v;
    }
}

// element e < 5 N: the sum over the splits, in split order
__global__ __launch_bounds__(256) void tsne_rows_kernel(const double* __restrict__ ws_part, int N, int splits,
                                                        double* __restrict__ ws_rows) {
  const size_t total = (size_t)N * 5, e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  double v = 0.0;
  for (int s = 0; s < splits; ++s) v += ws_part[(size_t)s * total + e];
  ws_rows[e] = v;
}

__global__ __launch_bounds__(1024) void tsne_finish_kernel(const double* __restrict__ ws_rows, int N, double p_scale,
                                                           float* __restrict__ grad, double* __restrict__ stats) {
  __shared__ double red[16];
  double z = 0.0;
  for (int i = threadIdx.x; i < N; i += 1024) z += ws_rows[(size_t)i * 5 + 4];
  const double Z = tsne_block_sum(z, red);
  double g2 = 0.0;
  for (int i = threadIdx.x; i < N; i += 1024) {
    const double* a = ws_rows + (size_t)i * 5;
    const float gx = (float)(4.0 * (p_scale * a[0] - a[2] / Z)), gy = (float)(4.0 * (p_scale * a[1] - a[3] / Z));
    grad[2 * (size_t)i] = gx;
    grad[2 * (size_t)i + 1] = gy;
    g2 += (double)gx * (double)gx + (double)gy * (double)gy;
  }
  g2 = tsne_block_sum(g2, red);
  if (threadIdx.x == 0) {
    stats[0] = Z;
    stats[1] = g2;
    stats[2] = __longlong_as_double(0x7ff8000000000000LL);          // NaN until a want_error launch fills it
  }
}

// the terms p log(max(p, eps) / max(q, eps)) of a workgroup's rows and column range, in float64, Z read from stats[0]
template <bool VEC>
__global__ __launch_bounds__(TSNE_THREADS) void tsne_kl_kernel(const float* __restrict__ y, const float* __restrict__ P,
                                                               int N, int splits, double p_scale,
                                                               const double* __restrict__ stats,
                                                               double* __restrict__ ws_kl) {
  __shared__ double red[16];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.x * TSNE_TILE, split = blockIdx.y;
  int t_begin, t_end;
  d2_split_range(N, split, splits, t_begin, t_end);
  const double Z = stats[0];
  double kl = 0.0;
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + ty * 4 + r;
    if (row >= N) continue;
    const double yx = (double)y[2 * (size_t)row], yy = (double)y[2 * (size_t)row + 1];
    for (int t = t_begin; t < t_end; ++t) {
      const int j = t * TSNE_TILE + tx * 4;
      const f32x4 p4 = tsne_p4<VEC>(P + (size_t)row * N, j, N);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (j + c >= N || j + c == row) continue;
        const double p = (double)p4[c] * p_scale;
        if (!(p > 0.0)) continue;                                   // 0 log(eps / q) = 0
        const double dx = yx - (double)y[2 * (size_t)(j + c)], dy = yy - (double)y[2 * (size_t)(j + c) + 1];
        const double q = 1.0 / (1.0 + (dx * dx + dy * dy)) / Z;
        kl += p * log(fmax(p, TSNE_EPS) / fmax(q, TSNE_EPS));
      }
    }
  }
  kl = tsne_block_sum(kl, red);
  if (tid == 0) ws_kl[(size_t)split * d2_tiles(N) + blockIdx.x] = kl;
}

__global__ __launch_bounds__(1024) void tsne_kl_finish_kernel(const double* __restrict__ ws_kl, size_t n,
                                                              double* __restrict__ stats) {
  __shared__ double red[16];
  double s = 0.0;
  for (size_t k = threadIdx.x; k < n; k += 1024) s += ws_kl[k];
  s = tsne_block_sum(s, red);
  if (threadIdx.x == 0) stats[2] = s;
}

// ---------------------------------------------------------------------------------------------- update
// Every product and sum is rounded on its own, as numpy rounds them in float32: hipcc contracts a * b + c into one fma
// by default, which rounds once and gives other bits (mix.hip): off from here to the end of the file.
#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void tsne_update_kernel(float* __restrict__ y, const float* __restrict__ grad,
                                                          float* __restrict__ update, float* __restrict__ gains, long n,
                                                          float momentum, float learning_rate, float min_gain) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float g = grad[e], u = update[e];
  const float prod = u * g;
  float gain = gains[e];
  gain = prod < 0.0f ? gain + 0.2f : gain * 0.8f;
  gain = gain < min_gain ? min_gain : gain;                         // a NaN stays a NaN, as in np.clip
  const float scaled = g * gain;
  const float mu = momentum * u, step = learning_rate * scaled;
  const float nu = mu - step;
  gains[e] = gain;
  update[e] = nu;
  y[e] = y[e] + nu;
}

// ---------------------------------------------------------------------------------------------- entry points
extern "C" size_t bsed_tsne_affinities_workspace(int N) {
  if (N < 2 || N > BSED_TSNE_MAX_POINTS) return 0;
  const size_t tiles = (size_t)d2_tiles(N);
  return tiles * tiles * sizeof(double);
}

extern "C" int bsed_tsne_affinities(const float* x, long long x_pitch, int N, int D, float perplexity, float* P,
                                    float* beta, double* sum_p, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "bsed_tsne_affinities";
  BSED_CHECK_ARG(x && P && beta && sum_p && workspace, "%s: null pointer", who);
  BSED_CHECK_ARG(N >= 2 && N <= BSED_TSNE_MAX_POINTS, "%s: 2 to %d points, got N=%d", who, BSED_TSNE_MAX_POINTS, N);
  BSED_CHECK_ARG(D >= 1, "%s: D must be at least 1, got %d", who, D);
  BSED_CHECK_ARG(x_pitch >= (long long)D, "%s: x_pitch=%lld is below D=%d", who, x_pitch, D);
  BSED_CHECK_ARG(perplexity > 0.f && perplexity < (float)N, "%s: the perplexity must lie in (0, N=%d), got %g", who, N,
                 (double)perplexity);
  BSED_CHECK_ARG(((uintptr_t)x % 4) == 0 && ((uintptr_t)P % 4) == 0 && ((uintptr_t)beta % 4) == 0 &&
                 ((uintptr_t)sum_p % 8) == 0, "%s: x, P and beta must be 4-byte aligned and sum_p 8-byte aligned", who);
  BSED_CHECK_ARG(((uintptr_t)workspace % 8) == 0, "%s: the workspace must be 8-byte aligned", who);
  const size_t need = bsed_tsne_affinities_workspace(N);
  BSED_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %zu bytes, %zu are needed (N=%d)", who, workspace_bytes,
                 need, N);
  hipStream_t s = (hipStream_t)stream;
  const int tiles = d2_tiles(N);
  double* partial = (double*)workspace;
  d2_launch(x, x_pitch, N, D, P, s);
  BSED_LAUNCH_CHECK();
  const double log_perplexity = log((double)perplexity);
  if (N <= TSNE_ROW_LDS_MAX) {
    static BsedLdsOnce once;
    BSED_HIP(bsed_max_lds(once, (const void*)tsne_search_kernel<true>, TSNE_ROW_LDS_MAX * (int)sizeof(float)));
    hipLaunchKernelGGL(tsne_search_kernel<true>, dim3(N), dim3(TSNE_THREADS), (size_t)N * sizeof(float), s, P, N,
                       log_perplexity, beta);
  } else {
    hipLaunchKernelGGL(tsne_search_kernel<false>, dim3(N), dim3(TSNE_THREADS), 0, s, P, N, log_perplexity, beta);
  }
  BSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsne_symmetrize_kernel, dim3(tiles, tiles), dim3(TSNE_THREADS), 0, s, P, N, partial);
  BSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsne_total_kernel, dim3(1), dim3(1024), 0, s, partial, (size_t)tiles * tiles, sum_p);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

extern "C" int bsed_tsne_gradient_splits(int N) { return N < 1 ? 1 : d2_auto_splits(N); }

extern "C" size_t bsed_tsne_gradient_workspace(int N, int splits) {
  if (N < 2 || N > BSED_TSNE_MAX_POINTS || splits < 0 || splits > D2_MAX_SPLITS) return 0;
  if (splits == 0) splits = d2_auto_splits(N);
  // the partials per (split, row), the sums per row, one KL partial per workgroup
  return ((size_t)splits * N * 5 + (size_t)N * 5 + (size_t)splits * d2_tiles(N)) * sizeof(double);
}

extern "C" int bsed_tsne_gradient(const float* y, const float* P, int N, double inv_sum_p, double exaggeration,
                                  int want_error, int splits, float* grad, double* stats, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  const char* who = "bsed_tsne_gradient";
  BSED_CHECK_ARG(y && P && grad && stats && workspace, "%s: null pointer", who);
  BSED_CHECK_ARG(N >= 2 && N <= BSED_TSNE_MAX_POINTS, "%s: 2 to %d points, got N=%d", who, BSED_TSNE_MAX_POINTS, N);
  BSED_CHECK_ARG(inv_sum_p > 0.0 && inv_sum_p < INFINITY && exaggeration > 0.0 && exaggeration < INFINITY,
                 "%s: inv_sum_p and exaggeration must be positive and finite, got %g and %g", who, inv_sum_p, exaggeration);
  BSED_CHECK_ARG(want_error == 0 || want_error == 1, "%s: want_error must be 0 or 1, got %d", who, want_error);
  BSED_CHECK_ARG(splits >= 0 && splits <= D2_MAX_SPLITS, "%s: splits must be 0 (automatic) to %d, got %d", who,
                 D2_MAX_SPLITS, splits);
  BSED_CHECK_ARG(((uintptr_t)y % 4) == 0 && ((uintptr_t)P % 4) == 0 && ((uintptr_t)grad % 4) == 0 &&
                 ((uintptr_t)stats % 8) == 0, "%s: y, P and grad must be 4-byte aligned and stats 8-byte aligned", who);
  BSED_CHECK_ARG(((uintptr_t)workspace % 8) == 0, "%s: the workspace must be 8-byte aligned", who);
  if (splits == 0) splits = d2_auto_splits(N);
  const size_t need = bsed_tsne_gradient_workspace(N, splits);
  BSED_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %zu bytes, %zu are needed (N=%d, splits=%d)", who,
                 workspace_bytes, need, N, splits);
  hipStream_t s = (hipStream_t)stream;
  const int tiles = d2_tiles(N);
  double* ws_part = (double*)workspace;
  double* ws_rows = ws_part + (size_t)splits * N * 5;
  double* ws_kl = ws_rows + (size_t)N * 5;
  const bool vec = d2_vec_ok(P, N);                                 // P's rows are N floats apart
  const double p_scale = exaggeration * inv_sum_p;
  D2_LAUNCH_VEC(vec, tsne_pairs_kernel, dim3(tiles, splits), 0, s, y, P, N, splits, ws_part);
  BSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsne_rows_kernel, dim3((unsigned)(((size_t)N * 5 + 255) / 256)), dim3(256), 0, s, ws_part, N, splits,
                     ws_rows);
  BSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsne_finish_kernel, dim3(1), dim3(1024), 0, s, ws_rows, N, p_scale, grad, stats);
  BSED_LAUNCH_CHECK();
  if (want_error) {
    D2_LAUNCH_VEC(vec, tsne_kl_kernel, dim3(tiles, splits), 0, s, y, P, N, splits, p_scale, stats, ws_kl);
    BSED_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_kl_finish_kernel, dim3(1), dim3(1024), 0, s, ws_kl, (size_t)splits * tiles, stats);
    BSED_LAUNCH_CHECK();
  }
  return BSED_OK;
}

extern "C" int bsed_tsne_update(float* y, const float* grad, float* update, float* gains, long n, float momentum,
                                float learning_rate, float min_gain, void* stream) {
  const char* who = "bsed_tsne_update";
  BSED_CHECK_ARG(y && grad && update && gains, "%s: null pointer", who);
  BSED_CHECK_ARG(n >= 1 && n <= 2L * BSED_TSNE_MAX_POINTS, "%s: 1 to %ld elements, got n=%ld", who,
                 2L * BSED_TSNE_MAX_POINTS, n);
  BSED_CHECK_ARG(((uintptr_t)y % 4) == 0 && ((uintptr_t)grad % 4) == 0 && ((uintptr_t)update % 4) == 0 &&
                 ((uintptr_t)gains % 4) == 0, "%s: misaligned pointer (4-byte elements)", who);
  hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, grad,
                     update, gains, n, momentum, learning_rate, min_gain);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
