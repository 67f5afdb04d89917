// The domain gap of an embedding: one all-pairs pass over N points of D float32 features (bsed_pair_stats, ABI 17).
// The definitions -- d2 by direct differences in float32, its correctly rounded root, the float64 sums per (point,
// group) of the roots and of expf(-(d2 * scale)), the nearest neighbour with the smallest index on a tie -- are stated
// in include/bsed.h; the silhouette, the nearest-neighbour domain accuracy and the multi-kernel MMD are host arithmetic
// on these sums (domain_gap.py).
//
// Two launches, no atomics, no fence:
//   pair_stats_kernel   grid (row tiles, splits), 256 threads.  A workgroup owns D2_TILE = 64 rows and the contiguous
//                       range [split * T / splits, (split + 1) * T / splits) of the T column tiles of 64 points
//                       (d2_split_range).  Per column tile the 64 x 64 squared distances are formed 4 x 4 per thread by
//                       d2_tile_acc (d2_tile.h: the staging through LDS, its pitch and its unrolling are argued there;
//                       the same device code as tsne.hip's and svc.hip's d2, so the same bits).  The tile's labels are
//                       published to LDS between the two barriers of its first chunk.  Epilogue per pair: label from LDS
//                       (-1 = masked, out of range, or the point itself), root, up to 8 expf; the four columns of a
//                       thread are added in float64 in column order per (row, group), the 16 threads of a row are folded
//                       by a fixed DPP tree (d2_row_sum) and the row's first thread adds the result to the workgroup's
//                       float64 sums in LDS (only it ever touches them).  At the end of its range the workgroup writes
//                       its sums and its nearest neighbours as partials of its split to the workspace.
//   pair_finish_kernel  adds the partials in split order and takes the nearest neighbour of the splits (smaller d2, then
//                       smaller index).
// Every sum has an order fixed by (N, D, G, S, splits): two launches with the same arguments give the same bits.
// LDS: 2 * 64 * 36 * 4 B of staging + 64 * 4 B of labels + 64 * G * (1 + S) * 8 B of sums (dynamic): 18.7 KB + 6 KB at
// G = 2, S = 5; 55.5 KB at G = 8, S = 8.
#include "../../include/bsed.h"
#include "bsed_common.h"
#include "d2_tile.h"
#include <math.h>

template <bool VEC>
__global__ __launch_bounds__(D2_THREADS) void pair_stats_kernel(
    const float* __restrict__ x, long long pitch, int N, int D, const int* __restrict__ group, int G,
    const float* __restrict__ scale, int S, int splits, double* __restrict__ ws_sum, float* __restrict__ ws_d2,
    int* __restrict__ ws_index) {
  __shared__ __attribute__((aligned(16))) float As[D2_TILE * D2_LD];
  __shared__ __attribute__((aligned(16))) float Bs[D2_TILE * D2_LD];
  __shared__ int lab[D2_TILE];
  extern __shared__ __attribute__((aligned(16))) double sums[];    // [64 rows][G][1 + S]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int Q = 1 + S;
  const int i0 = blockIdx.x * D2_TILE;
  const int split = blockIdx.y;
  int t_begin, t_end;
  d2_split_range(N, split, splits, t_begin, t_end);

  for (int i = tid; i < D2_TILE * G * Q; i += D2_THREADS) sums[i] = 0.0;
  float best[4];
  int best_j[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { best[r] = INFINITY; best_j[r] = -1; }

  for (int t = t_begin; t < t_end; ++t) {
    const int j0 = t * D2_TILE;
    int my_label = -1;
    if (tid < D2_TILE && j0 + tid < N) {
      const int g = group[j0 + tid];
      my_label = (g >= 0 && g < G) ? g : -1;                       // the only place a label is read: range-checked here
    }
    float acc[4][4];
    d2_tile_acc<VEC>(x, pitch, N, D, i0, j0, As, Bs, acc, [&] { if (tid < D2_TILE) lab[tid] = my_label; });

    // epilogue of the tile: lab[] was written before the barrier of chunk 0
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row_l = ty * 4 + r, row = i0 + row_l;
      int lb[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = j0 + tx + 16 * q;
        const float d2 = acc[r][q];
        lb[q] = col == row ? -1 : lab[tx + 16 * q];
        if (lb[q] >= 0 && (d2 < best[r] || (best_j[r] < 0 && d2 == best[r]))) { best[r] = d2; best_j[r] = col; }
      }
      // quantity 0: the root; quantity 1 + s: the kernel of scale s.  One quantity at a time keeps four values live
      for (int qi = 0; qi < Q; ++qi) {
        float v[4];
        if (qi == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = sqrtf(acc[r][q]);
        } else {
          const float sc = scale[qi - 1];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = expf(-(acc[r][q] * sc));
        }
        for (int g = 0; g < G; ++g) {
          double p = 0.0;
#pragma unroll
          for (int q = 0; q < 4; ++q) p += lb[q] == g ? (double)v[q] : 0.0;
          p = d2_row_sum(p);
          if (tx == 0) sums[((size_t)row_l * G + g) * Q + qi] += p;
        }
      }
    }
  }

  // the partials of this split.  Nearest neighbour of a row: smaller d2, then smaller index, over its 16 threads
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float b = best[r];
    int j = best_j[r];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const float ob = __shfl_xor(b, o, 16);
      const int oj = __shfl_xor(j, o, 16);
      if (oj >= 0 && (j < 0 || ob < b || (ob == b && oj < j))) { b = ob; j = oj; }
    }
    const int row = i0 + ty * 4 + r;
    if (tx == 0 && row < N) {
      ws_d2[(size_t)split * N + row] = b;
      ws_index[(size_t)split * N + row] = j;
    }
  }
  __syncthreads();                                                  // the sums of the last tile are in LDS
  const int per_row = G * Q;
  for (int i = tid; i < D2_TILE * per_row; i += D2_THREADS) {
    const int row = i0 + i / per_row;
    if (row < N) ws_sum[((size_t)split * N + row) * per_row + i % per_row] = sums[i];
  }
}

// element e < N * G * (1 + S): the sum over the splits, in split order, to dist_sum / kern_sum; e < N also: the nearest
// neighbour over the splits
__global__ __launch_bounds__(256) void pair_finish_kernel(const double* __restrict__ ws_sum, const float* __restrict__ ws_d2,
                                                          const int* __restrict__ ws_index, int N, int G, int S, int splits,
                                                          double* __restrict__ dist_sum, double* __restrict__ kern_sum,
                                                          float* __restrict__ nn_d2, int* __restrict__ nn_index) {
  const int Q = 1 + S;
  const size_t total = (size_t)N * G * Q;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < total) {
    double v = 0.0;
    for (int s = 0; s < splits; ++s) v += ws_sum[(size_t)s * total + e];
    const size_t ig = e / Q;
    const int q = (int)(e % Q);
    if (q == 0) dist_sum[ig] = v; else kern_sum[ig * S + (q - 1)] = v;
  }
  if (e < (size_t)N) {
    float b = INFINITY;
    int j = -1;
    for (int s = 0; s < splits; ++s) {
      const float ob = ws_d2[(size_t)s * N + e];
      const int oj = ws_index[(size_t)s * N + e];
      if (oj >= 0 && (j < 0 || ob < b || (ob == b && oj < j))) { b = ob; j = oj; }
    }
    nn_d2[e] = b;
    nn_index[e] = j;
  }
}

extern "C" int bsed_pair_stats_splits(int N, int D) {
  (void)D;                                                          // the choice depends on the number of tiles alone
  return N < 1 ? 1 : d2_auto_splits(N);
}

extern "C" size_t bsed_pair_stats_workspace(int N, int G, int S, int splits) {
  if (N < 1 || G < 1 || G > BSED_PAIR_MAX_GROUPS || S < 0 || S > BSED_PAIR_MAX_SCALES || splits < 0 ||
      splits > D2_MAX_SPLITS)
    return 0;
  if (splits == 0) splits = d2_auto_splits(N);
  return (size_t)splits * (size_t)N * ((size_t)G * (1 + S) * sizeof(double) + sizeof(float) + sizeof(int));
}

extern "C" int bsed_pair_stats(const float* x, long long x_pitch, int N, int D, const int* group, int G,
                               const float* scale, int S, int splits, double* dist_sum, double* kern_sum, float* nn_d2,
                               int* nn_index, void* workspace, size_t workspace_bytes, void* stream) {
  BSED_CHECK_ARG(N >= 1 && D >= 1 && N <= (1 << 30), "bsed_pair_stats: bad shape (N=%d, D=%d; N at most 2^30)", N, D);
  BSED_CHECK_ARG(G >= 1 && G <= BSED_PAIR_MAX_GROUPS, "bsed_pair_stats: 1 to %d groups, got G=%d", BSED_PAIR_MAX_GROUPS, G);
  BSED_CHECK_ARG(S >= 0 && S <= BSED_PAIR_MAX_SCALES, "bsed_pair_stats: 0 to %d scales, got S=%d", BSED_PAIR_MAX_SCALES, S);
  BSED_CHECK_ARG(x && group && dist_sum && nn_d2 && nn_index && workspace, "bsed_pair_stats: null tensor");
  BSED_CHECK_ARG(S == 0 || (scale && kern_sum), "bsed_pair_stats: null scale or kern_sum with S=%d", S);
  BSED_CHECK_ARG(x_pitch >= (long long)D, "bsed_pair_stats: x_pitch=%lld is below D=%d", x_pitch, D);
  BSED_CHECK_ARG(splits >= 0 && splits <= D2_MAX_SPLITS, "bsed_pair_stats: splits must be 0 (automatic) to %d, got %d",
                 D2_MAX_SPLITS, splits);
  BSED_CHECK_ARG(((uintptr_t)x % sizeof(float)) == 0 && ((uintptr_t)workspace % sizeof(double)) == 0,
                 "bsed_pair_stats: x must be 4-byte aligned and the workspace 8-byte aligned");
  if (splits == 0) splits = d2_auto_splits(N);
  const size_t need = bsed_pair_stats_workspace(N, G, S, splits);
  BSED_CHECK_ARG(workspace_bytes >= need, "bsed_pair_stats: the workspace holds %zu bytes, %zu are needed (N=%d, G=%d, S=%d, "
                 "splits=%d)", workspace_bytes, need, N, G, S, splits);
  const int Q = 1 + S;
  double* ws_sum = (double*)workspace;
  float* ws_d2 = (float*)(ws_sum + (size_t)splits * N * G * Q);
  int* ws_index = (int*)(ws_d2 + (size_t)splits * N);
  const size_t lds = (size_t)D2_TILE * G * Q * sizeof(double);
  D2_LAUNCH_VEC(d2_vec_ok(x, x_pitch), pair_stats_kernel, dim3(d2_tiles(N), splits), lds, (hipStream_t)stream, x, x_pitch, N,
                D, group, G, scale, S, splits, ws_sum, ws_d2, ws_index);
  BSED_LAUNCH_CHECK();
  const size_t total = (size_t)N * G * Q;                           // >= N
  hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws_sum,
                     ws_d2, ws_index, N, G, S, splits, dist_sum, kern_sum, nn_d2, nn_index);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
