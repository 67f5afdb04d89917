// The domain gap of an embedding: one all-pairs pass over N points of D float32 features (bsed_pair_stats, ABI 17).
// The definitions -- d2 by direct differences in float32, its correctly rounded root, the float64 sums per (point,
// group) of the roots and of expf(-(d2 * scale)), the nearest neighbour with the smallest index on a tie -- are stated
// in include/bsed.h; the silhouette, the nearest-neighbour domain accuracy and the multi-kernel MMD are host arithmetic
// on these sums (domain_gap.py).
//
// Two launches, no atomics, no fence:
//   pair_stats_kernel   grid (row tiles, splits), 256 threads.  A workgroup owns PAIR_TILE = 64 rows and the contiguous
//                       range [split * T / splits, (split + 1) * T / splits) of the T column tiles of 64 points.  Per
//                       column tile the 64 x 64 squared distances are formed 4 x 4 per thread: chunks of PAIR_KC = 32
//                       features of both point sets go through LDS (rows PAIR_LD = 36 floats apart: the 16 lanes
//                       that a ds_read_b128 serves in one LDS cycle read the rows tx = 0 .. 15 of the column set, and
//                       36 tx mod 64 takes 16 different multiples of 4, so their four-bank spans cover the 64 banks
//                       once; the row set's reads are broadcasts), the next chunk's global loads are in flight while the
//                       current one is multiplied, and the tail of D is zero-filled in LDS so the inner loop has no
//                       guard.  Global loads are 16 bytes wide when the base and the pitch allow it (chosen on the
//                       host), 4 bytes otherwise.  Epilogue per pair: label from LDS (-1 = masked, out of range, or
//                       the point itself), root, up to 8 expf; the four columns of a thread are added in float64 in
//                       column order per (row, group), the 16 threads of a row are folded by a fixed DPP tree and the
//                       row's first thread adds the result to the workgroup's float64 sums in LDS (only it ever
//                       touches them).  At the end of its range the workgroup writes its sums and its nearest
//                       neighbours as partials of its split to the workspace.
//   pair_finish_kernel  adds the partials in split order and takes the nearest neighbour of the splits (smaller d2, then
//                       smaller index).
// Every sum has an order fixed by (N, D, G, S, splits): two launches with the same arguments give the same bits.
// LDS: 2 * 64 * 36 * 4 B of staging + 64 * 4 B of labels + 64 * G * (1 + S) * 8 B of sums (dynamic): 18.7 KB + 6 KB at
// G = 2, S = 5; 55.5 KB at G = 8, S = 8.
#include "../../include/bsed.h"
#include "bsed_common.h"
#include <math.h>

#define PAIR_TILE 64
#define PAIR_KC 32
#define PAIR_LD 36                       // floats between two rows of a staged chunk
#define PAIR_THREADS 256
#define PAIR_TARGET_WORKGROUPS 1024      // what the automatic split aims at: 4 workgroups on each of 256 CUs
#define PAIR_MAX_SPLITS 65535            // grid.y

// the automatic number of column splits: enough workgroups to fill the chip, never more than there are column tiles
static int pair_auto_splits(int N) {
  const long tiles = ((long)N + PAIR_TILE - 1) / PAIR_TILE;
  long want = (PAIR_TARGET_WORKGROUPS + tiles - 1) / tiles;
  if (want > tiles) want = tiles;
  if (want > PAIR_MAX_SPLITS) want = PAIR_MAX_SPLITS;
  return want < 1 ? 1 : (int)want;
}

// four features k .. k + 3 of one point; zero beyond D and for a point that does not exist
template <bool VEC>
__device__ __forceinline__ f32x4 pair_load4(const float* __restrict__ x, long long pitch, int row, int N, int k, int D) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row >= N || k >= D) return v;
  const float* p = x + (size_t)row * (size_t)pitch + k;
  if (VEC && k + 4 <= D) return *reinterpret_cast<const f32x4*>(p);
  v[0] = p[0];
  if (k + 1 < D) v[1] = p[1];
  if (k + 2 < D) v[2] = p[2];
  if (k + 3 < D) v[3] = p[3];
  return v;
}

// p of the lane that the DPP control CTRL names, inside a row of 16 lanes: two 32-bit moves on the VALU, no trip
// through the LDS crossbar (every lane is active where this is called)
template <int CTRL>
__device__ __forceinline__ double pair_dpp(double p) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(p);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xF, 0xF, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// the sum of p over the 16 threads of a row (lanes 16 r .. 16 r + 15 of a wave: one DPP row), by a fixed tree: the
// neighbour in the quad (quad_perm [1,0,3,2]), the other pair of the quad ([2,3,0,1]), the other quad of the half
// (row_half_mirror: lane i takes 7 - i, which holds its quad's sum), the other half (row_mirror: 15 - i).  Against the
// same tree made of ds_bpermute (__shfl_xor): 0.350 -> 0.340 ms at N = 4096, D = 256, S = 5 and 15.75 -> 15.25 ms at
// N = 2048, D = 80128 (same box, alternating; DESIGN.md section 5, "Domain gap").
__device__ __forceinline__ double pair_row_sum(double p) {
  p += pair_dpp<0xB1>(p);
  p += pair_dpp<0x4E>(p);
  p += pair_dpp<0x141>(p);
  p += pair_dpp<0x140>(p);
  return p;
}

template <bool VEC>
__global__ __launch_bounds__(PAIR_THREADS) void pair_stats_kernel(
    const float* __restrict__ x, long long pitch, int N, int D, const int* __restrict__ group, int G,
    const float* __restrict__ scale, int S, int splits, double* __restrict__ ws_sum, float* __restrict__ ws_d2,
    int* __restrict__ ws_index) {
  __shared__ __attribute__((aligned(16))) float As[PAIR_TILE * PAIR_LD];
  __shared__ __attribute__((aligned(16))) float Bs[PAIR_TILE * PAIR_LD];
  __shared__ int lab[PAIR_TILE];
  extern __shared__ __attribute__((aligned(16))) double sums[];    // [64 rows][G][1 + S]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int Q = 1 + S;
  const int i0 = blockIdx.x * PAIR_TILE;
  const int split = blockIdx.y;
  const int tiles = (N + PAIR_TILE - 1) / PAIR_TILE;
  const int t_begin = (int)((long)split * tiles / splits), t_end = (int)((long)(split + 1) * tiles / splits);
  const int chunks = (D + PAIR_KC - 1) / PAIR_KC;

  for (int i = tid; i < PAIR_TILE * G * Q; i += PAIR_THREADS) sums[i] = 0.0;
  float best[4];
  int best_j[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { best[r] = INFINITY; best_j[r] = -1; }

  // staging: thread t moves features 4 (t & 7) .. + 3 of points (t >> 3) and (t >> 3) + 32 of both sets
  const int s_row = tid >> 3, s_k = (tid & 7) * 4;

  for (int t = t_begin; t < t_end; ++t) {
    const int j0 = t * PAIR_TILE;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    f32x4 pa0 = pair_load4<VEC>(x, pitch, i0 + s_row, N, s_k, D), pa1 = pair_load4<VEC>(x, pitch, i0 + s_row + 32, N, s_k, D);
    f32x4 pb0 = pair_load4<VEC>(x, pitch, j0 + s_row, N, s_k, D), pb1 = pair_load4<VEC>(x, pitch, j0 + s_row + 32, N, s_k, D);
    int my_label = -1;
    if (tid < PAIR_TILE && j0 + tid < N) {
      const int g = group[j0 + tid];
      my_label = (g >= 0 && g < G) ? g : -1;                       // the only place a label is read: range-checked here
    }
    for (int c = 0; c < chunks; ++c) {
      __syncthreads();                                              // the previous chunk (and epilogue) is done with LDS
      *reinterpret_cast<f32x4*>(&As[s_row * PAIR_LD + s_k]) = pa0;
      *reinterpret_cast<f32x4*>(&As[(s_row + 32) * PAIR_LD + s_k]) = pa1;
      *reinterpret_cast<f32x4*>(&Bs[s_row * PAIR_LD + s_k]) = pb0;
      *reinterpret_cast<f32x4*>(&Bs[(s_row + 32) * PAIR_LD + s_k]) = pb1;
      if (c == 0 && tid < PAIR_TILE) lab[tid] = my_label;
      __syncthreads();
      if (c + 1 < chunks) {                                         // in flight while this chunk is multiplied
        const int k = (c + 1) * PAIR_KC + s_k;
        pa0 = pair_load4<VEC>(x, pitch, i0 + s_row, N, k, D); pa1 = pair_load4<VEC>(x, pitch, i0 + s_row + 32, N, k, D);
        pb0 = pair_load4<VEC>(x, pitch, j0 + s_row, N, k, D); pb1 = pair_load4<VEC>(x, pitch, j0 + s_row + 32, N, k, D);
      }
      // two steps at a time: unrolled whole, the compiler hoists all 64 ds_read_b128 of the chunk and the kernel takes 220
      // registers (2 waves per SIMD); this way it takes 128 (4 waves per SIMD), nothing spilled: 0.375 -> 0.340 ms at
      // N = 4096, D = 256 and 15.45 -> 15.25 ms at N = 2048, D = 80128 (same box, alternating)
#pragma unroll 2
      for (int kk = 0; kk < PAIR_KC; kk += 4) {
        f32x4 a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = *reinterpret_cast<const f32x4*>(&As[(ty * 4 + r) * PAIR_LD + kk]);
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = *reinterpret_cast<const f32x4*>(&Bs[(tx + 16 * q) * PAIR_LD + kk]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float diff = a[r][e] - b[q][e];
              acc[r][q] = fmaf(diff, diff, acc[r][q]);
            }
      }
    }

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
          p = pair_row_sum(p);
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
  for (int i = tid; i < PAIR_TILE * per_row; i += PAIR_THREADS) {
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
  return N < 1 ? 1 : pair_auto_splits(N);
}

extern "C" size_t bsed_pair_stats_workspace(int N, int G, int S, int splits) {
  if (N < 1 || G < 1 || G > BSED_PAIR_MAX_GROUPS || S < 0 || S > BSED_PAIR_MAX_SCALES || splits < 0 ||
      splits > PAIR_MAX_SPLITS)
    return 0;
  if (splits == 0) splits = pair_auto_splits(N);
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
  BSED_CHECK_ARG(splits >= 0 && splits <= PAIR_MAX_SPLITS, "bsed_pair_stats: splits must be 0 (automatic) to %d, got %d",
                 PAIR_MAX_SPLITS, splits);
  BSED_CHECK_ARG(((uintptr_t)x % sizeof(float)) == 0 && ((uintptr_t)workspace % sizeof(double)) == 0,
                 "bsed_pair_stats: x must be 4-byte aligned and the workspace 8-byte aligned");
  if (splits == 0) splits = pair_auto_splits(N);
  const size_t need = bsed_pair_stats_workspace(N, G, S, splits);
  BSED_CHECK_ARG(workspace_bytes >= need, "bsed_pair_stats: the workspace holds %zu bytes, %zu are needed (N=%d, G=%d, S=%d, "
                 "splits=%d)", workspace_bytes, need, N, G, S, splits);
  const int Q = 1 + S;
  double* ws_sum = (double*)workspace;
  float* ws_d2 = (float*)(ws_sum + (size_t)splits * N * G * Q);
  int* ws_index = (int*)(ws_d2 + (size_t)splits * N);
  const int tiles = (N + PAIR_TILE - 1) / PAIR_TILE;
  const size_t lds = (size_t)PAIR_TILE * G * Q * sizeof(double);
  const bool vec = ((uintptr_t)x % 16) == 0 && (x_pitch % 4) == 0;
  if (vec)
    hipLaunchKernelGGL(pair_stats_kernel<true>, dim3(tiles, splits), dim3(PAIR_THREADS), lds, (hipStream_t)stream, x, x_pitch,
                       N, D, group, G, scale, S, splits, ws_sum, ws_d2, ws_index);
  else
    hipLaunchKernelGGL(pair_stats_kernel<false>, dim3(tiles, splits), dim3(PAIR_THREADS), lds, (hipStream_t)stream, x, x_pitch,
                       N, D, group, G, scale, S, splits, ws_sum, ws_d2, ws_index);
  BSED_LAUNCH_CHECK();
  const size_t total = (size_t)N * G * Q;                           // >= N
  hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws_sum,
                     ws_d2, ws_index, N, G, S, splits, dist_sum, kern_sum, nn_d2, nn_index);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
