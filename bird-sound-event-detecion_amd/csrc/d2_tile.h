// The dense matrix of squared distances d2(i, j) of bsed_pair_stats' definition (include/bsed.h), shared by tsne.hip
// (on its way to the affinities) and svc.hip (bsed_svc_d2): one copy of the device code, so the two hold the same bits.
//   d2_tile_kernel   grid (tiles, tiles), 256 threads: the 64 x 64 squared distances of a tile pair, 4 x 4 per thread,
//                    through the staging loop of pair_stats.hip (chunks of 32 features through LDS, rows 36 floats
//                    apart, the next chunk's loads in flight, the tail of D zero-filled; 16-byte loads when base and
//                    pitch allow it, 4-byte ones otherwise) -> out[i][j] = d2(i, j), rows N floats apart.
//                    (a - b)^2 and (b - a)^2 have the same bits and the chain over k has one order, so d2 is symmetric
//                    bit for bit and its diagonal is exactly 0.
// The kernel is static: each file that includes this header launches its own instance.
#pragma once
#include "bsed_common.h"

#define D2_TILE 64
#define D2_KC 32
#define D2_LD 36                         // floats between two rows of a staged chunk
#define D2_THREADS 256

static inline int d2_tiles(int N) { return (N + D2_TILE - 1) / D2_TILE; }

#if defined(__HIPCC__)
// four features k .. k + 3 of one point; zero beyond D and for a point that does not exist
template <bool VEC>
__device__ __forceinline__ f32x4 d2_load4(const float* __restrict__ x, long long pitch, int row, int N, int k, int D) {
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

template <bool VEC>
static __global__ __launch_bounds__(D2_THREADS) void d2_tile_kernel(const float* __restrict__ x, long long pitch, int N,
                                                                    int D, float* __restrict__ P) {
  __shared__ __attribute__((aligned(16))) float As[D2_TILE * D2_LD];
  __shared__ __attribute__((aligned(16))) float Bs[D2_TILE * D2_LD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.x * D2_TILE, j0 = blockIdx.y * D2_TILE;
  const int chunks = (D + D2_KC - 1) / D2_KC;
  const int s_row = tid >> 3, s_k = (tid & 7) * 4;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  f32x4 pa0 = d2_load4<VEC>(x, pitch, i0 + s_row, N, s_k, D), pa1 = d2_load4<VEC>(x, pitch, i0 + s_row + 32, N, s_k, D);
  f32x4 pb0 = d2_load4<VEC>(x, pitch, j0 + s_row, N, s_k, D), pb1 = d2_load4<VEC>(x, pitch, j0 + s_row + 32, N, s_k, D);
  for (int c = 0; c < chunks; ++c) {
    __syncthreads();
    *reinterpret_cast<f32x4*>(&As[s_row * D2_LD + s_k]) = pa0;
    *reinterpret_cast<f32x4*>(&As[(s_row + 32) * D2_LD + s_k]) = pa1;
    *reinterpret_cast<f32x4*>(&Bs[s_row * D2_LD + s_k]) = pb0;
    *reinterpret_cast<f32x4*>(&Bs[(s_row + 32) * D2_LD + s_k]) = pb1;
    __syncthreads();
    if (c + 1 < chunks) {
      const int k = (c + 1) * D2_KC + s_k;
      pa0 = d2_load4<VEC>(x, pitch, i0 + s_row, N, k, D); pa1 = d2_load4<VEC>(x, pitch, i0 + s_row + 32, N, k, D);
      pb0 = d2_load4<VEC>(x, pitch, j0 + s_row, N, k, D); pb1 = d2_load4<VEC>(x, pitch, j0 + s_row + 32, N, k, D);
    }
#pragma unroll 2
    for (int kk = 0; kk < D2_KC; kk += 4) {
      f32x4 a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = *reinterpret_cast<const f32x4*>(&As[(ty * 4 + r) * D2_LD + kk]);
#pragma unroll
      for (int q = 0; q < 4; ++q) b[q] = *reinterpret_cast<const f32x4*>(&Bs[(tx + 16 * q) * D2_LD + kk]);
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
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + ty * 4 + r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = j0 + tx + 16 * q;
      if (row < N && col < N) P[(size_t)row * N + col] = acc[r][q];
    }
  }
}

// the launch: the 16-byte loads when base and pitch allow them.  The caller runs BSED_LAUNCH_CHECK()
static inline void d2_launch(const float* x, long long x_pitch, int N, int D, float* out, hipStream_t s) {
  const int tiles = d2_tiles(N);
  if (((uintptr_t)x % 16) == 0 && (x_pitch % 4) == 0)
    hipLaunchKernelGGL(d2_tile_kernel<true>, dim3(tiles, tiles), dim3(D2_THREADS), 0, s, x, x_pitch, N, D, out);
  else
    hipLaunchKernelGGL(d2_tile_kernel<false>, dim3(tiles, tiles), dim3(D2_THREADS), 0, s, x, x_pitch, N, D, out);
}
#endif
