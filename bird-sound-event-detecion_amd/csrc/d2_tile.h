// The pair-tile core of the all-pairs kernels over N points of D float32 features: pair_stats.hip (the domain gap),
// tsne.hip (on its way to the affinities, and the gradient's tiling) and svc.hip (bsed_svc_d2).  One copy of the device
// code, so the three hold the same bits of d2(i, j) as bsed_pair_stats defines it (include/bsed.h).
//   d2_tile_acc      256 threads: the 64 x 64 squared distances of the tile pair (i0, j0), 4 x 4 per thread (thread
//                    (ty, tx) = (tid >> 4, tid & 15) holds rows i0 + 4 ty + r and columns j0 + tx + 16 q).  Chunks of
//                    D2_KC = 32 features of both point sets go through LDS, the next chunk's global loads are in flight
//                    while the current one is multiplied, and the tail of D is zero-filled in LDS so the inner loop has no
//                    guard (the zeros add exact zeros).  Global loads are 16 bytes wide when the base and the pitch allow
//                    it (d2_vec_ok, chosen on the host), 4 bytes otherwise.
//                    Rows are D2_LD = 36 floats apart in LDS: the 16 lanes that a ds_read_b128 serves in one LDS cycle
//                    read the rows tx = 0 .. 15 of the column set, and 36 tx mod 64 takes 16 different multiples of 4, so
//                    their four-bank spans cover the 64 banks once; the row set's reads are broadcasts.
//                    (a - b)^2 and (b - a)^2 have the same bits and the chain over k has one order, so d2 is symmetric
//                    bit for bit and its diagonal is exactly 0.
//   d2_tile_kernel   grid (tiles, tiles): d2_tile_acc of every tile pair -> out[i][j] = d2(i, j), rows N floats apart.
//                    The kernel is static: each file that includes this header launches its own instance.
//   d2_row_sum       the float64 sum over the 16 threads of a tile row, by a fixed DPP tree.
//   d2_auto_splits / d2_split_range   how the kernels that own 64 rows share the column tiles among grid.y workgroups.
#pragma once
#include "bsed_common.h"

#define D2_TILE 64
#define D2_KC 32
#define D2_LD 36                         // floats between two rows of a staged chunk
#define D2_THREADS 256
#define D2_TARGET_WORKGROUPS 1024        // what the automatic split aims at: 4 workgroups on each of 256 CUs
#define D2_MAX_SPLITS 65535              // grid.y

__host__ __device__ static inline int d2_tiles(int N) { return (N + D2_TILE - 1) / D2_TILE; }

// the automatic number of column splits: enough workgroups to fill the chip, never more than there are column tiles
static inline int d2_auto_splits(int N) {
  const long tiles = ((long)N + D2_TILE - 1) / D2_TILE;
  long want = (D2_TARGET_WORKGROUPS + tiles - 1) / tiles;
  if (want > tiles) want = tiles;
  if (want > D2_MAX_SPLITS) want = D2_MAX_SPLITS;
  return want < 1 ? 1 : (int)want;
}

// the 16-byte loads: the base on a 16-byte boundary, rows a multiple of four floats apart
static inline bool d2_vec_ok(const float* base, long long pitch) { return ((uintptr_t)base % 16) == 0 && (pitch % 4) == 0; }

// KERNEL<true> when vec, KERNEL<false> otherwise, with the same launch.  The caller runs BSED_LAUNCH_CHECK()
#define D2_LAUNCH_VEC(vec, KERNEL, grid, lds, stream, ...)                                              \
  do {                                                                                                  \
    if (vec) hipLaunchKernelGGL(KERNEL<true>, grid, dim3(D2_THREADS), lds, stream, __VA_ARGS__);        \
    else hipLaunchKernelGGL(KERNEL<false>, grid, dim3(D2_THREADS), lds, stream, __VA_ARGS__);           \
  } while (0)

// the contiguous range [t_begin, t_end) of the column tiles that split `split` of `splits` owns
__device__ __forceinline__ void d2_split_range(int N, int split, int splits, int& t_begin, int& t_end) {
  const int tiles = d2_tiles(N);
  t_begin = (int)((long)split * tiles / splits);
  t_end = (int)((long)(split + 1) * tiles / splits);
}

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

// acc[r][q] = d2(i0 + 4 ty + r, j0 + tx + 16 q) through As and Bs (D2_TILE * D2_LD floats each, 16-byte aligned).
// Staging: thread t moves features 4 (t & 7) .. + 3 of points (t >> 3) and (t >> 3) + 32 of both sets.  between()
// runs between the two barriers of chunk 0, where a caller publishes what its epilogue reads from LDS: the first
// barrier says that the previous tile's epilogue is done with it, the second that every thread sees the new values.
template <bool VEC, class Between>
__device__ __forceinline__ void d2_tile_acc(const float* __restrict__ x, long long pitch, int N, int D, int i0, int j0,
                                            float (&As)[D2_TILE * D2_LD], float (&Bs)[D2_TILE * D2_LD],
                                            float (&acc)[4][4], Between between) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int chunks = (D + D2_KC - 1) / D2_KC;
  const int s_row = tid >> 3, s_k = (tid & 7) * 4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  f32x4 pa0 = d2_load4<VEC>(x, pitch, i0 + s_row, N, s_k, D), pa1 = d2_load4<VEC>(x, pitch, i0 + s_row + 32, N, s_k, D);
  f32x4 pb0 = d2_load4<VEC>(x, pitch, j0 + s_row, N, s_k, D), pb1 = d2_load4<VEC>(x, pitch, j0 + s_row + 32, N, s_k, D);
  // the thread's rows in LDS, formed once: with (ty * 4 + r) * D2_LD + kk written out at each read, this function
  // (simplified on its own before it is inlined) leaves other address arithmetic and the kernels take 2 to 8 registers
  // more, pair_stats_kernel past 128
  const float* a_rows = &As[ty * 4 * D2_LD];
  const float* b_rows = &Bs[tx * D2_LD];
  for (int c = 0; c < chunks; ++c) {
    __syncthreads();                                                // the previous chunk (and epilogue) is done with LDS
    *reinterpret_cast<f32x4*>(&As[s_row * D2_LD + s_k]) = pa0;
    *reinterpret_cast<f32x4*>(&As[(s_row + 32) * D2_LD + s_k]) = pa1;
    *reinterpret_cast<f32x4*>(&Bs[s_row * D2_LD + s_k]) = pb0;
    *reinterpret_cast<f32x4*>(&Bs[(s_row + 32) * D2_LD + s_k]) = pb1;
    if (c == 0) between();
    __syncthreads();
    if (c + 1 < chunks) {                                           // in flight while this chunk is multiplied
      const int k = (c + 1) * D2_KC + s_k;
      pa0 = d2_load4<VEC>(x, pitch, i0 + s_row, N, k, D); pa1 = d2_load4<VEC>(x, pitch, i0 + s_row + 32, N, k, D);
      pb0 = d2_load4<VEC>(x, pitch, j0 + s_row, N, k, D); pb1 = d2_load4<VEC>(x, pitch, j0 + s_row + 32, N, k, D);
    }
    // two steps at a time: unrolled whole, the compiler hoists all 64 ds_read_b128 of the chunk and pair_stats_kernel
    // takes 220 registers (2 waves per SIMD); this way it takes 128 (4 waves per SIMD), nothing spilled: 0.375 -> 0.340 ms
    // at N = 4096, D = 256 and 15.45 -> 15.25 ms at N = 2048, D = 80128 (same box, alternating)
#pragma unroll 2
    for (int kk = 0; kk < D2_KC; kk += 4) {
      f32x4 a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = *reinterpret_cast<const f32x4*>(&a_rows[r * D2_LD + kk]);
#pragma unroll
      for (int q = 0; q < 4; ++q) b[q] = *reinterpret_cast<const f32x4*>(&b_rows[16 * q * D2_LD + kk]);
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
}

// p of the lane that the DPP control CTRL names, inside a row of 16 lanes: two 32-bit moves on the VALU, no trip
// through the LDS crossbar (every lane is active where this is called)
template <int CTRL>
__device__ __forceinline__ double d2_dpp(double p) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(p);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xF, 0xF, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// the sum of p over the 16 threads of a row (lanes 16 r .. 16 r + 15 of a wave: one DPP row), by a fixed tree: the
// neighbour in the quad (quad_perm [1,0,3,2]), the other pair of the quad ([2,3,0,1]), the other quad of the half
// (row_half_mirror: lane i takes 7 - i, which holds its quad's sum), the other half (row_mirror: 15 - i).  Against the
// same tree made of ds_bpermute (__shfl_xor) in pair_stats_kernel: 0.350 -> 0.340 ms at N = 4096, D = 256, S = 5 and
// 15.75 -> 15.25 ms at N = 2048, D = 80128 (same box, alternating; DESIGN.md section 5, "Domain gap").
__device__ __forceinline__ double d2_row_sum(double p) {
  p += d2_dpp<0xB1>(p);
  p += d2_dpp<0x4E>(p);
  p += d2_dpp<0x141>(p);
  p += d2_dpp<0x140>(p);
  return p;
}

template <bool VEC>
static __global__ __launch_bounds__(D2_THREADS) void d2_tile_kernel(const float* __restrict__ x, long long pitch, int N,
                                                                    int D, float* __restrict__ P) {
  __shared__ __attribute__((aligned(16))) float As[D2_TILE * D2_LD];
  __shared__ __attribute__((aligned(16))) float Bs[D2_TILE * D2_LD];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.x * D2_TILE, j0 = blockIdx.y * D2_TILE;
  float acc[4][4];
  d2_tile_acc<VEC>(x, pitch, N, D, i0, j0, As, Bs, acc, [] {});
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

static inline void d2_launch(const float* x, long long x_pitch, int N, int D, float* out, hipStream_t s) {
  const int tiles = d2_tiles(N);
  D2_LAUNCH_VEC(d2_vec_ok(x, x_pitch), d2_tile_kernel, dim3(tiles, tiles), 0, s, x, x_pitch, N, D, out);
}
