// Dataset scaler: per-band sum of x and sum of x^2 of the dB-mel features, for the reference's Scaler
// (src/utilities/Scaler.py:38-102), and the stand-alone form of its normalize().
//
//   scaler_accum_kernel<FROM_DB, VEC> : one read of the input, no dB tensor written.  FROM_DB = 0 reads LINEAR mel
//                      (B, T, n_mels) and makes the dB value on the fly with mel_db_kernel's expression (per-clip top_db
//                      floor included); frames T <= t < T_out are the 0 dB pad rows of PadOrTrunc and add nothing to
//                      either sum, frames t >= T_out are dropped.  FROM_DB = 1 reads a (B, T_out, n_mels) dB tensor.
//                      The square is taken in float32 and then widened (the reference squares a float32 array); both
//                      sums accumulate in float64.  Grid (row chunks, clips).  VEC = 1 (n_mels = 128, 16-byte aligned):
//                      a row is 32 lanes x float4, a wave takes two rows per load, a workgroup SC_ROWS rows whose loads
//                      are all issued before the first logarithm; the eight row groups meet in LDS and are added in
//                      fixed order.  VEC = 0 (any n_mels <= 256): thread = band, rows in sequence, no LDS.
//                      Every workgroup writes its (2, n_mels) float64 partial: no floating-point atomics.
//   scaler_finish_kernel : acc += partials in fixed order (32 columns per workgroup, 32 interleaved partial sequences
//                      per column, joined in LDS): two runs give the same bits.
//   scaler_normalize_kernel : float32((float64(x) - mean[m]) / std[m]) of an existing dB tensor (Scaler.normalize on
//                      the GPU); the front end's fused forms live in mel.hip.
#include "bsed_common.h"
#include "../../include/bsed.h"
#include <math.h>
#include <algorithm>

#define SC_THREADS 256
#define SC_ROWS 64                        // rows of one clip per workgroup
#define SC_PASSES (SC_ROWS / 8)           // VEC: 8 rows per pass (4 waves x 2 half-waves)
#define SF_COLS 32                        // finish: columns per workgroup
#define SF_SEQS 32                        // finish: interleaved partial sequences per column

template <int FROM_DB>
__device__ __forceinline__ void scaler_add(float a, float floor_db, double& s1, double& s2) {
  float v = a;
  if (!FROM_DB) v = fmaxf(10.0f * log10f(fmaxf(1e-10f, a * a)), floor_db);   // mel_db_kernel's expression
  s1 += (double)v;
  s2 += (double)__fmul_rn(v, v);          // float32 square, then widened
}

template <int FROM_DB, int VEC>
__global__ __launch_bounds__(SC_THREADS) void scaler_accum_kernel(const float* __restrict__ x, const float* __restrict__ clip_max,
                                                                   double* __restrict__ part, int T, int Tv, int n_mels,
                                                                   float top_db) {
  // T: rows per clip in x; Tv = min(T, T_out): rows that count (the rest of T_out is 0 dB)
  const int b = blockIdx.y, tid = threadIdx.x;
  float floor_db = 0.f;
  if (!FROM_DB) {
    const float mx = clip_max[b];
    floor_db = 10.0f * log10f(fmaxf(1e-10f, mx * mx)) - top_db;
  }
  double* dst = part + ((size_t)b * gridDim.x + blockIdx.x) * 2 * n_mels;
  const int t_begin = blockIdx.x * SC_ROWS;
  if (VEC) {
    __shared__ double red[2][8][128];     // [sum / sum of squares][row group][band]: 16 KB
    const int l = tid & 31, rg = tid >> 5;
    const float* xb = x + (size_t)b * T * 128 + 4 * l;
    float4 a4[SC_PASSES];
#pragma unroll
    for (int k = 0; k < SC_PASSES; ++k) {
      const int t = t_begin + rg + 8 * k;
      a4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < Tv) a4[k] = *reinterpret_cast<const float4*>(xb + (size_t)t * 128);
    }
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < SC_PASSES; ++k) {
      const int t = t_begin + rg + 8 * k;   // uniform over a half-wave
      if (t < Tv) {
        scaler_add<FROM_DB>(a4[k].x, floor_db, s1[0], s2[0]);
        scaler_add<FROM_DB>(a4[k].y, floor_db, s1[1], s2[1]);
        scaler_add<FROM_DB>(a4[k].z, floor_db, s1[2], s2[2]);
        scaler_add<FROM_DB>(a4[k].w, floor_db, s1[3], s2[3]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[0][rg][4 * l + j] = s1[j]; red[1][rg][4 * l + j] = s2[j]; }
    __syncthreads();
    const int which = tid >> 7, band = tid & 127;
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < 8; ++g) s += red[which][g][band];
    dst[which * 128 + band] = s;
  } else {
    if (tid >= n_mels) return;
    const float* xb = x + (size_t)b * T * n_mels + tid;
    const int t_end = min(t_begin + SC_ROWS, Tv);
    double s1 = 0.0, s2 = 0.0;
    for (int t = t_begin; t < t_end; ++t) scaler_add<FROM_DB>(xb[(size_t)t * n_mels], floor_db, s1, s2);
    dst[tid] = s1;
    dst[n_mels + tid] = s2;
  }
}

// acc[c] += part[0][c] + part[1][c] + ... over nparts rows of n2 = 2 * n_mels columns, in a fixed order
__global__ __launch_bounds__(SF_COLS * SF_SEQS) void scaler_finish_kernel(const double* __restrict__ part, double* __restrict__ acc,
                                                                           int nparts, int n2) {
  __shared__ double red[SF_SEQS][SF_COLS];
  const int c = threadIdx.x % SF_COLS, q = threadIdx.x / SF_COLS;
  const int col = blockIdx.x * SF_COLS + c;
  double s = 0.0;
  if (col < n2)
    for (int p = q; p < nparts; p += SF_SEQS) s += part[(size_t)p * n2 + col];
  red[q][c] = s;
  __syncthreads();
  if (q == 0 && col < n2) {
    double tot = acc[col];
    for (int g = 0; g < SF_SEQS; ++g) tot += red[g][c];
    acc[col] = tot;
  }
}

__global__ void scaler_normalize_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                        const double* __restrict__ sd, float* __restrict__ out, size_t n, int n_mels) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(i % n_mels);
    out[i] = (float)__ddiv_rn(__dsub_rn((double)x[i], mean[m]), sd[m]);
  }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static int scaler_chunks(int T, int T_out) { return ceil_div(T < T_out ? T : T_out, SC_ROWS); }

extern "C" long bsed_scaler_scratch_doubles(int B, int T, int T_out, int n_mels) {
  if (B <= 0 || T <= 0 || T_out <= 0 || n_mels <= 0) return -1;
  return (long)B * scaler_chunks(T, T_out) * 2 * n_mels;
}

template <int FROM_DB>
static int scaler_accum(const char* who, const float* x, const float* clip_max, int B, int T, int T_out, int n_mels,
                        float top_db, double* acc, double* scratch, hipStream_t s) {
  BSED_CHECK_ARG(x && acc && scratch && (FROM_DB || clip_max), "%s: null argument", who);
  BSED_CHECK_ARG(B > 0 && B <= 65535, "%s: B must be in 1..65535", who);
  BSED_CHECK_ARG(T > 0 && T_out > 0, "%s: bad shape (T %d, T_out %d)", who, T, T_out);
  BSED_CHECK_ARG(n_mels > 0 && n_mels <= 256, "%s: n_mels must be in 1..256 (got %d)", who, n_mels);
  BSED_CHECK_ARG(((uintptr_t)acc & 7) == 0 && ((uintptr_t)scratch & 7) == 0, "%s: acc and scratch must be 8-byte aligned", who);
  const int Tv = T < T_out ? T : T_out, nchunk = scaler_chunks(T, T_out);
  BSED_CHECK_ARG((long)B * nchunk < (1L << 31), "%s: too many partials", who);
  const dim3 grid(nchunk, B);
  if (n_mels == 128 && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL((scaler_accum_kernel<FROM_DB, 1>), grid, dim3(SC_THREADS), 0, s, x, clip_max, scratch, T, Tv, n_mels, top_db);
  else
    hipLaunchKernelGGL((scaler_accum_kernel<FROM_DB, 0>), grid, dim3(SC_THREADS), 0, s, x, clip_max, scratch, T, Tv, n_mels, top_db);
  hipLaunchKernelGGL(scaler_finish_kernel, dim3(ceil_div(2 * n_mels, SF_COLS)), dim3(SF_COLS * SF_SEQS), 0, s, scratch, acc,
                     B * nchunk, 2 * n_mels);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

extern "C" int bsed_scaler_accum(const float* mel_lin, const float* clip_max, int B, int T, int T_out, int n_mels,
                                 float top_db, double* acc, double* scratch, void* stream) {
  return scaler_accum<0>("bsed_scaler_accum", mel_lin, clip_max, B, T, T_out, n_mels, top_db, acc, scratch, (hipStream_t)stream);
}

extern "C" int bsed_scaler_accum_db(const float* x_db, int B, int T_out, int n_mels, double* acc, double* scratch,
                                    void* stream) {
  return scaler_accum<1>("bsed_scaler_accum_db", x_db, nullptr, B, T_out, T_out, n_mels, 0.f, acc, scratch, (hipStream_t)stream);
}

extern "C" int bsed_scaler_normalize(const float* x_db, long long n_rows, int n_mels, const double* mean, const double* stdev,
                                     float* out, void* stream) {
  BSED_CHECK_ARG(x_db && mean && stdev && out, "bsed_scaler_normalize: null argument");
  BSED_CHECK_ARG(n_rows > 0 && n_mels > 0 && n_mels <= 256, "bsed_scaler_normalize: bad shape (%lld rows of %d bands)", n_rows, n_mels);
  const size_t n = (size_t)n_rows * n_mels;
  const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(scaler_normalize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x_db, mean, stdev, out, n, n_mels);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
