// Polyphase FIR resampling of one interleaved recording (int16 or fp32, any channel count) to a mono fp32 waveform:
//   y[m] = sum_j x[j] * taps[m * down - j * up + half_len],   x = the mono mix of the frames, zero outside [0, n_in)
// One kernel for every rate ratio, the convert / mix-only case (up = down = 1, one tap) included.
//
// Output m = k * up + c (period k, residue c) reads, with a(c) = (c * down + half_len) / up and
// r(c) = (c * down + half_len) % up,
//   y[m] = sum_{i = 0}^{P - 1} x[k * down + a(c) - i] * taps[r(c) + i * up],        P = (2 * half_len) / up + 1,
// so the taps of an output depend on its residue alone.  The caller's table holds them by residue:
// table[c * P + i] = taps[r(c) + i * up], 0 where that index is past the filter's end.
//
// A workgroup takes CW consecutive residues (CW = the power of two that holds min(up, 64)) over NK = 1024 / CW
// consecutive periods: its CW table rows (at most 64 * P floats: 50 KB of the 245 KB table of 44.1 k -> 32 k) and the
// (NK - 1) * down + a(c0 + CW - 1) - a(c0) + P mono samples those outputs read go to LDS, the samples converted and
// mixed while they are loaded.  For up <= 64 that is the whole table and a block of consecutive outputs.  Lanes run
// along the residues, so a wave stores runs of CW consecutive outputs (256 bytes at CW = 64; all 64 lanes consecutive
// for up <= 2), and a thread keeps one residue and sums 4 periods at once: one tap read from LDS feeds 4
// multiply-adds.  Each output is ONE chain of P fmaf in ascending i (descending j): the value does not depend on the
// tiling, there are no atomics, and two launches give the same bits.  The table sits in LDS as [i][CW + 1]: a wave
// reads a row of it across the banks, and the staging stores (lanes along i) fall on distinct banks too.
// Sample and output positions are 64-bit per workgroup (k0 * down passes 2^32 after 5 minutes of 44.1 kHz audio);
// inside the workgroup every offset is below the LDS size and 32-bit.
#include "../../include/bsed.h"
#include "bsed_common.h"

#define RS_THREADS 256
#define RS_TILE 1024                   // outputs of a workgroup: RS_R per thread
#define RS_R (RS_TILE / RS_THREADS)
#define RS_MAX_CW 64
#define RS_LDS_BYTES (160 * 1024)

// the mono sample of frame j: BSED_PCM_S16: (float)(sum of the channels as int) * scale, scale = fp32(1 / (32768 * channels));
// BSED_PCM_F32: (((x0 + x1) + x2) + ...) * scale in fp32, scale = fp32(1 / channels)
template <int FMT>
__device__ __forceinline__ float rs_mono(const void* __restrict__ in, long j, int channels, float scale) {
  if (FMT == BSED_PCM_S16) {
    const short* p = reinterpret_cast<const short*>(in) + j * channels;
    int s = 0;
    for (int ch = 0; ch < channels; ++ch) s += p[ch];
    return (float)s * scale;
  }
  const float* p = reinterpret_cast<const float*>(in) + j * channels;
  float s = p[0];
  for (int ch = 1; ch < channels; ++ch) s += p[ch];
  return s * scale;
}

// grid.x = residue tiles (fastest, so the workgroups that read the same samples run together) x period groups
template <int FMT>
__global__ void __launch_bounds__(RS_THREADS) resample_poly_kernel(const void* __restrict__ in, long n_in, int channels,
                                                                    float scale, const float* __restrict__ table, int up,
                                                                    int down, int half_len, int P, int lgCW, int ctiles,
                                                                    int span_max, float* __restrict__ out, long n_out) {
  extern __shared__ float rs_lds[];
  const int CW = 1 << lgCW, NK = RS_TILE >> lgCW, pitch = CW + 1;
  float* ts = rs_lds;                       // [P][pitch]
  float* xs = rs_lds + (size_t)P * pitch;   // [span_max]
  const int c0 = (int)(blockIdx.x % ctiles) * CW;
  const long k0 = (long)(blockIdx.x / ctiles) * NK;
  const int rc = min(CW, up - c0);          // residues of this tile
  const long a0 = ((long)c0 * down + half_len) / up;
  const int a_last = (int)(((long)(c0 + rc - 1) * down + half_len) / up - a0);
  const int span = (NK - 1) * down + a_last + P;     // <= span_max (host)
  const long jlo = k0 * down + a0 - (P - 1);         // sample of xs[0]

  // table rows c0 .. c0 + rc - 1: a wave takes a row, lanes along i
  for (int cc = threadIdx.x >> 6; cc < rc; cc += RS_THREADS >> 6) {
    const float* row = table + (size_t)(c0 + cc) * P;
    for (int i = threadIdx.x & 63; i < P; i += 64) ts[i * pitch + cc] = row[i];
  }
  for (int i = threadIdx.x; i < span; i += RS_THREADS) {
    const long j = jlo + i;
    xs[i] = (j >= 0 && j < n_in) ? rs_mono<FMT>(in, j, channels, scale) : 0.f;
  }
  __syncthreads();

  const int cc = threadIdx.x & (CW - 1), row = threadIdx.x >> lgCW, rows = RS_THREADS >> lgCW;
  if (cc >= rc) return;
  const int a = (int)(((long)(c0 + cc) * down + half_len) / up - a0);
  // period row + q * rows of the tile reads xs[xo + q * xstep - i]
  const int xo = row * down + a + (P - 1), xstep = rows * down;
  const float* t = ts + cc;
  float acc[RS_R];
#pragma unroll
  for (int q = 0; q < RS_R; ++q) acc[q] = 0.f;
#pragma unroll 4
  for (int i = 0; i < P; ++i) {
    const float w = t[i * pitch];
#pragma unroll
    for (int q = 0; q < RS_R; ++q) acc[q] = fmaf(xs[xo + q * xstep - i], w, acc[q]);
  }
#pragma unroll
  for (int q = 0; q < RS_R; ++q) {
    const long m = (k0 + row + q * rows) * up + c0 + cc;
    if (m < n_out) out[m] = acc[q];
  }
}

static long rs_gcd(long a, long b) {
  while (b) { const long t = a % b; a = b; b = t; }
  return a;
}

extern "C" int bsed_resample_poly(const void* in, int format, long n_in, int channels, const float* table, int up, int down,
                                  int half_len, float* out, long n_out, void* stream) {
  BSED_CHECK_ARG(in && table && out, "bsed_resample_poly: null tensor");
  BSED_CHECK_ARG(format == BSED_PCM_F32 || format == BSED_PCM_S16,
                 "bsed_resample_poly: format must be BSED_PCM_F32 or BSED_PCM_S16 (got %d)", format);
  BSED_CHECK_ARG(n_in >= 1 && n_in < (1L << 40), "bsed_resample_poly: n_in must be in 1..2^40 frames (got %ld)", n_in);
  BSED_CHECK_ARG(channels >= 1 && channels <= 64, "bsed_resample_poly: channels must be in 1..64 (got %d)", channels);
  BSED_CHECK_ARG(up >= 1 && down >= 1 && up <= (1 << 20) && down <= (1 << 20) && half_len >= 0,
                 "bsed_resample_poly: up and down must be in 1..2^20 and half_len >= 0 (got up=%d, down=%d, half_len=%d)", up,
                 down, half_len);
  BSED_CHECK_ARG(rs_gcd(up, down) == 1, "bsed_resample_poly: up=%d and down=%d are not coprime", up, down);
  const long want = (n_in * up + down - 1) / down;
  BSED_CHECK_ARG(n_out == want, "bsed_resample_poly: n_out must be ceil(n_in * up / down) = %ld (got %ld)", want, n_out);
  const size_t esz = format == BSED_PCM_S16 ? 2 : 4;
  const uintptr_t i0 = (uintptr_t)in, i1 = i0 + (size_t)n_in * channels * esz, o0 = (uintptr_t)out, o1 = o0 + (size_t)n_out * 4;
  BSED_CHECK_ARG(i1 <= o0 || o1 <= i0, "bsed_resample_poly: input and output overlap");
  BSED_CHECK_ARG(i0 % esz == 0 && o0 % 4 == 0 && (uintptr_t)table % 4 == 0, "bsed_resample_poly: misaligned pointer");
  // the layout: CW residues x NK periods per workgroup, its table rows and its samples in LDS
  const long P = 2L * half_len / up + 1;
  int lgCW = 0;
  while ((1 << lgCW) < up && (1 << lgCW) < RS_MAX_CW) ++lgCW;
  const int CW = 1 << lgCW, NK = RS_TILE / CW;
  const long span_max = (long)(NK - 1) * down + ((long)(CW - 1) * down) / up + 1 + P;
  const long lds = 4 * (P * (CW + 1) + span_max);
  BSED_CHECK_ARG(lds <= RS_LDS_BYTES,
                 "bsed_resample_poly: table too large for the layout: %ld taps per phase, up=%d, down=%d need %ld bytes of LDS "
                 "per workgroup (%d table rows + %ld samples), %d available", P, up, down, lds, CW, span_max, RS_LDS_BYTES);
  const long ctiles = (up + CW - 1) / CW, periods = (n_out + up - 1) / up, kgroups = (periods + NK - 1) / NK;
  BSED_CHECK_ARG(ctiles * kgroups < (1L << 31), "bsed_resample_poly: too many workgroups (%ld)", ctiles * kgroups);
  static BsedLdsOnce once_f32, once_s16;
  const float scale = format == BSED_PCM_S16 ? (float)(1.0 / (32768.0 * channels)) : (float)(1.0 / channels);
  const dim3 grid((unsigned)(ctiles * kgroups));
  if (format == BSED_PCM_S16) {
    BSED_HIP(bsed_max_lds(once_s16, (const void*)resample_poly_kernel<BSED_PCM_S16>, RS_LDS_BYTES));
    hipLaunchKernelGGL(resample_poly_kernel<BSED_PCM_S16>, grid, dim3(RS_THREADS), (size_t)lds, (hipStream_t)stream, in, n_in,
                       channels, scale, table, up, down, half_len, (int)P, lgCW, (int)ctiles, (int)span_max, out, n_out);
  } else {
    BSED_HIP(bsed_max_lds(once_f32, (const void*)resample_poly_kernel<BSED_PCM_F32>, RS_LDS_BYTES));
    hipLaunchKernelGGL(resample_poly_kernel<BSED_PCM_F32>, grid, dim3(RS_THREADS), (size_t)lds, (hipStream_t)stream, in, n_in,
                       channels, scale, table, up, down, half_len, (int)P, lgCW, (int)ctiles, (int)span_max, out, n_out);
  }
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
