// Soundscape synthesis: a batch of training clips mixed from a device-resident bank of event snippets and backgrounds
// (bsed_synth_mix), and their strong / weak targets (bsed_synth_targets).  Stands in for the reference's offline
// desed / scaper generation (src/synth_data/synth_data_preprocess.py:116-188); include/bsed.h states the arithmetic.
//
// bsed_synth_mix: a workgroup owns SY_TILE consecutive samples of ONE clip.  Its first waves read the clip's event table
// into LDS once and mark the events that touch the tile; every thread then walks the marked events in table order, so
// an output sample is one chain  background, event 0, event 1, ...  of fp32 operations that depends on nothing but the
// tables: not on the tile size, the launch partition or B, and two launches give the same bits.  No atomics.
//
// Lanes take 4 consecutive samples and store them as 16 bytes.  Row b of the (B, n) output starts at element b * n, which
// is 16-byte aligned only when b * n is a multiple of 4, so the quads are laid on the FLAT output: a clip's tiles start
// hd = (b * n) & 3 samples before its first sample, and a quad that hangs over either end of the row (at most two per
// clip) stores its samples one by one.  A snippet sample sits at bank[src - on + j]: src - on is arbitrary, so a lane's
// four samples are one dword-aligned 16-byte load (gfx950 runs with unaligned access enabled: a global_load_dwordx4
// needs dword alignment only), taken only where all four lie inside the bank; a quad at the bank's edge, and the quad in
// which the background wraps, read sample by sample.  An index outside [0, bank_len) is never dereferenced and reads as 0.
//
// The background index (bg_phase + j) % bg_len costs one 64-bit division per thread: the later quads of the thread advance
// it by SY_STEP % bg_len with one conditional subtraction.
#include "../../include/bsed.h"
#include "bsed_common.h"

#define SY_THREADS 256
#define SY_R 4                                  // quads per thread
#define SY_STEP (SY_THREADS * 4)                // samples between two quads of a thread
#define SY_TILE (SY_STEP * SY_R)                // samples of a workgroup: 4096
#define SY_K BSED_SYNTH_MAX_EVENTS

typedef float sy_f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// bank[p .. p + 3]; indices outside [0, bank_len) read as 0 and are not dereferenced
__device__ __forceinline__ void sy_load4(const float* __restrict__ bank, long bank_len, long p, float* v) {
  if (p >= 0 && p + 4 <= bank_len) {
    const sy_f32x4u q = *reinterpret_cast<const sy_f32x4u*>(bank + p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (p + e >= 0 && p + e < bank_len) ? bank[p + e] : 0.f;
  }
}

__global__ void __launch_bounds__(SY_THREADS) synth_mix_kernel(
    const float* __restrict__ bank, long bank_len, const long* __restrict__ bg_off, const long* __restrict__ bg_len,
    const long* __restrict__ bg_phase, const float* __restrict__ bg_gain, const int* __restrict__ n_ev,
    const long* __restrict__ src, const long* __restrict__ on, const long* __restrict__ len, const float* __restrict__ g,
    const float* __restrict__ inv_fade, long n, int K, int tiles, float* __restrict__ out) {
  __shared__ long s_src[SY_K], s_on[SY_K], s_len[SY_K];
  __shared__ float s_g[SY_K], s_if[SY_K];
  __shared__ int s_hit[SY_K];
  __shared__ long s_bg[4];                      // offset, length, (phase - hd) mod length, SY_STEP mod length
  const long b = blockIdx.x / tiles;
  const int hd = (int)((b * n) & 3);
  const long t0 = (long)(blockIdx.x % tiles) * SY_TILE - hd;     // first sample of the tile (may be -hd .. -1)
  const int ne = min(max(n_ev[b], 0), K);
  if (threadIdx.x < ne) {
    const size_t e = (size_t)b * K + threadIdx.x;
    const long o = on[e], l = len[e];
    s_src[threadIdx.x] = src[e] - o;            // bank index of clip sample 0
    s_on[threadIdx.x] = o;
    s_len[threadIdx.x] = l;
    s_g[threadIdx.x] = g[e];
    s_if[threadIdx.x] = inv_fade[e];
    s_hit[threadIdx.x] = l > 0 && o < t0 + SY_TILE && o + l > t0;
  }
  if (threadIdx.x == 64) {
    const long l = bg_len[b];
    s_bg[0] = bg_off[b];
    s_bg[1] = l;
    if (l > 0) {
      long ph = (bg_phase[b] - hd) % l;
      s_bg[2] = ph < 0 ? ph + l : ph;
      s_bg[3] = SY_STEP % l;
    }
  }
  __syncthreads();

  const long boff = s_bg[0], blen = s_bg[1];
  const float bgain = bg_gain[b];
  long r = 0, rstep = 0;
  if (blen > 0) {                               // r = (bg_phase + j0) mod blen for the thread's first quad
    r = s_bg[2] + (t0 + hd + threadIdx.x * 4) % blen;
    if (r >= blen) r -= blen;
    rstep = s_bg[3];
  }
  float* row = out + b * n;
#pragma unroll 1
  for (int it = 0; it < SY_R; ++it) {
    const long j0 = t0 + it * SY_STEP + threadIdx.x * 4;
    if (j0 >= n) break;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (blen > 0) {
      float x[4];
      if (r + 4 <= blen) {
        sy_load4(bank, bank_len, boff + r, x);
      } else {                                  // the background wraps inside the quad (or is shorter than it)
        long rr = r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long p = boff + rr;
          x[e] = (p >= 0 && p < bank_len) ? bank[p] : 0.f;
          if (++rr >= blen) rr = 0;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __fmul_rn(x[e], bgain);
      r += rstep;
      if (r >= blen) r -= blen;
    }
    for (int k = 0; k < ne; ++k) {
      if (!s_hit[k]) continue;                  // the same for every lane of the workgroup
      const long o = s_on[k], l = s_len[k];
      const long i0 = j0 - o;
      if (i0 + 3 < 0 || i0 >= l) continue;      // no sample of this quad inside the event
      float x[4];
      sy_load4(bank, bank_len, s_src[k] + j0, x);
      const float gk = s_g[k], f = s_if[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long i = i0 + e;
        if (i >= 0 && i < l) {
          const float w = fminf(fminf(1.f, __fmul_rn((float)(i + 1), f)), fminf(1.f, __fmul_rn((float)(l - i), f)));
          acc[e] = fmaf(__fmul_rn(x[e], w), gk, acc[e]);
        }
      }
    }
    if (j0 >= 0 && j0 + 4 <= n) {
      *reinterpret_cast<f32x4*>(row + j0) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j0 + e >= 0 && j0 + e < n) row[j0 + e] = acc[e];
    }
  }
}

extern "C" int bsed_synth_mix(const float* bank, long bank_len, const long* bg_off, const long* bg_len, const long* bg_phase,
                              const float* bg_gain, const int* n_ev, const long* src, const long* on, const long* len,
                              const float* g, const float* inv_fade, int B, long n, int K, float* out, void* stream) {
  BSED_CHECK_ARG(bank && bg_off && bg_len && bg_phase && bg_gain && n_ev && src && on && len && g && inv_fade && out,
                 "bsed_synth_mix: null pointer");
  BSED_CHECK_ARG(B >= 1 && n >= 1, "bsed_synth_mix: B and n must be at least 1 (got B=%d, n=%ld)", B, n);
  BSED_CHECK_ARG(K >= 0 && K <= BSED_SYNTH_MAX_EVENTS, "bsed_synth_mix: K must be in 0..%d (got %d)", BSED_SYNTH_MAX_EVENTS, K);
  BSED_CHECK_ARG(bank_len >= 1, "bsed_synth_mix: bank_len must be at least 1 (got %ld)", bank_len);
  BSED_CHECK_ARG((uintptr_t)out % 16 == 0, "bsed_synth_mix: out must be 16-byte aligned");
  BSED_CHECK_ARG((uintptr_t)bank % 4 == 0 && (uintptr_t)bg_gain % 4 == 0 && (uintptr_t)n_ev % 4 == 0 && (uintptr_t)g % 4 == 0 &&
                 (uintptr_t)inv_fade % 4 == 0 && (uintptr_t)bg_off % 8 == 0 && (uintptr_t)bg_len % 8 == 0 &&
                 (uintptr_t)bg_phase % 8 == 0 && (uintptr_t)src % 8 == 0 && (uintptr_t)on % 8 == 0 && (uintptr_t)len % 8 == 0,
                 "bsed_synth_mix: misaligned table");
  BSED_CHECK_ARG(n < (1L << 40), "bsed_synth_mix: n must be below 2^40 samples (got %ld)", n);
  const long tiles = (n + 3 + SY_TILE - 1) / SY_TILE;           // the tiles of a clip start up to 3 samples early
  BSED_CHECK_ARG(tiles * B < (1L << 31), "bsed_synth_mix: too many workgroups (%ld)", tiles * B);
  hipLaunchKernelGGL(synth_mix_kernel, dim3((unsigned)(tiles * B)), dim3(SY_THREADS), 0, (hipStream_t)stream, bank, bank_len,
                     bg_off, bg_len, bg_phase, bg_gain, n_ev, src, on, len, g, inv_fade, n, K, (int)tiles, out);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

// one workgroup per clip: the event table to LDS, then every (frame, class) element and the clip's weak row
__global__ void __launch_bounds__(SY_THREADS) synth_targets_kernel(const int* __restrict__ n_ev, const int* __restrict__ cls,
                                                                    const int* __restrict__ on_f, const int* __restrict__ off_f,
                                                                    int K, int T, int C, float* __restrict__ strong,
                                                                    float* __restrict__ weak) {
  __shared__ int s_c[SY_K], s_a[SY_K], s_z[SY_K];
  const int b = blockIdx.x;
  const int ne = min(max(n_ev[b], 0), K);
  if (threadIdx.x < ne) {
    const size_t e = (size_t)b * K + threadIdx.x;
    s_c[threadIdx.x] = cls[e];
    s_a[threadIdx.x] = max(on_f[e], 0);
    s_z[threadIdx.x] = min(off_f[e], T);        // an empty or inverted interval covers no frame
  }
  __syncthreads();
  float* y = strong + (size_t)b * T * C;
  const int total = T * C;
  for (int i = threadIdx.x; i < total; i += SY_THREADS) {
    const int t = i / C, c = i - t * C;
    bool hit = false;
    for (int k = 0; k < ne; ++k) hit |= s_c[k] == c && s_a[k] <= t && t < s_z[k];
    y[i] = hit ? 1.f : 0.f;
  }
  for (int c = threadIdx.x; c < C; c += SY_THREADS) {
    bool hit = false;
    for (int k = 0; k < ne; ++k) hit |= s_c[k] == c && s_a[k] < s_z[k];
    weak[(size_t)b * C + c] = hit ? 1.f : 0.f;
  }
}

extern "C" int bsed_synth_targets(const int* n_ev, const int* cls, const int* on_f, const int* off_f, int B, int K, int T, int C,
                                  float* strong, float* weak, void* stream) {
  BSED_CHECK_ARG(n_ev && cls && on_f && off_f && strong && weak, "bsed_synth_targets: null pointer");
  BSED_CHECK_ARG(B >= 1 && T >= 1 && C >= 1, "bsed_synth_targets: B, T and C must be at least 1 (got B=%d, T=%d, C=%d)", B, T, C);
  BSED_CHECK_ARG(K >= 0 && K <= BSED_SYNTH_MAX_EVENTS, "bsed_synth_targets: K must be in 0..%d (got %d)", BSED_SYNTH_MAX_EVENTS,
                 K);
  BSED_CHECK_ARG((long)T * C < (1L << 31), "bsed_synth_targets: T * C must be below 2^31 (got %d x %d)", T, C);
  BSED_CHECK_ARG((uintptr_t)strong % 4 == 0 && (uintptr_t)weak % 4 == 0 && (uintptr_t)n_ev % 4 == 0 && (uintptr_t)cls % 4 == 0 &&
                 (uintptr_t)on_f % 4 == 0 && (uintptr_t)off_f % 4 == 0, "bsed_synth_targets: misaligned pointer");
  hipLaunchKernelGGL(synth_targets_kernel, dim3((unsigned)B), dim3(SY_THREADS), 0, (hipStream_t)stream, n_ev, cls, on_f, off_f, K,
                     T, C, strong, weak);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
