// Recording-level detection: cut one long waveform into overlapping clip-sized windows, stitch the windows'
// probabilities back onto the recording's frame grid, and decode contiguous regions along a long time axis.
// All four kernels are memory-bound and stateless: no atomics, a fixed order of summation, results bitwise repeatable.
#include "../../include/bsed.h"
#include "bsed_common.h"

// ---------------------------------------------------------------------------------------------
// bsed_gather_windows: out[w, :] = wave[starts[w] * frame_samples : ... + win], bit for bit.  frame_samples and win are
// multiples of 4 and both base pointers are 16-byte aligned (checked by the entry point), so every row moves as
// 16-byte loads and stores; adjacent lanes move adjacent 16-byte pieces of one row.  A window that does not lie inside
// [0, n) cannot be a slice of the recording: its row is zero-filled, nothing outside the recording is read.
// grid (x: pieces of a row, grid-strided; y: window)
// ---------------------------------------------------------------------------------------------
__global__ void gather_windows_kernel(const float* __restrict__ wave, long n, const int* __restrict__ starts, int win4,
                                      int frame_samples, float* __restrict__ out) {
  const int w = blockIdx.y;
  const long s = (long)starts[w] * frame_samples;
  const bool inside = s >= 0 && s + 4L * win4 <= n;
  const f32x4* src = reinterpret_cast<const f32x4*>(wave + (inside ? s : 0));
  f32x4* dst = reinterpret_cast<f32x4*>(out + (size_t)w * 4 * win4);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < win4; i += gridDim.x * blockDim.x)
    dst[i] = inside ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f};
}

extern "C" int bsed_gather_windows(const float* wave, long n, const int* starts, int W, int win, int frame_samples,
                                   float* out, void* stream) {
  BSED_CHECK_ARG(wave && starts && out, "bsed_gather_windows: null tensor");
  BSED_CHECK_ARG(n > 0 && W > 0 && W <= 65535 && win > 0 && win <= n && frame_samples > 0,
                 "bsed_gather_windows: bad shape (n=%ld, W=%d, win=%d, frame_samples=%d)", n, W, win, frame_samples);
  BSED_CHECK_ARG(win % 4 == 0 && frame_samples % 4 == 0,
                 "bsed_gather_windows: win (%d) and frame_samples (%d) must be multiples of 4 (rows move as 16-byte pieces)",
                 win, frame_samples);
  BSED_CHECK_ARG((uintptr_t)wave % 16 == 0 && (uintptr_t)out % 16 == 0, "bsed_gather_windows: wave and out must be 16-byte aligned");
  const int win4 = win / 4;
  const int gx = ceil_div(win4, 256) < 64 ? ceil_div(win4, 256) : 64;
  hipLaunchKernelGGL(gather_windows_kernel, dim3(gx, W), dim3(256), 0, (hipStream_t)stream, wave, n, starts, win4,
                     frame_samples, out);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

// ---------------------------------------------------------------------------------------------
// bsed_stitch_windows: out[f, c] = sum_w wgt(f - starts[w]) p[w, f - starts[w], c] / sum_w wgt(f - starts[w]) over the windows
// that cover frame f, in ascending window order.  Windows 0 .. W-2 start at w * hop (the caller's contract, checked on
// the host side of the package), so the ones that cover f are w in [ceil((f - Tp + 1) / hop), f / hop]; the last window
// may be aligned to the end of the recording instead and is tested on its own start.  One thread per V consecutive
// classes of one output frame (V = 4 when C is a multiple of 4: 16-byte accesses), adjacent lanes adjacent elements of
// the flattened output, so every read of a window row and the store are contiguous across the wave.
// Arithmetic per element with k covering windows: k fused multiply-adds, the sum of the integer weights (exact), one
// correctly rounded division.  A frame covered once is copied (weighted mean of one value), so windows that do not
// overlap concatenate bit for bit in both weightings.
// ---------------------------------------------------------------------------------------------
template <int V>
__global__ void stitch_windows_kernel(const float* __restrict__ p, const int* __restrict__ starts, int W, int Tp, int C,
                                      int hop, int T_total, int triangular, float* __restrict__ out) {
  typedef float vec __attribute__((ext_vector_type(V)));
  const int CV = C / V;
  const long total = (long)T_total * CV;
  const int s_last = starts[W - 1];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int f = (int)(i / CV), cv = (int)(i % CV);
    const int whi = min(f / hop, W - 2);
    const int wlo = f < Tp ? 0 : (f - Tp) / hop + 1;
    vec acc, first;
    for (int q = 0; q < V; ++q) { acc[q] = 0.f; first[q] = 0.f; }
    float wsum = 0.f;
    int k = 0;
    auto add = [&](int w, int j) {
      const vec v = *reinterpret_cast<const vec*>(p + ((size_t)w * Tp + j) * C + (size_t)cv * V);
      const float wgt = triangular ? (float)min(j + 1, Tp - j) : 1.f;
      for (int q = 0; q < V; ++q) acc[q] = fmaf(wgt, v[q], acc[q]);
      if (k == 0) first = v;
      wsum += wgt;
      ++k;
    };
    for (int w = wlo; w <= whi; ++w) add(w, f - w * hop);
    if (f >= s_last && f - s_last < Tp) add(W - 1, f - s_last);
    vec r;
    for (int q = 0; q < V; ++q) r[q] = k == 1 ? first[q] : (k ? acc[q] / wsum : 0.f);
    *reinterpret_cast<vec*>(out + (size_t)f * C + (size_t)cv * V) = r;
  }
}

extern "C" int bsed_stitch_windows(const float* p, const int* starts, int W, int Tp, int C, int hop_frames, int T_total,
                                   int weighting, float* out, void* stream) {
  BSED_CHECK_ARG(p && starts && out && p != out, "bsed_stitch_windows: null tensor");
  BSED_CHECK_ARG(W > 0 && Tp > 0 && C > 0 && T_total >= Tp, "bsed_stitch_windows: bad shape (W=%d, Tp=%d, C=%d, T_total=%d)",
                 W, Tp, C, T_total);
  BSED_CHECK_ARG(hop_frames >= 1 && hop_frames <= Tp, "bsed_stitch_windows: hop_frames must be in 1..Tp (got %d, Tp=%d)",
                 hop_frames, Tp);
  // the last window ends at T_total and starts no later than one hop after window W-2: no frame is left uncovered
  BSED_CHECK_ARG((long)T_total - Tp <= (long)(W - 1) * hop_frames && (W == 1 || (long)T_total - Tp > (long)(W - 2) * hop_frames),
                 "bsed_stitch_windows: T_total=%d does not fit %d windows of %d frames every %d", T_total, W, Tp, hop_frames);
  BSED_CHECK_ARG(weighting == BSED_STITCH_UNIFORM || weighting == BSED_STITCH_TRIANGULAR,
                 "bsed_stitch_windows: weighting must be BSED_STITCH_UNIFORM or BSED_STITCH_TRIANGULAR (got %d)", weighting);
  const bool v4 = C % 4 == 0 && (uintptr_t)p % 16 == 0 && (uintptr_t)out % 16 == 0;
  const long total = (long)T_total * (v4 ? C / 4 : C);
  const dim3 grid((unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256));
  if (v4)
    hipLaunchKernelGGL(stitch_windows_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p, starts, W, Tp, C, hop_frames,
                       T_total, weighting == BSED_STITCH_TRIANGULAR, out);
  else
    hipLaunchKernelGGL(stitch_windows_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p, starts, W, Tp, C, hop_frames,
                       T_total, weighting == BSED_STITCH_TRIANGULAR, out);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

// ---------------------------------------------------------------------------------------------
// Contiguous-region decode of ONE (T, C) mask with a long time axis (bsed_decode_count / _write walk a whole column in
// one thread: right for 256 clips of 313 frames, twenty busy lanes for an hour of audio).  Onsets and region ends are
// local: frame t opens a region iff on[t] && !on[t-1], and closes one iff on[t] && !on[t+1] (the offset frame is t + 1;
// frames outside [0, T) are off); within a class the k-th onset belongs to the k-th end.  The time axis is cut into
// chunks of BSED_DECODE_LONG_FRAMES = 64 frames, one workgroup each:
//   * the chunk's frames plus one frame on either side are (64 + 2) * C consecutive floats of the mask: the workgroup
//     reads them with adjacent lanes on adjacent floats and keeps one byte per element in LDS;
//   * a wave then takes a class with lane = frame; the ballot of the onset (end) flags gives the chunk's count as a
//     popcount and each event's rank inside the chunk as the popcount of the lower lanes.
// count writes counts[c * nchunks + chunk]; the caller takes the exclusive prefix in that (class-major) order; write
// puts the onsets at offset + rank, and the ends at the same ranks: the ends before a chunk are the onsets before it,
// less one if a region is open across the chunk's first frame (on[t0 - 1] && on[t0]) -- no state passes between chunks.
// ---------------------------------------------------------------------------------------------
#define DL_F BSED_DECODE_LONG_FRAMES
static_assert(DL_F == 64, "one lane per frame of a chunk");

// s[(l + 1) * C + c] = on(t0 + l, c) for l in -1 .. DL_F
__device__ __forceinline__ void decode_long_stage(const float* __restrict__ mask, int T, int C, unsigned char* s) {
  const long lo = ((long)blockIdx.x * DL_F - 1) * C, total = (long)T * C;
  for (int i = threadIdx.x; i < (DL_F + 2) * C; i += blockDim.x) {
    const long g = lo + i;
    s[i] = (g >= 0 && g < total && mask[g] != 0.f) ? 1 : 0;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(256) decode_long_count_kernel(const float* __restrict__ mask, int T, int C, int nchunks,
                                                                int* __restrict__ counts) {
  extern __shared__ unsigned char dl_s[];
  decode_long_stage(mask, T, C, dl_s);
  const int lane = threadIdx.x & 63;
  for (int c = threadIdx.x >> 6; c < C; c += blockDim.x >> 6) {
    const bool onset = dl_s[(lane + 1) * C + c] && !dl_s[lane * C + c];
    const unsigned long long b = __ballot(onset);
    if (lane == 0) counts[(size_t)c * nchunks + blockIdx.x] = __popcll(b);
  }
}

__global__ void __launch_bounds__(256) decode_long_write_kernel(const float* __restrict__ mask, const int* __restrict__ offsets,
                                                                int T, int C, int nchunks, double scale, double max_len,
                                                                int* __restrict__ ev_class, int* __restrict__ ev_frames,
                                                                double* __restrict__ ev_seconds) {
  extern __shared__ unsigned char dl_s[];
  decode_long_stage(mask, T, C, dl_s);
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * DL_F + lane;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int c = threadIdx.x >> 6; c < C; c += blockDim.x >> 6) {
    const bool on = dl_s[(lane + 1) * C + c];
    const bool onset = on && !dl_s[lane * C + c], end = on && !dl_s[(lane + 2) * C + c];
    const unsigned long long bo = __ballot(onset), be = __ballot(end);
    const int base = offsets[(size_t)c * nchunks + blockIdx.x];
    const int open = (dl_s[c] && dl_s[C + c]) ? 1 : 0;       // a region runs across the chunk's first frame
    if (onset) {
      const size_t k = (size_t)base + __popcll(bo & below);
      ev_class[k] = c;
      ev_frames[2 * k] = t;
      ev_seconds[2 * k] = fmin(fmax((double)t * scale, 0.0), max_len);
    }
    if (end) {
      const size_t k = (size_t)(base - open) + __popcll(be & below);
      ev_frames[2 * k + 1] = t + 1;
      ev_seconds[2 * k + 1] = fmin(fmax((double)(t + 1) * scale, 0.0), max_len);
    }
  }
}

#define DL_MAX_C 512   // (64 + 2) * C bytes of LDS per workgroup

extern "C" int bsed_decode_long_count(const float* mask, int T, int C, int* counts, void* stream) {
  BSED_CHECK_ARG(mask && counts, "bsed_decode_long_count: null tensor");
  BSED_CHECK_ARG(T > 0 && C > 0 && C <= DL_MAX_C, "bsed_decode_long_count: bad shape (T=%d, C=%d; C <= %d)", T, C, DL_MAX_C);
  const int nchunks = ceil_div(T, DL_F);
  hipLaunchKernelGGL(decode_long_count_kernel, dim3(nchunks), dim3(256), (size_t)(DL_F + 2) * C, (hipStream_t)stream, mask, T,
                     C, nchunks, counts);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

extern "C" int bsed_decode_long_write(const float* mask, const int* offsets, int T, int C, double scale, double max_len,
                                      int* ev_class, int* ev_frames, double* ev_seconds, void* stream) {
  BSED_CHECK_ARG(mask && offsets && ev_class && ev_frames && ev_seconds, "bsed_decode_long_write: null tensor");
  BSED_CHECK_ARG(T > 0 && C > 0 && C <= DL_MAX_C, "bsed_decode_long_write: bad shape (T=%d, C=%d; C <= %d)", T, C, DL_MAX_C);
  const int nchunks = ceil_div(T, DL_F);
  hipLaunchKernelGGL(decode_long_write_kernel, dim3(nchunks), dim3(256), (size_t)(DL_F + 2) * C, (hipStream_t)stream, mask,
                     offsets, T, C, nchunks, scale, max_len, ev_class, ev_frames, ev_seconds);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
