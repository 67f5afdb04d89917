// Clip-level tagging on the GPU (ABI 7): the tp / fp / fn / tn counts of a whole threshold sweep from one launch
// (bsed_tag_counts: the reference's get_f_measure_by_class, src/evaluation_measures.py:386-427, counting as
// intermediate_at_measures does, :442-446) and the pseudo-labels of a batch as one bit mask per clip (bsed_tag_masks:
// src/audio_tagging_inference.py:289-316).  Integer counting on float compares: the results equal a host restatement
// exactly and two runs give the same bits (the only atomics are integer adds).
#include "../../include/bsed.h"
#include "bsed_common.h"
#include <limits.h>
#include <math.h>

#define TAG_THREADS 256
#define TAG_MAX_CLIPS 64                  // clips of one workgroup
#define TAG_WG_ELEMS 16384                // a workgroup's clips hold about this many elements of the larger tensor
#define TAG_LDS_MAX (64 * 1024)
#define TAG_UNSTAGED_CLIPS 4

// ---------------------------------------------------------------------------------------------
// The time maximum.  numpy's max over an axis propagates NaN, and a NaN weak score then fails `> threshold` (est = 0);
// fmaxf would drop the NaN.  So the running maximum keeps a NaN once it has met one, and the cross-thread maximum is an
// unsigned max over an order-preserving key in which every NaN is the top value.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float tag_max(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ unsigned tag_key(float v) {
  if (v != v) return 0xFFFFFFFFu;
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);       // never 0: the tile's initial value lies below every key
}
__device__ __forceinline__ float tag_unkey(unsigned k) {
  if (k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// tile[q * C + c] for the clips b0 .. b0 + nclips of one workgroup; ends with a barrier.
//   T == 0: src is (B, C) and is copied (one contiguous run of nclips * C floats);
//   T >= 1: src is (B, T, C): the maximum over time.  The (T, C) tile of a clip is walked flat: thread j < G * C (G =
//           256 / C whole frames) starts at element j and steps G * C elements, so a wave's loads are contiguous, every
//           thread stays on class j % C and keeps its maximum in a register; the G partial maxima of a class meet in
//           LDS through one unsigned max each.  C > 256: G = 1 and a thread walks the classes j, j + 256, ...
//   BIN:    the reduced value is binarised with `> 0.5` (the reference's label path, :394-398).
template <bool BIN>
__device__ void tag_fill(const float* __restrict__ src, int T, int C, size_t b0, int nclips, float* tile) {
  const int n = nclips * C;
  if (T == 0) {
    const float* p = src + b0 * C;
    for (int i = threadIdx.x; i < n; i += TAG_THREADS) tile[i] = p[i];
    __syncthreads();
    return;
  }
  unsigned* keys = reinterpret_cast<unsigned*>(tile);
  for (int i = threadIdx.x; i < n; i += TAG_THREADS) keys[i] = 0u;
  __syncthreads();
  const int Cx = C < TAG_THREADS ? C : TAG_THREADS, G = TAG_THREADS / Cx;
  const int cl = threadIdx.x % Cx, g = threadIdx.x / Cx;
  if (g < G && g < T) {
    for (int q = 0; q < nclips; ++q) {
      const float* clip = src + (b0 + q) * (size_t)T * C;
      for (int c = cl; c < C; c += Cx) {
        float m = -INFINITY;
#pragma unroll 4
        for (int t = g; t < T; t += G) m = tag_max(m, clip[(size_t)t * C + c]);
        atomicMax(&keys[q * C + c], tag_key(m));
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += TAG_THREADS) {
    const float v = tag_unkey(keys[i]);
    tile[i] = BIN ? (v > 0.5f ? 1.0f : 0.0f) : v;
  }
  __syncthreads();
}

// the same value for one (clip, class) straight from global memory (the path without a tile)
template <bool BIN>
__device__ __forceinline__ float tag_value(const float* __restrict__ src, int T, int C, size_t b, int c) {
  if (T == 0) return src[b * C + c];
  const float* clip = src + b * (size_t)T * C + c;
  float m = -INFINITY;
  for (int t = 0; t < T; ++t) m = tag_max(m, clip[(size_t)t * C]);
  return BIN ? (m > 0.5f ? 1.0f : 0.0f) : m;
}

// ---------------------------------------------------------------------------------------------
// bsed_tag_counts.  One workgroup per `clips` clips.  Their weak scores and reference values are reduced into two LDS
// tiles (nclips, C) -- every input element is read from HBM once -- and every (threshold, class) pair is then counted
// from the tiles by ONE thread: adjacent lanes adjacent classes (adjacent banks), lanes of one class and different
// thresholds read one address (a broadcast).  The thread sums its four counts over the workgroup's clips in registers
// and adds the non-zero ones to counts (S, C, 4) with 64-bit integer atomics: at most one add per workgroup per (s, c,
// kind).  The compares are intermediate_at_measures' own (est + ref == 2, est - ref == 1, ref - est == 1, est + ref == 0)
// in float64, as numpy evaluates them on a float label array, so a target of -1 or 2 or 0.3 counts as it does there.
// STAGED = false (a single clip's two rows exceed the LDS budget, C > 8192): the pairs read global memory, where the
// repeated reads of the thresholds are served by the caches.  Same results, no size limit.
// ---------------------------------------------------------------------------------------------
template <bool STAGED>
__global__ __launch_bounds__(TAG_THREADS) void tag_counts_kernel(const float* __restrict__ scores, int Ts,
                                                                 const float* __restrict__ targets, int Tt,
                                                                 const float* __restrict__ thresholds, int per_class, int S,
                                                                 int B, int C, int clips,
                                                                 unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) float tag_tile[];
  const size_t b0 = (size_t)blockIdx.x * clips;
  const int nclips = (int)(((size_t)B - b0) < (size_t)clips ? (size_t)B - b0 : (size_t)clips);
  float* tile_s = tag_tile;
  float* tile_r = tag_tile + (size_t)clips * C;
  if (STAGED) {
    tag_fill<false>(scores, Ts, C, b0, nclips, tile_s);
    if (Tt == 0) tag_fill<false>(targets, 0, C, b0, nclips, tile_r);
    else tag_fill<true>(targets, Tt, C, b0, nclips, tile_r);
  }
  for (int i = threadIdx.x; i < S * C; i += TAG_THREADS) {
    const int s = i / C, c = i % C;
    const float thr = thresholds[per_class ? i : s];
    unsigned tp = 0, fp = 0, fn = 0, tn = 0;
    for (int q = 0; q < nclips; ++q) {
      float score, ref;
      if (STAGED) {
        score = tile_s[q * C + c];
        ref = tile_r[q * C + c];
      } else {
        score = tag_value<false>(scores, Ts, C, b0 + q, c);
        ref = Tt == 0 ? tag_value<false>(targets, 0, C, b0 + q, c) : tag_value<true>(targets, Tt, C, b0 + q, c);
      }
      const double e = score > thr ? 1.0 : 0.0, r = (double)ref;
      tp += (e + r == 2.0);
      fp += (e - r == 1.0);
      fn += (r - e == 1.0);
      tn += (e + r == 0.0);
    }
    unsigned long long* a = counts + 4 * (size_t)i;   // i = s * C + c
    if (tp) atomicAdd(a, (unsigned long long)tp);
    if (fp) atomicAdd(a + 1, (unsigned long long)fp);
    if (fn) atomicAdd(a + 2, (unsigned long long)fn);
    if (tn) atomicAdd(a + 3, (unsigned long long)tn);
  }
}

// clips per workgroup: about TAG_WG_ELEMS elements of the larger tensor, at most TAG_MAX_CLIPS
static int tag_clips(int Ts, int Tt, int C) {
  const long per_clip = (long)(Ts > Tt ? Ts : Tt) * C;     // T * C <= INT_MAX / 2 was checked
  long clips = per_clip > 0 ? TAG_WG_ELEMS / per_clip : TAG_MAX_CLIPS;
  if (clips > TAG_MAX_CLIPS) clips = TAG_MAX_CLIPS;
  return clips < 1 ? 1 : (int)clips;
}

extern "C" int bsed_tag_counts(const float* scores, int T_scores, const float* targets, int T_targets,
                               const float* thresholds, int per_class, int S, int B, int C, long long* counts,
                               void* stream) {
  BSED_CHECK_ARG(S > 0 && B >= 0 && C > 0 && T_scores >= 0 && T_targets >= 0,
                 "bsed_tag_counts: bad shape (S=%d, B=%d, C=%d, T_scores=%d, T_targets=%d)", S, B, C, T_scores, T_targets);
  BSED_CHECK_ARG((long)T_scores * C <= INT_MAX / 2 && (long)T_targets * C <= INT_MAX / 2 && (long)S * C <= INT_MAX / 4,
                 "bsed_tag_counts: T * C or S * C too large (S=%d, C=%d, T_scores=%d, T_targets=%d)", S, C, T_scores,
                 T_targets);
  BSED_CHECK_ARG(per_class == 0 || per_class == 1, "bsed_tag_counts: per_class must be 0 or 1, got %d", per_class);
  if (B == 0) return BSED_OK;                          // nothing to count: the accumulator stays as it is
  BSED_CHECK_ARG(scores && targets && thresholds && counts, "bsed_tag_counts: null tensor");
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(counts);
  int clips = tag_clips(T_scores, T_targets, C);
  const long fit = TAG_LDS_MAX / (2L * C * (long)sizeof(float));   // clips whose two rows fit the tile
  if (fit >= 1) {
    if (clips > fit) clips = (int)fit;
    const size_t lds = 2 * (size_t)clips * C * sizeof(float);
    hipLaunchKernelGGL((tag_counts_kernel<true>), dim3(ceil_div(B, clips)), dim3(TAG_THREADS), lds, (hipStream_t)stream,
                       scores, T_scores, targets, T_targets, thresholds, per_class, S, B, C, clips, acc);
  } else {
    clips = TAG_UNSTAGED_CLIPS;
    hipLaunchKernelGGL((tag_counts_kernel<false>), dim3(ceil_div(B, clips)), dim3(TAG_THREADS), 0, (hipStream_t)stream,
                       scores, T_scores, targets, T_targets, thresholds, per_class, S, B, C, clips, acc);
  }
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

// ---------------------------------------------------------------------------------------------
// bsed_tag_masks.  The same score tile; then one wave per clip: lane c holds class c (C <= 64), the clip's mask is ONE
// 64-bit ballot of `score > threshold`, stored by lane 0 at masks[row_offset + b].  The non-empty clips of the workgroup
// are summed in LDS and added to the device counter with one 64-bit integer atomic per workgroup.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TAG_THREADS) void tag_masks_kernel(const float* __restrict__ scores, int Ts,
                                                                const float* __restrict__ class_thresholds,
                                                                float threshold, int B, int C, int clips,
                                                                unsigned long long* __restrict__ masks,
                                                                unsigned long long* __restrict__ nonempty) {
  extern __shared__ __attribute__((aligned(16))) float tag_tile[];
  __shared__ unsigned wg_nonempty;
  const size_t b0 = (size_t)blockIdx.x * clips;
  const int nclips = (int)(((size_t)B - b0) < (size_t)clips ? (size_t)B - b0 : (size_t)clips);
  if (threadIdx.x == 0) wg_nonempty = 0;
  tag_fill<false>(scores, Ts, C, b0, nclips, tag_tile);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = lane < C;
  const float thr = live && class_thresholds ? class_thresholds[lane] : threshold;
  unsigned mine = 0;
  for (int q = wave; q < nclips; q += TAG_THREADS / 64) {
    const float v = live ? tag_tile[q * C + lane] : 0.f;
    const unsigned long long m = __ballot(live && v > thr);
    if (lane == 0) {
      masks[b0 + q] = m;
      mine += m != 0;
    }
  }
  if (lane == 0 && mine) atomicAdd(&wg_nonempty, mine);
  __syncthreads();
  if (threadIdx.x == 0 && wg_nonempty) atomicAdd(nonempty, (unsigned long long)wg_nonempty);
}

extern "C" int bsed_tag_masks(const float* scores, int T_scores, const float* class_thresholds, float threshold, int B,
                              int C, long row_offset, long N, uint64_t* masks, long long* nonempty, void* stream) {
  BSED_CHECK_ARG(B >= 0 && C > 0 && T_scores >= 0, "bsed_tag_masks: bad shape (B=%d, C=%d, T_scores=%d)", B, C, T_scores);
  BSED_CHECK_ARG(C <= 64, "bsed_tag_masks: a mask holds at most 64 classes, got C=%d", C);
  BSED_CHECK_ARG((long)T_scores * C <= INT_MAX / 2, "bsed_tag_masks: T * C too large (C=%d, T_scores=%d)", C, T_scores);
  BSED_CHECK_ARG(row_offset >= 0 && N >= 0 && row_offset <= N && (long)B <= N - row_offset,
                 "bsed_tag_masks: rows %ld .. %ld do not lie inside the buffer of %ld", row_offset, row_offset + B, N);
  if (B == 0) return BSED_OK;
  BSED_CHECK_ARG(scores && masks && nonempty, "bsed_tag_masks: null tensor");
  const int clips = tag_clips(T_scores, 0, C);
  hipLaunchKernelGGL(tag_masks_kernel, dim3(ceil_div(B, clips)), dim3(TAG_THREADS), (size_t)clips * C * sizeof(float),
                     (hipStream_t)stream, scores, T_scores, class_thresholds, threshold, B, C, clips,
                     reinterpret_cast<unsigned long long*>(masks) + row_offset,
                     reinterpret_cast<unsigned long long*>(nonempty));
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
