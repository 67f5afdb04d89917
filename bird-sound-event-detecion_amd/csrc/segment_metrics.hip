// Validation on the GPU, third scorer: the segment-based counts behind sed_eval's SegmentBasedMetrics
// (bsed_segment_counts, ABI 16).  The rules are stated in include/bsed.h; nothing here is floating-point beyond ONE
// float64 division per event end (floor(onset / resolution), ceil(offset / resolution)) and a maximum, so the counts
// equal a host restatement exactly and are compared with ==.
//
// One launch, no workspace.  Grid (x, y, z) = (segment tiles, clips, thresholds), every dimension a grid stride:
//   z  a workgroup keeps ONE threshold s at a time: its counts stay in registers / LDS over all its clips and tiles and
//      are added to global memory once -- at most one 64-bit add per workgroup per (s, class, kind);
//   y  the clips b of that threshold;
//   x  the tiles of SEG_TILE segments of clip (s, b).  The host sizes x from expected_seconds alone (the list lengths are
//      device data); a workgroup walks the tiles x, x + gridDim.x, ... below the clip's segment count, so any x gives the
//      same counts, and a workgroup whose first tile starts past the last segment leaves the clip at once.
// Per clip the workgroup loads the C + 1 list offsets of both sides into LDS and, with length_seconds == 0, takes the
// maximum offset of every event of the clip (ceil(max / resolution) is the largest ceil(offset / resolution): both are
// monotone).  Per tile: two arrays of SEG_TILE 64-bit class masks (estimate, reference) are zeroed, every wave scans its
// share of the clip's events and ORs the class bit of those that reach into the tile into the segments they cover
// (seg_mark; LDS atomics: the lists may overlap and need no order), then one lane per segment takes the three popcounts
// behind Sub / Del / Ins, and per class two wave-wide ballots give the 64 segments' membership on both sides: lane c
// keeps class c's Ntp / Nfp / Nfn in registers; Ntn is the number of segments minus the three.
// Every workgroup of a clip scans all of the clip's events: a long recording is spread over its tiles, each of which
// reads the lists from L2 ("Segment-based metric", has the measurements).
// LDS: 2 * 1024 * 8 B masks + waves * (64 + 64 * UNROLL) * 4 B queues + 2 * 65 * 4 B offsets + 64 * 3 * 8 B + 3 * 8 B sums
// + waves * 8 B maxima: 21 KB (256 threads, 2 ahead) or 36.5 KB (512 threads, 8 ahead).
#include "../../include/bsed.h"
#include "bsed_common.h"
#include <limits.h>
#include <math.h>

// Two instances of one kernel <THREADS, UNROLL = events a lane loads ahead in the scan of a list>, chosen on the host by
// the tile columns the hint asks for -- the counts are the same, only the time differs:
//   clips of one tile (a validation batch: S x B workgroups with a few dozen events each): 256 threads, 2 ahead --
//     21 KB of LDS and few registers, so that the whole grid is resident at once (with the wide instance below the
//     1200 workgroups of case (a) of tools/segment_bench.py took three rounds: 61 us against 21 us);
//   longer clips (every workgroup scans ALL events of its clip): 512 threads, 8 ahead -- 36.5 KB of LDS.
#define SEG_SHORT_THREADS 256
#define SEG_SHORT_UNROLL 2
#define SEG_LONG_THREADS 512
#define SEG_LONG_UNROLL 8
#define SEG_OWN 8                         // segments up to which an event is marked by its own lane
#define SEG_TILE 1024                     // segments of one tile
#define SEG_MAX_TILES_X 1024              // grid.x
#define SEG_MAX_THRESHOLDS_Z 1024         // grid.z
#define SEG_MAX_WORKGROUPS 16384          // what grid.y is cut to fit

// class of event e of a clip: the largest c in [0, C) with off[c] <= e, for off[0] <= e < off[C]
__device__ __forceinline__ int seg_class(const int* off, int C, int e) {
  int lo = 0, hi = C;                                 // invariant: off[lo] <= e < off[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// One wave's share of the events e0 .. e1 of one side: each ORs its class bit into mask[t - t0] for its segments t in
// [t0, t0 + n).  Three steps, so that neither a sparse hit nor a long event leaves 63 lanes idle:
//   scan   SEG_UNROLL events per lane and round, all loads issued before the first use (the scan of a long list is bound
//          by the latency of its loads).  Most events of a long clip lie outside the tile: they are dropped by two
//          compares in seconds, without a division.  The bounds keep a whole segment of margin, far more than the
//          rounding of the products here and of the quotients below, so only events that certainly miss the tile are
//          dropped.  The others are pushed, by ballot and prefix count, onto the wave's queue of event indices in LDS.
//   rule   once the queue holds 64 (or the list ends), 64 lanes take one queued event each and apply the exact rule:
//          [max(0, floor(on / res)), ceil(off / res)) cut to the tile, nothing when the upper end is not above the lower;
//          the class by a binary search of the clip's offsets.
//   mark   an event of at most SEG_OWN segments is marked by its own lane (the short events of a validation clip: all at
//          once); a longer one by the WHOLE wave, event by event, lane l taking segments lo + l, lo + l + 64, ...
// queue: 64 + 64 * SEG_UNROLL ints of this wave (at most 63 left over + 64 * SEG_UNROLL pushed in a round); only this wave touches
// it, and LDS serves a wave's instructions in order, so the fences below are for the compiler.
template <int SEG_THREADS, int SEG_UNROLL>
__device__ __forceinline__ void seg_mark(const double* __restrict__ seconds, int e0, int e1, const int* off, int C,
                                         double resolution, long t0, int n, unsigned long long* mask, int* queue) {
  const int lane = threadIdx.x & 63;
  const double first = (double)t0, last = (double)(t0 + n);         // exact: both below 2^32
  const double before = (first - 1.0) * resolution, after = (last + 1.0) * resolution;
  int count = 0;                                                    // queued events: the same in every lane
  // whole waves stay in the loop together (the ballots need them); long: e1 may be near 2^31
  for (long base = (long)e0 + threadIdx.x; base - lane < e1; base += SEG_UNROLL * SEG_THREADS) {
    double on[SEG_UNROLL], end[SEG_UNROLL];
#pragma unroll
    for (int k = 0; k < SEG_UNROLL; ++k) {
      const long e = base + k * SEG_THREADS;
      const bool in = e < e1;
      on[k] = in ? seconds[2 * (size_t)e] : 0.0;
      end[k] = in ? seconds[2 * (size_t)e + 1] : before;            // beyond the list: dropped by the first compare
    }
#pragma unroll
    for (int k = 0; k < SEG_UNROLL; ++k) {
      const bool near = !(end[k] <= before || on[k] >= after);
      const unsigned long long votes = __ballot(near);
      if (near) queue[count + __popcll(votes & ((1ull << lane) - 1ull))] = (int)(base + k * SEG_THREADS);
      count += __popcll(votes);
    }
    const bool list_ends = base - lane + SEG_UNROLL * SEG_THREADS >= e1;
    while (count >= 64 || (list_ends && count > 0)) {
      const int m = count < 64 ? count : 64;
      count -= m;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      int lo_i = 0, hi_i = 0, cls = 0;
      if (lane < m) {
        const int e = queue[count + lane];
        const double lo = fmax(fmax(floor(seconds[2 * (size_t)e] / resolution), 0.0), first);
        const double hi = fmin(ceil(seconds[2 * (size_t)e + 1] / resolution), last);
        if (hi > lo) {
          lo_i = (int)(lo - first); hi_i = (int)(hi - first);
          cls = seg_class(off, C, e);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (hi_i - lo_i <= SEG_OWN)
        for (int i = lo_i; i < hi_i; ++i) atomicOr(&mask[i], 1ull << cls);
      for (unsigned long long todo = __ballot(hi_i - lo_i > SEG_OWN); todo; todo &= todo - 1ull) {
        const int j = __ffsll((long long)todo) - 1;
        const int i1 = __shfl(hi_i, j, 64);
        const unsigned long long bit = 1ull << __shfl(cls, j, 64);
        for (int i = __shfl(lo_i, j, 64) + lane; i < i1; i += 64) atomicOr(&mask[i], bit);
      }
    }
  }
}

__device__ __forceinline__ unsigned long long seg_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int SEG_THREADS, int SEG_UNROLL>
// the short instance asks for 5 waves per SIMD (96 registers; 6 would spill): 5 workgroups per CU, 1280 on the chip
__global__ __launch_bounds__(SEG_THREADS, SEG_THREADS == 256 ? 5 : 4) void segment_counts_kernel(
    const int* __restrict__ est_offsets, const double* __restrict__ est_seconds, const int* __restrict__ ref_offsets,
    const double* __restrict__ ref_seconds, const unsigned char* __restrict__ evaluated, int S, int B, int C,
    double resolution, int fixed_segments /* < 0: from the lists */, unsigned long long* __restrict__ class_acc,
    unsigned long long* __restrict__ overall) {
  __shared__ unsigned long long mask[2][SEG_TILE];                  // [0] estimate, [1] reference
  __shared__ int off[2][BSED_SEGMENT_MAX_CLASSES + 1];
  __shared__ unsigned long long wg_class[BSED_SEGMENT_MAX_CLASSES][3];
  __shared__ unsigned long long wg_overall[3];
  constexpr int SEG_WAVES = SEG_THREADS / 64;
  __shared__ double wg_max[SEG_WAVES];
  __shared__ int queue[SEG_WAVES][64 + 64 * SEG_UNROLL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int s = blockIdx.z; s < S; s += gridDim.z) {
    for (int i = tid; i < BSED_SEGMENT_MAX_CLASSES * 3; i += SEG_THREADS) (&wg_class[0][0])[i] = 0ull;
    if (tid < 3) wg_overall[tid] = 0ull;
    __syncthreads();
    unsigned long long tp = 0, fp = 0, fn = 0;                      // of class `lane`, over this wave's segments
    unsigned long long sub = 0, del = 0, ins = 0;                   // of this lane's segments
    unsigned long long segments = 0;                                // of the workgroup (the same in every thread)

    for (int b = blockIdx.y; b < B; b += gridDim.y) {
      if (evaluated && !evaluated[b]) continue;                     // the same in every thread
      __syncthreads();                                              // the previous clip's offsets are no longer read
      if (tid <= C) {
        off[0][tid] = est_offsets[((size_t)s * B + b) * C + tid];
        off[1][tid] = ref_offsets[(size_t)b * C + tid];
      }
      __syncthreads();
      const int e0 = off[0][0], e1 = off[0][C], r0 = off[1][0], r1 = off[1][C];
      int nseg = fixed_segments;
      if (nseg < 0) {
        double mx = -INFINITY;
#pragma unroll 4
        for (long e = (long)e0 + tid; e < e1; e += SEG_THREADS) mx = fmax(mx, est_seconds[2 * (size_t)e + 1]);
#pragma unroll 4
        for (long r = (long)r0 + tid; r < r1; r += SEG_THREADS) mx = fmax(mx, ref_seconds[2 * (size_t)r + 1]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
        if (lane == 0) wg_max[wave] = mx;
        __syncthreads();
        mx = wg_max[0];
#pragma unroll
        for (int w = 1; w < SEG_WAVES; ++w) mx = fmax(mx, wg_max[w]);
        const double d = ceil(mx / resolution);                     // -inf (no event) and negatives give 0 segments
        nseg = d > 0.0 ? (d >= (double)INT_MAX ? INT_MAX : (int)d) : 0;
      }

      for (long t0 = (long)blockIdx.x * SEG_TILE; t0 < nseg; t0 += (long)gridDim.x * SEG_TILE) {
        const int n = (int)((long)nseg - t0 < SEG_TILE ? (long)nseg - t0 : SEG_TILE);
        __syncthreads();                                            // the previous tile is counted
        for (int i = tid; i < n; i += SEG_THREADS) mask[0][i] = mask[1][i] = 0ull;
        __syncthreads();
        seg_mark<SEG_THREADS, SEG_UNROLL>(est_seconds, e0, e1, off[0], C, resolution, t0, n, mask[0], queue[wave]);
        seg_mark<SEG_THREADS, SEG_UNROLL>(ref_seconds, r0, r1, off[1], C, resolution, t0, n, mask[1], queue[wave]);
        __syncthreads();
        segments += (unsigned long long)n;
        for (int i0 = wave * 64; i0 < n; i0 += SEG_THREADS) {       // whole waves: the ballots need them
          const bool live = i0 + lane < n;
          const unsigned long long est = live ? mask[0][i0 + lane] : 0ull, ref = live ? mask[1][i0 + lane] : 0ull;
          const int nsys = __popcll(est), nref = __popcll(ref), ntp = __popcll(est & ref);
          sub += (unsigned long long)((nref < nsys ? nref : nsys) - ntp);
          del += (unsigned long long)(nref > nsys ? nref - nsys : 0);
          ins += (unsigned long long)(nsys > nref ? nsys - nref : 0);
          for (int c = 0; c < C; ++c) {
            const unsigned long long in_est = __ballot((est >> c) & 1ull), in_ref = __ballot((ref >> c) & 1ull);
            if (lane == c) {
              tp += __popcll(in_est & in_ref);
              fp += __popcll(in_est & ~in_ref);
              fn += __popcll(in_ref & ~in_est);
            }
          }
        }
      }
    }

    // the workgroup's sums of threshold s: waves meet in LDS, then one global add per (class, kind) that is not zero
    if (lane < C) {
      if (tp) atomicAdd(&wg_class[lane][0], tp);
      if (fp) atomicAdd(&wg_class[lane][1], fp);
      if (fn) atomicAdd(&wg_class[lane][2], fn);
    }
    sub = seg_wave_sum(sub); del = seg_wave_sum(del); ins = seg_wave_sum(ins);
    if (lane == 0) {
      if (sub) atomicAdd(&wg_overall[0], sub);
      if (del) atomicAdd(&wg_overall[1], del);
      if (ins) atomicAdd(&wg_overall[2], ins);
    }
    __syncthreads();
    if (segments) {
      if (tid < C) {
        const unsigned long long a = wg_class[tid][0], p = wg_class[tid][1], q = wg_class[tid][2];
        unsigned long long* dst = class_acc + 4 * ((size_t)s * C + tid);
        if (a) atomicAdd(dst, a);
        if (p) atomicAdd(dst + 1, p);
        if (q) atomicAdd(dst + 2, q);
        if (segments - a - p - q) atomicAdd(dst + 3, segments - a - p - q);
      } else if (tid >= 64 && tid < 68) {
        const int k = tid - 64;
        const unsigned long long v = k < 3 ? wg_overall[k] : segments;
        if (v) atomicAdd(overall + 4 * (size_t)s + k, v);
      }
    }
    __syncthreads();                                                // before the next threshold zeroes the sums
  }
}

extern "C" int bsed_segment_counts(const int* est_offsets, const double* est_seconds, const int* ref_offsets,
                                   const double* ref_seconds, const unsigned char* evaluated, int S, int B, int C,
                                   double resolution, double length_seconds, double expected_seconds,
                                   long long* class_acc, long long* overall, void* stream) {
  BSED_CHECK_ARG(est_offsets && est_seconds && ref_offsets && ref_seconds && class_acc && overall,
                 "bsed_segment_counts: null tensor");
  BSED_CHECK_ARG(S > 0 && B > 0 && C > 0, "bsed_segment_counts: bad shape (S=%d, B=%d, C=%d)", S, B, C);
  BSED_CHECK_ARG(C <= BSED_SEGMENT_MAX_CLASSES, "bsed_segment_counts: a segment's class mask holds at most %d classes, got C=%d",
                 BSED_SEGMENT_MAX_CLASSES, C);
  BSED_CHECK_ARG(isfinite(resolution) && resolution > 0.0, "bsed_segment_counts: resolution must be a positive finite number");
  BSED_CHECK_ARG(isfinite(length_seconds) && length_seconds >= 0.0,
                 "bsed_segment_counts: length_seconds must be 0 (from the lists) or a positive finite number");
  BSED_CHECK_ARG(isfinite(expected_seconds) && expected_seconds > 0.0,
                 "bsed_segment_counts: expected_seconds must be a positive finite number");
  BSED_CHECK_ARG((long)S * B <= INT_MAX && (long)S * B * C < INT_MAX,
                 "bsed_segment_counts: S * B * C + 1 offsets must fit int32 (S=%d, B=%d, C=%d)", S, B, C);
  int fixed_segments = -1;
  if (length_seconds > 0.0) {
    const double d = ceil(length_seconds / resolution);
    BSED_CHECK_ARG(d <= (double)INT_MAX, "bsed_segment_counts: length_seconds / resolution segments must fit int32");
    fixed_segments = (int)d;
  }
  // the tile dimension: what a clip of expected_seconds needs, so that such a clip is walked in one round
  const double want = ceil(ceil(expected_seconds / resolution) / (double)SEG_TILE);
  const int gx = want >= (double)SEG_MAX_TILES_X ? SEG_MAX_TILES_X : (want > 1.0 ? (int)want : 1);
  const int gz = S < SEG_MAX_THRESHOLDS_Z ? S : SEG_MAX_THRESHOLDS_Z;
  const int room = SEG_MAX_WORKGROUPS / (gx * gz);
  const int gy = B < room ? B : (room > 1 ? room : 1);
  unsigned long long* ca = reinterpret_cast<unsigned long long*>(class_acc);
  unsigned long long* ov = reinterpret_cast<unsigned long long*>(overall);
  if (gx == 1)
    hipLaunchKernelGGL((segment_counts_kernel<SEG_SHORT_THREADS, SEG_SHORT_UNROLL>), dim3(gx, gy, gz),
                       dim3(SEG_SHORT_THREADS), 0, (hipStream_t)stream, est_offsets, est_seconds, ref_offsets, ref_seconds,
                       evaluated, S, B, C, resolution, fixed_segments, ca, ov);
  else
    hipLaunchKernelGGL((segment_counts_kernel<SEG_LONG_THREADS, SEG_LONG_UNROLL>), dim3(gx, gy, gz),
                       dim3(SEG_LONG_THREADS), 0, (hipStream_t)stream, est_offsets, est_seconds, ref_offsets, ref_seconds,
                       evaluated, S, B, C, resolution, fixed_segments, ca, ov);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
