// Validation on the GPU, second scorer: the intersection-based counts behind psds_eval's macro F1 and PSDS
// (bsed_intersection_counts).  The criteria are stated in include/bsed.h; the arithmetic below is that statement and
// nothing else: per pair one fmin, one fmax, one subtraction, one compare and -- where the pair intersects -- ONE float64
// division, added to a running float64 sum in the list order of the other side.  No product, so nothing a fused
// multiply-add could contract; float64 division is correctly rounded (the build has no fast-math): a host that loops the
// same way sees the same bits, and the counts are compared with == (tests/intersection_reference.py).
//
// Two launches, neither with a cap on a list length, neither using LDS:
//   intersect_est_kernel  one lane per estimated event e < E = est_offsets[S*B*C] (read on the device: no host sync).
//                         Its group (threshold s, clip b, class j) is found by a binary search of est_offsets.  The lane
//                         walks ref[b][j] for the DTC sum, writes the DTC flag byte of e and, when the event fails, walks
//                         the other classes' lists of the clip (one contiguous range of ref_seconds) for the CTTC sums.
//   intersect_ref_kernel  one lane per (threshold s, reference event r < R = ref_offsets[B*C]); its (clip, class) by a
//                         binary search of ref_offsets.  The lane walks est[s][b][k], adds the coverage of the events
//                         whose flag is set and compares with gtc.
// Both are grid-stride loops over a fixed grid (the totals live on the device), so any E and R are covered.
// Nsys / Nfp / Ntp / Nref: the lanes of a wave that share a destination (s, class) are counted with ballots and ONE lane
// adds the count -- events are ordered by group, so a wave holds a handful of destinations.  Cross triggers are rare and
// scattered over (k, j): one 64-bit add per (event, k).  All atomics are integer adds: two runs give the same bits.
#include "../../include/bsed.h"
#include "bsed_common.h"
#include <limits.h>
#include <math.h>

#define ISECT_THREADS 256
#define ISECT_MAX_BLOCKS 2048

// largest g in [0, n) with offsets[g] <= i, for 0 <= i < offsets[n]: the group of flat index i (empty groups are skipped
// because their offsets equal the next group's)
__device__ __forceinline__ int isect_group(const int* __restrict__ offsets, int n, int i) {
  int lo = 0, hi = n;                                 // invariant: offsets[lo] <= i < offsets[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// sum over list[r0 .. r1) of  it / len  for the pairs with it = fmin(off, off_r) - fmax(on, on_r) > 0, left to right
__device__ __forceinline__ double isect_sum_over(const double* __restrict__ list, int r0, int r1, double on, double off,
                                                 double len) {
  double sum = 0.0;
  for (int r = r0; r < r1; ++r) {
    const double it = fmin(off, list[2 * (size_t)r + 1]) - fmax(on, list[2 * (size_t)r]);
    if (it > 0.0) sum += it / len;
  }
  return sum;
}

// every active lane of the wave has a destination `key` and up to two 0/1 votes: per distinct key ONE lane adds the
// two popcounts to a[0] and a[1] of dst + stride * key
__device__ __forceinline__ void isect_wave_add(bool active, int key, bool vote0, bool vote1,
                                               unsigned long long* __restrict__ dst, int stride, int lane) {
  for (unsigned long long todo = __ballot(active); todo;) {
    const int leader = __ffsll((long long)todo) - 1;
    const int k = __shfl(key, leader);
    const bool mine = active && key == k;
    const unsigned long long n0 = __popcll(__ballot(mine && vote0)), n1 = __popcll(__ballot(mine && vote1));
    if (lane == leader) {
      if (n0) atomicAdd(dst + (size_t)stride * k, n0);
      if (n1) atomicAdd(dst + (size_t)stride * k + 1, n1);
    }
    todo &= ~__ballot(mine);
  }
}

__global__ __launch_bounds__(ISECT_THREADS) void intersect_est_kernel(
    const int* __restrict__ est_offsets, const double* __restrict__ est_seconds, const int* __restrict__ ref_offsets,
    const double* __restrict__ ref_seconds, const unsigned char* __restrict__ evaluated, int S, int B, int C, double dtc,
    double cttc, unsigned char* __restrict__ dtc_flags, unsigned long long* __restrict__ acc,
    unsigned long long* __restrict__ ct) {
  const int G = S * B * C;
  const long E = est_offsets[G];
  const int lane = threadIdx.x & 63;
  const long stride = (long)gridDim.x * ISECT_THREADS;
  // whole waves stay in the loop together (the ballots need them): the bound is rounded up to the wave
  for (long i = (long)blockIdx.x * ISECT_THREADS + threadIdx.x; i - lane < E; i += stride) {
    bool scored = false, fails = false;
    int key = 0;
    if (i < E) {
      const int e = (int)i;
      const int g = isect_group(est_offsets, G, e);
      const int j = g % C, b = (g / C) % B, s = g / (B * C);
      bool pass = false;
      if (!evaluated || evaluated[b]) {
        const double on = est_seconds[2 * (size_t)e], off = est_seconds[2 * (size_t)e + 1];
        const double len = off - on;
        const int* ro = ref_offsets + (size_t)b * C;
        pass = isect_sum_over(ref_seconds, ro[j], ro[j + 1], on, off, len) >= dtc;
        scored = true; fails = !pass; key = s * C + j;
        if (fails) {
          for (int k = 0; k < C; ++k) {
            if (k == j || ro[k] == ro[k + 1]) continue;
            if (isect_sum_over(ref_seconds, ro[k], ro[k + 1], on, off, len) >= cttc)
              atomicAdd(ct + ((size_t)s * C + k) * C + j, 1ull);
          }
        }
      }
      dtc_flags[e] = pass ? 1 : 0;
    }
    isect_wave_add(scored, key, fails, true, acc + 1, 4, lane);          // Nfp, Nsys
  }
}

__global__ __launch_bounds__(ISECT_THREADS) void intersect_ref_kernel(
    const int* __restrict__ est_offsets, const double* __restrict__ est_seconds, const int* __restrict__ ref_offsets,
    const double* __restrict__ ref_seconds, const unsigned char* __restrict__ evaluated, int S, int B, int C, double gtc,
    const unsigned char* __restrict__ dtc_flags, unsigned long long* __restrict__ acc) {
  const int R = ref_offsets[B * C];
  const long total = (long)S * R;
  const int lane = threadIdx.x & 63;
  const long stride = (long)gridDim.x * ISECT_THREADS;
  for (long i = (long)blockIdx.x * ISECT_THREADS + threadIdx.x; i - lane < total; i += stride) {
    bool scored = false, tp = false;
    int key = 0;
    if (i < total) {
      const int s = (int)(i / R), r = (int)(i % R);
      const int q = isect_group(ref_offsets, B * C, r);                  // q = b * C + k
      const int k = q % C, b = q / C;
      if (!evaluated || evaluated[b]) {
        const double on = ref_seconds[2 * (size_t)r], off = ref_seconds[2 * (size_t)r + 1];
        const double len = off - on;
        const size_t g = (size_t)s * B * C + q;
        double sum = 0.0;
        for (int e = est_offsets[g], e1 = est_offsets[g + 1]; e < e1; ++e) {
          if (!dtc_flags[e]) continue;                                   // only DTC-passing detections cover
          const double it = fmin(est_seconds[2 * (size_t)e + 1], off) - fmax(est_seconds[2 * (size_t)e], on);
          if (it > 0.0) sum += it / len;
        }
        scored = true; tp = sum >= gtc; key = s * C + k;
      }
    }
    // acc[key] = (Ntp, Nfp, Nsys, Nref): Ntp at +0, Nref at +3
    for (unsigned long long todo = __ballot(scored); todo;) {
      const int leader = __ffsll((long long)todo) - 1;
      const int kk = __shfl(key, leader);
      const bool mine = scored && key == kk;
      const unsigned long long ntp = __popcll(__ballot(mine && tp)), nref = __popcll(__ballot(mine));
      if (lane == leader) {
        if (ntp) atomicAdd(acc + 4 * (size_t)kk, ntp);
        atomicAdd(acc + 4 * (size_t)kk + 3, nref);
      }
      todo &= ~__ballot(mine);
    }
  }
}

extern "C" int bsed_intersection_counts(const int* est_offsets, const double* est_seconds, const int* ref_offsets,
                                        const double* ref_seconds, const unsigned char* evaluated, int S, int B, int C,
                                        double dtc, double gtc, double cttc, unsigned char* dtc_flags, long long* acc,
                                        long long* ct, void* stream) {
  BSED_CHECK_ARG(est_offsets && est_seconds && ref_offsets && ref_seconds && dtc_flags && acc && ct,
                 "bsed_intersection_counts: null tensor");
  BSED_CHECK_ARG(S > 0 && B > 0 && C > 0, "bsed_intersection_counts: bad shape (S=%d, B=%d, C=%d)", S, B, C);
  BSED_CHECK_ARG((long)S * C <= INT_MAX / C, "bsed_intersection_counts: S * C * C must fit int32 (S=%d, C=%d)", S, C);
  BSED_CHECK_ARG((long)B * C < INT_MAX && (long)S * B <= INT_MAX && (long)S * B * C < INT_MAX,
                 "bsed_intersection_counts: S * B * C + 1 offsets must fit int32 (S=%d, B=%d, C=%d)", S, B, C);
  BSED_CHECK_ARG(dtc > 0.0 && dtc <= 1.0 && gtc > 0.0 && gtc <= 1.0 && cttc > 0.0 && cttc <= 1.0,
                 "bsed_intersection_counts: dtc, gtc and cttc must lie in (0, 1]");
  // a grid that covers the usual totals in one round (2048 x 256 lanes); larger ones take more rounds of the same loop
  hipLaunchKernelGGL(intersect_est_kernel, dim3(ISECT_MAX_BLOCKS), dim3(ISECT_THREADS), 0, (hipStream_t)stream, est_offsets,
                     est_seconds, ref_offsets, ref_seconds, evaluated, S, B, C, dtc, cttc, dtc_flags,
                     reinterpret_cast<unsigned long long*>(acc), reinterpret_cast<unsigned long long*>(ct));
  BSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(intersect_ref_kernel, dim3(ISECT_MAX_BLOCKS), dim3(ISECT_THREADS), 0, (hipStream_t)stream, est_offsets,
                     est_seconds, ref_offsets, ref_seconds, evaluated, S, B, C, gtc, dtc_flags,
                     reinterpret_cast<unsigned long long*>(acc));
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
