// Validation on the GPU: the event lists of MANY thresholds from one launch (bsed_sweep_count / bsed_sweep_write), and the
// collar-based event counts Ntp / Nsys / Nref of those lists against reference events (bsed_event_match).  Everything
// here is integer counting on float comparisons: the results equal a host restatement exactly, and two runs give the
// same bits (the only atomics are integer adds).
#include "../../include/bsed.h"
#include "bsed_common.h"
#include <limits.h>
#include <math.h>

// ---------------------------------------------------------------------------------------------
// Threshold sweep.  For threshold s the events are what bsed_binarize_median(thresholds[s], windows[c]) followed by
// bsed_decode_count / bsed_decode_write give (csrc/head.hip): the same `> threshold` compare, scipy's window
// [t - win/2, t - win/2 + win) with the 'reflect' boundary of period 2T, the same need = win - win/2, the same
// fmin(fmax((double)frame * scale, 0.0), max_len).
//
// One workgroup per clip.  The clip's (T, C) tile is copied from HBM to LDS once (313 x 20 x 4 B = 25 KB) and every
// (threshold, class) column is walked from there by one thread: adjacent lanes adjacent classes (adjacent banks), lanes
// of the same class and different thresholds read one address (a broadcast).  The median is a sliding count: the
// window of frame 0 is counted once (win % 2T reads, plus one pass over the column for the whole periods a window longer
// than 2T holds), then every step adds the bit that enters and drops the bit that leaves, both through a position that
// walks the reflected period -- win + 2T reads per column instead of win * T.
// A tile that does not fit 160 KB of LDS (T * C > 40960) is not staged: the STAGED = false instance walks the columns
// in global memory, where the repeated reads of the thresholds are served by the caches.  Same results, no size limit.
// Two passes like the decode: count, then write at the caller's exclusive prefix, so that the list is ordered by
// threshold, clip, class, time without atomics.
// ---------------------------------------------------------------------------------------------
template <bool WRITE, bool STAGED>
__global__ __launch_bounds__(256) void sweep_kernel(const float* __restrict__ strong, const float* __restrict__ thresholds,
                                                    const int* __restrict__ windows, const int* __restrict__ offsets, int S,
                                                    int B, int T, int C, double scale, double max_len,
                                                    int* __restrict__ counts, int* __restrict__ ev_frames,
                                                    double* __restrict__ ev_seconds) {
  extern __shared__ __attribute__((aligned(16))) float sweep_tile[];
  const int b = blockIdx.x;
  const float* src = strong + (size_t)b * T * C;
  if (STAGED) {
    for (int i = threadIdx.x; i < T * C; i += blockDim.x) sweep_tile[i] = src[i];
    __syncthreads();
  }
  const int T2 = 2 * T;
  for (int i = threadIdx.x; i < S * C; i += blockDim.x) {
    const int s = i / C, c = i % C;
    const size_t g = ((size_t)s * B + b) * C + c;
    const int win = windows[c];
    if (win <= 0) {                                   // a dropped class: no events
      if (!WRITE) counts[g] = 0;
      continue;
    }
    const float thr = thresholds[s];
    auto bit = [&](int t) -> int { return (STAGED ? sweep_tile[t * C + c] : src[(size_t)t * C + c]) > thr ? 1 : 0; };
    auto refl = [&](int p) -> int { return p < T ? p : T2 - 1 - p; };   // position in the period 2T -> frame
    const int need = win - win / 2;
    int cnt = 0;
    if (win >= T2) {                                  // whole periods inside the window: each holds every frame twice
      int tot = 0;
      for (int t = 0; t < T; ++t) tot += bit(t);
      cnt = (win / T2) * 2 * tot;
    }
    int lo = (-(win / 2)) % T2;                       // where the window of frame 0 starts
    if (lo < 0) lo += T2;
    int hi = lo;                                      // one past its last position, modulo the period
    for (int k = win % T2; k > 0; --k) {
      cnt += bit(refl(hi));
      hi = hi + 1 == T2 ? 0 : hi + 1;
    }
    int n = WRITE ? offsets[g] : 0;
    int onset = 0;
    bool prev = false;
    for (int t = 0; t <= T; ++t) {
      const bool on = t < T && cnt >= need;
      if (on && !prev) onset = t;
      if (!on && prev) {
        if (WRITE) {
          ev_frames[2 * (size_t)n] = onset;
          ev_frames[2 * (size_t)n + 1] = t;
          ev_seconds[2 * (size_t)n] = fmin(fmax((double)onset * scale, 0.0), max_len);
          ev_seconds[2 * (size_t)n + 1] = fmin(fmax((double)t * scale, 0.0), max_len);
        }
        ++n;
      }
      prev = on;
      if (t < T) {                                    // slide: the window of frame t + 1
        cnt += bit(refl(hi)) - bit(refl(lo));
        hi = hi + 1 == T2 ? 0 : hi + 1;
        lo = lo + 1 == T2 ? 0 : lo + 1;
      }
    }
    if (!WRITE) counts[g] = n;
  }
}

#define SWEEP_LDS_MAX (160 * 1024)
static BsedLdsOnce g_sweep_lds[2];

// shape checks shared by the two passes; no HIP call
static int sweep_geometry(const char* who, int S, int B, int T, int C) {
  BSED_CHECK_ARG(S > 0 && B > 0 && T > 0 && C > 0, "%s: bad shape (S=%d, B=%d, T=%d, C=%d)", who, S, B, T, C);
  BSED_CHECK_ARG((long)T * C <= INT_MAX / 2 && (long)S * C <= INT_MAX, "%s: T * C or S * C too large (S=%d, T=%d, C=%d)", who, S,
                 T, C);
  // a column of T frames holds at most ceil(T / 2) on-runs: the worst-case list must be addressable with int32
  long worst = (long)S * B;                           // < 2^62
  const long half = ((long)T + 1) / 2;
  const bool fits = worst <= INT_MAX && (worst *= C) <= INT_MAX && (worst *= half) <= INT_MAX;
  BSED_CHECK_ARG(fits, "%s: worst-case event total S*B*C*ceil(T/2) exceeds 2^31 - 1 (S=%d, B=%d, T=%d, C=%d)", who, S, B, T, C);
  return BSED_OK;
}

template <bool WRITE>
static int sweep_launch(const float* strong, const float* thresholds, const int* windows, const int* offsets, int S, int B,
                        int T, int C, double scale, double max_len, int* counts, int* ev_frames, double* ev_seconds,
                        void* stream) {
  const size_t lds = (size_t)T * C * sizeof(float);
  const int threads = (int)((((long)S * C + 63) / 64 > 4 ? 4 : ((long)S * C + 63) / 64) * 64);
  if (lds <= SWEEP_LDS_MAX) {
    if (lds > 64 * 1024) BSED_HIP(bsed_max_lds(g_sweep_lds[WRITE], (const void*)sweep_kernel<WRITE, true>, SWEEP_LDS_MAX));
    hipLaunchKernelGGL((sweep_kernel<WRITE, true>), dim3(B), dim3(threads), lds, (hipStream_t)stream, strong, thresholds,
                       windows, offsets, S, B, T, C, scale, max_len, counts, ev_frames, ev_seconds);
  } else {
    hipLaunchKernelGGL((sweep_kernel<WRITE, false>), dim3(B), dim3(threads), 0, (hipStream_t)stream, strong, thresholds,
                       windows, offsets, S, B, T, C, scale, max_len, counts, ev_frames, ev_seconds);
  }
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

extern "C" int bsed_sweep_count(const float* strong, const float* thresholds, const int* windows, int S, int B, int T, int C,
                                int* counts, void* stream) {
  BSED_CHECK_ARG(strong && thresholds && windows && counts, "bsed_sweep_count: null tensor");
  if (int rc = sweep_geometry("bsed_sweep_count", S, B, T, C)) return rc;
  return sweep_launch<false>(strong, thresholds, windows, nullptr, S, B, T, C, 0.0, 0.0, counts, nullptr, nullptr, stream);
}

extern "C" int bsed_sweep_write(const float* strong, const float* thresholds, const int* windows, const int* offsets, int S,
                                int B, int T, int C, double scale, double max_len, int* ev_frames, double* ev_seconds,
                                void* stream) {
  BSED_CHECK_ARG(strong && thresholds && windows && offsets && ev_frames && ev_seconds, "bsed_sweep_write: null tensor");
  if (int rc = sweep_geometry("bsed_sweep_write", S, B, T, C)) return rc;
  BSED_CHECK_ARG(!isnan(scale) && !isnan(max_len), "bsed_sweep_write: scale and max_len must be numbers");
  return sweep_launch<true>(strong, thresholds, windows, offsets, S, B, T, C, scale, max_len, nullptr, ev_frames, ev_seconds,
                            stream);
}

// ---------------------------------------------------------------------------------------------
// Event matching (sed_eval's event-based metric with its "optimal" matching).  A reference event and an estimated event
// of the same clip and class hit when, in float64 exactly as written,
//   fabs(ref_on - est_on) <= t_collar   and   fabs(ref_off - est_off) <= fmax(t_collar, percentage_of_length * (ref_off - ref_on)).
// No sum follows the one product, so there is nothing a fused multiply-add could contract: the compare sees the same
// bits as a host that rounds the product on its own.
// Ntp of a (threshold, clip, class) problem is the size of a MAXIMUM bipartite matching of the hit graph; Nsys and Nref
// are the list lengths.
//
// One wave per 64 (threshold, class) pairs and BSED_MATCH_CLIPS clips: lane l owns pair blockIdx.x * 64 + l, sums the
// three counts of its problems in registers and adds them to acc (S, C, 3) with three 64-bit integer vector atomics at
// the end.  A problem with an empty side (most of them) is finished by those sums alone.  The others are matched by
// the whole wave, one after the other: lane j holds reference event j (at most BSED_MATCH_MAX_REF = 64 per problem, the
// caller's check), the hit row of an estimated event is ONE ballot (a 64-bit mask), and an augmenting path from each
// estimated event in turn is searched breadth-first over the reference side:
//   matched (lane j)  the estimated event matched to reference j, or -1
//   parent  (lane j)  the reference through whose partner j was reached in this search, or -1 from the root
//   visited, frontier wave-uniform 64-bit masks
// so the whole state is two registers per lane and a few scalars: no stack, no recursion, no LDS, no scratch.  The
// estimated side may be of any length and any order of overlap; its rows are recomputed from the two seconds whenever
// a partner is expanded (at most 64 ballots per estimated event).
// ---------------------------------------------------------------------------------------------
#define BSED_MATCH_CLIPS 8

__device__ __forceinline__ int wave_match(const double* __restrict__ est, int e0, int e1, const double* __restrict__ ref,
                                          int r0, int nr, double collar, double pct, int lane) {
  const bool valid = lane < nr;
  const double ron = valid ? ref[2 * (size_t)(r0 + lane)] : 0.0;
  const double roff = valid ? ref[2 * (size_t)(r0 + lane) + 1] : 0.0;
  const double tol = fmax(collar, pct * (roff - ron));
  auto row = [&](int e) -> unsigned long long {
    const double on = est[2 * (size_t)e], off = est[2 * (size_t)e + 1];
    return __ballot(valid && fabs(ron - on) <= collar && fabs(roff - off) <= tol);
  };
  int matched = -1, parent = -1, ntp = 0;
  for (int e = e0; e < e1; ++e) {
    unsigned long long visited = row(e);
    if (!visited) continue;
    unsigned long long frontier = visited;
    if ((frontier >> lane) & 1) parent = -1;
    int found = -1;
    for (;;) {
      const unsigned long long open = __ballot(matched < 0) & frontier;
      if (open) { found = __ffsll((long long)open) - 1; break; }
      unsigned long long next = 0;
      for (unsigned long long f = frontier; f; f &= f - 1) {
        const int j = __ffsll((long long)f) - 1;
        const unsigned long long fresh = row(__shfl(matched, j)) & ~visited;
        if ((fresh >> lane) & 1) parent = j;
        visited |= fresh;
        next |= fresh;
      }
      if (!next) break;
      frontier = next;
    }
    if (found < 0) continue;
    ++ntp;
    for (int j = found;;) {                           // flip the path back to the root
      const int pj = __shfl(parent, j);
      const int take = __shfl(matched, pj < 0 ? 0 : pj);
      if (lane == j) matched = pj < 0 ? e : take;
      if (pj < 0) break;
      j = pj;
    }
  }
  return ntp;
}

__global__ __launch_bounds__(64) void event_match_kernel(const int* __restrict__ est_offsets, const double* __restrict__ est_seconds,
                                                         const int* __restrict__ ref_offsets, const double* __restrict__ ref_seconds,
                                                         int S, int B, int C, double collar, double pct,
                                                         unsigned long long* __restrict__ acc) {
  const int lane = threadIdx.x;
  const int pair = blockIdx.x * 64 + lane;
  const bool live = pair < S * C;
  const int s = live ? pair / C : 0, c = live ? pair % C : 0;
  const int b0 = blockIdx.y * BSED_MATCH_CLIPS, b1 = min(B, b0 + BSED_MATCH_CLIPS);
  unsigned long long ntp = 0, nsys = 0, nref = 0;
  for (int b = b0; b < b1; ++b) {
    int e0 = 0, e1 = 0, r0 = 0, r1 = 0;
    if (live) {
      const size_t g = ((size_t)s * B + b) * C + c;
      e0 = est_offsets[g]; e1 = est_offsets[g + 1];
      r0 = ref_offsets[b * C + c]; r1 = ref_offsets[b * C + c + 1];
    }
    nsys += (unsigned long long)max(e1 - e0, 0);
    nref += (unsigned long long)max(r1 - r0, 0);
    for (unsigned long long todo = __ballot(e1 > e0 && r1 > r0); todo; todo &= todo - 1) {
      const int k = __ffsll((long long)todo) - 1;
      const int ke0 = __shfl(e0, k), ke1 = __shfl(e1, k), kr0 = __shfl(r0, k), kr1 = __shfl(r1, k);
      const int m = wave_match(est_seconds, ke0, ke1, ref_seconds, kr0, min(kr1 - kr0, BSED_MATCH_MAX_REF), collar, pct, lane);
      if (lane == k) ntp += (unsigned long long)m;
    }
  }
  if (live) {
    unsigned long long* a = acc + 3 * (size_t)pair;   // pair = s * C + c
    if (ntp) atomicAdd(a, ntp);
    if (nsys) atomicAdd(a + 1, nsys);
    if (nref) atomicAdd(a + 2, nref);
  }
}

extern "C" int bsed_event_match(const int* est_offsets, const double* est_seconds, const int* ref_offsets,
                                const double* ref_seconds, int S, int B, int C, double t_collar, double percentage_of_length,
                                long long* acc, void* stream) {
  BSED_CHECK_ARG(est_offsets && est_seconds && ref_offsets && ref_seconds && acc, "bsed_event_match: null tensor");
  BSED_CHECK_ARG(S > 0 && B > 0 && C > 0, "bsed_event_match: bad shape (S=%d, B=%d, C=%d)", S, B, C);
  BSED_CHECK_ARG((long)S * C <= INT_MAX / 4 && (long)B * C < INT_MAX && (long)S * B <= INT_MAX && (long)S * B * C < INT_MAX,
                 "bsed_event_match: S * B * C + 1 offsets must fit int32 (S=%d, B=%d, C=%d)", S, B, C);
  BSED_CHECK_ARG(t_collar >= 0.0 && isfinite(t_collar) && percentage_of_length >= 0.0 && isfinite(percentage_of_length),
                 "bsed_event_match: t_collar and percentage_of_length must be finite and not negative");
  const int gy = ceil_div(B, BSED_MATCH_CLIPS);
  BSED_CHECK_ARG(gy <= 65535, "bsed_event_match: at most %d clips per call (B=%d)", 65535 * BSED_MATCH_CLIPS, B);
  hipLaunchKernelGGL(event_match_kernel, dim3(ceil_div((long)S * C, 64), gy), dim3(64), 0, (hipStream_t)stream, est_offsets,
                     est_seconds, ref_offsets, ref_seconds, S, B, C, t_collar, percentage_of_length,
                     reinterpret_cast<unsigned long long*>(acc));
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
