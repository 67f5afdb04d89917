// The fp32 slab reducers: dst[tap*s_tap + k*s_k + n*s_n] (+)= sum_g part[g][tap][k][n].
//
// The weight-gradient kernels (wgrad.hip and the fused GLU, first-block and head backward kernels) write one partial slab
// per workgroup instead of using float atomics; this file sums the G slabs in a fixed order.  ONE order, whichever
// kernel runs: with S = the slab shares of the reduction (reduce_shares below: the one statement of the split rule),
// share w takes slabs w, w + S, w + 2 S, ...; its i-th slab goes to running sum i mod 4 while four remain, the rest to
// sum 0; the share's value is (s0 + s1) + (s2 + s3); the S shares are added in increasing w.  So an immediate
// (bsed_reduce_partials) and a queued reduction (bsed_reduce_partials_batch, ops.deferred_reductions) give the same
// bits: tests/test_stats_kernels_gpu.py::test_reduce_partials_immediate_and_batched holds them to it.
//
//   reduce_partials_kernel        bsed_reduce_partials, S = 1: one thread per output element
//   reduce_partials_split_kernel  bsed_reduce_partials, S > 1: 64 elements per workgroup of S waves
//   reduce_partials_batch_kernel  bsed_reduce_partials_batch: up to 40 jobs, any S, 16-wave workgroups; the only one
//                                 a train step launches from its queue
// The two immediate kernels stay because they are faster as single launches than the batch kernel with one job
// (its 3.5 KB job table as kernel arguments, half as many workgroups of twice the size).  Measured on one MI355X,
// 5 x 200 back-to-back launches, us per call, immediate kernel / batch kernel of one job: the head's dW
// (rows x 40 x 256) at 96 rows 3.5 / 4.5 and at 512 rows 4.6 / 7.2; 9 x 128 x 64 at G = 9 3.5 / 4.6; 9 x 128 x 128 at
// G = 64 7.9 / 8.3.
//
// The fp64 statistics reducers of BatchNorm (stats_chunk / stats_finish, colsum) are a different contract and live in
// cnn_ops.hip.
#include "bsed_common.h"

__global__ void reduce_partials_kernel(const float* __restrict__ part, int G, int ntaps, int KP, int NP, int K,
                                       int N, float* __restrict__ dst, long s_tap, long s_k, long s_n,
                                       int accumulate) {
  const long total = (long)ntaps * KP * NP;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int n = (int)(e % NP);
    const long r = e / NP;
    const int k = (int)(r % KP), tap = (int)(r / KP);
    if (n >= N || k >= K) continue;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int g = 0;
    for (; g + 4 <= G; g += 4) {
      s0 += part[(size_t)g * total + e];
      s1 += part[(size_t)(g + 1) * total + e];
      s2 += part[(size_t)(g + 2) * total + e];
      s3 += part[(size_t)(g + 3) * total + e];
    }
    for (; g < G; ++g) s0 += part[(size_t)g * total + e];
    const float s = (s0 + s1) + (s2 + s3);
    float* d = dst + tap * s_tap + k * s_k + n * s_n;
    *d = accumulate ? *d + s : s;
  }
}

// Small outputs (a 16x16 or 32x32 dW reduced over ~1000 slabs) starve the kernel above of parallelism: one thread
// per output element walks all G slabs.  Here a workgroup owns 64 consecutive elements and its S waves split the
// slabs (wave w takes g = w, w+S, ...); the S partial sums are combined through LDS in a fixed order (deterministic).
__global__ __launch_bounds__(1024) void reduce_partials_split_kernel(
    const float* __restrict__ part, int G, int ntaps, int KP, int NP, int K, int N, float* __restrict__ dst,
    long s_tap, long s_k, long s_n, int accumulate) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, S = blockDim.x >> 6;
  const long total = (long)ntaps * KP * NP;
  const long e = (long)blockIdx.x * 64 + lane;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (e < total) {
    int g = w;
    for (; g + 7 * S < G; g += 8 * S) {   // eight slabs in flight per lane
      const float a0 = part[(size_t)g * total + e], a1 = part[(size_t)(g + S) * total + e];
      const float a2 = part[(size_t)(g + 2 * S) * total + e], a3 = part[(size_t)(g + 3 * S) * total + e];
      const float a4 = part[(size_t)(g + 4 * S) * total + e], a5 = part[(size_t)(g + 5 * S) * total + e];
      const float a6 = part[(size_t)(g + 6 * S) * total + e], a7 = part[(size_t)(g + 7 * S) * total + e];
      s0 += a0; s1 += a1; s2 += a2; s3 += a3;
      s0 += a4; s1 += a5; s2 += a6; s3 += a7;
    }
    for (; g + 3 * S < G; g += 4 * S) {
      s0 += part[(size_t)g * total + e];
      s1 += part[(size_t)(g + S) * total + e];
      s2 += part[(size_t)(g + 2 * S) * total + e];
      s3 += part[(size_t)(g + 3 * S) * total + e];
    }
    for (; g < G; g += S) s0 += part[(size_t)g * total + e];
  }
  red[w][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (w == 0 && e < total) {
    float s = red[0][lane];
    for (int i = 1; i < S; ++i) s += red[i][lane];
    const int n = (int)(e % NP);
    const long r = e / NP;
    const int k = (int)(r % KP), tap = (int)(r / KP);
    if (n < N && k < K) {
      float* d = dst + tap * s_tap + k * s_k + n * s_n;
      *d = accumulate ? *d + s : s;
    }
  }
}

// Up to BSED_REDUCE_MAX_JOBS partial-slab reductions in ONE launch.  A training step ends ~30 contractions with such a
// reduction (weight gradients, bias gradients), each a 10-12 us launch for microseconds of work: the results are only
// needed by the optimizer (or the gradient all-reduce), so the host queues them and flushes the queue once.  A
// workgroup (16 waves) owns 64 * (16 / S) consecutive elements of one job and its waves split that job's slabs S ways
// (S = 16 for the smallest outputs); partial sums are combined through LDS in a fixed order: deterministic.
struct RpJob {
  const float* part; float* dst;
  int G, KP, NP, K, N, S, accumulate, wg0;   // wg0 = first workgroup of this job
  long total, s_tap, s_k, s_n;
};
struct RpBatch { RpJob j[BSED_REDUCE_MAX_JOBS]; int njobs; };

__global__ __launch_bounds__(1024) void reduce_partials_batch_kernel(const RpBatch Bt) {
  __shared__ float red[16][64];
  int ji = 0;
  for (int k = 1; k < Bt.njobs; ++k)
    if ((int)blockIdx.x >= Bt.j[k].wg0) ji = k;
  const RpJob& J = Bt.j[ji];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, S = J.S;
  const int sub = w / S, ws = w % S;             // 16 / S element groups per workgroup, S slab shares each
  const long total = J.total;
  const long e = ((long)(blockIdx.x - J.wg0) * (16 / S) + sub) * 64 + lane;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (e < total) {
    const float* part = J.part;
    const int G = J.G;
    int g = ws;
    for (; g + 7 * S < G; g += 8 * S) {   // eight slabs in flight per lane
      const float a0 = part[(size_t)g * total + e], a1 = part[(size_t)(g + S) * total + e];
      const float a2 = part[(size_t)(g + 2 * S) * total + e], a3 = part[(size_t)(g + 3 * S) * total + e];
      const float a4 = part[(size_t)(g + 4 * S) * total + e], a5 = part[(size_t)(g + 5 * S) * total + e];
      const float a6 = part[(size_t)(g + 6 * S) * total + e], a7 = part[(size_t)(g + 7 * S) * total + e];
      s0 += a0; s1 += a1; s2 += a2; s3 += a3;
      s0 += a4; s1 += a5; s2 += a6; s3 += a7;
    }
    for (; g + 3 * S < G; g += 4 * S) {   // (same assignment of slabs to the four sums as bsed_reduce_partials:
      s0 += part[(size_t)g * total + e];  //  a queued and an immediate reduction give the same bits)
      s1 += part[(size_t)(g + S) * total + e];
      s2 += part[(size_t)(g + 2 * S) * total + e];
      s3 += part[(size_t)(g + 3 * S) * total + e];
    }
    for (; g < G; g += S) s0 += part[(size_t)g * total + e];
  }
  red[w][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ws == 0 && e < total) {
    float s = red[w][lane];
    for (int i = 1; i < S; ++i) s += red[w + i][lane];
    const int n = (int)(e % J.NP);
    const long r = e / J.NP;
    const int k = (int)(r % J.KP), tap = (int)(r / J.KP);
    if (n < J.N && k < J.K) {
      float* d = J.dst + tap * J.s_tap + k * J.s_k + n * J.s_n;
      *d = J.accumulate ? *d + s : s;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The split rule: too few elements to fill the chip (fewer than 1024 groups of 64) and at least 8 slabs: the slabs are
// split over S waves, doubling S while the groups x S stay below 1024 and every share keeps four slabs.  1 = no split.
static int reduce_shares(long chunks, int G) {
  int S = 1;
  if (chunks < 1024 && G >= 8)
    while (S < 16 && chunks * S < 1024 && 4 * S <= G) S *= 2;
  return S;
}

// The argument check of one reduction (`who` = the entry point, for the message) and what every kernel derives from
// it: the element count and S.  wg0 is the batch entry point's.
static int reduce_job(const char* who, int i, const BsedReduceJob& q, RpJob& J) {
  BSED_CHECK_ARG(q.part && q.dst && q.G > 0 && q.ntaps > 0 && q.KP >= q.K && q.NP >= q.N && q.K > 0 && q.N > 0,
                 "%s: bad argument (job %d)", who, i);
  J.part = q.part; J.dst = q.dst; J.G = q.G; J.KP = q.KP; J.NP = q.NP; J.K = q.K; J.N = q.N;
  J.accumulate = q.accumulate; J.s_tap = q.s_tap; J.s_k = q.s_k; J.s_n = q.s_n;
  J.total = (long)q.ntaps * q.KP * q.NP;
  J.S = reduce_shares(ceil_div(J.total, 64), q.G);
  J.wg0 = 0;
  return BSED_OK;
}

extern "C" int bsed_reduce_partials(const float* part, int G, int ntaps, int KP, int NP, int K, int N, float* dst,
                                    long s_tap, long s_k, long s_n, int accumulate, void* stream) {
  const BsedReduceJob q{part, dst, G, ntaps, KP, NP, K, N, accumulate, s_tap, s_k, s_n};
  RpJob J;
  const int rc = reduce_job("bsed_reduce_partials", 0, q, J);
  if (rc) return rc;
  if (J.S > 1)
    hipLaunchKernelGGL(reduce_partials_split_kernel, dim3((unsigned)ceil_div(J.total, 64)), dim3(64 * J.S), 0,
                       (hipStream_t)stream, part, G, ntaps, KP, NP, K, N, dst, s_tap, s_k, s_n, accumulate);
  else
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)std::min<long>(ceil_div(J.total, 256), 4096)), dim3(256), 0,
                       (hipStream_t)stream, part, G, ntaps, KP, NP, K, N, dst, s_tap, s_k, s_n, accumulate);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

extern "C" int bsed_reduce_partials_batch(const BsedReduceJob* jobs, int njobs, void* stream) {
  BSED_CHECK_ARG(jobs && njobs > 0 && njobs <= BSED_REDUCE_MAX_JOBS, "bsed_reduce_partials_batch: 1..%d jobs",
                 BSED_REDUCE_MAX_JOBS);
  RpBatch Bt;
  Bt.njobs = njobs;
  long wg = 0;
  for (int i = 0; i < njobs; ++i) {
    RpJob& J = Bt.j[i];
    const int rc = reduce_job("bsed_reduce_partials_batch", i, jobs[i], J);
    if (rc) return rc;
    for (int k = 0; k < i; ++k)
      BSED_CHECK_ARG(jobs[k].dst != jobs[i].dst, "bsed_reduce_partials_batch: jobs %d and %d write the same destination "
                     "(flush between them)", k, i);
    J.wg0 = (int)wg;
    wg += ceil_div(ceil_div(J.total, 64), 16 / J.S);
    BSED_CHECK_ARG(wg < (1L << 31), "bsed_reduce_partials_batch: too many workgroups");
  }
  hipLaunchKernelGGL(reduce_partials_batch_kernel, dim3((unsigned)wg), dim3(1024), 0, (hipStream_t)stream, Bt);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
