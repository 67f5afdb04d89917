// The domain classifier (bsed_svc_d2 / bsed_svc_solve / bsed_svc_decision, ABI 20): an RBF C-SVC by libsvm's rules on
// the dense squared distances of an embedding; svc.py runs the cross-validation of src/visualize.py on it.  The rules
// -- the kernel values, the working-set selection and its ties, the pair update, rho, what a bad problem leaves behind
// -- are stated in include/bsed.h.  No atomics, no fence, no waiting on another workgroup.
//   d2_tile_kernel        (d2_tile.h, shared with tsne.hip; its loop also with pair_stats.hip) the squared distances.
//   svc_solve_kernel      one workgroup of 256 threads (four waves) per problem; thread r owns the positions r, r + 256,
//                         ...  An iteration is two scans and one update of the owned positions with three barriers:
//                           scan 1   -y G over I_up and y G over I_low -> one workgroup arg-max (Gmax, i, Gmax2);
//                           scan 2   row i of K on the fly -> the arg-max of b^2 / a (the arg-min of -b^2 / a): j;
//                           update   every thread forms the new alpha_i, alpha_j from the same values; barrier; rows i
//                                    and j of K on the fly -> G of the owned positions; the owners of i and j store alpha.
//                         A workgroup arg-max is a shuffle tree inside each wave (ties to the smaller position), one LDS
//                         slot per wave, ONE barrier, then every thread folds the four slots in wave order; the slots
//                         alternate between two sets, so the next reduction never overwrites what a slow wave still
//                         reads.  The kernel is latency bound (at n = 1600 a thread owns 6 or 7 positions); the rows of
//                         d2 it gathers from come out of the L2.
//                         LDS = true: alpha, G and the packed (index, label) of every position in dynamic LDS (20 bytes
//                         a point); false: alpha in its output, G and the packed words in the workspace.
//   svc_decision_kernel   one wavefront per test entry: 64 strided partial sums, one xor tree.
#include "../../include/bsed.h"
#include "bsed_common.h"
#include "d2_tile.h"
#include <limits.h>
#include <math.h>

#define SVC_THREADS 256
#define SVC_WAVES (SVC_THREADS / 64)
#define SVC_TAU 1e-12
#define SVC_NONE INT_MAX                 // the position of "no candidate"
#define SVC_BYTES_PER_POINT 20           // alpha, G, the packed word

struct SvcGammas { float g[BSED_SVC_MAX_PROBLEMS]; };

// the slots of the workgroup arg-max: two sets used in turn
struct SvcSlots {
  double v[2][SVC_WAVES];
  double w[2][SVC_WAVES];
  int t[2][SVC_WAVES];
};

// (v, t) <- the largest v of the workgroup and its position, the smallest position on a tie (SVC_NONE when every v is
// -infinity);  w <- the largest w.  The same values in every thread.  One barrier.
__device__ __forceinline__ void svc_argmax(double& v, int& t, double& w, SvcSlots& slots, int& set) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64), ow = __shfl_xor(w, o, 64);
    const int ot = __shfl_xor(t, o, 64);
    if (ov > v || (ov == v && ot < t)) { v = ov; t = ot; }
    if (ow > w) w = ow;
  }
  if ((threadIdx.x & 63) == 0) {
    const int wave = threadIdx.x >> 6;
    slots.v[set][wave] = v; slots.w[set][wave] = w; slots.t[set][wave] = t;
  }
  __syncthreads();
  v = slots.v[set][0]; t = slots.t[set][0]; w = slots.w[set][0];
#pragma unroll
  for (int k = 1; k < SVC_WAVES; ++k) {
    const double ov = slots.v[set][k], ow = slots.w[set][k];
    const int ot = slots.t[set][k];
    if (ov > v || (ov == v && ot < t)) { v = ov; t = ot; }
    if (ow > w) w = ow;
  }
  set ^= 1;
}

enum { SVC_SUM, SVC_MIN, SVC_MAX };
// the sum / minimum / maximum of v over the workgroup, the same value in every thread: a fixed tree inside each wave,
// then the waves in order.  Two barriers (used after the loop only)
template <int OP>
__device__ __forceinline__ double svc_fold(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_xor(v, o, 64);
    v = OP == SVC_SUM ? v + u : (OP == SVC_MIN ? fmin(v, u) : fmax(v, u));
  }
  __syncthreads();                                                  // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int k = 1; k < SVC_WAVES; ++k) s = OP == SVC_SUM ? s + red[k] : (OP == SVC_MIN ? fmin(s, red[k]) : fmax(s, red[k]));
  return s;
}

__device__ __forceinline__ double svc_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// K of two global points, as include/bsed.h defines it
__device__ __forceinline__ float svc_k(const float* __restrict__ d2row, int g, float gamma) {
  return expf(-(gamma * d2row[g]));
}

template <bool LDS>
__global__ __launch_bounds__(SVC_THREADS) void svc_solve_kernel(
    const float* __restrict__ d2, int N, const int* __restrict__ y, const int* __restrict__ train_offsets,
    const int* __restrict__ train_index, int total_train, int max_train, SvcGammas gammas, double C, double tol,
    int max_iter, double* __restrict__ alpha, double* __restrict__ rho, double* __restrict__ gap, int* __restrict__ info,
    double* __restrict__ ws_G, int* __restrict__ ws_code) {
  extern __shared__ __attribute__((aligned(16))) unsigned char svc_lds[];
  __shared__ SvcSlots slots;
  __shared__ double red[SVC_WAVES];
  const int tid = threadIdx.x, p = blockIdx.x;
  const int begin = train_offsets[p], end = train_offsets[p + 1];
  // uniform: every thread read the same two offsets
  if (begin < 0 || end < begin || end > total_train || end - begin > max_train) {
    if (tid == 0) { info[2 * p] = 0; info[2 * p + 1] = BSED_SVC_BAD_OFFSETS; rho[p] = svc_nan(); }
    return;
  }
  const int n = end - begin;
  // the checks, before anything is written: an index is an address only once it lies in [0, N)
  int bad_index = 0, bad_label = 0, has_pos = 0, has_neg = 0;
  for (int t = tid; t < n; t += SVC_THREADS) {
    const int g = train_index[begin + t];
    if (g < 0 || g >= N) { bad_index = 1; continue; }
    const int l = y[g];
    if (l == 1) has_pos = 1;
    else if (l == -1) has_neg = 1;
    else bad_label = 1;
  }
  bad_index = __syncthreads_or(bad_index);
  bad_label = __syncthreads_or(bad_label);
  has_pos = __syncthreads_or(has_pos);
  has_neg = __syncthreads_or(has_neg);
  if (bad_index || bad_label || !has_pos || !has_neg) {
    if (tid == 0) {
      info[2 * p] = 0;
      info[2 * p + 1] = bad_index ? BSED_SVC_BAD_INDEX : (bad_label ? BSED_SVC_BAD_LABEL : BSED_SVC_ONE_CLASS);
      rho[p] = svc_nan();
    }
    return;
  }
  double* G;
  double* A;
  int* code;                                                        // 2 * global index + (label == +1)
  if (LDS) {
    G = reinterpret_cast<double*>(svc_lds);
    A = G + max_train;
    code = reinterpret_cast<int*>(A + max_train);
  } else {
    G = ws_G + begin;
    A = alpha + begin;
    code = ws_code + begin;
  }
  for (int t = tid; t < n; t += SVC_THREADS) {
    const int g = train_index[begin + t];
    code[t] = 2 * g + (y[g] == 1 ? 1 : 0);
    A[t] = 0.0;
    G[t] = -1.0;
  }
  __syncthreads();
  const float gamma = gammas.g[p];
  int iter = 0, status = BSED_SVC_CONVERGED, set = 0;
  double last_gap;
  for (;;) {
    // scan 1: i, Gmax, Gmax2
    double bv = -INFINITY, bw = -INFINITY;
    int bt = SVC_NONE;
    for (int t = tid; t < n; t += SVC_THREADS) {
      const double a = A[t], g = G[t];
      const bool pos = code[t] & 1, at_upper = a >= C, at_lower = a <= 0.0;
      const double v = pos ? -g : g;                                // -y G
      if ((pos ? !at_upper : !at_lower) && v > bv) { bv = v; bt = t; }
      if ((pos ? !at_lower : !at_upper) && -v > bw) bw = -v;
    }
    svc_argmax(bv, bt, bw, slots, set);
    last_gap = bv + bw;
    if (!(last_gap >= tol) || bt == SVC_NONE) break;                // uniform: every thread holds the same values
    if (iter == max_iter) { status = BSED_SVC_NOT_CONVERGED; break; }
    const int i = bt, ci = code[i];
    const double gmax = bv;
    const float* __restrict__ row_i = d2 + (size_t)(ci >> 1) * N;
    // scan 2: j maximises b^2 / a, which is the arg-min of -b^2 / a with the same ties
    double ov = -INFINITY, unused = -INFINITY;
    int ot = SVC_NONE;
    for (int t = tid; t < n; t += SVC_THREADS) {
      const double a = A[t], g = G[t];
      const int c = code[t];
      const bool pos = c & 1;
      if (pos ? a <= 0.0 : a >= C) continue;                        // not in I_low
      const double b = gmax + (pos ? g : -g);
      if (!(b > 0.0)) continue;
      double q = 2.0 - 2.0 * (double)svc_k(row_i, c >> 1, gamma);
      if (!(q > 0.0)) q = SVC_TAU;
      const double o = (b * b) / q;
      if (o > ov) { ov = o; ot = t; }
    }
    svc_argmax(ov, ot, unused, slots, set);
    if (ot == SVC_NONE) break;                                      // only with non-finite values: nothing to step along
    // the pair update, formed by every thread from the same values
    const int j = ot, cj = code[j];
    const double Gi = G[i], Gj = G[j], old_i = A[i], old_j = A[j];
    double quad = 2.0 - 2.0 * (double)svc_k(row_i, cj >> 1, gamma);
    if (!(quad > 0.0)) quad = SVC_TAU;
    double ai = old_i, aj = old_j;
    if ((ci ^ cj) & 1) {                                            // y_i != y_j
      const double delta = (-Gi - Gj) / quad, diff = ai - aj;
      ai += delta;
      aj += delta;
      if (diff > 0.0) {
        if (aj < 0.0) { aj = 0.0; ai = diff; }
      } else if (ai < 0.0) { ai = 0.0; aj = -diff; }
      if (diff > 0.0) {                                             // C_i - C_j = 0
        if (ai > C) { ai = C; aj = C - diff; }
      } else if (aj > C) { aj = C; ai = C + diff; }
    } else {
      const double delta = (Gi - Gj) / quad, sum = ai + aj;
      ai -= delta;
      aj += delta;
      if (sum > C) {
        if (ai > C) { ai = C; aj = sum - C; }
      } else if (aj < 0.0) { aj = 0.0; ai = sum; }
      if (sum > C) {
        if (aj > C) { aj = C; ai = sum - C; }
      } else if (ai < 0.0) { ai = 0.0; aj = sum; }
    }
    const double yi = (ci & 1) ? 1.0 : -1.0, yj = (cj & 1) ? 1.0 : -1.0;
    const double dai = yi * (ai - old_i), daj = yj * (aj - old_j);   // times y_i, y_j: exact
    const float* __restrict__ row_j = d2 + (size_t)(cj >> 1) * N;
    __syncthreads();                                                // every thread has read G and alpha of i and j
    for (int t = tid; t < n; t += SVC_THREADS) {
      const int c = code[t];
      const double ki = (double)svc_k(row_i, c >> 1, gamma), kj = (double)svc_k(row_j, c >> 1, gamma);
      const double step = ki * dai + kj * daj;
      G[t] += (c & 1) ? step : -step;
      if (t == i) A[t] = ai;
      else if (t == j) A[t] = aj;
    }
    ++iter;
  }
  // rho (calculate_rho) and the outputs; every thread reads only the positions it owns
  double ub = INFINITY, lb = -INFINITY, sum_free = 0.0, n_free = 0.0;
  for (int t = tid; t < n; t += SVC_THREADS) {
    const double a = A[t], g = G[t];
    const bool pos = code[t] & 1;
    const double yg = pos ? g : -g;
    if (a >= C) {
      if (pos) lb = fmax(lb, yg); else ub = fmin(ub, yg);
    } else if (a <= 0.0) {
      if (pos) ub = fmin(ub, yg); else lb = fmax(lb, yg);
    } else {
      sum_free += yg;
      n_free += 1.0;
    }
    if (LDS) alpha[begin + t] = a;
  }
  ub = svc_fold<SVC_MIN>(ub, red);
  lb = svc_fold<SVC_MAX>(lb, red);
  sum_free = svc_fold<SVC_SUM>(sum_free, red);
  n_free = svc_fold<SVC_SUM>(n_free, red);
  if (tid == 0) {
    rho[p] = n_free > 0.0 ? sum_free / n_free : (ub + lb) / 2.0;
    gap[p] = last_gap;
    info[2 * p] = iter;
    info[2 * p + 1] = status;
  }
}

__global__ __launch_bounds__(64) void svc_decision_kernel(
    const float* __restrict__ d2, int N, const int* __restrict__ y, const int* __restrict__ train_offsets,
    const int* __restrict__ train_index, const int* __restrict__ test_offsets, const int* __restrict__ test_index, int P,
    int total_train, SvcGammas gammas, const double* __restrict__ alpha, const double* __restrict__ rho,
    const int* __restrict__ info, double* __restrict__ dec) {
  const int e = blockIdx.x, lane = threadIdx.x;
  int p = -1;
  for (int q = 0; q < P && p < 0; ++q)
    if (e >= test_offsets[q] && e < test_offsets[q + 1]) p = q;
  bool ok = p >= 0;
  int begin = 0, end = 0, ti = 0;
  if (ok) {
    const int status = info[2 * p + 1];
    begin = train_offsets[p];
    end = train_offsets[p + 1];
    ti = test_index[e];
    ok = (status == BSED_SVC_CONVERGED || status == BSED_SVC_NOT_CONVERGED) && begin >= 0 && end >= begin &&
         end <= total_train && ti >= 0 && ti < N;
  }
  if (!ok) {                                                        // uniform
    if (lane == 0) dec[e] = svc_nan();
    return;
  }
  const float gamma = gammas.g[p];
  const float* __restrict__ row = d2 + (size_t)ti * N;
  double s = 0.0;
  int bad = 0;
  for (int k = begin + lane; k < end; k += 64) {
    const int g = train_index[k];
    if (g < 0 || g >= N) { bad = 1; continue; }
    const double a = alpha[k];
    if (a != 0.0) s += a * (double)y[g] * (double)svc_k(row, g, gamma);   // a zero alpha adds an exact zero: skipped
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    bad |= __shfl_xor(bad, o, 64);
  }
  if (lane == 0) dec[e] = bad ? svc_nan() : s - rho[p];
}

// ---------------------------------------------------------------------------------------------- entry points
static bool svc_positive_finite(double v) { return v > 0.0 && v < INFINITY; }

extern "C" int bsed_svc_d2(const float* x, long long x_pitch, int N, int D, float* d2, void* stream) {
  const char* who = "bsed_svc_d2";
  BSED_CHECK_ARG(x && d2, "%s: null pointer", who);
  BSED_CHECK_ARG(N >= 1 && N <= BSED_SVC_MAX_POINTS, "%s: 1 to %d points, got N=%d", who, BSED_SVC_MAX_POINTS, N);
  BSED_CHECK_ARG(D >= 1, "%s: D must be at least 1, got %d", who, D);
  BSED_CHECK_ARG(x_pitch >= (long long)D, "%s: x_pitch=%lld is below D=%d", who, x_pitch, D);
  BSED_CHECK_ARG(((uintptr_t)x % 4) == 0 && ((uintptr_t)d2 % 4) == 0, "%s: x and d2 must be 4-byte aligned", who);
  d2_launch(x, x_pitch, N, D, d2, (hipStream_t)stream);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

extern "C" size_t bsed_svc_solve_workspace(int P, int total_train) {
  if (P < 1 || P > BSED_SVC_MAX_PROBLEMS || total_train < 1 || (long long)total_train > (long long)P * BSED_SVC_MAX_POINTS)
    return 0;
  // G, then the packed words, rounded up to a multiple of 8 bytes
  return (size_t)total_train * sizeof(double) + (((size_t)total_train + 1) / 2) * 2 * sizeof(int);
}

// the checks bsed_svc_solve and bsed_svc_decision share; fills the by-value copy of gamma
static int svc_common_args(const char* who, const float* d2, int N, const int* y, const int* train_offsets,
                           const int* train_index, int P, int total_train, const float* gamma, SvcGammas& gammas) {
  BSED_CHECK_ARG(d2 && y && train_offsets && train_index && gamma, "%s: null pointer", who);
  BSED_CHECK_ARG(N >= 2 && N <= BSED_SVC_MAX_POINTS, "%s: 2 to %d points, got N=%d", who, BSED_SVC_MAX_POINTS, N);
  BSED_CHECK_ARG(P >= 1 && P <= BSED_SVC_MAX_PROBLEMS, "%s: 1 to %d problems, got P=%d", who, BSED_SVC_MAX_PROBLEMS, P);
  BSED_CHECK_ARG(total_train >= 1 && (long long)total_train <= (long long)P * BSED_SVC_MAX_POINTS,
                 "%s: total_train must lie in 1..P * %d, got %d", who, BSED_SVC_MAX_POINTS, total_train);
  BSED_CHECK_ARG(((uintptr_t)d2 % 4) == 0 && ((uintptr_t)y % 4) == 0 && ((uintptr_t)train_offsets % 4) == 0 &&
                 ((uintptr_t)train_index % 4) == 0 && ((uintptr_t)gamma % 4) == 0,
                 "%s: d2, y, the offsets, the indices and gamma must be 4-byte aligned", who);
  for (int p = 0; p < P; ++p) {
    BSED_CHECK_ARG(svc_positive_finite((double)gamma[p]), "%s: gamma[%d] must be positive and finite, got %g", who, p,
                   (double)gamma[p]);
    gammas.g[p] = gamma[p];
  }
  for (int p = P; p < BSED_SVC_MAX_PROBLEMS; ++p) gammas.g[p] = 0.f;
  return BSED_OK;
}

extern "C" int bsed_svc_solve(const float* d2, int N, const int* y, const int* train_offsets, const int* train_index,
                              int P, int total_train, int max_train, const float* gamma, double C, double tol,
                              int max_iter, double* alpha, double* rho, double* gap, int* info, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const char* who = "bsed_svc_solve";
  SvcGammas gammas;
  BSED_CHECK_ARG(alpha && rho && gap && info && workspace, "%s: null pointer", who);
  const int rc = svc_common_args(who, d2, N, y, train_offsets, train_index, P, total_train, gamma, gammas);
  if (rc) return rc;
  BSED_CHECK_ARG(max_train >= 1 && max_train <= BSED_SVC_MAX_POINTS, "%s: max_train must lie in 1..%d, got %d", who,
                 BSED_SVC_MAX_POINTS, max_train);
  BSED_CHECK_ARG(svc_positive_finite(C) && svc_positive_finite(tol),
                 "%s: C and tol must be positive and finite, got %g and %g", who, C, tol);
  BSED_CHECK_ARG(max_iter >= 1 && max_iter <= BSED_SVC_MAX_ITER, "%s: max_iter must lie in 1..%d, got %d", who,
                 BSED_SVC_MAX_ITER, max_iter);
  BSED_CHECK_ARG(((uintptr_t)info % 4) == 0 && ((uintptr_t)alpha % 8) == 0 && ((uintptr_t)rho % 8) == 0 &&
                 ((uintptr_t)gap % 8) == 0 && ((uintptr_t)workspace % 8) == 0,
                 "%s: info must be 4-byte aligned, alpha, rho, gap and the workspace 8-byte aligned", who);
  const size_t need = bsed_svc_solve_workspace(P, total_train);
  BSED_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %zu bytes, %zu are needed (P=%d, total_train=%d)", who,
                 workspace_bytes, need, P, total_train);
  hipStream_t s = (hipStream_t)stream;
  double* ws_G = (double*)workspace;
  int* ws_code = (int*)(ws_G + total_train);
  if (max_train <= BSED_SVC_LDS_POINTS) {
    static BsedLdsOnce once;
    BSED_HIP(bsed_max_lds(once, (const void*)svc_solve_kernel<true>, BSED_SVC_LDS_POINTS * SVC_BYTES_PER_POINT));
    hipLaunchKernelGGL(svc_solve_kernel<true>, dim3(P), dim3(SVC_THREADS), (size_t)max_train * SVC_BYTES_PER_POINT, s, d2,
                       N, y, train_offsets, train_index, total_train, max_train, gammas, C, tol, max_iter, alpha, rho, gap,
                       info, ws_G, ws_code);
  } else {
    hipLaunchKernelGGL(svc_solve_kernel<false>, dim3(P), dim3(SVC_THREADS), 0, s, d2, N, y, train_offsets, train_index,
                       total_train, max_train, gammas, C, tol, max_iter, alpha, rho, gap, info, ws_G, ws_code);
  }
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

extern "C" int bsed_svc_decision(const float* d2, int N, const int* y, const int* train_offsets, const int* train_index,
                                 const int* test_offsets, const int* test_index, int P, int total_train, int total_test,
                                 const float* gamma, const double* alpha, const double* rho, const int* info, double* dec,
                                 void* stream) {
  const char* who = "bsed_svc_decision";
  SvcGammas gammas;
  BSED_CHECK_ARG(test_offsets && test_index && alpha && rho && info && dec, "%s: null pointer", who);
  const int rc = svc_common_args(who, d2, N, y, train_offsets, train_index, P, total_train, gamma, gammas);
  if (rc) return rc;
  BSED_CHECK_ARG(total_test >= 1 && (long long)total_test <= (long long)P * BSED_SVC_MAX_POINTS,
                 "%s: total_test must lie in 1..P * %d, got %d", who, BSED_SVC_MAX_POINTS, total_test);
  BSED_CHECK_ARG(((uintptr_t)test_offsets % 4) == 0 && ((uintptr_t)test_index % 4) == 0 && ((uintptr_t)info % 4) == 0 &&
                 ((uintptr_t)alpha % 8) == 0 && ((uintptr_t)rho % 8) == 0 && ((uintptr_t)dec % 8) == 0,
                 "%s: the test offsets, the test indices and info must be 4-byte aligned, alpha, rho and dec 8-byte aligned",
                 who);
  hipLaunchKernelGGL(svc_decision_kernel, dim3(total_test), dim3(64), 0, (hipStream_t)stream, d2, N, y, train_offsets,
                     train_index, test_offsets, test_index, P, total_train, gammas, alpha, rho, info, dec);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
