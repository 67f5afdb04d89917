// Integrated loudness (ITU-R BS.1770-4, mono) of S segments of one flat fp32 buffer; include/bsed.h states the rules.
//
// The K-weighting is a 4th-order recurrence, serial in the sample index.  Parallelism comes from the segments and from
// two splits of one segment:
//
//   chunks (across workgroups, WARM-UP): a workgroup owns HC consecutive 100 ms hops of ONE segment and writes
//     their sums of y^2 with plain stores: every hop has one owner, so there are no partial sums and no atomics.  It
//     starts the recurrence W samples before its first hop from zero state.  W = ceil(50 / -ln r), r the largest pole
//     radius of the two biquads at this rate (the double pole of the high-pass: 0.21 s at every rate), so what the zero
//     start leaves behind, at most about W * r^W = W * e^-50 of the input's size, is below one unit in the last place of
//     a double: even a DC offset 2^24 times the signal -- the most a float32 input can hold -- does not reach the 1e-6 LU
//     bar.  A chunk that starts inside the first W samples starts at sample 0 with the rule's own zero state.
//   pieces (across the lanes of a workgroup, EXACT): the chunk is walked in tiles of 256 pieces of 32 samples.  A tile is
//     staged in LDS with 16-byte loads (segment offsets are arbitrary: dword-aligned 16-byte loads, as in synth.hip; all
//     of a tile's loads before its first LDS store where the tile lies inside the segment and the buffer) at m + m / 32, so that the lanes, each reading its own piece, fall on distinct banks.  Pass 1: every lane filters its
//     piece from zero output state (with the true two preceding inputs) and keeps the 4-value end state (p[-1], p[-2],
//     q[-1], q[-2]: the outputs of the two stages).  The state obeys s_end = M s_in + v with M = A^32, A the zero-input
//     step, the same for every lane: a Hillis-Steele scan over the 256 lanes with the host's M^(2^j), j = 0..7 (eight
//     steps through LDS, one barrier each), seeded with the state the previous tile ended in, gives every lane its
//     true s_in.  Pass 2 filters again from it and sums y^2, split at the one hop boundary a piece can contain (a hop is
//     at least 336 samples).  The last lane's end state of pass 2 carries into the next tile.
//
// Hop sums: per wave and hop a fixed xor-butterfly over the lanes, added by the wave's lane 0 to the wave's own LDS
// accumulator; at the end the four waves' accumulators are added in wave order.  Every sum has a fixed order: two
// launches give the same bits.  The second kernel forms the blocks of a segment from four hop sums and applies the two
// gates, one segment per wave.
#include "../../include/bsed.h"
#include "bsed_common.h"
#include <math.h>

#define LD_THREADS 256
#define LD_P 32                                  // samples of a piece
#define LD_TILE (LD_THREADS * LD_P)              // samples of a tile: 8192
#define LD_PRE 4                                 // samples staged in front of a tile (two are read: v[-1], v[-2])
#define LD_XS (LD_TILE + LD_PRE + (LD_TILE + LD_PRE) / 32 + 1)
#define LD_MAX_HC 32                             // most hops of a chunk
#define LD_MIN_SR 3364                           // the shelf's centre (1681.97 Hz) must lie below sr / 2
#define LD_GATE_THREADS 256                     // four segments of a workgroup, one per wave

static const double LD_SHELF_F0 = 1681.974450955533, LD_SHELF_G = 3.999843853973347, LD_SHELF_Q = 0.7071752369554196;
static const double LD_SHELF_VB_EXP = 0.4996667741545416;
static const double LD_HP_F0 = 38.13547087602444, LD_HP_Q = 0.5003270373238773;
static const double LD_PI = 3.141592653589793238462643383279502884;

struct LdParams {
  double b0, b1, b2, a1, a2;                     // stage 1 (shelf)
  double c1, c2;                                 // stage 2 (high-pass): b = 1, -2, 1; a1, a2
  double M[8][16];                               // (A^32)^(2^j), row-major, state order p1, p2, q1, q2
};

typedef float ld_f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// effective length of a segment: whole repetitions of a short one up to at least half a second
__device__ __host__ __forceinline__ long ld_n_eff(long len, int half) {
  return len >= half ? len : len * ((half + len - 1) / len);
}
// number of whole hops in n samples: the largest m with (m * sr) / 10 <= n
__device__ __host__ __forceinline__ long ld_whole_hops(long n, int sr) { return (10 * (n + 1) - 1) / sr; }

// sample i of the segment's signal (0 for i < 0): x[off + i % len], 0 outside the buffer
__device__ __forceinline__ float ld_sample(const float* __restrict__ x, long x_len, long off, long len, bool tiled, long i) {
  if (i < 0) return 0.f;
  const long pos = (long)((unsigned long)off + (unsigned long)(tiled ? i % len : i));
  return (pos >= 0 && pos < x_len) ? x[pos] : 0.f;
}

__device__ __forceinline__ int ld_addr(int m) { return m + (m >> 5); }

// s += Mj * w
__device__ __forceinline__ void ld_matvec_add(const double* __restrict__ Mj, const double* w, double* s) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    s[r] = fma(Mj[4 * r + 3], w[3], fma(Mj[4 * r + 2], w[2], fma(Mj[4 * r + 1], w[1], fma(Mj[4 * r], w[0], s[r]))));
}

// n samples of a piece through both stages from the state (p1, p2, q1, q2), v1 / v2 the two inputs before it; with ENERGY,
// y^2 of the samples before `bnd` is added to eA and of the others to eB.  Called with the constant LD_P for a whole piece
// (the common case: the loop unrolls and the LDS reads run ahead of the recurrence) and with the count for a ragged one.
template <bool ENERGY>
__device__ __forceinline__ void ld_filter(const float* xp, int m0, int n, const LdParams& prm, double v1, double v2, double& p1,
                                          double& p2, double& q1, double& q2, int bnd, double& eA, double& eB) {
#pragma unroll 8
  for (int j = 0; j < n; ++j) {
    const double v = (double)xp[ld_addr(m0 + j)];
    const double p = fma(-prm.a1, p1, fma(-prm.a2, p2, fma(prm.b2, v2, fma(prm.b1, v1, prm.b0 * v))));
    const double q = fma(-prm.c1, q1, fma(-prm.c2, q2, fma(-2.0, p1, p + p2)));
    v2 = v1; v1 = v; p2 = p1; p1 = p; q2 = q1; q1 = q;
    if (ENERGY) {
      const bool first = j < bnd;
      eA = fma(q, first ? q : 0.0, eA);
      eB = fma(q, first ? 0.0 : q, eB);
    }
  }
}

__global__ void __launch_bounds__(LD_THREADS) loudness_hops_kernel(const float* __restrict__ x, long x_len,
                                                                    const long* __restrict__ seg_off,
                                                                    const long* __restrict__ seg_len, long max_len, int sr,
                                                                    int half, long W, int HC, int nch, long Hmax,
                                                                    const LdParams prm, double* __restrict__ hops) {
  __shared__ float xs[LD_XS];
  __shared__ double sbuf[2][4][LD_THREADS];
  __shared__ double wacc[LD_THREADS / 64][LD_MAX_HC];
  __shared__ double carry[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long seg = blockIdx.x / nch;
  long len = seg_len[seg];
  if (len < 1) return;
  len = min(len, max_len);
  const long n_eff = ld_n_eff(len, half);
  const bool tiled = len < n_eff;
  const long Hn = ld_whole_hops(n_eff, sr);
  const long h0 = (long)(blockIdx.x % nch) * HC;
  if (Hn < 4 || h0 >= Hn) return;                // no block, or no hop of this chunk (the same for the whole workgroup)
  const long h1 = min(h0 + HC, Hn);
  const long off = seg_off[seg];
  const long lo = (h0 * sr) / 10, hi = (h1 * sr) / 10;
  const long start = max(0L, lo - W);

  if (tid < (LD_THREADS / 64) * LD_MAX_HC) (&wacc[0][0])[tid] = 0.0;
  if (tid < 4) carry[tid] = 0.0;

  for (long ts = start; ts < hi; ts += LD_TILE) {
    __syncthreads();                             // the previous tile's reads of xs and sbuf, and its carry
    // a tile inside an untiled segment and inside the buffer (most are): every load is issued before the first LDS store, so
    // the tile pays one memory latency, not one per 1024 samples
    const long pbase = (long)((unsigned long)off + (unsigned long)(ts - LD_PRE));
    const bool interior = !tiled && ts >= LD_PRE && pbase >= 0 && pbase <= x_len - (LD_TILE + LD_PRE);
    if (interior) {
      ld_f32x4u t[LD_TILE / 4 / LD_THREADS], tl;
#pragma unroll
      for (int k = 0; k < LD_TILE / 4 / LD_THREADS; ++k)
        t[k] = *reinterpret_cast<const ld_f32x4u*>(x + pbase + 4 * (tid + k * LD_THREADS));
      if (tid == 0) tl = *reinterpret_cast<const ld_f32x4u*>(x + pbase + LD_TILE);
#pragma unroll
      for (int k = 0; k < LD_TILE / 4 / LD_THREADS; ++k) {
        const int a = ld_addr(4 * (tid + k * LD_THREADS));
#pragma unroll
        for (int e = 0; e < 4; ++e) xs[a + e] = t[k][e];
      }
      if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) xs[ld_addr(LD_TILE) + e] = tl[e];
      }
    } else
    for (int q = tid; q < (LD_TILE + LD_PRE) / 4; q += LD_THREADS) {
      const long i0 = ts - LD_PRE + 4 * q;
      const long p0 = (long)((unsigned long)off + (unsigned long)i0);
      float v[4];
      if (!tiled && i0 >= 0 && p0 >= 0 && p0 <= x_len - 4) {
        const ld_f32x4u t = *reinterpret_cast<const ld_f32x4u*>(x + p0);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (i0 + e < hi) ? ld_sample(x, x_len, off, len, tiled, i0 + e) : 0.f;
      }
      const int a = ld_addr(4 * q);              // 4 * q .. 4 * q + 3 lie in one group of 32
#pragma unroll
      for (int e = 0; e < 4; ++e) xs[a + e] = v[e];
    }
    __syncthreads();

    const long is = ts + (long)tid * LD_P;       // first sample of the lane's piece
    const int cnt = (int)max(0L, min((long)LD_P, hi - is));
    const int m0 = LD_PRE + tid * LD_P;
    const double vm1 = (double)xs[ld_addr(m0 - 1)], vm2 = (double)xs[ld_addr(m0 - 2)];

    // pass 1: zero output state -> v = the state after the piece
    double s[4] = {0.0, 0.0, 0.0, 0.0}, eA = 0.0, eB = 0.0;
    if (cnt == LD_P) ld_filter<false>(xs, m0, LD_P, prm, vm1, vm2, s[0], s[1], s[2], s[3], 0, eA, eB);
    else ld_filter<false>(xs, m0, cnt, prm, vm1, vm2, s[0], s[1], s[2], s[3], 0, eA, eB);
    if (tid == 0) {                              // the state the previous tile ended in enters through lane 0
      const double c[4] = {carry[0], carry[1], carry[2], carry[3]};
      ld_matvec_add(prm.M[0], c, s);
    }
    // inclusive scan of s_t <- M s_(t-1) + s_t over the 256 lanes (Hillis-Steele: after step j, s_t holds the pieces
    // t - 2^(j+1) + 1 .. t).  The two halves of sbuf alternate, so a step needs one barrier: what a step overwrites was
    // last read before the previous step's barrier.
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = 1 << j;
#pragma unroll
      for (int r = 0; r < 4; ++r) sbuf[j & 1][r][tid] = s[r];
      __syncthreads();
      if (tid >= d) {
        double w[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = sbuf[j & 1][r][tid - d];
        ld_matvec_add(prm.M[j], w, s);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) sbuf[0][r][tid] = s[r];
    const double c_in[4] = {carry[0], carry[1], carry[2], carry[3]};
    __syncthreads();
    double p1, p2, q1, q2;
    if (tid == 0) { p1 = c_in[0]; p2 = c_in[1]; q1 = c_in[2]; q2 = c_in[3]; }
    else { p1 = sbuf[0][0][tid - 1]; p2 = sbuf[0][1][tid - 1]; q1 = sbuf[0][2][tid - 1]; q2 = sbuf[0][3][tid - 1]; }

    // pass 2: from the true state; y^2 summed per hop (the piece holds at most one hop boundary)
    const long hA = ld_whole_hops(is, sr);       // the hop of sample `is`
    const int bnd = (int)min((long)LD_P, ((hA + 1) * sr) / 10 - is);
    if (cnt == LD_P) ld_filter<true>(xs, m0, LD_P, prm, vm1, vm2, p1, p2, q1, q2, bnd, eA, eB);
    else ld_filter<true>(xs, m0, cnt, prm, vm1, vm2, p1, p2, q1, q2, bnd, eA, eB);
    if (tid == LD_THREADS - 1) { carry[0] = p1; carry[1] = p2; carry[2] = q1; carry[3] = q2; }   // read after the next barrier

    // the wave's hops inside the chunk
    const long wfirst = ts + (long)wave * 64 * LD_P, wend = min(wfirst + 64 * LD_P, hi);
    if (wfirst < wend) {
      const long ha = max(ld_whole_hops(wfirst, sr), h0), hb = min(ld_whole_hops(wend - 1, sr), h1 - 1);
      for (long h = ha; h <= hb; ++h) {
        double e = (hA == h ? eA : 0.0) + (hA + 1 == h ? eB : 0.0);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) e += __shfl_xor(e, d, 64);
        if (lane == 0) wacc[wave][h - h0] += e;
      }
    }
  }
  __syncthreads();
  if (tid < h1 - h0 && h0 + tid < Hmax) hops[seg * Hmax + h0 + tid] = ((wacc[0][tid] + wacc[1][tid]) + wacc[2][tid]) + wacc[3][tid];
}

// z_j of block j from four hop sums, and its L_j
__device__ __forceinline__ double ld_block(const double* __restrict__ h, int j, int sr, double* Lj) {
  const double z = (((h[j] + h[j + 1]) + h[j + 2]) + h[j + 3]) / (double)(((long)(j + 4) * sr) / 10 - ((long)j * sr) / 10);
  *Lj = -0.691 + 10.0 * log10(z);
  return z;
}

// sum over the wave in a fixed order; every lane gets it
__device__ __forceinline__ double ld_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// blocks of four hops and the two gates: one segment per wave, lane l takes blocks l, l + 64, ... (a thread that walked
// all blocks of a 30 s segment alone would wait for 600 dependent loads)
__global__ void __launch_bounds__(LD_GATE_THREADS) loudness_gate_kernel(const long* __restrict__ seg_len, int S, long max_len,
                                                                        int sr, int half, long Hmax,
                                                                        const double* __restrict__ hops,
                                                                        double* __restrict__ loud, int* __restrict__ counts) {
  const int s = blockIdx.x * (LD_GATE_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= S) return;                            // the same for the whole wave
  double result = -INFINITY;
  int nb = 0, nA = 0, nG = 0;
  long len = seg_len[s];
  if (len >= 1) {
    len = min(len, max_len);
    const long Hn = ld_whole_hops(ld_n_eff(len, half), sr);
    nb = Hn >= 4 ? (int)(Hn - 3) : 0;
    const double* h = hops + (long)s * Hmax;
    double sumA = 0.0, cA = 0.0, Lj;
    for (int j = lane; j < nb; j += 64) {
      const double z = ld_block(h, j, sr, &Lj);
      if (Lj > -70.0) { cA += 1.0; sumA += z; }
    }
    sumA = ld_wave_sum(sumA);
    nA = (int)ld_wave_sum(cA);
    if (nA > 0) {
      const double gamma = -0.691 + 10.0 * log10(sumA / nA) - 10.0;
      double sumG = 0.0, cG = 0.0;
      for (int j = lane; j < nb; j += 64) {
        const double z = ld_block(h, j, sr, &Lj);
        if (Lj > -70.0 && Lj > gamma) { cG += 1.0; sumG += z; }
      }
      sumG = ld_wave_sum(sumG);
      nG = (int)ld_wave_sum(cG);
      if (nG > 0) result = -0.691 + 10.0 * log10(sumG / nG);
    }
  }
  if (lane == 0) {
    loud[s] = result;
    if (counts) { counts[3 * s] = nb; counts[3 * s + 1] = nA; counts[3 * s + 2] = nG; }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static bool ld_sr_ok(int sr) { return sr >= 1000 && sr <= 384000; }

static void ld_biquads(int sr, double* out) {
  {
    const double K = tan(LD_PI * LD_SHELF_F0 / sr), Vh = pow(10.0, LD_SHELF_G / 20.0), Vb = pow(Vh, LD_SHELF_VB_EXP);
    const double a0 = 1.0 + K / LD_SHELF_Q + K * K;
    out[0] = (Vh + Vb * K / LD_SHELF_Q + K * K) / a0;
    out[1] = 2.0 * (K * K - Vh) / a0;
    out[2] = (Vh - Vb * K / LD_SHELF_Q + K * K) / a0;
    out[3] = 2.0 * (K * K - 1.0) / a0;
    out[4] = (1.0 - K / LD_SHELF_Q + K * K) / a0;
  }
  {
    const double K = tan(LD_PI * LD_HP_F0 / sr), a0 = 1.0 + K / LD_HP_Q + K * K;
    out[5] = 1.0; out[6] = -2.0; out[7] = 1.0;
    out[8] = 2.0 * (K * K - 1.0) / a0;
    out[9] = (1.0 - K / LD_HP_Q + K * K) / a0;
  }
}

extern "C" int bsed_kweight_coefs(int sr, double* out) {
  BSED_CHECK_ARG(out, "bsed_kweight_coefs: null pointer");
  BSED_CHECK_ARG(ld_sr_ok(sr), "bsed_kweight_coefs: sr must be in 1000..384000 (got %d)", sr);
  ld_biquads(sr, out);
  return BSED_OK;
}

// largest pole radius of z^2 + a1 z + a2
static double ld_pole_radius(double a1, double a2) {
  const double disc = a1 * a1 - 4.0 * a2;
  if (disc < 0.0) return sqrt(a2);
  return (fabs(a1) + sqrt(disc)) / 2.0;
}

static void ld_matmul(const double* A, const double* B, double* C) {
  double T[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 4; ++k) acc = fma(A[4 * r + k], B[4 * k + c], acc);
      T[4 * r + c] = acc;
    }
  for (int i = 0; i < 16; ++i) C[i] = T[i];
}

// the launch geometry of (S, max_len, sr): one answer for the workspace query and the launch
struct LdGeom { int half, HC, nch; long Hmax, W; LdParams prm; };

static int ld_geometry(const char* who, int S, long max_len, int sr, LdGeom* g) {
  BSED_CHECK_ARG(S >= 1, "%s: S must be at least 1 (got %d)", who, S);
  BSED_CHECK_ARG(max_len >= 1 && max_len < (1L << 40), "%s: max_len must be in 1..2^40 samples (got %ld)", who, max_len);
  BSED_CHECK_ARG(ld_sr_ok(sr), "%s: sr must be in 1000..384000 (got %d)", who, sr);
  BSED_CHECK_ARG(sr >= LD_MIN_SR, "%s: sr = %d is below %d: the shelf's centre frequency lies above sr / 2 and the "
                 "recurrence is not stable", who, sr, LD_MIN_SR);
  double c[10];
  ld_biquads(sr, c);
  LdParams& p = g->prm;
  p.b0 = c[0]; p.b1 = c[1]; p.b2 = c[2]; p.a1 = c[3]; p.a2 = c[4]; p.c1 = c[8]; p.c2 = c[9];
  const double r = fmax(ld_pole_radius(p.a1, p.a2), ld_pole_radius(p.c1, p.c2));
  BSED_CHECK_ARG(r > 0.0 && r < 1.0, "%s: the K-weighting is not stable at sr = %d", who, sr);
  g->W = (long)ceil(50.0 / -log(r));
  g->half = (sr + 1) / 2;
  // a segment shorter than half is tiled to less than half + its length
  const long tiled_max = (long)g->half + (max_len < g->half ? max_len : (long)g->half);
  const long n_eff_max = max_len > tiled_max ? max_len : tiled_max;
  g->Hmax = (10 * (n_eff_max + 1) - 1) / sr;
  if (g->Hmax < 1) g->Hmax = 1;
  // about 2048 workgroups where the work allows it; a chunk is 2 .. LD_MAX_HC hops (its warm-up costs 2.1 more)
  long HC = ((long)S * g->Hmax + 2047) / 2048;
  HC = HC < 2 ? 2 : HC > LD_MAX_HC ? LD_MAX_HC : HC;
  g->HC = (int)HC;
  const long nch = (g->Hmax + HC - 1) / HC;
  BSED_CHECK_ARG(nch * S < (1L << 31), "%s: too many workgroups (%ld)", who, nch * S);
  g->nch = (int)nch;
  // zero-input step of the state (p1, p2, q1, q2), then M = A^32 and its squares
  const double A[16] = {-p.a1, -p.a2, 0.0, 0.0,   1.0, 0.0, 0.0, 0.0,   -p.a1 - 2.0, 1.0 - p.a2, -p.c1, -p.c2,   0.0, 0.0, 1.0, 0.0};
  double M[16];
  for (int i = 0; i < 16; ++i) M[i] = A[i];
  for (int k = 0; k < 5; ++k) ld_matmul(M, M, M);                                     // 2^5 = LD_P
  for (int j = 0; j < 8; ++j) {
    for (int i = 0; i < 16; ++i) p.M[j][i] = M[i];
    ld_matmul(M, M, M);
  }
  return BSED_OK;
}

extern "C" long bsed_loudness_ws_bytes(int S, long max_len, int sr) {
  LdGeom g;
  if (ld_geometry("bsed_loudness_ws_bytes", S, max_len, sr, &g) != BSED_OK) return -1;
  return 8L * S * g.Hmax;
}

extern "C" int bsed_loudness(const float* x, long x_len, const long* seg_off, const long* seg_len, int S, long max_len, int sr,
                             void* ws, long ws_bytes, double* loud, int* counts, void* stream) {
  BSED_CHECK_ARG(x && seg_off && seg_len && ws && loud, "bsed_loudness: null pointer");
  BSED_CHECK_ARG(x_len >= 1 && x_len < (1L << 40), "bsed_loudness: x_len must be in 1..2^40 samples (got %ld)", x_len);
  LdGeom g;
  const int rc = ld_geometry("bsed_loudness", S, max_len, sr, &g);
  if (rc != BSED_OK) return rc;
  BSED_CHECK_ARG(ws_bytes >= 8L * S * g.Hmax, "bsed_loudness: workspace too small: %ld bytes, bsed_loudness_ws_bytes gives %ld",
                 ws_bytes, 8L * S * g.Hmax);
  BSED_CHECK_ARG((uintptr_t)x % 4 == 0 && (uintptr_t)seg_off % 8 == 0 && (uintptr_t)seg_len % 8 == 0 && (uintptr_t)ws % 8 == 0 &&
                 (uintptr_t)loud % 8 == 0 && (uintptr_t)counts % 4 == 0, "bsed_loudness: misaligned table");
  static_assert(LD_P == 32 && LD_MIN_SR / 10 >= LD_P, "a piece holds at most one hop boundary");
  hipLaunchKernelGGL(loudness_hops_kernel, dim3((unsigned)((long)S * g.nch)), dim3(LD_THREADS), 0, (hipStream_t)stream, x, x_len,
                     seg_off, seg_len, max_len, sr, g.half, g.W, g.HC, g.nch, g.Hmax, g.prm, (double*)ws);
  BSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(loudness_gate_kernel, dim3((unsigned)((S + LD_GATE_THREADS / 64 - 1) / (LD_GATE_THREADS / 64))), dim3(LD_GATE_THREADS), 0,
                     (hipStream_t)stream, seg_len, S, max_len, sr, g.half, g.Hmax, (const double*)ws, loud, counts);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
