// Row mixing for interpolation consistency training (mixup): out[r] = lam * in[r] + oml * in[perm[r]] over the rows of
// up to BSED_MIX_MAX_JOBS tensors in ONE launch (include/bsed.h: bsed_mix_rows).  A streaming kernel: 12 bytes of traffic
// and three flops per element, nothing to reuse but the perm entry of a row.
#include "bsed_common.h"

// The two products are rounded separately, then the sum: what torch and numpy compute on the host in float32 for
// `lam * x + (1 - lam) * x[index]`.  hipcc contracts a * b + c into one fma by default (and its __fmul_rn / __fadd_rn
// are plain operators the contraction sees through), which rounds once and gives other bits: off for this file.
#pragma clang fp contract(off)

#define MIX_THREADS 256   // one tile = 256 consecutive 4-element chunks of ONE job: the job of a tile is wave-uniform

struct MixJob {
  const float* in; float* out; const int* perm;
  float lam, oml;
  int rows, vec;             // vec: every chunk of the job is one aligned 16-byte load pair and store
  unsigned cpr, chunks;      // chunks per row = ceil(row_len / 4); chunks of the job = rows * cpr (below 2^31)
  int tile0;                 // first tile of the job in the launch's flat tile space
  long row_len;
};
struct MixBatch { MixJob j[BSED_MIX_MAX_JOBS]; int njobs, tiles; };

__device__ __forceinline__ float mix1(float a, float b, float lam, float oml) {
  const float pa = lam * a, pb = oml * b;
  return pa + pb;
}

__global__ __launch_bounds__(MIX_THREADS) void mix_rows_kernel(const MixBatch Bt) {
  for (int t = blockIdx.x; t < Bt.tiles; t += gridDim.x) {
    int ji = 0;
    for (int k = 1; k < Bt.njobs; ++k)
      if (t >= Bt.j[k].tile0) ji = k;
    const MixJob& J = Bt.j[ji];                                 // uniform index: the fields arrive as scalar loads
    const unsigned c = (unsigned)(t - J.tile0) * MIX_THREADS + threadIdx.x;
    if (c >= J.chunks) continue;
    const unsigned r = c / J.cpr, q = c - r * J.cpr;
    // perm is not validated: an entry outside 0 .. rows - 1 is clamped, so only rows of `in` are read
    const int pr = min(max(J.perm[r], 0), J.rows - 1);
    const size_t col = (size_t)q * 4;
    const float* a = J.in + (size_t)r * J.row_len + col;
    const float* b = J.in + (size_t)pr * J.row_len + col;
    float* o = J.out + (size_t)r * J.row_len + col;
    if (J.vec) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(a), vb = *reinterpret_cast<const f32x4*>(b);
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = mix1(va[e], vb[e], J.lam, J.oml);
      *reinterpret_cast<f32x4*>(o) = v;
    } else {
      const long left = J.row_len - (long)col;                  // the last chunk of a row may be short
      const int n = left < 4 ? (int)left : 4;
      for (int e = 0; e < n; ++e) o[e] = mix1(a[e], b[e], J.lam, J.oml);
    }
  }
}

extern "C" int bsed_mix_rows(const void* in, const void* out, const void* perm, const float* lam, const float* oml,
                             const int* rows, const long* row_len, int njobs, void* stream) {
  BSED_CHECK_ARG(in && out && perm && lam && oml && rows && row_len, "bsed_mix_rows: null job table");
  BSED_CHECK_ARG(njobs >= 1 && njobs <= BSED_MIX_MAX_JOBS, "bsed_mix_rows: 1..%d jobs (got %d)", BSED_MIX_MAX_JOBS, njobs);
  const float* const* ins = static_cast<const float* const*>(in);
  float* const* outs = static_cast<float* const*>(out);
  const int* const* perms = static_cast<const int* const*>(perm);
  MixBatch Bt;
  Bt.njobs = njobs;
  int tiles = 0;
  for (int i = 0; i < njobs; ++i) {
    MixJob& J = Bt.j[i];
    J.in = ins[i]; J.out = outs[i]; J.perm = perms[i]; J.lam = lam[i]; J.oml = oml[i];
    J.rows = rows[i]; J.row_len = row_len[i];
    BSED_CHECK_ARG(J.in && J.out && J.perm, "bsed_mix_rows: null pointer in job %d", i);
    BSED_CHECK_ARG(J.rows >= 1, "bsed_mix_rows: job %d: rows must be >= 1 (got %d)", i, J.rows);
    BSED_CHECK_ARG(J.row_len >= 1, "bsed_mix_rows: job %d: row_len must be >= 1 (got %ld)", i, J.row_len);
    const long cpr = (J.row_len + 3) / 4;
    BSED_CHECK_ARG(cpr <= ((1L << 31) - 1) / J.rows, "bsed_mix_rows: job %d too large: rows * ceil(row_len / 4) must be "
                   "below 2^31", i);
    const uintptr_t pi = (uintptr_t)J.in, po = (uintptr_t)J.out, bytes = (uintptr_t)J.rows * J.row_len * 4;
    BSED_CHECK_ARG(pi % 4 == 0 && po % 4 == 0 && (uintptr_t)J.perm % 4 == 0, "bsed_mix_rows: misaligned pointer in job %d "
                   "(4-byte elements)", i);
    // every output row reads ANOTHER row of the input: in place, a row could be overwritten before it is gathered
    BSED_CHECK_ARG(pi != po && (pi + bytes <= po || po + bytes <= pi), "bsed_mix_rows: job %d: in and out overlap", i);
    J.vec = pi % 16 == 0 && po % 16 == 0 && J.row_len % 4 == 0;
    J.cpr = (unsigned)cpr;
    J.chunks = (unsigned)(cpr * J.rows);
    J.tile0 = tiles;
    tiles += ceil_div(J.chunks, MIX_THREADS);     // below 8 * 2^23
  }
  Bt.tiles = tiles;
  // 8 workgroups of 4 waves per CU, the rest of the tiles by stride
  hipLaunchKernelGGL(mix_rows_kernel, dim3((unsigned)std::min(tiles, 2048)), dim3(MIX_THREADS), 0, (hipStream_t)stream, Bt);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
