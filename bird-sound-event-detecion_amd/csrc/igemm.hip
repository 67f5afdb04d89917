// The fp32 forward contraction on v_mfma_f32_32x32x2_f32 (exact fp32 matrix cores of gfx950): igemm_kernel behind
// bsed_igemm, and pack_weight_kernel (bsed_pack_weight), which lays the weights out for this kernel only.
//
//   igemm_kernel : out[p][n] = sum_{tap,k} in[p + off(tap)][k] * w[tap][k][n]   (NHWC, zero padding)
//                  M = 128 output positions of a TH x TW spatial tile, N = 32/64/128 channels,
//                  K = taps x CIN, staged through LDS in (tap, 32-channel) slabs.
//                  One kernel body serves (reference call sites in brackets):
//                    conv 3x3 forward + BatchNorm batch statistics   [src/models/CNN.py:46-49]
//                    conv 3x3 data gradient (flipped taps)           [autograd of the above]
//                    GLU: BN-apply on load, 1x1 contraction, sigmoid gate, dropout, avg-pool
//                         fused in the epilogue                      [src/models/CNN.py:5-16,59-67]
//                    GLU backward pre/post stages
//                    GRU input projections / their data gradients    [src/models/RNN.py:12 (nn.GRU)]
//
// The weight gradients of the same layers (fp32 cores and split-fp32) are in wgrad.hip; the reduction of their partial
// slabs is in reduce.hip.  The tile constants and the C-layout row map that igemm.hip and wgrad.hip share are in bsed_common.h.
//
// Lane maps (pinned on hardware by bsed_selftest_mfma): A[i=lane&31][k=lane>>5],
// B[k=lane>>5][j=lane&31], C[row=(r&3)+8*(r>>2)+4*(lane>>5)][col=lane&31].
#include "bsed_common.h"
#include "../../include/bsed.h"
#include <algorithm>
#include <type_traits>

enum { EPI_PLAIN = 0, EPI_STATS = 1, EPI_GLU_POOL = 2, EPI_GLU_BWD = 3, EPI_ADD_STATS2 = 4 };

struct IgemmParams {
  BsedIgemmDesc d;
  int PW, PH, PP, lgTW, b_off, pw_magic;  // derived on the host; pos / PW == (pos * pw_magic) >> 20
  const uint64_t* seed_add;               // device-resident addend of d.seed (HIP-graph replays), or null
};

template <int KC, int BN, int EPI>
__global__ __launch_bounds__(IG_THREADS) void igemm_kernel(const IgemmParams P) {
  constexpr int NT = BN / 32;
  constexpr int AP = KC + 1;
  const BsedIgemmDesc& p = P.d;
  extern __shared__ __align__(16) float smem[];
  float* As = smem;
  float* Bs = smem + P.b_off;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  int tile = blockIdx.x;
  const int tw_i = tile % p.tilesW; tile /= p.tilesW;
  const int th_i = tile % p.tilesH;
  const int nb = tile / p.tilesH;
  const int th0 = th_i * p.TH, tw0 = tw_i * p.TW;
  const int n0 = blockIdx.y * BN;
  const int PW = P.PW;
  const int m = wave * 32 + li;
  const int abase = (((m >> P.lgTW) + p.hh) * PW + (m & (p.TW - 1)) + p.hw) * AP;

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const float* inb = p.in + (size_t)nb * p.H * p.W * p.in_pitch;
  for (int c0 = 0; c0 < p.CIN; c0 += KC) {
    __syncthreads();
    // global loads are issued four at a time before any LDS store so their latencies overlap
    const int a_total = P.PP * (KC / 4);
    for (int e0 = tid; e0 < a_total; e0 += 4 * IG_THREADS) {
      float4 v[4];
      bool okv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * IG_THREADS;
        const int c4 = e % (KC / 4), pos = e / (KC / 4);
        const int pr = (pos * P.pw_magic) >> 20, pc = pos - pr * PW;
        const int gh = th0 - p.hh + pr, gw = tw0 - p.hw + pc;
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        okv[u] = e < a_total && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W;
        if (okv[u]) v[u] = *reinterpret_cast<const float4*>(inb + ((size_t)gh * p.W + gw) * p.in_pitch + c0 + 4 * c4);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * IG_THREADS;
        if (e < a_total) {
          const int c4 = e % (KC / 4), pos = e / (KC / 4);
          if (p.a_scale && okv[u]) {
            const float4 sc = *reinterpret_cast<const float4*>(p.a_scale + c0 + 4 * c4);
            const float4 sh = *reinterpret_cast<const float4*>(p.a_shift + c0 + 4 * c4);
            v[u].x = fmaf(v[u].x, sc.x, sh.x); v[u].y = fmaf(v[u].y, sc.y, sh.y);
            v[u].z = fmaf(v[u].z, sc.z, sh.z); v[u].w = fmaf(v[u].w, sc.w, sh.w);
          }
          float* dst = As + pos * AP + 4 * c4;
          dst[0] = v[u].x; dst[1] = v[u].y; dst[2] = v[u].z; dst[3] = v[u].w;
        }
      }
    }
    for (int tap = 0; tap < p.ntaps; ++tap) {
      if (tap > 0) __syncthreads();
      const float* wsrc = p.w + ((size_t)tap * p.CIN + c0) * p.NP + n0;
      for (int e = tid; e < KC * BN / 4; e += IG_THREADS) {
        const int k = e / (BN / 4), n4 = e % (BN / 4);
        *reinterpret_cast<float4*>(Bs + k * BN + 4 * n4) =
            *reinterpret_cast<const float4*>(wsrc + (size_t)k * p.NP + 4 * n4);
      }
      __syncthreads();
      const float* arow = As + abase + (p.dh[tap] * PW + p.dw[tap]) * AP + lh;
      const float* brow = Bs + lh * BN + li;
#pragma unroll 4
      for (int kk = 0; kk < KC; kk += 2) {
        const float a = arow[kk];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const float b = brow[kk * BN + 32 * j];
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[j], 0, 0, 0);
        }
      }
    }
  }

  // ------------------------------------------------------------------------------------ epilogue
  // VALU-lean by construction: position math once per accumulator register (not per channel tile),
  // pooling windows are 1 or 2 (shifts, no integer division), dropout from a 32-bit mix hash.
  float s0[NT], s1[NT];
  float bias[NT], esc[NT], esh[NT];
  bool nok[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    s0[j] = 0.f; s1[j] = 0.f;
    const int n = n0 + 32 * j + li;
    nok[j] = n < p.N;
    bias[j] = (p.bias && nok[j]) ? p.bias[n] : 0.f;
    esc[j] = 0.f; esh[j] = 0.f;
    if (EPI == EPI_GLU_POOL || EPI == EPI_GLU_BWD) {
      if (nok[j]) { esc[j] = p.e_scale[n]; esh[j] = p.e_shift[n]; }
    }
  }
  if (EPI == EPI_GLU_POOL) __syncthreads();  // As/Bs are recycled as the pooling stage
  float* Cs = smem;                          // [128][BN+1]
  const int sph = p.ph >> 1, spw = p.pw >> 1;  // pooling windows are 1 or 2
  const float inv_pool = 1.0f / (float)(p.ph * p.pw);
  const uint32_t dkey = drop_key(p.rng_stream, p.seed + (P.seed_add ? *P.seed_add : 0));
  const uint32_t dthr = drop_threshold(p.drop_p);
  const float dscale = p.drop_p > 0.f ? 1.0f / (1.0f - p.drop_p) : 1.0f;
  const int nbase = n0 + li;

  // Side inputs (pre-BN activation, pooled gradient, residual) are fetched for FOUR accumulator rows at a time
  // before any store: a store to `out` may alias those loads as far as the compiler knows (and does alias for the
  // in-place residual form), which would otherwise serialise one exposed global-load latency per element.
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    float ev[4][NT], dv[4][NT], rv[4][NT];
    size_t posv[4];
    int mmv[4];
    bool pokv[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int r = rg * 4 + rr;
      const int mm = wave * 32 + crow(r, lh);
      const int gh = th0 + (mm >> P.lgTW), gw = tw0 + (mm & (p.TW - 1));
      const bool pok = gh < (p.valid_h > 0 ? p.valid_h : p.H) && gw < (p.valid_w > 0 ? p.valid_w : p.W);
      const size_t pos = ((size_t)nb * p.H + gh) * p.W + gw;
      mmv[rr] = mm; pokv[rr] = pok; posv[rr] = pos;
      bool pooled_ok = false;
      const float* dprow = nullptr;
      if (EPI == EPI_GLU_BWD) {
        const int gph = gh >> sph, gpw = gw >> spw;
        pooled_ok = pok && gph < p.Hp && gpw < p.Wp;
        dprow = p.e_dpool + (((size_t)nb * p.Hp + gph) * p.Wp + gpw) * p.N + nbase;
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const bool ok = pok && nok[j];
        ev[rr][j] = 0.f; dv[rr][j] = 0.f; rv[rr][j] = 0.f;
        if (EPI == EPI_GLU_POOL || EPI == EPI_GLU_BWD || EPI == EPI_ADD_STATS2)
          if (ok) ev[rr][j] = p.e_src[pos * p.e_pitch + nbase + 32 * j];
        if (EPI == EPI_GLU_BWD)
          if (pooled_ok && nok[j]) dv[rr][j] = dprow[32 * j];
        if (EPI == EPI_ADD_STATS2)
          if (ok) rv[rr][j] = p.out2[pos * p.out_pitch + nbase + 32 * j];
      }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int r = rg * 4 + rr;
      const size_t pos = posv[rr];
      float* orow = p.out + pos * p.out_pitch + nbase;
      const uint64_t ebase = (uint64_t)pos * p.N + nbase;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const bool ok = pokv[rr] && nok[j];
        const float v = acc[j][r] + bias[j];
        if (EPI == EPI_PLAIN) {
          if (ok) orow[32 * j] = v;
        } else if (EPI == EPI_STATS) {
          if (ok) {
            orow[32 * j] = v;
            s0[j] += v;
            s1[j] = fmaf(v, v, s1[j]);
          }
        } else if (EPI == EPI_GLU_POOL) {
          float res = 0.f;
          if (ok) {
            const float xn = fmaf(ev[rr][j], esc[j], esh[j]);
            res = v * sigmoid_fast(xn) * drop_mul(ebase + 32 * j, dkey, dthr, dscale);
          }
          Cs[mmv[rr] * (BN + 1) + 32 * j + li] = res;
        } else if (EPI == EPI_GLU_BWD) {
          if (ok) {
            const float xn = fmaf(ev[rr][j], esc[j], esh[j]);
            const float sg = sigmoid_fast(xn);
            const float dres = dv[rr][j] * inv_pool * drop_mul(ebase + 32 * j, dkey, dthr, dscale);
            const float dlin = dres * sg;
            orow[32 * j] = dlin;
            p.out2[pos * p.out_pitch + nbase + 32 * j] = dres * v * sg * (1.0f - sg);
            s0[j] += dlin;
          }
        } else {  // EPI_ADD_STATS2: g = acc + residual ; stats = (sum g, sum g*y)
          if (ok) {
            const float g = v + rv[rr][j];
            orow[32 * j] = g;
            s0[j] += g;
            s1[j] = fmaf(g, ev[rr][j], s1[j]);
          }
        }
      }
    }
  }

  if (EPI == EPI_GLU_POOL) {
    __syncthreads();
    const int lgtpw = P.lgTW - spw;
    const int tpw = 1 << lgtpw, tph = p.TH >> sph;
    for (int e = tid; e < tph * tpw * BN; e += IG_THREADS) {
      const int n = e % BN, pp = e / BN;
      const int pr = pp >> lgtpw, pc = pp & (tpw - 1);
      const int gph = (th0 >> sph) + pr, gpw = (tw0 >> spw) + pc;
      if (gph < p.Hp && gpw < p.Wp && n0 + n < p.N) {
        const float* c0 = Cs + (((pr << sph) << P.lgTW) + (pc << spw)) * (BN + 1) + n;
        float s = c0[0];
        if (spw) s += c0[BN + 1];
        if (sph) {
          s += c0[p.TW * (BN + 1)];
          if (spw) s += c0[(p.TW + 1) * (BN + 1)];
        }
        p.out[(((size_t)nb * p.Hp + gph) * p.Wp + gpw) * p.out_pitch + n0 + n] = s * inv_pool;
      }
    }
  }

  if (EPI == EPI_STATS || EPI == EPI_GLU_BWD || EPI == EPI_ADD_STATS2) {
    __syncthreads();
    float* red = smem;  // [4][2][BN]
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float a = s0[j] + __shfl_xor(s0[j], 32, 64);
      const float b = s1[j] + __shfl_xor(s1[j], 32, 64);
      if (lh == 0) {
        red[(wave * 2 + 0) * BN + 32 * j + li] = a;
        red[(wave * 2 + 1) * BN + 32 * j + li] = b;
      }
    }
    __syncthreads();
    if (tid < 2 * BN) {
      const int which = tid / BN, n = tid % BN;
      if (n0 + n < p.N) {
        const float s = red[(0 * 2 + which) * BN + n] + red[(1 * 2 + which) * BN + n] +
                        red[(2 * 2 + which) * BN + n] + red[(3 * 2 + which) * BN + n];
        p.stats[((size_t)blockIdx.x * 2 + which) * p.N + n0 + n] = s;
      }
    }
  }
}

// wpk[tap][k][n] = src[tap*s_tap + k*s_k + n*s_n], zero for n >= N
__global__ void pack_weight_kernel(const float* __restrict__ src, float* __restrict__ dst, int ntaps, int K, int N,
                                   int NP, long s_tap, long s_k, long s_n) {
  const long total = (long)ntaps * K * NP;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int n = (int)(e % NP);
    const long r = e / NP;
    const int k = (int)(r % K), tap = (int)(r / K);
    dst[e] = n < N ? src[tap * s_tap + k * s_k + n * s_n] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <int KC, int BN>
static int launch_igemm_epi(const IgemmParams& P, const BsedLaunch& L) {
  switch (P.d.epilogue) {
#define CASE(E)                                                                                       \
  case E: {                                                                                           \
    BSED_LABEL_ONLY(L, "igemm_kernel<%d, %d, %d>", KC, BN, E);                                        \
    static BsedLdsOnce once;                                                                         \
    BSED_HIP(bsed_max_lds(once, (const void*)igemm_kernel<KC, BN, E>));                              \
    hipLaunchKernelGGL((igemm_kernel<KC, BN, E>), L.grid, dim3(IG_THREADS), L.smem, L.s, P);          \
    break;                                                                                            \
  }
    CASE(EPI_PLAIN)
    CASE(EPI_STATS)
    CASE(EPI_GLU_POOL)
    CASE(EPI_GLU_BWD)
    CASE(EPI_ADD_STATS2)
#undef CASE
    default:
      bsed_set_error("bsed_igemm: unknown epilogue %d", P.d.epilogue);
      return BSED_ERR_ARG;
  }
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

// bsed_igemm (plan == null: pointer checks and the launch) and its plan (the label only) after ONE prepare step: every
// shape check, the derived geometry, the LDS bytes and the grid
int bsed_run_igemm(const BsedIgemmDesc* desc, void* stream, BsedContractPlan* plan) {
  BSED_CHECK_ARG(desc, "bsed_igemm: null descriptor");
  IgemmParams P;
  P.d = *desc;
  BsedIgemmDesc& d = P.d;
  const int ntiles = bsed_tile_geometry(P, "bsed_igemm", 16, 4);
  if (ntiles < 0) return ntiles;
  BSED_CHECK_ARG(d.out_pitch >= d.N, "bsed_igemm: bad pitch");
  const int KC = (d.CIN % 32 == 0) ? 32 : 16, BN = bsed_contract_bn(d.NP);
  P.b_off = (P.PP * (KC + 1) + 3) & ~3;
  size_t fl = (size_t)P.b_off + (size_t)KC * BN;
  const bool pooled = (d.ph == 1 || d.ph == 2) && (d.pw == 1 || d.pw == 2) && d.Hp == d.H / d.ph && d.Wp == d.W / d.pw;
  if (d.epilogue == EPI_GLU_POOL) {
    BSED_CHECK_ARG((d.ph == 1 || d.ph == 2) && (d.pw == 1 || d.pw == 2) && d.TH % d.ph == 0 && d.TW % d.pw == 0,
                   "bsed_igemm: pooling windows must be 1 or 2 and divide the tile");
    BSED_CHECK_ARG(pooled, "bsed_igemm: bad pooled shape");
    fl = std::max(fl, (size_t)IG_TILE_M * (BN + 1));
  }
  if (d.epilogue == EPI_GLU_POOL || d.epilogue == EPI_GLU_BWD)
    BSED_CHECK_ARG(d.e_pitch >= d.N, "bsed_igemm: GLU epilogue needs e_src/e_scale/e_shift");
  if (d.epilogue == EPI_GLU_BWD) BSED_CHECK_ARG(pooled, "bsed_igemm: GLU_BWD epilogue needs e_dpool/out2/stats and pooled shape");
  if (d.epilogue == EPI_ADD_STATS2) BSED_CHECK_ARG(d.e_pitch >= d.N, "bsed_igemm: ADD_STATS2 needs out2/e_src/stats");
  fl = std::max(fl, (size_t)8 * BN);
  BsedLaunch L{dim3((unsigned)ntiles, d.NP / BN), fl * sizeof(float), (hipStream_t)stream, nullptr};
  BSED_CHECK_ARG(L.smem <= 160 * 1024, "bsed_igemm: tile needs %zu B of LDS", L.smem);
  if (plan) L = bsed_plan_begin(plan, ntiles, ntiles, ntiles);   // one workgroup and one statistics row per tile
  else {
    P.seed_add = bsed_seed_add_ptr();
    BSED_CHECK_ARG(d.in && d.w && d.out, "bsed_igemm: null tensor");
    if (d.epilogue == EPI_GLU_POOL || d.epilogue == EPI_GLU_BWD)
      BSED_CHECK_ARG(d.e_src && d.e_scale && d.e_shift, "bsed_igemm: GLU epilogue needs e_src/e_scale/e_shift");
    if (d.epilogue == EPI_GLU_BWD)
      BSED_CHECK_ARG(d.e_dpool && d.out2 && d.stats, "bsed_igemm: GLU_BWD epilogue needs e_dpool/out2/stats and pooled shape");
    if (d.epilogue == EPI_ADD_STATS2) BSED_CHECK_ARG(d.out2 && d.e_src && d.stats, "bsed_igemm: ADD_STATS2 needs out2/e_src/stats");
    if (d.epilogue == EPI_STATS) BSED_CHECK_ARG(d.stats, "bsed_igemm: STATS epilogue needs a stats buffer");
  }
  if (KC == 32) {
    if (BN == 128) return launch_igemm_epi<32, 128>(P, L);
    if (BN == 64) return launch_igemm_epi<32, 64>(P, L);
    return launch_igemm_epi<32, 32>(P, L);
  }
  if (BN == 128) return launch_igemm_epi<16, 128>(P, L);
  if (BN == 64) return launch_igemm_epi<16, 64>(P, L);
  return launch_igemm_epi<16, 32>(P, L);
}
extern "C" int bsed_igemm(const BsedIgemmDesc* desc, void* stream) { return bsed_run_igemm(desc, stream, nullptr); }

extern "C" int bsed_pack_weight(const float* src, float* dst, int ntaps, int K, int N, int NP, long s_tap, long s_k,
                                long s_n, void* stream) {
  BSED_CHECK_ARG(src && dst && ntaps > 0 && K > 0 && N > 0 && NP >= N, "bsed_pack_weight: bad argument");
  const long total = (long)ntaps * K * NP;
  hipLaunchKernelGGL(pack_weight_kernel, dim3((unsigned)std::min<long>(ceil_div(total, 256), 4096)), dim3(256), 0,
                     (hipStream_t)stream, src, dst, ntaps, K, N, NP, s_tap, s_k, s_n);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
