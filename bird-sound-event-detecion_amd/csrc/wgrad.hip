// Weight gradients of the tiled contractions (bsed_wgrad, bsed_wgrad3):
//   dW[tap][k][n] = sum_p in[p + off(tap)][k] * dy[p][n]      (K of the GEMM = positions, NHWC, zero padding)
// Every kernel is persistent over 128-position tiles and writes one partial slab part[g][tap][CINP][NP] per
// workgroup along grid.x; reduce.hip sums the G slabs into the gradient.  One descriptor (BsedWgradDesc), one prepare
// step (wgrad_prepare) and one plan (wgrad3_plan) choose among four kernels:
//
//   wgrad_kernel    bsed_wgrad: fp32 matrix cores (v_mfma_f32_32x32x2_f32), any shape the descriptor allows.  The
//                   "fp32" mode of the train step and the reference of the split-fp32 forms.
//   wgrad3_kernel   bsed_wgrad3, the TILE form: split-fp32 operands on the bf16 matrix cores (bf16x3, see igemm3.hip),
//                   one tile staged, then multiplied.  Takes what the two kernels below do not: 1-tap shapes that do not
//                   tile into 128 x 128 blocks (or ask for BatchNorm backward on load), multi-tap shapes with four
//                   (tap, chunk) items or fewer, shapes whose two tile buffers or per-thread prefetch do not fit
//                   (wgrad3_pipelined), and every shape while BSED_WGRAD3_NOPIPE is set.
//   wgrad3p_kernel  bsed_wgrad3, the PIPELINED form for the multi-tap convolutions: one 8-wave workgroup per CU, four
//                   waves stage tile t + 1 while four multiply tile t (wgrad3_pipelined); the network's six layer
//                   geometries are also built with compile-time LDS offsets (w3_geo).
//   wgrad1_kernel   bsed_wgrad3, the ONE-TAP STREAMING form (GLU linears, GRU input / recurrent weights) for slabs that
//                   tile into 128 x 128 blocks (wgrad1_streaming): 64-position tiles through two LDS stages with the
//                   global loads two tiles ahead.
// The three split-fp32 kernels form the same products and add them in the same order per slab; with act_bf16 they read
// bf16 activations and use one MFMA per product.  BatchNorm backward on load (bn_y) is built into wgrad3_kernel and
// wgrad3p_kernel.  The block above each kernel says why it has its shape.
//
// Lane maps as in igemm.hip; IG_TILE_M and crow() come from bsed_common.h.  wgrad_tiles.h holds the device code that
// more than one site uses and that could be shared without costing any instance registers: the tile decode, the
// BatchNorm-backward coefficients and the K step (DESIGN.md section 5 has the figures that kept the rest apart).
#include "wgrad_tiles.h"
#include <algorithm>
#include <type_traits>

#define W3_DY_BYTES (2 * IG_TILE_M * 32 * 2)  // bf16x3 weight gradient: LDS bytes of one 32-channel dy tile (hi + lo planes)

// ---------------------------------------------------------------------------------------------
// weight-gradient kernel on the fp32 matrix cores
// ---------------------------------------------------------------------------------------------
struct WgradParams {
  BsedWgradDesc d;
  int PW, PH, PP, lgTW, dy_off, ntiles, nct, ntw;  // nct = CC/32, ntw = 32-wide dy tiles per workgroup
  int CC, lgc4, pw_magic;                          // input-channel chunk per workgroup (grid.z), log2(CC/4)
  int pack2;                                       // CIN <= 16: two taps share one 32-row MFMA tile
};

// NW waves per workgroup share one staged (activation patch, dy tile) pair: 8 waves double the resident waves per
// byte of LDS, which is what hides the tile-load latency here (occupancy, not prefetching, is the lever).
template <int MAXS, int NW>
__global__ __launch_bounds__(NW * 64) void wgrad_kernel(const WgradParams P) {
  constexpr int NTHR = NW * 64;
  const BsedWgradDesc& p = P.d;
  extern __shared__ __align__(16) float smem[];
  const int XP = P.CC + 1;
  const int cz0 = blockIdx.z * P.CC;
  float* Xs = smem;
  float* DYs = smem + P.dy_off;  // [128][32*ntw]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int DYW = 32 * P.ntw;
  const int n0 = blockIdx.y * DYW;
  const int PW = P.PW;
  const int ntap_items = P.pack2 ? (p.ntaps + 1) / 2 : p.ntaps;
  const int nitems = ntap_items * P.nct * P.ntw;

  int xoff[MAXS], boff[MAXS];
  bool valid[MAXS];
  f32x16 acc[MAXS];
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    const int it = wave + NW * s;
    valid[s] = it < nitems;
    // item -> (input-channel tile, dy tile, tap); a wave's items share the channel tile when ntw == 4
    const int cit = valid[s] ? it % P.nct : 0, rr = valid[s] ? it / P.nct : 0;
    const int nt = rr % P.ntw, tap = rr / P.ntw;
    if (P.pack2) {
      // rows 0..15 of the tile: tap 2*tap, rows 16..31: tap 2*tap+1 (channels 16..31 of the staged patch are zero,
      // which is what the upper rows read when the second tap does not exist)
      const int ta = 2 * tap, tb = 2 * tap + 1;
      if (li < 16 || tb >= p.ntaps) xoff[s] = (p.dh[ta] * PW + p.dw[ta]) * XP + li;
      else xoff[s] = (p.dh[tb] * PW + p.dw[tb]) * XP + (li - 16);
    } else {
      xoff[s] = (p.dh[tap] * PW + p.dw[tap]) * XP + cit * 32 + li;
    }
    boff[s] = nt * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
  }

  for (int tile0 = blockIdx.x; tile0 < P.ntiles; tile0 += gridDim.x) {
    int tile = tile0;
    const int tw_i = tile % p.tilesW; tile /= p.tilesW;
    const int th_i = tile % p.tilesH;
    const int nb = tile / p.tilesH;
    const int th0 = th_i * p.TH, tw0 = tw_i * p.TW;
    const float* inb = p.in + (size_t)nb * p.H * p.W * p.in_pitch;
    const float* dyb = p.dy + (size_t)nb * p.H * p.W * p.dy_pitch;
    __syncthreads();
    const int c4n = 1 << P.lgc4;
    const int x_total = P.PP * c4n;
    for (int e0 = tid; e0 < x_total; e0 += 4 * NTHR) {
      float4 v[4];
      bool okv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * NTHR;
        const int c4 = e & (c4n - 1), pos = e >> P.lgc4;
        const int pr = (pos * P.pw_magic) >> 20, pc = pos - pr * PW;
        const int gh = th0 - p.hh + pr, gw = tw0 - p.hw + pc;
        const int cg = cz0 + 4 * c4;
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        okv[u] = e < x_total && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W && cg < p.CIN;
        if (okv[u]) v[u] = *reinterpret_cast<const float4*>(inb + ((size_t)gh * p.W + gw) * p.in_pitch + cg);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * NTHR;
        if (e < x_total) {
          const int c4 = e & (c4n - 1), pos = e >> P.lgc4;
          if (p.a_scale && okv[u]) {
            const int cg = cz0 + 4 * c4;
            const float4 sc = *reinterpret_cast<const float4*>(p.a_scale + cg);
            const float4 sh = *reinterpret_cast<const float4*>(p.a_shift + cg);
            v[u].x = fmaf(v[u].x, sc.x, sh.x); v[u].y = fmaf(v[u].y, sc.y, sh.y);
            v[u].z = fmaf(v[u].z, sc.z, sh.z); v[u].w = fmaf(v[u].w, sc.w, sh.w);
          }
          float* dst = Xs + pos * XP + 4 * c4;
          dst[0] = v[u].x; dst[1] = v[u].y; dst[2] = v[u].z; dst[3] = v[u].w;
        }
      }
    }
    const int n4n = 8 * P.ntw;
    const int lgn4 = P.ntw == 4 ? 5 : (P.ntw == 2 ? 4 : 3);
    for (int e0 = tid; e0 < IG_TILE_M * n4n; e0 += 4 * NTHR) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * NTHR;
        const int n4 = e & (n4n - 1), mm = e >> lgn4;
        const int gh = th0 + (mm >> P.lgTW), gw = tw0 + (mm & (p.TW - 1));
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < IG_TILE_M * n4n && gh < p.H && gw < p.W && n0 + 4 * n4 < p.N)
          v[u] = *reinterpret_cast<const float4*>(dyb + ((size_t)gh * p.W + gw) * p.dy_pitch + n0 + 4 * n4);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * NTHR;
        const int n4 = e & (n4n - 1), mm = e >> lgn4;
        if (e < IG_TILE_M * n4n) *reinterpret_cast<float4*>(DYs + mm * DYW + 4 * n4) = v[u];
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int kp = 0; kp < IG_TILE_M; kp += 2) {
      const int mk = kp + lh;
      const float* dyrow = DYs + mk * DYW;
      const float* xrow = Xs + (((mk >> P.lgTW) + p.hh) * PW + (mk & (p.TW - 1)) + p.hw) * XP;
      // straight-line on purpose: padded slots (it >= nitems) repeat item 0 and are dropped in the epilogue, so
      // the LDS reads of all slots issue ahead of the MFMAs instead of one exposed LDS latency per MFMA
      float av[MAXS], bv[MAXS];
#pragma unroll
      for (int s = 0; s < MAXS; ++s) {
        av[s] = xrow[xoff[s]];
        bv[s] = dyrow[boff[s]];
      }
#pragma unroll
      for (int s = 0; s < MAXS; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc[s], 0, 0, 0);
    }
  }
  const int NPo = gridDim.y * DYW;
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    if (valid[s]) {
      const int it = wave + NW * s;
      const int cit = it % P.nct, rr = it / P.nct;
      const int nt = rr % P.ntw, tap = rr / P.ntw;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int ci = cz0 + cit * 32 + crow(r, lh), tp = tap;
        if (P.pack2) {
          const int row = crow(r, lh);
          tp = 2 * tap + (row >> 4);
          ci = row & 15;
          if (tp >= p.ntaps) continue;
        }
        p.part[(((size_t)blockIdx.x * p.ntaps + tp) * p.CINP + ci) * NPo + n0 + nt * 32 + li] = acc[s][r];
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------
// weight gradient with split-fp32 operands on the bf16 matrix cores (bf16x3, see igemm3.hip).  K of the GEMM is the
// position index, so a lane's fragment is 8 POSITIONS of one channel:
//   * dy is staged TRANSPOSED ([n][128 positions], bf16 hi / lo planes) -> one 16-byte read per fragment, and a wave
//     whose work items all share the dy tile reads it once per K step;
//   * the activation patch stays position-major (as it arrives from HBM) in two bf16 planes (hi, lo); the tap-shifted
//     fragment comes out of gfx950's transposing LDS read: one ds_read_b64_tr_b16 hands every lane 4 consecutive
//     positions of its channel, whatever the row pitch, so a tap shift is an address offset.  4 such reads (2 LDS cycles
//     each, no VALU) replace the 8 ds_read_b32 + 8 v_perm of a word-packed patch, which had made this kernel
//     LDS-bandwidth bound (4 SIMDs x 24 LDS cycles per 96 MFMA cycles).
// Rows of 32 channels are 64-byte chunks; a fragment read touches 4 consecutive patch columns of one chunk, so the
// chunk index is XOR-swizzled with the patch COLUMN (invariant under row steps): 4 columns x 64 B tile the 64 banks.
// ---------------------------------------------------------------------------------------------
// the 1- and 2-slot 4-wave forms (conv1 16 -> 32 channels: 39 KB of LDS) are pinned to 128 registers so that FOUR
// workgroups share a CU: 0.753 (three, 136 registers) -> 0.651 ms, 4.9 TB/s
#define W3_WPE(MAXS, NW) ((MAXS) <= 2 && (NW) == 4 ? 4 : 2)
// (this kernel calls nothing from wgrad_tiles.h: with any one of its pieces <9, 4, false, 0> spills more -- 406 -> 414
//  VGPRs with the tile decode or the coefficients, 664 -> 780 B of scratch with the K step -- and <2, 8, *, 1> changes
//  occupancy 3 -> 4; profiles/wgrad_tiles.json)
template <int MAXS, int NW, bool BS, int ABF>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(W3_WPE(MAXS, NW)))) void wgrad3_kernel(const WgradParams P) {
  constexpr int NTHR = NW * 64;
  const BsedWgradDesc& p = P.d;
  extern __shared__ __align__(16) uint32_t smw[];
  const int CC = P.CC;
  const int cz0 = blockIdx.z * CC;
  const int DYW = 32 * P.ntw;
  w3_lds_u16* Xh = (w3_lds_u16*)smw;               // [PP][CC] bf16, chunk-swizzled
  w3_lds_u16* Xl = Xh + P.PP * CC;
  w3_lds_u16* DYh = Xh + 2 * P.dy_off;             // [128][DYW] bf16, chunk-swizzled
  w3_lds_u16* DYl = DYh + IG_TILE_M * DYW;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.y * DYW;
  const int PW = P.PW;
  const int ntap_items = P.pack2 ? (p.ntaps + 1) / 2 : p.ntaps;
  const int nitems = ntap_items * P.nct * P.ntw;
  // transposing read: lane 16g + 4q + c4 supplies the address of row (position) q, columns 4*c4 .. 4*c4+3 of its
  // 16-lane group's 4 x 16 block and receives column (lane & 15), rows 0..3 -- the operand layout of v_mfma_32x32x16
  // (row / column = lane & 31 = 16 * (g & 1) + block column, k = 8 * (lane >> 5) + 4 * read + block row)
  const int gq = (lane >> 2) & 3, gc = 4 * (lane & 3), gh = (lane >> 4) & 1;

  constexpr int NB_ = BS ? 1 : MAXS;
  const uint32_t xh0 = (uint32_t)(uintptr_t)Xh, dh0 = (uint32_t)(uintptr_t)DYh;
  const uint32_t xlo = 2 * P.PP * CC, dlo = 2 * IG_TILE_M * DYW;  // byte distance hi plane -> lo plane
  uint32_t xa[MAXS][2], xb[NB_][2];
  bool valid[MAXS];
  f32x16 acc[MAXS];
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    const int it = wave + NW * s;
    valid[s] = it < nitems;
    const int cit = valid[s] ? it % P.nct : 0, rr = valid[s] ? it / P.nct : 0;
    const int nt = rr % P.ntw, tap = rr / P.ntw;
    int tp = tap, col = 16 * gh + gc;
    if (P.pack2) {
      // rows 0..15 of the tile: tap 2*tap, rows 16..31: tap 2*tap+1 (channels 16..31 of the staged patch are zero,
      // which is what the upper rows read when the second tap does not exist)
      const int tb = 2 * tap + 1;
      tp = 2 * tap;
      if (gh && tb < p.ntaps) { tp = tb; col = gc; }
    }
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
      const int mk = 8 * lh + 4 * rd + gq;
      const int pr = (mk >> P.lgTW) + p.hh + p.dh[tp], pc = (mk & (p.TW - 1)) + p.hw + p.dw[tp];
      xa[s][rd] = xh0 + 2 * ((pr * PW + pc) * CC + (w3_chunk(cit, pc, P.nct) << 5) + col);
      if (!BS || s == 0) xb[BS ? 0 : s][rd] = dh0 + 2 * (mk * DYW + (w3_chunk(nt, mk, P.ntw) << 5) + 16 * gh + gc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
  }
  // BS: all of a wave's items sit on one dy tile (the wave stride NW is a multiple of channel tiles x dy tiles), so
  // its fragment is read once per K step
  const uint32_t kstep = 2 * (16 >> P.lgTW) * PW * CC;  // bytes; 16 positions = (16 / TW) tile rows (TW <= 16)
  const uint32_t bstep = 2 * 16 * DYW;
  // the fused input affine (BN apply of the previous layer): a thread's elements all sit in one channel quad, because
  // the thread count is a multiple of the quads per position -- loaded once, not once per element per tile
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p.a_scale && cz0 + 4 * (tid & ((1 << P.lgc4) - 1)) < p.CIN) {
    sc = *reinterpret_cast<const float4*>(p.a_scale + cz0 + 4 * (tid & ((1 << P.lgc4) - 1)));
    sh = *reinterpret_cast<const float4*>(p.a_shift + cz0 + 4 * (tid & ((1 << P.lgc4) - 1)));
  }
  // BatchNorm backward on load (bn_y set): d_y = A g + B y + (C - B mean) for the thread's own channel quad of dy
  float4 cA = make_float4(1.f, 1.f, 1.f, 1.f), cB = make_float4(0.f, 0.f, 0.f, 0.f), cC = cB;
  if (p.bn_y && n0 + 4 * (tid & (8 * P.ntw - 1)) < p.N) {
    const int cn = n0 + 4 * (tid & (8 * P.ntw - 1));
    cA = *reinterpret_cast<const float4*>(p.bn_coef + cn);
    cB = *reinterpret_cast<const float4*>(p.bn_coef + p.N + cn);
    const float4 c2 = *reinterpret_cast<const float4*>(p.bn_coef + 2 * p.N + cn);
    const float4 mu = *reinterpret_cast<const float4*>(p.bn_mean + cn);
    cC = make_float4(fmaf(-cB.x, mu.x, c2.x), fmaf(-cB.y, mu.y, c2.y), fmaf(-cB.z, mu.z, c2.z), fmaf(-cB.w, mu.w, c2.w));
  }

  for (int tile0 = blockIdx.x; tile0 < P.ntiles; tile0 += gridDim.x) {
    int tile = tile0;
    const int tw_i = tile % p.tilesW; tile /= p.tilesW;
    const int th_i = tile % p.tilesH;
    const int nb = tile / p.tilesH;
    const int th0 = th_i * p.TH, tw0 = tw_i * p.TW;
    const float* inb = p.in + (size_t)nb * p.H * p.W * p.in_pitch;
    const float* dyb = p.dy + (size_t)nb * p.H * p.W * p.dy_pitch;
    __syncthreads();
    // Both tiles arrive as coalesced float4 rows and stay position-major.  The loads of a round are all issued before
    // any is consumed: the staging phase is a chain of global-load latencies, so fewer, wider rounds is what counts
    // (a 180-position x 64-channel patch is 12 float4 per thread: two rounds of 6 instead of three of 4).
    constexpr int UX = 6, UD = 8;
    const int c4n = 1 << P.lgc4;
    const int x_total = P.PP * c4n;
    for (int e0 = tid; e0 < x_total; e0 += UX * NTHR) {
      float4 v[UX];
      bool okv[UX];
      int ov[UX];
#pragma unroll
      for (int u = 0; u < UX; ++u) {
        const int e = e0 + u * NTHR;
        const int c4 = e & (c4n - 1), pos = e >> P.lgc4;
        const int pr = (pos * P.pw_magic) >> 20, pc = pos - pr * PW;
        const int gh_ = th0 - p.hh + pr, gw = tw0 - p.hw + pc;
        const int cg = cz0 + 4 * c4;
        ov[u] = pos * CC + (w3_chunk(c4 >> 3, pc, P.nct) << 5) + 4 * (c4 & 7);
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        okv[u] = e < x_total && gh_ >= 0 && gh_ < p.H && gw >= 0 && gw < p.W && cg < p.CIN;
        if (okv[u]) v[u] = w3_ld4<ABF>(p.in, inb + ((size_t)gh_ * p.W + gw) * p.in_pitch + cg);
      }
#pragma unroll
      for (int u = 0; u < UX; ++u) {
        const int e = e0 + u * NTHR;
        if (e < x_total) {
          if (p.a_scale && okv[u]) {
            v[u].x = fmaf(v[u].x, sc.x, sh.x); v[u].y = fmaf(v[u].y, sc.y, sh.y);
            v[u].z = fmaf(v[u].z, sc.z, sh.z); v[u].w = fmaf(v[u].w, sc.w, sh.w);
          }
          w3_store4<ABF>(Xh, Xl, ov[u], v[u]);
        }
      }
    }
    const int n4n = 8 * P.ntw, lgn4 = P.ntw == 4 ? 5 : (P.ntw == 2 ? 4 : 3);
    const int d_total = IG_TILE_M * n4n;
    for (int e0 = tid; e0 < d_total; e0 += UD * NTHR) {
      float4 v[UD];
#pragma unroll
      for (int u = 0; u < UD; ++u) {
        const int e = e0 + u * NTHR;
        const int n4 = e & (n4n - 1), mm = e >> lgn4;
        const int gh_ = th0 + (mm >> P.lgTW), gw = tw0 + (mm & (p.TW - 1));
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < d_total && gh_ < p.H && gw < p.W && n0 + 4 * n4 < p.N) {
          const size_t o = ((size_t)nb * p.H * p.W + (size_t)gh_ * p.W + gw) * p.dy_pitch + n0 + 4 * n4;
          v[u] = w3_ld4<ABF>(p.dy, p.dy + o);
          if (p.bn_y) {
            // BatchNorm backward on load (NTHR is a multiple of n4n: the channel quad is the thread's own, cA/cB/cC)
            const float4 yv = w3_ld4<ABF>(p.bn_y, p.bn_y + o);
            v[u].x = fmaf(cA.x, v[u].x, fmaf(cB.x, yv.x, cC.x)); v[u].y = fmaf(cA.y, v[u].y, fmaf(cB.y, yv.y, cC.y));
            v[u].z = fmaf(cA.z, v[u].z, fmaf(cB.z, yv.z, cC.z)); v[u].w = fmaf(cA.w, v[u].w, fmaf(cB.w, yv.w, cC.w));
            if (p.dy_out && blockIdx.z == 0) w3_st4<ABF>(p.dy_out, p.dy_out + o, v[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UD; ++u) {
        const int e = e0 + u * NTHR;
        const int n4 = e & (n4n - 1), mm = e >> lgn4;
        if (e < d_total) w3_store4<ABF>(DYh, DYl, mm * DYW + (w3_chunk(n4 >> 3, mm, P.ntw) << 5) + 4 * (n4 & 7), v[u]);
      }
    }
    __syncthreads();
    // slots go through the matrix cores in small groups: the fragments of group g+1 are requested before the MFMAs of
    // group g issue (sched_barrier pins that order), so one LDS latency is exposed per K step, not one per group,
    // and at most two groups of fragments are live (the 9-slot form has 144 accumulator registers)
    constexpr int SG = MAXS > 5 ? 2 : 3, NG = (MAXS + SG - 1) / SG;
    constexpr int SB = BS ? 1 : SG;
    uint32_t ko = 0, kb = 0;
#pragma unroll 1
    for (int kp = 0; kp < IG_TILE_M; kp += 16, ko += kstep, kb += bstep) {
      w3_bf16x8 ah[2][SG], al[2][SG], bh[2][SB], bl[2][SB];
#pragma unroll
      for (int g = 0; g <= NG; ++g) {
        if (g < NG) {
#pragma unroll
          for (int j = 0; j < SG; ++j) {
            const int sl = g * SG + j;
            if (sl < MAXS) {
              ah[g & 1][j] = w3_frag(xa[sl][0] + ko, xa[sl][1] + ko);
              al[g & 1][j] = w3_frag(xa[sl][0] + ko + xlo, xa[sl][1] + ko + xlo);
              if (!BS || sl == 0) {
                bh[g & 1][BS ? 0 : j] = w3_frag(xb[BS ? 0 : sl][0] + kb, xb[BS ? 0 : sl][1] + kb);
                bl[g & 1][BS ? 0 : j] = w3_frag(xb[BS ? 0 : sl][0] + kb + dlo, xb[BS ? 0 : sl][1] + kb + dlo);
              }
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (g > 0) {
#pragma unroll
          for (int j = 0; j < SG; ++j) {
            const int sl = (g - 1) * SG + j;
            if (sl < MAXS) {
              const w3_bf16x8 b_hi = BS ? bh[0][0] : bh[(g - 1) & 1][BS ? 0 : j];
              const w3_bf16x8 b_lo = BS ? bl[0][0] : bl[(g - 1) & 1][BS ? 0 : j];
              acc[sl] = w3_mfma<ABF>(ah[(g - 1) & 1][j], al[(g - 1) & 1][j], b_hi, b_lo, acc[sl]);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  const int NPo = gridDim.y * DYW;
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    if (valid[s]) {
      const int it = wave + NW * s;
      const int cit = it % P.nct, rr = it / P.nct;
      const int nt = rr % P.ntw, tap = rr / P.ntw;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int ci = cz0 + cit * 32 + crow(r, lh), tp = tap;
        if (P.pack2) {
          const int row = crow(r, lh);
          tp = 2 * tap + (row >> 4);
          ci = row & 15;
          if (tp >= p.ntaps) continue;
        }
        p.part[(((size_t)blockIdx.x * p.ntaps + tp) * p.CINP + ci) * NPo + n0 + nt * 32 + li] = acc[s][r];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// 1-tap weight gradient (GLU linears, GRU input / recurrent weights) as a STREAMING kernel.
//
// dW (CIN x N) = sum over positions of in^T dy reads each activation byte once and does 2 N (or 2 CIN) FLOP per byte:
// a read-only, HBM-bound pass (a tuned read-only stream gets 6.3 TB/s on this part, tools/probe/hbm_read_probe.hip).
// wgrad3_kernel runs these shapes with ONE 128-position tile in 128 KB of LDS: a single workgroup per CU whose loads,
// operand split and MFMAs follow each other -- nothing is in flight while it computes (3.0-3.2 TB/s on the large shapes,
// 1.1-1.7 on the GRU ones).  Here a workgroup (8 waves, one per CU) owns a 128 x 128 slab of dW and streams 64-position
// tiles through TWO LDS stages (bf16 hi / lo planes, 64 KB each) with the global loads running TWO tiles ahead in
// registers: while tile t is in the matrix cores, tile t+1 waits in registers or is being split into the other stage
// and tile t+2 is in flight -- 64-128 KB of loads outstanding per CU at any time, one barrier per tile.
// Operand images, swizzle and the transposing fragment reads are those of wgrad3_kernel (results are bit-identical:
// same products, same accumulation order per slab; only the tile boundaries of the partial slabs differ).
// ---------------------------------------------------------------------------------------------
#define W1_TP 64
#define W1_THREADS 512
#define W1_PLANE (W1_TP * 128 * 2)   // bytes of one bf16 plane of a stage
#define W1_STAGE (4 * W1_PLANE)      // Xh | Xl | DYh | DYl

struct W1Set { float4 x[4], d[4]; };

template <bool SHIFT, int ABF>
__global__ __launch_bounds__(W1_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void wgrad1_kernel(const WgradParams P) {
  const BsedWgradDesc& p = P.d;
  extern __shared__ __align__(16) uint32_t smw[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int cz0 = blockIdx.z * 128, n0 = blockIdx.y * 128;
  const long M = (long)p.NB * p.H * p.W;
  const int ntile = (int)((M + W1_TP - 1) / W1_TP);
  // this wave's two 32 x 32 blocks: input-channel chunk cit, dy tiles nt0 and nt0 + 2
  const int cit = wave & 3, nt0 = wave >> 2;
  const int gq = (lane >> 2) & 3, gc = 4 * (lane & 3), gh = (lane >> 4) & 1;
  const uint32_t base = (uint32_t)(uintptr_t)smw;
  uint32_t xa[2], xb[2][2];
#pragma unroll
  for (int rd = 0; rd < 2; ++rd) {
    const int mk = 8 * lh + 4 * rd + gq;
    xa[rd] = base + 2 * (mk * 128 + (w3_chunk(cit, mk, 4) << 5) + 16 * gh + gc);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      xb[s][rd] = base + 2 * W1_PLANE + 2 * (mk * 128 + (w3_chunk(nt0 + 2 * s, mk, 4) << 5) + 16 * gh + gc);
  }
  f32x16 acc[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;

  // loads: thread -> channel quad c4 (constant) of positions p0 + 16 u
  const int c4 = tid & 31, p0 = tid >> 5;
  const bool xok = cz0 + 4 * c4 < p.CIN, dok = n0 + 4 * c4 < p.N;
  const float* xsrc = p.in + cz0 + 4 * (xok ? c4 : 0);
  const float* dsrc = p.dy + n0 + 4 * (dok ? c4 : 0);
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p.a_scale && xok) {
    sc = *reinterpret_cast<const float4*>(p.a_scale + cz0 + 4 * c4);
    sh = *reinterpret_cast<const float4*>(p.a_shift + cz0 + 4 * c4);
  }
  const int shift = SHIFT ? p.dh[0] * p.W + p.dw[0] : 0;
  const int so = p0 * 128 + (w3_chunk(c4 >> 3, p0, 4) << 5) + 4 * (c4 & 7);   // ushorts; + 16 u * 128 per u
  w3_lds_u16* lds = (w3_lds_u16*)smw;

  uint32_t xmask = 0, dmask = 0;   // validity bits of the set being loaded are recomputed at convert time
  auto issue = [&](int tile, W1Set& S) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long m = (long)tile * W1_TP + p0 + 16 * u;
      const long mc = m < M ? m : M - 1;   // clamped: no branch around the loads, idle rows are zeroed at convert time
      long ms = mc;
      if (SHIFT) {
        ms = mc + shift;
        ms = ms < 0 ? 0 : (ms >= M ? M - 1 : ms);
      }
      S.x[u] = w3_ld4<ABF>(p.in, xsrc + (size_t)ms * p.in_pitch);
      S.d[u] = w3_ld4<ABF>(p.dy, dsrc + (size_t)mc * p.dy_pitch);
    }
  };
  auto convert = [&](int tile, const W1Set& S, int stage) {
    w3_lds_u16* xh = lds + stage * (W1_STAGE / 2);
    w3_lds_u16* xl = xh + W1_PLANE / 2;
    w3_lds_u16* dh_ = xh + W1_PLANE;
    w3_lds_u16* dl = dh_ + W1_PLANE / 2;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long m = (long)tile * W1_TP + p0 + 16 * u;
      bool okx = m < M && xok;
      if (SHIFT) {
        const int rem = (int)(m % ((long)p.H * p.W));
        const int h = rem / p.W + p.dh[0], w = rem % p.W + p.dw[0];
        okx = okx && h >= 0 && h < p.H && w >= 0 && w < p.W;
      }
      const bool okd = m < M && dok;
      float4 v = S.x[u];
      v.x = okx ? fmaf(v.x, sc.x, sh.x) : 0.f; v.y = okx ? fmaf(v.y, sc.y, sh.y) : 0.f;
      v.z = okx ? fmaf(v.z, sc.z, sh.z) : 0.f; v.w = okx ? fmaf(v.w, sc.w, sh.w) : 0.f;
      w3_store4<ABF>(xh, xl, so + 16 * u * 128, v);
      float4 g = S.d[u];
      g.x = okd ? g.x : 0.f; g.y = okd ? g.y : 0.f; g.z = okd ? g.z : 0.f; g.w = okd ? g.w : 0.f;
      w3_store4<ABF>(dh_, dl, so + 16 * u * 128, g);
    }
  };
  auto mma = [&](int stage) {
    const uint32_t so_ = stage * W1_STAGE;
#pragma unroll
    for (int k = 0; k < W1_TP / 16; ++k) {
      const uint32_t ko = so_ + k * 16 * 128 * 2;
      const w3_bf16x8 ah = w3_frag(xa[0] + ko, xa[1] + ko);
      const w3_bf16x8 al = w3_frag(xa[0] + ko + W1_PLANE, xa[1] + ko + W1_PLANE);
      w3_bf16x8 bh[2], bl[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bh[s] = w3_frag(xb[s][0] + ko, xb[s][1] + ko);
        bl[s] = w3_frag(xb[s][0] + ko + W1_PLANE, xb[s][1] + ko + W1_PLANE);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        acc[s] = w3_mfma<ABF>(ah, al, bh[s], bl[s], acc[s]);
      }
    }
  };
  (void)xmask; (void)dmask;

  // tiles of this workgroup: t0, t0 + G, ...   (n of them; tile indices past the end load clamped rows that convert
  // zeroes and nobody multiplies)
  const int t0 = blockIdx.x, G = gridDim.x;
  const int n = t0 < ntile ? (ntile - t0 + G - 1) / G : 0;
  W1Set A, B;
  if (n > 0) {
    issue(t0, A);
    issue(t0 + G, B);
    convert(t0, A, 0);
    __syncthreads();
    for (int i = 0; i < n; i += 2) {
      // even step: tile i in stage 0; A is free, B holds tile i + 1
      issue(t0 + (i + 2) * G, A);
      mma(0);
      convert(t0 + (i + 1) * G, B, 1);
      __syncthreads();
      if (i + 1 >= n) break;
      // odd step: tile i + 1 in stage 1; B is free, A holds tile i + 2
      issue(t0 + (i + 3) * G, B);
      mma(1);
      convert(t0 + (i + 2) * G, A, 0);
      __syncthreads();
    }
  }
  const int NPo = gridDim.y * 128;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = cz0 + cit * 32 + crow(r, lh);
      p.part[((size_t)blockIdx.x * p.CINP + ci) * NPo + n0 + (nt0 + 2 * s) * 32 + li] = acc[s][r];
    }
}

// ---------------------------------------------------------------------------------------------
// Producer / consumer form of the bf16x3 weight gradient for the multi-tap convolutions: ONE 8-wave workgroup per CU
// with two LDS tile buffers.  Waves 0-3 (one per SIMD) only run the MFMA loop of tile t; waves 4-7 (one per SIMD) only
// load, split and write tile t+1 into the other buffer; one barrier per tile hands the buffers over.  In
// wgrad3_kernel the two co-resident workgroups run in phase (stage, then compute), so the staging time adds to the
// MFMA time; here a SIMD always has one wave of each kind and the staging hides behind the matrix cores.
// Same tiles, same products, same accumulation order as wgrad3_kernel.
// ---------------------------------------------------------------------------------------------
#define W3P_UX 13  // float4 of the activation patch per producer thread (256 threads): PP * CC <= 13312 elements
#define W3P_UD 8   // float4 of the dy tile per producer thread: 128 positions x 64 channels

// GEO > 0: the tile geometry of one of the network's layer shapes is a compile-time constant: every LDS offset of the
// MFMA waves' K loop becomes an instruction immediate and the loop is unrolled (20 instead of 640 v_add per tile and no
// spills: -7 %).  GEO = 0 keeps everything at run time (any other shape).
struct W3Geo { int CC, lgTW, PW, PP, ntw; };
__host__ __device__ constexpr W3Geo w3_geo(int g) {
  return g == 1 ? W3Geo{64, 4, 18, 180, 2}     // 64 -> 128 channels on the 216 x 16 map
       : g == 2 ? W3Geo{64, 3, 10, 180, 2}     // 128 -> 128, 216 x 8
       : g == 3 ? W3Geo{32, 4, 18, 180, 2}     // 32 -> 64, 216 x 32
       : g == 4 ? W3Geo{64, 2, 6, 204, 1}      // 128 -> 128, 216 x 4
       : g == 5 ? W3Geo{32, 1, 4, 264, 2}      // 128 -> 128, 216 x 2
       : g == 6 ? W3Geo{32, 4, 18, 180, 1}     // 16 -> 32 (two taps per MFMA tile; also 32 -> 32), 432 x 64
                : W3Geo{0, 0, 0, 0, 0};
}
#define W3_NGEO 6

template <int MAXS, int GEO, int ABF>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void wgrad3p_kernel(const WgradParams P) {
  constexpr int NTHR = 256, NW = 4, UX = W3P_UX, UD = W3P_UD;
  const BsedWgradDesc& p = P.d;
  extern __shared__ __align__(16) uint32_t smw[];
  const int CC = P.CC;
  const int cz0 = blockIdx.z * CC;
  const int DYW = 32 * P.ntw;
  w3_lds_u16* Xh = (w3_lds_u16*)smw;
  w3_lds_u16* Xl = Xh + P.PP * CC;
  w3_lds_u16* DYh = Xh + 2 * P.dy_off;
  w3_lds_u16* DYl = DYh + IG_TILE_M * DYW;
  const int buf_u16 = 2 * P.dy_off + 2 * IG_TILE_M * DYW;  // ushorts per tile buffer
  const int n0 = blockIdx.y * DYW;
  const int PW = P.PW;

  if (threadIdx.x >= NTHR) {
    // ------------------------------------------------------------------ producer waves
    const int tid = threadIdx.x - NTHR;
    const int c4n = 1 << P.lgc4;
    const int x_total = P.PP * c4n;
    const int n4n = 8 * P.ntw, lgn4 = P.ntw == 4 ? 5 : (P.ntw == 2 ? 4 : 3);
    const int d_total = IG_TILE_M * n4n;
    // the fused input affine (BN apply of the previous layer): a thread's elements all sit in one channel quad
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.a_scale && cz0 + 4 * (tid & (c4n - 1)) < p.CIN) {
      sc = *reinterpret_cast<const float4*>(p.a_scale + cz0 + 4 * (tid & (c4n - 1)));
      sh = *reinterpret_cast<const float4*>(p.a_shift + cz0 + 4 * (tid & (c4n - 1)));
    }
    // BatchNorm backward on load: d_y = A g + B y + (C - B mean); a thread's dy elements all sit in one channel quad
    const bool bnb = p.bn_y != nullptr;
    const bool dy_store = bnb && p.dy_out != nullptr && blockIdx.z == 0;   // one CIN chunk writes d_y out
    W3Bn bn = w3_bn_identity();
    if (bnb) bn = w3_bn_coef(p, n0 + 4 * (tid & (n4n - 1)) < p.N ? n0 + 4 * (tid & (n4n - 1)) : 0);
    const float4 cA = bn.A, cB = bn.B, cC = bn.C;
    if constexpr (ABF) {
      // ---- bf16 activations: 16-byte pieces of EIGHT channels (half the load / store / LDS-write instructions of the
      // four-channel pieces), no hi / lo split: a piece goes to the hi plane as it arrives
      constexpr int UX8 = (UX + 1) / 2, UD8 = UD / 2;
      const int lgc8 = P.lgc4 - 1, c8n = 1 << lgc8, x_total8 = P.PP * c8n;
      const int n8n = 4 * P.ntw, lgn8 = lgn4 - 1, d_total8 = IG_TILE_M * n8n;
      // (same software pipeline and straight-line period as the fp32 producers below -- see the comment there)
      constexpr W3Geo Gm = w3_geo(GEO);
      const int x_tot = GEO ? Gm.PP * (Gm.CC / 8) : x_total8, d_tot = GEO ? IG_TILE_M * 4 * Gm.ntw : d_total8;
      const int gW = p.W, gH = p.H;
      const bool xch_ok = cz0 + 8 * (tid & (c8n - 1)) < p.CIN, dch_ok = n0 + 8 * (tid & (n8n - 1)) < p.N;
      const int xcoff = xch_ok ? cz0 + 8 * (tid & (c8n - 1)) : 0, dcoff = dch_ok ? n0 + 8 * (tid & (n8n - 1)) : 0;
      // eight channels: the coefficients of two quads (dcoff is quad 0's where the piece lies beyond N)
      W3Bn b0 = w3_bn_identity(), b1 = b0;
      if (bnb) { b0 = w3_bn_coef(p, dcoff); b1 = w3_bn_coef(p, dcoff + 4); }
      const float cA8[8] = {b0.A.x, b0.A.y, b0.A.z, b0.A.w, b1.A.x, b1.A.y, b1.A.z, b1.A.w};
      const float cB8[8] = {b0.B.x, b0.B.y, b0.B.z, b0.B.w, b1.B.x, b1.B.y, b1.B.z, b1.B.w};
      const float cC8[8] = {b0.C.x, b0.C.y, b0.C.z, b0.C.w, b1.C.x, b1.C.y, b1.C.z, b1.C.w};
      float sc8[8], sh8[8];
      const bool affine = p.a_scale != nullptr;
#pragma unroll
      for (int q = 0; q < 8; ++q) { sc8[q] = 1.f; sh8[q] = 0.f; }
      if (affine && xch_ok) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          sc8[q] = p.a_scale[xcoff + q];
          sh8[q] = p.a_shift[xcoff + q];
        }
      }
      int xo[UX8], xrc[UX8], dyo[UD8], drc[UD8];
#pragma unroll
      for (int u = 0; u < UX8; ++u) {
        const int e = tid + u * NTHR;
        const int c8 = e & (c8n - 1), pos = e >> lgc8;
        const int pr = GEO ? pos / (GEO ? Gm.PW : 1) : (pos * P.pw_magic) >> 20, pc = pos - pr * PW;
        xo[u] = pos * CC + (w3_chunk(c8 >> 2, pc, P.nct) << 5) + 8 * (c8 & 3);
        xrc[u] = (e < x_tot && xch_ok) ? ((pr - p.hh) << 16) | ((pc - p.hw) & 0xffff) : (0x4000 << 16);
      }
#pragma unroll
      for (int u = 0; u < UD8; ++u) {
        const int e = tid + u * NTHR;
        const int n8 = e & (n8n - 1), mm = e >> lgn8;
        const int r = mm >> P.lgTW, c = mm & (p.TW - 1);
        dyo[u] = mm * DYW + (w3_chunk(n8 >> 2, mm, P.ntw) << 5) + 8 * (n8 & 3);
        drc[u] = (e < d_tot && dch_ok) ? (r << 16) | c : (0x4000 << 16);
      }
      const unsigned short* in16 = reinterpret_cast<const unsigned short*>(p.in);
      const unsigned short* dy16 = reinterpret_cast<const unsigned short*>(p.dy);
      const unsigned short* y16 = reinterpret_cast<const unsigned short*>(p.bn_y);
      unsigned short* out16 = reinterpret_cast<unsigned short*>(p.dy_out);
      auto unpack8 = [](const bsed_u32x4& r, float* v) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { v[2 * q] = __uint_as_float(r[q] << 16); v[2 * q + 1] = __uint_as_float(r[q] & 0xFFFF0000u); }
      };
      auto pack8 = [](const float* v) {
        bsed_u32x4 r;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x2 t = {v[2 * q], v[2 * q + 1]};
          r[q] = __builtin_bit_cast(uint32_t, __builtin_convertvector(t, bsed_bf16x2));
        }
        return r;
      };
      auto x_at = [&](int u, const W3Tile& g, bool& ok) {
        const int gh_ = g.th0 + (xrc[u] >> 16), gw = g.tw0 + (int)(short)(xrc[u] & 0xffff);
        ok = (unsigned)gh_ < (unsigned)gH && (unsigned)gw < (unsigned)gW;
        return (uint32_t)((min(max(gh_, 0), gH - 1) * gW + min(max(gw, 0), gW - 1)) * p.in_pitch + xcoff) << 1;
      };
      auto d_at = [&](int u, const W3Tile& g, bool& ok) {
        const int gh_ = g.th0 + (drc[u] >> 16), gw = g.tw0 + (drc[u] & 0xffff);
        ok = gh_ < gH && gw < gW;
        return (uint32_t)((min(gh_, gH - 1) * gW + min(gw, gW - 1)) * p.dy_pitch + dcoff) << 1;
      };
      auto ld16 = [](const unsigned short* base, size_t img, uint32_t byte_off) {
        return *reinterpret_cast<const bsed_u32x4*>(reinterpret_cast<const char*>(base + img) + byte_off);
      };
      const bsed_u32x4 zero = {0u, 0u, 0u, 0u};
      auto produce = [&](auto bnb_c, auto store_c, auto aff_c) {
        constexpr bool BNB = decltype(bnb_c)::value, STORE = decltype(store_c)::value, AFF = decltype(aff_c)::value;
        bsed_u32x4 vx[UX8], vd[UD8], vy[BNB ? UD8 : 1];
        int tile = blockIdx.x, buf = 0;
        if (tile >= P.ntiles) return;
        W3Tile gc = w3_tile(p, tile);
#pragma unroll
        for (int u = 0; u < UD8; ++u) {
          if (GEO && u * NTHR >= d_tot) continue;
          bool ok;
          const uint32_t o = d_at(u, gc, ok);
          vd[u] = ld16(dy16, gc.dy_img, o);
          if (BNB) vy[u] = ld16(y16, gc.dy_img, o);
        }
#pragma unroll
        for (int u = 0; u < UX8; ++u) {
          if (GEO && u * NTHR >= x_tot) continue;
          bool ok;
          vx[u] = ld16(in16, gc.in_img, x_at(u, gc, ok));
        }
        for (; tile < P.ntiles; buf ^= 1) {
          const int nxt = tile + gridDim.x;
          const W3Tile gn = w3_tile(p, nxt < P.ntiles ? nxt : tile);
          const int bo = buf * buf_u16;
#pragma unroll
          for (int u = 0; u < UD8; ++u) {
            if (GEO && u * NTHR >= d_tot) continue;
            bool ok, okn;
            const uint32_t o = d_at(u, gc, ok);
            bsed_u32x4 v = vd[u];
            if (BNB) {
              float g8[8], y8[8];
              unpack8(v, g8); unpack8(vy[u], y8);
#pragma unroll
              for (int q = 0; q < 8; ++q) g8[q] = fmaf(cA8[q], g8[q], fmaf(cB8[q], y8[q], cC8[q]));
              v = pack8(g8);
              // unconditional (see the fp32 producers): a clamped piece stores the value its position's owner stores
              if (STORE) *reinterpret_cast<bsed_u32x4*>(reinterpret_cast<char*>(out16 + gc.dy_img) + o) = v;
            }
            if (!ok) v = zero;
            if (tid + u * NTHR < d_tot)
              *reinterpret_cast<__attribute__((address_space(3))) bsed_u32x4*>(DYh + bo + dyo[u]) = v;
            const uint32_t on = d_at(u, gn, okn);
            vd[u] = ld16(dy16, gn.dy_img, on);
            if (BNB) vy[u] = ld16(y16, gn.dy_img, on);
          }
#pragma unroll
          for (int u = 0; u < UX8; ++u) {
            if (GEO && u * NTHR >= x_tot) continue;
            bool ok, okn;
            (void)x_at(u, gc, ok);
            bsed_u32x4 v = vx[u];
            if (AFF) {
              float x8[8];
              unpack8(v, x8);
#pragma unroll
              for (int q = 0; q < 8; ++q) x8[q] = fmaf(x8[q], sc8[q], sh8[q]);
              v = pack8(x8);
            }
            if (!ok) v = zero;
            if (tid + u * NTHR < x_tot)
              *reinterpret_cast<__attribute__((address_space(3))) bsed_u32x4*>(Xh + bo + xo[u]) = v;
            vx[u] = ld16(in16, gn.in_img, x_at(u, gn, okn));
          }
          gc = gn; tile = nxt;
          __syncthreads();
        }
      };
      using T_ = std::true_type; using F_ = std::false_type;
      if (!bnb) { if (affine) produce(F_{}, F_{}, T_{}); else produce(F_{}, F_{}, F_{}); }
      else if (!dy_store) { if (affine) produce(T_{}, F_{}, T_{}); else produce(T_{}, F_{}, F_{}); }
      else { if (affine) produce(T_{}, T_{}, T_{}); else produce(T_{}, T_{}, F_{}); }
      __syncthreads();  // pairs with the consumers' barrier after their last tile
      return;
    }
    // ---- fp32 activations.  Tile-invariant element geometry: LDS offset and patch row / col of each piece.  A thread's
    // pieces all sit in one channel quad (256 threads are a multiple of the quads per position).
    //
    // SOFTWARE PIPELINE over tiles: the registers of a piece are refilled with the NEXT tile's piece right after the
    // piece has been split into LDS, so a tile's loads have a whole tile period (one MFMA pass of the consumers) to
    // arrive.  (Loading, waiting and converting inside one period took longer than the consumers' MFMA pass: the matrix
    // cores idled behind the producers.)  Everything between two barriers is STRAIGHT-LINE code -- rows / columns outside
    // the map are clamped for the address and zeroed at conversion, the last period re-requests its own tile -- because
    // hipcc's wait-count insertion falls back to vmcnt(0) as soon as a load sits inside a branch, which would serialise
    // the refills against the conversions.
    constexpr W3Geo Gm = w3_geo(GEO);
    const int x_tot = GEO ? Gm.PP * (Gm.CC / 4) : x_total, d_tot = GEO ? IG_TILE_M * 8 * Gm.ntw : d_total;
    const int gW = p.W, gH = p.H;
    int xo[UX], xrc[UX], dyo[UD], drc[UD];
    const bool xch_ok = cz0 + 4 * (tid & (c4n - 1)) < p.CIN, dch_ok = n0 + 4 * (tid & (n4n - 1)) < p.N;
    const int xcoff = xch_ok ? cz0 + 4 * (tid & (c4n - 1)) : 0, dcoff = dch_ok ? n0 + 4 * (tid & (n4n - 1)) : 0;
#pragma unroll
    for (int u = 0; u < UX; ++u) {
      const int e = tid + u * NTHR;
      const int c4 = e & (c4n - 1), pos = e >> P.lgc4;
      const int pr = GEO ? pos / (GEO ? Gm.PW : 1) : (pos * P.pw_magic) >> 20, pc = pos - pr * PW;
      xo[u] = pos * CC + (w3_chunk(c4 >> 3, pc, P.nct) << 5) + 4 * (c4 & 7);
      xrc[u] = (e < x_tot && xch_ok) ? ((pr - p.hh) << 16) | ((pc - p.hw) & 0xffff) : (0x4000 << 16);
    }
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      const int e = tid + u * NTHR;
      const int n4 = e & (n4n - 1), mm = e >> lgn4;
      const int r = mm >> P.lgTW, c = mm & (p.TW - 1);
      dyo[u] = mm * DYW + (w3_chunk(n4 >> 3, mm, P.ntw) << 5) + 4 * (n4 & 7);
      drc[u] = (e < d_tot && dch_ok) ? (r << 16) | c : (0x4000 << 16);
    }
    // byte offset of a piece inside its image (clamped into the map) and whether the piece is inside the map
    auto x_at = [&](int u, const W3Tile& g, bool& ok) {
      const int gh_ = g.th0 + (xrc[u] >> 16), gw = g.tw0 + (int)(short)(xrc[u] & 0xffff);
      ok = (unsigned)gh_ < (unsigned)gH && (unsigned)gw < (unsigned)gW;
      return (uint32_t)((min(max(gh_, 0), gH - 1) * gW + min(max(gw, 0), gW - 1)) * p.in_pitch + xcoff) << 2;
    };
    auto d_at = [&](int u, const W3Tile& g, bool& ok) {
      const int gh_ = g.th0 + (drc[u] >> 16), gw = g.tw0 + (drc[u] & 0xffff);
      ok = gh_ < gH && gw < gW;
      return (uint32_t)((min(gh_, gH - 1) * gW + min(gw, gW - 1)) * p.dy_pitch + dcoff) << 2;
    };
    auto ld16 = [](const float* base, size_t img, uint32_t byte_off) {
      return *reinterpret_cast<const w3_f32x4*>(reinterpret_cast<const char*>(base + img) + byte_off);
    };
    auto produce = [&](auto bnb_c, auto store_c) {
      constexpr bool BNB = decltype(bnb_c)::value, STORE = decltype(store_c)::value;
      w3_f32x4 vx[UX], vd[UD], vy[BNB ? UD : 1];  // native vectors: arrays of HIP float4 structs end up in scratch
      int tile = blockIdx.x, buf = 0;
      if (tile >= P.ntiles) return;
      W3Tile gc = w3_tile(p, tile);
#pragma unroll
      for (int u = 0; u < UD; ++u) {
        if (GEO && u * NTHR >= d_tot) continue;
        bool ok;
        const uint32_t o = d_at(u, gc, ok);
        vd[u] = ld16(p.dy, gc.dy_img, o);
        if (BNB) vy[u] = ld16(p.bn_y, gc.dy_img, o);
      }
#pragma unroll
      for (int u = 0; u < UX; ++u) {
        if (GEO && u * NTHR >= x_tot) continue;
        bool ok;
        vx[u] = ld16(p.in, gc.in_img, x_at(u, gc, ok));
      }
      for (; tile < P.ntiles; buf ^= 1) {
        const int nxt = tile + gridDim.x;
        const W3Tile gn = w3_tile(p, nxt < P.ntiles ? nxt : tile);
        // (the buffer being written was last read before the previous barrier)
        const int bo = buf * buf_u16;
#pragma unroll
        for (int u = 0; u < UD; ++u) {
          if (GEO && u * NTHR >= d_tot) continue;
          bool ok, okn;
          const uint32_t o = d_at(u, gc, ok);
          w3_f32x4 v = vd[u];
          if (BNB) {
            // BatchNorm backward on load: d_y is formed here and (one CIN chunk only) written out for the dgrad
            v[0] = fmaf(cA.x, v[0], fmaf(cB.x, vy[u][0], cC.x));
            v[1] = fmaf(cA.y, v[1], fmaf(cB.y, vy[u][1], cC.y));
            v[2] = fmaf(cA.z, v[2], fmaf(cB.z, vy[u][2], cC.z));
            v[3] = fmaf(cA.w, v[3], fmaf(cB.w, vy[u][3], cC.w));
            // unconditional: a piece outside the map was loaded from the clamped position, so it carries -- and stores
            // -- exactly the value the owner of that position stores (no branch around a memory instruction)
            if (STORE) *reinterpret_cast<w3_f32x4*>(reinterpret_cast<char*>(p.dy_out + gc.dy_img) + o) = v;
          }
          const float4 w = make_float4(ok ? v[0] : 0.f, ok ? v[1] : 0.f, ok ? v[2] : 0.f, ok ? v[3] : 0.f);
          if (tid + u * NTHR < d_tot) w3_store4<ABF>(DYh, DYl, bo + dyo[u], w);
          const uint32_t on = d_at(u, gn, okn);
          vd[u] = ld16(p.dy, gn.dy_img, on);
          if (BNB) vy[u] = ld16(p.bn_y, gn.dy_img, on);
        }
#pragma unroll
        for (int u = 0; u < UX; ++u) {
          if (GEO && u * NTHR >= x_tot) continue;
          bool ok, okn;
          (void)x_at(u, gc, ok);
          const w3_f32x4 v = vx[u];
          const float4 w = make_float4(ok ? fmaf(v[0], sc.x, sh.x) : 0.f, ok ? fmaf(v[1], sc.y, sh.y) : 0.f,
                                       ok ? fmaf(v[2], sc.z, sh.z) : 0.f, ok ? fmaf(v[3], sc.w, sh.w) : 0.f);
          if (tid + u * NTHR < x_tot) w3_store4<ABF>(Xh, Xl, bo + xo[u], w);
          vx[u] = ld16(p.in, gn.in_img, x_at(u, gn, okn));
        }
        gc = gn; tile = nxt;
        __syncthreads();
      }
    };
    if (!bnb) produce(std::false_type{}, std::false_type{});
    else if (!dy_store) produce(std::true_type{}, std::false_type{});
    else produce(std::true_type{}, std::true_type{});
    __syncthreads();  // pairs with the consumers' barrier after their last tile
    return;
  }

  // -------------------------------------------------------------------- consumer waves
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int ntap_items = P.pack2 ? (p.ntaps + 1) / 2 : p.ntaps;
  const int nitems = ntap_items * P.nct * P.ntw;
  const int gq = (lane >> 2) & 3, gc = 4 * (lane & 3), gh = (lane >> 4) & 1;  // see wgrad3_kernel
  // (set-up and epilogue are this kernel's own: as shared functions they take <9, 0, 0> from 48 to 52 B of scratch)
  const uint32_t xh0 = (uint32_t)(uintptr_t)Xh, dh0 = (uint32_t)(uintptr_t)DYh;
  const uint32_t xlo = 2 * P.PP * CC, dlo = 2 * IG_TILE_M * DYW;
  uint32_t xa[MAXS][2], xb[1][2];
  bool valid[MAXS];
  f32x16 acc[MAXS];
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    const int it = wave + NW * s;
    valid[s] = it < nitems;
    const int cit = valid[s] ? it % P.nct : 0, rr = valid[s] ? it / P.nct : 0;
    const int nt = rr % P.ntw, tap = rr / P.ntw;
    int tp = tap, col = 16 * gh + gc;
    if (P.pack2) {
      const int tb = 2 * tap + 1;
      tp = 2 * tap;
      if (gh && tb < p.ntaps) { tp = tb; col = gc; }
    }
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
      const int mk = 8 * lh + 4 * rd + gq;
      const int pr = (mk >> P.lgTW) + p.hh + p.dh[tp], pc = (mk & (p.TW - 1)) + p.hw + p.dw[tp];
      xa[s][rd] = xh0 + 2 * ((pr * PW + pc) * CC + (w3_chunk(cit, pc, P.nct) << 5) + col);
      // the host only picks this kernel when all items of a wave share the dy tile (4 % (nct * ntw) == 0)
      if (s == 0) xb[0][rd] = dh0 + 2 * (mk * DYW + (w3_chunk(nt, mk, P.ntw) << 5) + 16 * gh + gc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
  }
  __syncthreads();  // tile 0 is in buffer 0
  int buf = 0;
  constexpr int SG = 2;   // w3_kstep: two slot groups live at a time
  for (int tile = blockIdx.x; tile < P.ntiles; tile += gridDim.x, buf ^= 1) {
    if constexpr (GEO > 0) {
      // compile-time geometry: every offset of the K loop is an instruction immediate and the loop is unrolled
      constexpr W3Geo Gm = w3_geo(GEO);
      constexpr uint32_t kstep = 2 * (16 >> Gm.lgTW) * Gm.PW * Gm.CC, bstep = 2 * 16 * 32 * Gm.ntw;
      constexpr uint32_t xloc = 2 * Gm.PP * Gm.CC, dloc = 2 * IG_TILE_M * 32 * Gm.ntw;
      const uint32_t bo = 2 * buf * buf_u16;
      uint32_t xab[MAXS][2], xbb[1][2];
#pragma unroll
      for (int s = 0; s < MAXS; ++s) { xab[s][0] = xa[s][0] + bo; xab[s][1] = xa[s][1] + bo; }
      xbb[0][0] = xb[0][0] + bo; xbb[0][1] = xb[0][1] + bo;
#pragma unroll
      for (int kpi = 0; kpi < IG_TILE_M / 16; ++kpi) w3_kstep<MAXS, SG, true, ABF>(xab, xbb, kpi * kstep, kpi * bstep, xloc, dloc, acc);
    } else {
      const uint32_t kstep = 2 * (16 >> P.lgTW) * PW * CC;
      const uint32_t bstep = 2 * 16 * DYW;
      uint32_t ko = 2 * buf * buf_u16, kb = ko;
#pragma unroll 1
      for (int kp = 0; kp < IG_TILE_M; kp += 16, ko += kstep, kb += bstep) w3_kstep<MAXS, SG, true, ABF>(xa, xb, ko, kb, xlo, dlo, acc);
    }
    __syncthreads();
  }
  const int NPo = gridDim.y * DYW;
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    if (valid[s]) {
      const int it = wave + NW * s;
      const int cit = it % P.nct, rr = it / P.nct;
      const int nt = rr % P.ntw, tap = rr / P.ntw;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int ci = cz0 + cit * 32 + crow(r, lh), tp = tap;
        if (P.pack2) {
          const int row = crow(r, lh);
          tp = 2 * tap + (row >> 4);
          ci = row & 15;
          if (tp >= p.ntaps) continue;
        }
        p.part[(((size_t)blockIdx.x * p.ntaps + tp) * p.CINP + ci) * NPo + n0 + nt * 32 + li] = acc[s][r];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <int MAXS, int NW>
static int launch_wgrad(const WgradParams& P, const BsedLaunch& L) {
  BSED_LABEL_ONLY(L, "wgrad_kernel<%d, %d>", MAXS, NW);
  static BsedLdsOnce once;
  BSED_HIP(bsed_max_lds(once, (const void*)wgrad_kernel<MAXS, NW>));
  hipLaunchKernelGGL((wgrad_kernel<MAXS, NW>), L.grid, dim3(NW * 64), L.smem, L.s, P);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

// Host-side prepare step of bsed_wgrad and bsed_wgrad3 (mode3), shared with their plan: every shape check, the derived
// geometry, the LDS bytes and grid.y / grid.z.  The entry points add the pointer and G checks and the launch.
static int wgrad_prepare(const BsedWgradDesc* desc, WgradParams& P, size_t& smem, dim3& grid_yz, int mode3 = 0) {
  BSED_CHECK_ARG(desc, "bsed_wgrad: null descriptor");
  P.d = *desc;
  BsedWgradDesc& d = P.d;
  P.ntiles = bsed_tile_geometry(P, "bsed_wgrad", 4, 4);
  if (P.ntiles < 0) return P.ntiles;
  BSED_CHECK_ARG(d.N % 4 == 0, "bsed_wgrad: N must be a multiple of 4");
  BSED_CHECK_ARG(d.CINP % 32 == 0 && d.CINP >= d.CIN, "bsed_wgrad: bad padding");
  BSED_CHECK_ARG(d.dy_pitch >= d.N && d.dy_pitch % 4 == 0, "bsed_wgrad: bad pitch");
  BSED_CHECK_ARG((d.bn_y == nullptr) == (d.bn_coef == nullptr) && (d.bn_y == nullptr) == (d.bn_mean == nullptr),
                 "bsed_wgrad: bn_y, bn_coef and bn_mean come together (BatchNorm backward applied on load) or not at all");
  BSED_CHECK_ARG(d.bn_y || !d.dy_out, "bsed_wgrad: dy_out only goes with bn_y");
  BSED_CHECK_ARG(!d.bn_y || mode3, "bsed_wgrad: BatchNorm backward on load is built into the split-fp32 kernels (bsed_wgrad3) only");
  BSED_CHECK_ARG(!d.dy_out || (d.dy_out != d.dy && d.dy_out != d.bn_y), "bsed_wgrad: dy_out must not alias dy or bn_y "
                 "(other workgroups still read them)");
  // input channels are contracted in chunks of CC per workgroup (grid.z): 64 for the 9-tap convolutions so that
  // two workgroups fit in a CU's LDS and one's tile load overlaps the other's MFMAs, 128 for the 1-tap forms
  const bool wide1 = d.ntaps == 1;
  P.CC = 32;
  for (int cand = (wide1 ? 128 : 64); cand >= 32; cand >>= 1)
    if (d.CINP % cand == 0) { P.CC = cand; break; }
  // tall narrow tiles (W = 2: 66 x 4 halo patch) would leave a single workgroup per CU with 64-channel chunks
  if (mode3 && d.ntaps > 1 && P.CC > 32 && (size_t)P.PP * P.CC * 4 + (size_t)W3_DY_BYTES > 80 * 1024) P.CC = 32;
  BSED_CHECK_ARG(d.CINP % P.CC == 0 && d.CINP / P.CC <= 65535, "bsed_wgrad: CINP must be a multiple of 32");
  P.lgc4 = ilog2_exact(P.CC / 4);
  P.nct = P.CC / 32;
  P.pack2 = (d.CIN <= 16 && d.CINP == 32 && d.ntaps > 1) ? 1 : 0;
  P.dy_off = mode3 ? P.PP * P.CC : ((P.PP * (P.CC + 1) + 3) & ~3);  // in 4-byte words
  // 1-tap contractions have one MFMA per LDS pair: widen the dy tile to 128 channels so the activation tile is
  // staged once per 4 output tiles (4x fewer HBM/L2 re-reads of `in`) when it fits in LDS
  // (the 9-tap forms get 2 dy tiles when two workgroups still fit in one CU's LDS: the activation patch is then
  // staged once per 64 output channels and the per-CU load rate stops being the limiter)
  P.ntw = 1;
  const int tap_items = P.pack2 ? (d.ntaps + 1) / 2 : d.ntaps;
  for (int cand = 4; cand >= 2; cand >>= 1) {
    const size_t need = mode3 ? (size_t)P.dy_off * 4 + (size_t)W3_DY_BYTES * cand
                              : ((size_t)P.dy_off + IG_TILE_M * 32 * cand) * sizeof(float);
    const size_t budget = wide1 ? 160 * 1024 : 80 * 1024;
    if (d.NP % (32 * cand) == 0 && tap_items * P.nct * cand <= 36 && need <= budget) { P.ntw = cand; break; }
  }
  smem = mode3 ? (size_t)P.dy_off * 4 + (size_t)W3_DY_BYTES * P.ntw
               : ((size_t)P.dy_off + IG_TILE_M * 32 * P.ntw) * sizeof(float);
  BSED_CHECK_ARG(tap_items * P.nct * P.ntw <= 36, "bsed_wgrad: %d work items per workgroup exceed the 36 supported",
                 tap_items * P.nct * P.ntw);
  BSED_CHECK_ARG(smem <= 160 * 1024, "bsed_wgrad: tile needs %zu B of LDS", smem);
  grid_yz = dim3(1, d.NP / (32 * P.ntw), d.CINP / P.CC);
  return BSED_OK;
}

// number of partial slabs G such that G x (n tiles) x (channel chunks) is about three workgroups per CU
static int wgrad_auto_g(const WgradParams& P, size_t smem, dim3 gyz) {
  // exactly one resident round of workgroups (2 per CU when two tiles fit in LDS): no partial tail round
  const long slots = smem <= 80 * 1024 ? 512 : 256;
  const long want = std::max<long>(1, slots / ((long)gyz.y * gyz.z));
  return (int)std::max<long>(1, std::min<long>(want, P.ntiles));
}

// The ONE choice of wgrad_kernel<MAXS, NW> for a shape, as MAXS * 16 + NW
static int wgrad_variant(const WgradParams& P) {
  const BsedWgradDesc& d = P.d;
  const int nitems = (P.pack2 ? (d.ntaps + 1) / 2 : d.ntaps) * P.nct * P.ntw;
  if (nitems >= 16 && d.ntaps == 1) {  // 1-tap forms: 8 waves per staged tile (measured +55 %); 9-tap forms are faster with 4
    const int slots8 = ceil_div(nitems, 8);
    if (slots8 <= 2) return 2 * 16 + 8;
    if (slots8 <= 3) return 3 * 16 + 8;
    if (slots8 <= 5) return 5 * 16 + 8;
  }
  const int slots = ceil_div(nitems, 4);
  const int m = slots <= 1 ? 1 : slots <= 2 ? 2 : slots <= 3 ? 3 : slots <= 5 ? 5 : 9;
  return m * 16 + 4;
}

static int wgrad_dispatch(const WgradParams& P, const BsedLaunch& L) {
  switch (wgrad_variant(P)) {
#define CASE(MAXS, NW) \
  case MAXS * 16 + NW: return launch_wgrad<MAXS, NW>(P, L);
    CASE(2, 8) CASE(3, 8) CASE(5, 8)
    CASE(1, 4) CASE(2, 4) CASE(3, 4) CASE(5, 4) CASE(9, 4)
#undef CASE
  }
  bsed_set_error("bsed_wgrad: no kernel instance for variant %d", wgrad_variant(P));
  return BSED_ERR_ARG;
}

template <int MAXS, int NW, bool BS>
static int launch_wgrad3(const WgradParams& P, const BsedLaunch& L) {
  BSED_LABEL_ONLY(L, "wgrad3_kernel<%d, %d, %s, %d>", MAXS, NW, BS ? "true" : "false", P.d.act_bf16 ? 1 : 0);
  static BsedLdsOnce once, onceb;
  if (P.d.act_bf16) {
    BSED_HIP(bsed_max_lds(onceb, (const void*)wgrad3_kernel<MAXS, NW, BS, 1>));
    hipLaunchKernelGGL((wgrad3_kernel<MAXS, NW, BS, 1>), L.grid, dim3(NW * 64), L.smem, L.s, P);
  } else {
    BSED_HIP(bsed_max_lds(once, (const void*)wgrad3_kernel<MAXS, NW, BS, 0>));
    hipLaunchKernelGGL((wgrad3_kernel<MAXS, NW, BS, 0>), L.grid, dim3(NW * 64), L.smem, L.s, P);
  }
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

template <int MAXS, int GEO>
static int launch_wgrad3p_geo(const WgradParams& P, const BsedLaunch& L) {
  BSED_LABEL_ONLY(L, "wgrad3p_kernel<%d, %d, %d>", MAXS, GEO, P.d.act_bf16 ? 1 : 0);
  static BsedLdsOnce once, onceb;
  if (P.d.act_bf16) {
    BSED_HIP(bsed_max_lds(onceb, (const void*)wgrad3p_kernel<MAXS, GEO, 1>));
    hipLaunchKernelGGL((wgrad3p_kernel<MAXS, GEO, 1>), L.grid, dim3(512), 2 * L.smem, L.s, P);
  } else {
    BSED_HIP(bsed_max_lds(once, (const void*)wgrad3p_kernel<MAXS, GEO, 0>));
    hipLaunchKernelGGL((wgrad3p_kernel<MAXS, GEO, 0>), L.grid, dim3(512), 2 * L.smem, L.s, P);
  }
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

// which compile-time geometry (w3_geo) matches this launch, 0 = none
static int wgrad3p_geo(const WgradParams& P) {
  for (int g = 1; g <= W3_NGEO; ++g) {
    const W3Geo G = w3_geo(g);
    if (P.CC == G.CC && P.lgTW == G.lgTW && P.PW == G.PW && P.PP == G.PP && P.ntw == G.ntw) return g;
  }
  return 0;
}

// the MAXS each compile-time geometry is built for (GEO = 0, run-time geometry, is built for MAXS = 3, 5 and 9)
static constexpr int w3p_geo_maxs(int g) { return g <= 2 ? 9 : (g <= 5 ? 5 : 3); }

// the pipelined kernel takes the multi-tap shapes whose two tile buffers fit in LDS and whose per-thread prefetch fits
// its register arrays; everything else (1-tap forms, tall narrow patches) stays on wgrad3_kernel
static bool wgrad3_pipelined(const WgradParams& P, size_t smem) {
  const int nitems = (P.pack2 ? (P.d.ntaps + 1) / 2 : P.d.ntaps) * P.nct * P.ntw;
  // fewest (tap, chunk) items the pipelined kernel takes: 4, i.e. the 16 -> 32 channel layer (5 items: two taps per MFMA
  // tile) included.  With run-time geometry the pipelined kernel lost to wgrad3_kernel there with fp32 activations (0.78
  // vs 0.69 ms; bf16: 0.41 vs 0.65); with the layer's geometry compiled in (w3_geo(6)) it wins in both modes: 0.60 ms
  // fp32, 0.28 ms bf16 (against 8 items, the earlier threshold).  BSED_WGRAD3_NOPIPE (read per call: tests switch
  // inside one process) keeps every shape on wgrad3_kernel.
  return P.d.ntaps > 1 && nitems > 4 &&
         P.d.H < 16384 && P.d.W < 16384 && 2 * smem <= 160 * 1024 && 4 % (P.nct * P.ntw) == 0 && nitems <= 36 &&
         P.PP * (P.CC / 4) <= W3P_UX * 256 && IG_TILE_M * 8 * P.ntw <= W3P_UD * 256 && !getenv("BSED_WGRAD3_NOPIPE");
}

// the streaming 1-tap kernel takes the shapes whose slabs tile into 128 x 128 blocks
static bool wgrad1_streaming(const WgradParams& P) {
  const BsedWgradDesc& d = P.d;
  return d.ntaps == 1 && P.CC == 128 && P.ntw == 4 && d.CINP % 128 == 0 && d.NP % 128 == 0 && !d.bn_y &&
         (long)d.NB * d.H * d.W < (1L << 31) - 4 * 65536;
}

// The ONE choice of the split-fp32 weight-gradient kernel for a shape: bsed_wgrad3 launches it, its plan names it and
// wgrad3_auto_g sizes its grid.
enum W3Kind { W3_TILE, W3_PIPE, W3_STREAM1 };
struct W3Plan {
  W3Kind kind;
  int maxs, nw, geo;   // wgrad3_kernel<MAXS, NW, BS>, wgrad3p_kernel<MAXS, GEO>
  bool bs, shifted;    // BS; wgrad1_kernel<SHIFT>
};
static W3Plan wgrad3_plan(const WgradParams& P, size_t smem) {
  if (wgrad1_streaming(P)) return {W3_STREAM1, 0, 0, 0, false, P.d.dh[0] != 0 || P.d.dw[0] != 0};
  const int v = wgrad_variant(P), maxs = v / 16, nw = v % 16;
  if (wgrad3_pipelined(P, smem)) {
    const int m = maxs <= 3 ? 3 : (maxs <= 5 ? 5 : 9), g = wgrad3p_geo(P);
    return {W3_PIPE, m, 1, g && w3p_geo_maxs(g) == m ? g : 0, false, false};
  }
  return {W3_TILE, maxs, nw, 0, nw % (P.nct * P.ntw) == 0, false};
}

template <int GEO = W3_NGEO>
static int launch_wgrad3p(const W3Plan& pl, const WgradParams& P, const BsedLaunch& L) {
  if constexpr (GEO > 0) {
    if (pl.geo == GEO) return launch_wgrad3p_geo<w3p_geo_maxs(GEO), GEO>(P, L);
    return launch_wgrad3p<GEO - 1>(pl, P, L);
  } else {
    if (pl.maxs == 3) return launch_wgrad3p_geo<3, 0>(P, L);
    if (pl.maxs == 5) return launch_wgrad3p_geo<5, 0>(P, L);
    return launch_wgrad3p_geo<9, 0>(P, L);
  }
}

template <bool SHIFT>
static int launch_wgrad1(const WgradParams& P, const BsedLaunch& L) {
  BSED_LABEL_ONLY(L, "wgrad1_kernel<%s, %d>", SHIFT ? "true" : "false", P.d.act_bf16 ? 1 : 0);
  static BsedLdsOnce once, onceb;
  if (P.d.act_bf16) {
    BSED_HIP(bsed_max_lds(onceb, (const void*)wgrad1_kernel<SHIFT, 1>));
    hipLaunchKernelGGL((wgrad1_kernel<SHIFT, 1>), L.grid, dim3(W1_THREADS), 2 * W1_STAGE, L.s, P);
  } else {
    BSED_HIP(bsed_max_lds(once, (const void*)wgrad1_kernel<SHIFT, 0>));
    hipLaunchKernelGGL((wgrad1_kernel<SHIFT, 0>), L.grid, dim3(W1_THREADS), 2 * W1_STAGE, L.s, P);
  }
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

template <int MAXS, int NW>
static int launch_wgrad3_tile(const W3Plan& pl, const WgradParams& P, const BsedLaunch& L) {
  return pl.bs ? launch_wgrad3<MAXS, NW, true>(P, L) : launch_wgrad3<MAXS, NW, false>(P, L);
}

// the recommended number of partial slabs G of bsed_wgrad3 (it differs between the three kernels)
static int wgrad3_auto_g(const WgradParams& P, const W3Plan& pl, size_t smem, dim3 gyz) {
  long slots = pl.kind == W3_PIPE ? 256 : smem <= 80 * 1024 ? 512 : 256;
  // small tiles (conv1 16 -> 32 channel gradient: 39 KB, 136 registers): a third workgroup per CU fits and hides more of
  // the stage / barrier / MFMA serialisation: 0.956 -> 0.753 ms; a fourth (the kernel pinned to 128 registers) 0.651 ms
  if (pl.kind != W3_PIPE && smem <= 52 * 1024 && wgrad_variant(P) / 16 <= 2) slots = 1024;
  long want = std::max<long>(1, slots / ((long)gyz.y * gyz.z));
  // XCD affinity: workgroup (x, y, z) has linear id x + G * (y + gy * z) and lands on XCD id % 8.  The gy * gz
  // workgroups of one tile sequence x read the same activation / dy tiles at about the same time; with G a multiple of
  // 8 they share an XCD, hence its L2, and the re-reads stop going to HBM
  if (gyz.y * gyz.z > 1 && (want % 8) * 16 <= want) want -= want % 8;  // <= 6 % fewer workgroups
  return (int)std::max<long>(1, std::min<long>(want, P.ntiles));
}

static int wgrad3_dispatch(const WgradParams& P, const W3Plan& pl, const BsedLaunch& L) {
  if (pl.kind == W3_STREAM1) return pl.shifted ? launch_wgrad1<true>(P, L) : launch_wgrad1<false>(P, L);
  if (pl.kind == W3_PIPE) return launch_wgrad3p(pl, P, L);
  if (pl.nw == 8) {
    if (pl.maxs == 2) return launch_wgrad3_tile<2, 8>(pl, P, L);
    if (pl.maxs == 3) return launch_wgrad3_tile<3, 8>(pl, P, L);
    return launch_wgrad3_tile<5, 8>(pl, P, L);
  }
  if (pl.maxs == 1) return launch_wgrad3_tile<1, 4>(pl, P, L);
  if (pl.maxs == 2) return launch_wgrad3_tile<2, 4>(pl, P, L);
  if (pl.maxs == 3) return launch_wgrad3_tile<3, 4>(pl, P, L);
  if (pl.maxs == 5) return launch_wgrad3_tile<5, 4>(pl, P, L);
  return launch_wgrad3_tile<9, 4>(pl, P, L);
}

// both weight-gradient entry points (pointer and G checks, launch) and their plan (recommended G, label only)
int bsed_run_wgrad(const BsedWgradDesc* desc, int mode3, void* stream, BsedContractPlan* plan) {
  WgradParams P;
  size_t smem;
  dim3 gyz;
  const int rc = wgrad_prepare(desc, P, smem, gyz, mode3);
  if (rc != BSED_OK) return rc;
  const BsedWgradDesc& d = P.d;
  const W3Plan pl = mode3 ? wgrad3_plan(P, smem) : W3Plan{};
  BsedLaunch L;
  if (plan) L = bsed_plan_begin(plan, mode3 ? wgrad3_auto_g(P, pl, smem, gyz) : wgrad_auto_g(P, smem, gyz), P.ntiles, 0);
  else {
    const char* who = mode3 ? "bsed_wgrad3" : "bsed_wgrad";
    BSED_CHECK_ARG(d.in && d.dy && d.part, "%s: null tensor", who);
    BSED_CHECK_ARG(d.G > 0 && d.G <= P.ntiles, "%s: G (%d) must be in 1..%d tiles", who, d.G, P.ntiles);
    L = BsedLaunch{dim3((unsigned)d.G, gyz.y, gyz.z), smem, (hipStream_t)stream, nullptr};
  }
  return mode3 ? wgrad3_dispatch(P, pl, L) : wgrad_dispatch(P, L);
}
extern "C" int bsed_wgrad(const BsedWgradDesc* desc, void* stream) { return bsed_run_wgrad(desc, 0, stream, nullptr); }
extern "C" int bsed_wgrad3(const BsedWgradDesc* desc, void* stream) { return bsed_run_wgrad(desc, 1, stream, nullptr); }
