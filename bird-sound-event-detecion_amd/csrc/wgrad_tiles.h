// Device code of the split-fp32 weight-gradient family that is stated once: the tile decode (both producer forms of
// wgrad3p_kernel), the BatchNorm-backward coefficients (wgrad3p_kernel, wgrad.hip, and cbwd3_kernel, conv_bwd.hip) and
// the K step (both K loops of wgrad3p_kernel).  What differs between the callers comes in as data -- a channel, byte
// offsets -- and no piece knows who called it.  Every function is __forceinline__ and every array a fully unrolled
// register array: a caller that passes constants gets them folded (wgrad3p_kernel's compile-time geometries rely on it).
// A piece is here only where EVERY instance of its callers keeps the parent form's occupancy, scratch and spill counts;
// DESIGN.md section 5 lists what stayed with its kernel and the figures.
#pragma once
#include "bsed_common.h"
#include "../../include/bsed.h"

// ----------------------------------------------------------------------------------------------
// 1. Tile index -> image nb, first row / column of the tile, element offsets of the image in `in` and `dy`
// ----------------------------------------------------------------------------------------------
struct W3Tile { int nb, th0, tw0; size_t in_img, dy_img; };
__device__ __forceinline__ W3Tile w3_tile(const BsedWgradDesc& p, int tile) {
  int t = tile;
  const int tw_i = t % p.tilesW; t /= p.tilesW;
  const int th_i = t % p.tilesH;
  W3Tile g;
  g.nb = t / p.tilesH;
  g.th0 = th_i * p.TH; g.tw0 = tw_i * p.TW;
  g.in_img = (size_t)g.nb * p.H * p.W * p.in_pitch;
  g.dy_img = (size_t)g.nb * p.H * p.W * p.dy_pitch;
  return g;
}

// ----------------------------------------------------------------------------------------------
// 2. BatchNorm backward on load: d_y = A g + B y + (C - B mean) for the four channels cn .. cn + 3.  A thread's pieces
// of dy all sit in one channel quad (the thread count is a multiple of the quads per position), so the coefficients are
// loaded once per thread.  The pipelined kernels pass quad 0 for a thread whose quad lies beyond N: its loads stay inside
// the tensor, its LDS image is zeroed, and what it stores to dy_out is the value quad 0's owner stores there as well.
// ----------------------------------------------------------------------------------------------
struct W3Bn { float4 A, B, C; };
__device__ __forceinline__ W3Bn w3_bn_identity() {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  return W3Bn{make_float4(1.f, 1.f, 1.f, 1.f), z, z};
}
__device__ __forceinline__ W3Bn w3_bn_coef(const BsedWgradDesc& p, int cn) {
  W3Bn c;
  c.A = *reinterpret_cast<const float4*>(p.bn_coef + cn);
  c.B = *reinterpret_cast<const float4*>(p.bn_coef + p.N + cn);
  const float4 c2 = *reinterpret_cast<const float4*>(p.bn_coef + 2 * p.N + cn);
  const float4 mu = *reinterpret_cast<const float4*>(p.bn_mean + cn);
  c.C = make_float4(fmaf(-c.B.x, mu.x, c2.x), fmaf(-c.B.y, mu.y, c2.y), fmaf(-c.B.z, mu.z, c2.z), fmaf(-c.B.w, mu.w, c2.w));
  return c;
}

// ----------------------------------------------------------------------------------------------
// 3. One K step (16 positions) of a wave's slots.  Slots go through the matrix cores in groups of SG: the fragments of
// group g + 1 are requested before the MFMAs of group g issue (sched_barrier pins that order), so one LDS latency is
// exposed per K step, not one per group, and at most two groups of fragments are live (a 9-slot wave has 144
// accumulator registers).  ko / kb: byte offsets of this K step (and tile buffer) in the patch and in the dy image;
// xlo / dlo: byte distance from a hi plane to its lo plane.  Constant offsets become instruction immediates; the
// caller's loop decides the unrolling.  BS: one dy fragment address pair serves every slot (all of a wave's items sit on
// one dy chunk); otherwise one per slot.
// ----------------------------------------------------------------------------------------------
template <int MAXS, int SG, bool BS, int ABF>
__device__ __forceinline__ void w3_kstep(const uint32_t (&xa)[MAXS][2], const uint32_t (&xb)[BS ? 1 : MAXS][2], uint32_t ko, uint32_t kb,
                                         uint32_t xlo, uint32_t dlo, f32x16 (&acc)[MAXS]) {
  constexpr int NG = (MAXS + SG - 1) / SG, SB = BS ? 1 : SG;
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
