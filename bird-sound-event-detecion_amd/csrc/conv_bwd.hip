// Both gradients of a 3 x 3 / pad 1 convolution that feeds a train-mode BatchNorm, in ONE pass over HBM (bsed_conv_bwd3):
//   d_y[p][n]        = A[n] g[p][n] + B[n] (y[p][n] - mean[n]) + C[n]          BatchNorm backward, formed on load
//   dW[tap][k][n]    = sum_p in[p + off(tap)][k] * d_y[p][n]                   partial slabs, as bsed_wgrad3 writes them
//   d_in[p][k]       = sum_{tap, n} d_y[p - off(tap)][n] * w[tap][k][n]        what bsed_igemm3n computes from dy_out
// The two-kernel route writes d_y (wgrad3p_kernel, dy_out) and reads it straight back (the data gradient): at 16 -> 32
// and 32 -> 64 channels both kernels run at the HBM rate, and that round trip is 40 % of their bytes.  Here d_y never
// leaves the chip.
//
// Structure: wgrad3p_kernel's (wgrad.hip) -- one persistent 8-wave workgroup per CU, two LDS tile buffers, one barrier
// per tile; waves 4-7 load, convert and write tile t + 1 while waves 0-3 multiply tile t.  What differs:
//   * the producers form d_y for the tile PLUS its one-position ring (the data gradient of the tile's border positions
//     reads it), zeros outside the image -- never the neighbouring image's rows -- and keep it as bf16 hi / lo planes in
//     [patch position][channel] rows, like the activation patch;
//   * that one image serves both contractions: the weight gradient (K = positions) reads it through the transposing
//     fragment reads, the data gradient (K = output channels, the tap a position shift) reads plain 16-byte pieces of 8
//     channels.  A piece's place in its row is XOR-swizzled with the patch column (chunk: w3_chunk; piece in the chunk:
//     bits 2-3 of the column) and the row pitch is padded to a multiple of 4 positions (256 B), so that the 16 lanes a
//     ds_read_b128 services together -- 16 different columns of one or two tile rows -- hit 16 different 4-bank groups
//     while a transposing read's 4 columns x 64 B still tile the 64 banks;
//   * after the weight-gradient MFMAs of a tile the consumer waves (one 32-position row block each) run the data-gradient
//     MFMAs against the flipped weights -- fragments of the bsed_pack_weight3s table of the transposed weight, fetched
//     from global memory / L2 one step ahead as in igemm3n_kernel -- and store the d_in tile.
// Accumulation order: per partial slab that of wgrad3p_kernel; per d_in element that of the kernel the two-kernel route
// runs for the layer: for 16 -> 32 channels (the compile-time form) igemm3s_kernel's 16 x 16 x 32 contraction (tap, lo*hi,
// hi*lo, hi*hi), for the other 32-channel d_y shapes its 32 x 32 x 16 one (k half, tap, ...): the same bits as that route.
// With 64 channels of d_y: igemm3n_kernel's 32 x 32 x 16 form (chunk, tap, k half, ...), bitwise that form's.
// Tiles go to workgroups XCD-affine (a round's 32 consecutive tiles per XCD): the ring a tile re-reads is its
// neighbours' interior, fetched by the same XCD's L2 at about the same time.
#include "wgrad_tiles.h"
#include <algorithm>
#include <type_traits>

struct CbwdParams {
  BsedWgradDesc d;
  int PW, PH, PP, lgTW, pw_magic, ntiles;   // bsed_tile_geometry: the tile plus its ring
  int PWL, PPL;                             // d_y image: positions per patch row in LDS (PW rounded up to 4), rows * PWL
  int ntw, pack2;                           // 32-channel d_y chunks; CIN <= 16: two taps share one 32-row MFMA tile
};

typedef __attribute__((address_space(3))) w3_bf16x8 cb_lds_v8;

// GEO = 1: the 16 x 8 tile of the wide maps (W a multiple of 16) with every LDS offset a compile-time constant;
// GEO = 0: tile width and patch pitches at run time.  NTW = N / 32.  MAXS = weight-gradient items per consumer wave.
// WL = 1: the data gradient's weight fragments live in LDS behind the two tile buffers (copied once per workgroup);
// WL = 0: they come from global memory / L2 one step ahead.
template <int MAXS, int NTW, int GEO, int WL>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void cbwd3_kernel(const CbwdParams P) {
  constexpr int NTHR = 256, NW = 4, DYW = 32 * NTW;
  const BsedWgradDesc& p = P.d;
  extern __shared__ __align__(16) uint32_t smw[];
  const int lgTW = GEO ? 4 : P.lgTW, TWm = (1 << lgTW) - 1;
  const int PW = GEO ? 18 : P.PW, PP = GEO ? 180 : P.PP, PWL = GEO ? 20 : P.PWL, PPL = GEO ? 200 : P.PPL;
  const int XPL = PP * 32, DPL = PPL * DYW;   // ushorts per plane
  const int buf_u16 = 2 * XPL + 2 * DPL;      // one tile buffer: Xh | Xl | DYh | DYl
  w3_lds_u16* Xh = (w3_lds_u16*)smw;
  w3_lds_u16* Xl = Xh + XPL;
  w3_lds_u16* DYh = Xh + 2 * XPL;
  w3_lds_u16* DYl = DYh + DPL;
  // XCD-affine tile order (bijective on 0 .. G-1 for any G): workgroup b runs on XCD b % 8
  int tile_first;
  {
    const int nt = gridDim.x, bid = blockIdx.x, q = nt >> 3, r = nt & 7, x = bid & 7;
    tile_first = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
  }

  if (threadIdx.x >= NTHR) {
    // ------------------------------------------------------------------ producer waves
    const int tid = threadIdx.x - NTHR;
    constexpr int UX = GEO ? 6 : 10, UD = GEO ? 6 * NTW : (NTW == 1 ? 10 : 14);   // 16-byte pieces per thread
    constexpr int n4n = 8 * NTW, lgn4 = NTW == 2 ? 4 : 3;
    const int x_tot = PP * 8, d_tot = PP * n4n;
    const int gW = p.W, gH = p.H;
    // a thread's pieces all sit in one channel quad (256 threads are a multiple of the quads per position)
    const bool xch_ok = 4 * (tid & 7) < p.CIN, dch_ok = 4 * (tid & (n4n - 1)) < p.N;
    const int xcoff = xch_ok ? 4 * (tid & 7) : 0, dcoff = dch_ok ? 4 * (tid & (n4n - 1)) : 0;
    // BatchNorm backward on load.  (The coefficients are all this kernel takes from wgrad_tiles.h: with the shared tile
    // decode <3, 2, 0, 0> spills 6 SGPRs for 4, with the shared set-up or epilogue <3, 1, 0, 0> 4 for 0 and <5, 2, 0, 0>
    // 11-12 for 9; profiles/wgrad_tiles.json.)
    const W3Bn bn = w3_bn_coef(p, dcoff);
    const float4 cA = bn.A, cB = bn.B, cC = bn.C;
    // tile-invariant geometry of a piece in ONE register: LDS offset (ushorts, bits 0-15), patch column (16-23), patch row
    // (24-31).  The producers are issue-bound beside the consumers' MFMAs: every VALU instruction per piece counts.
    uint32_t xg[UX], dg[UD];
    const int xq4 = 4 * (tid & 7), dc = 4 * (tid & (n4n - 1));
#pragma unroll
    for (int u = 0; u < UX; ++u) {
      const int pos = (tid + u * NTHR) >> 3;
      const int pr = GEO ? pos / 18 : (pos * P.pw_magic) >> 20, pc = pos - pr * PW;
      xg[u] = (uint32_t)((pos * 32 + xq4) & 0xffff) | ((uint32_t)pc << 16) | ((uint32_t)pr << 24);
    }
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      const int pos = (tid + u * NTHR) >> lgn4;
      const int pr = GEO ? pos / 18 : (pos * P.pw_magic) >> 20, pc = pos - pr * PW;
      const int o = (pr * PWL + pc) * DYW + (w3_chunk(dc >> 5, pc, NTW) << 5) + ((((dc >> 3) & 3) ^ ((pc >> 2) & 3)) << 3) + (dc & 7);
      dg[u] = (uint32_t)(o & 0xffff) | ((uint32_t)pc << 16) | ((uint32_t)pr << 24);
    }
    struct TGeo { int th0, tw0; size_t in_img, dy_img; };
    auto tgeo = [&](int tile) {
      int t = tile;
      const int tw_i = t % p.tilesW; t /= p.tilesW;
      const int th_i = t % p.tilesH;
      const int nb = t / p.tilesH;
      TGeo g;
      g.th0 = th_i * p.TH; g.tw0 = tw_i * p.TW;
      g.in_img = (size_t)nb * p.H * p.W * p.in_pitch;
      g.dy_img = (size_t)nb * p.H * p.W * p.dy_pitch;
      return g;
    };
    // byte offset of a piece inside its image (clamped into the map) and whether the piece is inside the map
    auto at = [&](uint32_t geo, const TGeo& g, int pitch, int coff, bool& ok) {
      const int gh_ = g.th0 - 1 + (int)(geo >> 24), gw = g.tw0 - 1 + (int)((geo >> 16) & 0xff);
      ok = (unsigned)gh_ < (unsigned)gH && (unsigned)gw < (unsigned)gW;
      return (uint32_t)((min(max(gh_, 0), gH - 1) * gW + min(max(gw, 0), gW - 1)) * pitch + coff) << 2;
    };
    // (a thread whose channel quad lies beyond the tensor loads quad 0 instead and writes zeros)
    auto ld16 = [](const float* base, size_t img, uint32_t byte_off) {
      return *reinterpret_cast<const w3_f32x4*>(reinterpret_cast<const char*>(base + img) + byte_off);
    };
    // software pipeline over tiles, straight-line between two barriers (see wgrad3p_kernel): a piece's registers are
    // refilled with the next tile's piece right after the piece has been split into LDS
    w3_f32x4 vx[UX], vd[UD], vy[UD];
    uint32_t xin = 0, din = 0;   // bit u: piece u of the tile in the registers lies inside the map (and the tensor's channels)
    int tile = tile_first, buf = 0;
    TGeo gc = tgeo(tile);
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      if (GEO && u * NTHR >= d_tot) continue;
      bool ok;
      const uint32_t o = at(dg[u], gc, p.dy_pitch, dcoff, ok);
      vd[u] = ld16(p.dy, gc.dy_img, o);
      vy[u] = ld16(p.bn_y, gc.dy_img, o);
      din |= (uint32_t)(ok && dch_ok) << u;
    }
#pragma unroll
    for (int u = 0; u < UX; ++u) {
      if (GEO && u * NTHR >= x_tot) continue;
      bool ok;
      vx[u] = ld16(p.in, gc.in_img, at(xg[u], gc, p.in_pitch, xcoff, ok));
      xin |= (uint32_t)(ok && xch_ok) << u;
    }
    for (; tile < P.ntiles; buf ^= 1) {
      const int nxt = tile + gridDim.x;
      const TGeo gn = tgeo(nxt < P.ntiles ? nxt : tile);
      const int bo = buf * buf_u16;   // (the buffer being written was last read before the previous barrier)
      uint32_t xnx = 0, dnx = 0;
#pragma unroll
      for (int u = 0; u < UD; ++u) {
        if (GEO && u * NTHR >= d_tot) continue;
        bool okn;
        const bool ok = (din >> u) & 1;
        const w3_f32x4 g = vd[u], y = vy[u];
        const float4 w = make_float4(ok ? fmaf(cA.x, g[0], fmaf(cB.x, y[0], cC.x)) : 0.f, ok ? fmaf(cA.y, g[1], fmaf(cB.y, y[1], cC.y)) : 0.f,
                                     ok ? fmaf(cA.z, g[2], fmaf(cB.z, y[2], cC.z)) : 0.f, ok ? fmaf(cA.w, g[3], fmaf(cB.w, y[3], cC.w)) : 0.f);
        if (tid + u * NTHR < d_tot) w3_store4<0>(DYh, DYl, bo + (int)(dg[u] & 0xffff), w);
        const uint32_t on = at(dg[u], gn, p.dy_pitch, dcoff, okn);
        vd[u] = ld16(p.dy, gn.dy_img, on);
        vy[u] = ld16(p.bn_y, gn.dy_img, on);
        dnx |= (uint32_t)(okn && dch_ok) << u;
      }
#pragma unroll
      for (int u = 0; u < UX; ++u) {
        if (GEO && u * NTHR >= x_tot) continue;
        bool okn;
        const bool ok = (xin >> u) & 1;
        const w3_f32x4 v = vx[u];
        const float4 w = make_float4(ok ? v[0] : 0.f, ok ? v[1] : 0.f, ok ? v[2] : 0.f, ok ? v[3] : 0.f);
        if (tid + u * NTHR < x_tot) w3_store4<0>(Xh, Xl, bo + (int)(xg[u] & 0xffff), w);
        vx[u] = ld16(p.in, gn.in_img, at(xg[u], gn, p.in_pitch, xcoff, okn));
        xnx |= (uint32_t)(okn && xch_ok) << u;
      }
      gc = gn; tile = nxt; xin = xnx; din = dnx;
      __syncthreads();
    }
    __syncthreads();  // pairs with the consumers' barrier after their last tile
    return;
  }

  // -------------------------------------------------------------------- consumer waves
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nitems = (P.pack2 ? 5 : 9) * NTW;
  const int gq = (lane >> 2) & 3, gc = 4 * (lane & 3), gh = (lane >> 4) & 1;  // transposing reads: see wgrad3_kernel
  const uint32_t xh0 = (uint32_t)(uintptr_t)Xh, dh0 = (uint32_t)(uintptr_t)DYh;
  const uint32_t xlo = 2 * XPL, dlo = 2 * DPL;   // bytes from a hi plane to its lo plane
  // ---- weight gradient: items (tap or tap pair, d_y chunk) wave + 4 s; all of a wave's items share the d_y chunk
  uint32_t xa[MAXS][2], xb[2];
  bool valid[MAXS];
  f32x16 acc[MAXS];
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    const int it = wave + NW * s;
    valid[s] = it < nitems;
    const int rr = valid[s] ? it : 0;
    const int nt = rr % NTW, tap = rr / NTW;
    int tp = tap, col = 16 * gh + gc;
    if (P.pack2) {
      // rows 0..15 of the MFMA tile: tap 2*tap, rows 16..31: tap 2*tap+1 (channels 16..31 of the patch are zero, which
      // is what the upper rows read when the second tap does not exist)
      const int tb = 2 * tap + 1;
      tp = 2 * tap;
      if (gh && tb < 9) { tp = tb; col = gc; }
    }
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
      const int mk = 8 * lh + 4 * rd + gq;
      const int pr0 = (mk >> lgTW) + 1, pc0 = (mk & TWm) + 1;
      xa[s][rd] = xh0 + 2 * (((pr0 + p.dh[tp]) * PW + pc0 + p.dw[tp]) * 32 + col);
      if (s == 0)
        xb[rd] = dh0 + 2 * ((pr0 * PWL + pc0) * DYW + (w3_chunk(nt, pc0, NTW) << 5) +
                            (((2 * gh + (gc >> 3)) ^ ((pc0 >> 2) & 3)) << 3) + (gc & 7));
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
  }
  const uint32_t kstep = 2 * (16 >> lgTW) * PW * 32, bstep = 2 * (16 >> lgTW) * PWL * DYW;   // bytes per 16 positions
  // ---- data gradient: this wave's 32 positions (lane li), 8 k values per lane half; tap t reads the position shifted by
  // (1 - t / 3, 1 - t % 3).  av[j][i]: byte address of piece pair i = 2 chunk + k half at column shift j - 1, one patch
  // row ABOVE the lane's position (the three row shifts are then + 0, 1, 2 rows: uniform, non-negative offsets)
  const int m = 32 * wave + li, mr = m >> lgTW, mc = (m & TWm) + 1;
  uint32_t av[3][2 * NTW];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int pc = mc + j - 1, ps = (pc >> 2) & 3, cs = NTW == 2 ? (pc >> 1) & 1 : 0;
#pragma unroll
    for (int i = 0; i < 2 * NTW; ++i)
      av[j][i] = dh0 + 2 * ((mr * PWL + pc) * DYW + ((i ^ ((cs << 1) | (ps >> 1))) << 4) + ((lh ^ (ps & 1)) << 3));
  }
  const uint32_t rstep = 2 * PWL * DYW;   // bytes per patch row
  constexpr int KS = 2 * NTW;             // k16 steps per tap of the weight table
  const bsed_u32x4* wb = reinterpret_cast<const bsed_u32x4*>(p.w3s) + lane;
  const bool cok = li < p.CIN;
  const uint32_t wl0 = xh0 + 4 * buf_u16 + 16 * lane;   // WL: this lane's piece of fragment 0
  if (WL) {
    typedef __attribute__((address_space(3))) bsed_u32x4 lds_u4;
    lds_u4* Wl = (lds_u4*)(Xh + 2 * buf_u16);
    for (int i = tid; i < 9 * KS * 2 * 64; i += NTHR) Wl[i] = reinterpret_cast<const bsed_u32x4*>(p.w3s)[i];
  }

  __syncthreads();  // tile 0 is in buffer 0 (and the weight fragments are in place)
  int buf = 0;
  constexpr int SG = 2, NG = (MAXS + SG - 1) / SG;
  for (int tile = tile_first; tile < P.ntiles; tile += gridDim.x, buf ^= 1) {
    const uint32_t bo = 2 * buf * buf_u16;
    // weight fragments of the data gradient's first step (chunk 0, tap 0): requested here, used after the K loop below
    bsed_u32x4 bq[4];
    if (!WL) {
#pragma unroll
      for (int f = 0; f < 4; ++f) bq[f] = wb[f * 64];
    }
    {
      uint32_t xab[MAXS][2], xbb[2];
#pragma unroll
      for (int s = 0; s < MAXS; ++s) { xab[s][0] = xa[s][0] + bo; xab[s][1] = xa[s][1] + bo; }
      xbb[0] = xb[0] + bo; xbb[1] = xb[1] + bo;
      // (not w3_kstep: this loop keeps fragments live ACROSS K steps, a different schedule from the shared K step's)
      // stages (K step, slot group) in order; the fragments of stage st + 1 are requested before the MFMAs of stage st
      // issue, across K steps too (two stages live at a time, the d_y fragment double-buffered per K step): a consumer
      // wave is alone on its SIMD with the matrix cores, so an LDS latency it waits for is not hidden by anyone
      constexpr int NST = (IG_TILE_M / 16) * NG;
      w3_bf16x8 ah[2][SG], al[2][SG], bh[2], bl[2];
      auto request = [&](int st) {
        const int kpi = st / NG, g = st % NG;
        const uint32_t ko = kpi * kstep, kb = kpi * bstep;
#pragma unroll
        for (int j = 0; j < SG; ++j) {
          const int sl = g * SG + j;
          if (sl < MAXS) {
            ah[st & 1][j] = w3_frag(xab[sl][0] + ko, xab[sl][1] + ko);
            al[st & 1][j] = w3_frag(xab[sl][0] + (ko + xlo), xab[sl][1] + (ko + xlo));
          }
        }
        if (g == 0) {
          bh[kpi & 1] = w3_frag(xbb[0] + kb, xbb[1] + kb);
          bl[kpi & 1] = w3_frag(xbb[0] + (kb + dlo), xbb[1] + (kb + dlo));
        }
      };
      request(0);
#pragma unroll
      for (int st = 0; st < NST; ++st) {
        if (st + 1 < NST) request(st + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < SG; ++j) {
          const int sl = (st % NG) * SG + j;
          if (sl < MAXS) acc[sl] = w3_mfma<0>(ah[st & 1][j], al[st & 1][j], bh[(st / NG) & 1], bl[(st / NG) & 1], acc[sl]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- data gradient of the tile from the same d_y image
    if constexpr (GEO && WL) {
      // The 16 -> 32 layer (32 channels of d_y in, 16 out): v_mfma_f32_16x16x32_bf16, as igemm3s_kernel's 16-channel form
      // contracts it on the two-kernel route -- a 16-column tile is exactly the output and K = 32 exactly the chunk, half
      // the matrix cycles of the 32 x 32 x 16 form -- in its order (tap, lo*hi, hi*lo, hi*hi): d_in keeps that route's
      // bits.  Lane (i = lane & 15, kg = lane >> 4): row i of the wave's row tile rt, channels 8 kg .. 8 kg + 7; the
      // weight operand is lane (i, half kg & 1) of the table's 32 x 32 x 16 fragment of k step kg >> 1.
      const int li16 = lane & 15, kg = lane >> 4;
      uint32_t a16[2][3];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const int m16 = 32 * wave + 16 * rt + li16, mr16 = m16 >> lgTW, mc16 = (m16 & TWm) + 1;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int pc = mc16 + j - 1;
          a16[rt][j] = dh0 + 2 * ((mr16 * PWL + pc) * DYW + ((kg ^ ((pc >> 2) & 3)) << 3));
        }
      }
      const uint32_t w16 = xh0 + 4 * buf_u16 + ((kg >> 1) * 2) * 1024 + (li16 + 32 * (kg & 1)) * 16;   // + (t * 4 + hl) * 1024
      typedef __attribute__((address_space(3))) bsed_u32x4 lds_u4;
      f32x4 acc16[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      w3_bf16x8 a_hi[2][2], a_lo[2][2];
      bsed_u32x4 bw[2][2];
      auto request = [&](int t) {
        const uint32_t ao = bo + (uint32_t)(2 - t / 3) * rstep;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          const uint32_t a = a16[rt][2 - t % 3] + ao;
          a_hi[t & 1][rt] = *(cb_lds_v8*)(uintptr_t)a;
          a_lo[t & 1][rt] = *(cb_lds_v8*)(uintptr_t)(a + dlo);
        }
        bw[t & 1][0] = *(lds_u4*)(uintptr_t)(w16 + (t * 4 + 0) * 1024);
        bw[t & 1][1] = *(lds_u4*)(uintptr_t)(w16 + (t * 4 + 1) * 1024);
      };
      request(0);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        if (t + 1 < 9) request(t + 1);
        __builtin_amdgcn_sched_barrier(0);
        const w3_bf16x8 b_hi = __builtin_bit_cast(w3_bf16x8, bw[t & 1][0]), b_lo = __builtin_bit_cast(w3_bf16x8, bw[t & 1][1]);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) acc16[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo[t & 1][rt], b_hi, acc16[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) acc16[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi[t & 1][rt], b_lo, acc16[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) acc16[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi[t & 1][rt], b_hi, acc16[rt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // result fragment of a 16 x 16 tile: column li16, rows 4 kg + r: position 32 wave + 16 rt [uniform] + 4 kg [lane] + r
      int t_ = tile;
      const int tw_i = t_ % p.tilesW; t_ /= p.tilesW;
      const int th_i = t_ % p.tilesH;
      const int nb = t_ / p.tilesH;
      const int th0 = th_i * p.TH, tw0 = tw_i * p.TW;
      auto eoff = [&](int mm) { return ((mm >> lgTW) * p.W + (mm & TWm)) * p.din_pitch; };
      float* ob = p.d_in + (((size_t)nb * p.H + th0) * p.W + tw0) * p.din_pitch;
      const uint32_t voff = (uint32_t)(eoff(4 * kg) + li16);
      const bool full = th0 + p.TH <= p.H;
      if (li16 < p.CIN) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int mu = 32 * wave + 16 * rt;
            if (full || th0 + ((mu + 4 * kg + r) >> lgTW) < p.H) (ob + (uint32_t)(eoff(mu) + eoff(r)))[voff] = acc16[rt][r];
          }
      }
    } else {
    f32x16 dacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) dacc[r] = 0.f;
    // steps (chunk, tap) in order; the operands of step s + 1 -- two k halves of d_y (hi, lo) from LDS, four weight
    // fragments from LDS (WL) or global memory -- are requested before the MFMAs of step s issue
    // (NTW = 1: the steps run k half OUTSIDE the taps -- igemm3s_kernel's order, the kernel that computes these layers'
    //  data gradient on the two-kernel route, so that d_in keeps that route's bits; NTW = 2: igemm3n_kernel's order)
    constexpr bool KOUT = NTW == 1;
    constexpr int NS = KOUT ? 18 : 9 * NTW;
    w3_bf16x8 a_hi[2][2], a_lo[2][2];
    bsed_u32x4 bn[2][4];
    auto request_a = [&](int sidx) {
      const int ch = KOUT ? 0 : sidx / 9, t = sidx % 9, k0 = KOUT ? sidx / 9 : 0, k1 = KOUT ? k0 + 1 : 2;
      const uint32_t ao = bo + (uint32_t)(2 - t / 3) * rstep;
#pragma unroll
      for (int kk = k0; kk < k1; ++kk) {
        const uint32_t a = av[2 - t % 3][(ch << 1) | kk] + ao;
        a_hi[sidx & 1][kk] = *(cb_lds_v8*)(uintptr_t)a;
        a_lo[sidx & 1][kk] = *(cb_lds_v8*)(uintptr_t)(a + dlo);
      }
    };
    auto request_b = [&](int sidx) {
      const int ch = KOUT ? 0 : sidx / 9, t = sidx % 9, k0 = KOUT ? sidx / 9 : 0, k1 = KOUT ? k0 + 1 : 2;
#pragma unroll
      for (int f = 2 * k0; f < 2 * k1; ++f) {
        const int fi = (t * KS + 2 * ch) * 2 + f;
        if (WL) bn[sidx & 1][f] = *(__attribute__((address_space(3))) bsed_u32x4*)(uintptr_t)(wl0 + fi * 1024);
        else bn[sidx & 1][f] = wb[fi * 64];
      }
    };
    request_a(0);
    if (WL) request_b(0);
    else {
#pragma unroll
      for (int f = 0; f < 4; ++f) bn[0][f] = bq[f];
    }
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) {
      if (sidx + 1 < NS) { request_b(sidx + 1); request_a(sidx + 1); }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = (KOUT ? sidx / 9 : 0); kk < (KOUT ? sidx / 9 + 1 : 2); ++kk) {
        const w3_bf16x8 b_hi = __builtin_bit_cast(w3_bf16x8, bn[sidx & 1][2 * kk]), b_lo = __builtin_bit_cast(w3_bf16x8, bn[sidx & 1][2 * kk + 1]);
        dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo[sidx & 1][kk], b_hi, dacc, 0, 0, 0);
        dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi[sidx & 1][kk], b_lo, dacc, 0, 0, 0);
        dacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi[sidx & 1][kk], b_hi, dacc, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- store the d_in tile: accumulator register r holds position 32 wave + crow(r, lh) of channel li
    {
      int t = tile;
      const int tw_i = t % p.tilesW; t /= p.tilesW;
      const int th_i = t % p.tilesH;
      const int nb = t / p.tilesH;
      const int th0 = th_i * p.TH, tw0 = tw_i * p.TW;
      // position 32 wave + 8 (r >> 2) [uniform] + 4 lh [lane] + (r & 3) [uniform]: three disjoint bit ranges, so the
      // element offset is the sum of the parts' offsets -- a scalar base per store, ONE per-lane offset (igemm3n_kernel)
      auto eoff = [&](int mm) { return ((mm >> lgTW) * p.W + (mm & TWm)) * p.din_pitch; };
      float* ob = p.d_in + (((size_t)nb * p.H + th0) * p.W + tw0) * p.din_pitch;
      const uint32_t voff = (uint32_t)(eoff(4 * lh) + li);
      if (th0 + p.TH <= p.H) {
        if (cok) {
#pragma unroll
          for (int r = 0; r < 16; ++r) (ob + (uint32_t)(eoff(32 * wave + 8 * (r >> 2)) + eoff(r & 3)))[voff] = dacc[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int mm = 32 * wave + crow(r, lh);
          if (cok && th0 + (mm >> lgTW) < p.H) (ob + (uint32_t)(eoff(32 * wave + 8 * (r >> 2)) + eoff(r & 3)))[voff] = dacc[r];
        }
      }
    }
    }
    __syncthreads();
  }
  // ---- partial slab of this workgroup: slab tile_first holds tiles tile_first + i G in order, as slab b of
  // wgrad3p_kernel does, whatever CU ran them
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    if (valid[s]) {
      const int it = wave + NW * s;
      const int nt = it % NTW, tap = it / NTW;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int ci = crow(r, lh), tp = tap;
        if (P.pack2) {
          tp = 2 * tap + (ci >> 4);
          ci &= 15;
          if (tp >= 9) continue;
        }
        p.part[(((size_t)tile_first * 9 + tp) * 32 + ci) * DYW + nt * 32 + li] = acc[s][r];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// every shape check, the derived geometry and the LDS bytes of the two tile buffers; no HIP call
static int cbwd_prepare(const BsedWgradDesc* desc, CbwdParams& P, size_t& smem) {
  const char* who = "bsed_conv_bwd3";
  BSED_CHECK_ARG(desc, "%s: null descriptor", who);
  P.d = *desc;
  BsedWgradDesc& d = P.d;
  P.ntiles = bsed_tile_geometry(P, who, 4, 4);
  if (P.ntiles < 0) return P.ntiles;
  BSED_CHECK_ARG(d.act_bf16 == 0, "%s: fp32 activations only (act_bf16 = %d)", who, d.act_bf16);
  BSED_CHECK_ARG(d.ntaps == 9 && d.hh == 1 && d.hw == 1, "%s: built for the nine taps of a 3 x 3 convolution", who);
  for (int t = 0; t < 9; ++t)
    BSED_CHECK_ARG(d.dh[t] == t / 3 - 1 && d.dw[t] == t % 3 - 1, "%s: tap %d is not (%d, %d): row-major 3 x 3 taps only", who, t,
                   t / 3 - 1, t % 3 - 1);
  BSED_CHECK_ARG(d.TW <= 16, "%s: tile width %d exceeds the 16 supported", who, d.TW);
  BSED_CHECK_ARG(d.CIN <= 32 && d.CINP == 32, "%s: built for CIN <= 32, CINP = 32 (got %d, %d)", who, d.CIN, d.CINP);
  BSED_CHECK_ARG((d.N == 32 || d.N == 64) && d.NP == d.N, "%s: built for N = NP = 32 or 64 (got %d, %d)", who, d.N, d.NP);
  BSED_CHECK_ARG(d.dy_pitch >= d.N && d.dy_pitch % 4 == 0 && d.din_pitch >= d.CIN, "%s: bad pitch", who);
  BSED_CHECK_ARG(d.H < 16384 && d.W < 16384 &&
                 (size_t)d.H * d.W * std::max(std::max(d.in_pitch, d.dy_pitch), d.din_pitch) < (1ull << 29),
                 "%s: an image of 2^29 elements or more", who);
  P.PWL = (P.PW + 3) & ~3;
  P.PPL = P.PH * P.PWL;
  P.ntw = d.N / 32;
  P.pack2 = d.CIN <= 16 ? 1 : 0;
  smem = 2 * ((size_t)2 * P.PP * 32 + (size_t)2 * P.PPL * d.N) * sizeof(unsigned short);
  BSED_CHECK_ARG(smem <= 160 * 1024, "%s: two tile buffers need %zu B of LDS (160 KB per workgroup)", who, smem);
  // the producers' per-thread register arrays of the run-time-geometry builds
  BSED_CHECK_ARG(P.PP * 8 <= 10 * 256 && P.PP * 8 * P.ntw <= (P.ntw == 1 ? 10 : 14) * 256,
                 "%s: patch of %d positions exceeds the producers' prefetch", who, P.PP);
  return BSED_OK;
}

#define CBWD_WTAB(NTW) (9 * 2 * (NTW) * 2 * 64 * 16)   // bytes of the data gradient's weight-fragment table
struct CbwdPlan { int maxs, ntw, geo; };
static CbwdPlan cbwd_plan(const CbwdParams& P) {
  const int nitems = (P.pack2 ? 5 : 9) * P.ntw;
  const bool wide = P.lgTW == 4 && P.PW == 18 && P.PP == 180;
  // compile-time geometry: the two layers of the network this kernel is for (16 -> 32 on 432 x 64, 32 -> 64 on 216 x 32)
  if (wide && P.pack2 && P.ntw == 1) return {2, 1, 1};
  if (wide && !P.pack2 && P.ntw == 2) return {5, 2, 1};
  return {nitems <= 12 ? 3 : 5, P.ntw, 0};
}

// The ONE rule that sends a layer to this kernel (BsedContractPlan.G > 0) or keeps it on bsed_wgrad3 + bsed_igemm3n
// (G = 0).  Measured on MI355X at B = 256 (profiles/conv_bwd_fused.json):
//   16 -> 32 channels, 432 x 64: 0.66 ms against 0.60 + 0.32 ms of the two kernels -> this kernel;
//   32 -> 64 channels, 216 x 32: 0.86 ms against 0.30 + 0.27 ms -> the two kernels: with 64 output channels the two
//     contractions are 228 MFMAs per wave and tile, the weight fragments do not fit in LDS beside the tile buffers and
//     the build spills; the matrix work, not HBM, sets its time;
//   the run-time-geometry builds are not measured on a product layer: not recommended.
// G: wgrad3_auto_g's rule for the pipelined kernel, one workgroup per CU.  With the same G and the same tiles per slab
// the slabs, and so dW after the reduction, keep the bits of bsed_wgrad3.  (More rounds of workgroups measured faster --
// 256 / 512 / 1024 / 2048 slabs: 0.99 / 0.87 / 0.85 / 0.83 ms with the wrapper's overhead -- but change the slab
// boundaries and with them the rounding of dW; not taken.)
static int cbwd_auto_g(const CbwdParams& P, const CbwdPlan& pl) {
  return pl.geo && pl.ntw == 1 ? (int)std::min<long>(256, P.ntiles) : 0;
}

template <int MAXS, int NTW, int GEO, int WL>
static int launch_cbwd(const CbwdParams& P, const BsedLaunch& L) {
  BSED_LABEL_ONLY(L, "cbwd3_kernel<%d, %d, %d, %d>", MAXS, NTW, GEO, WL);
  static BsedLdsOnce once;
  BSED_HIP(bsed_max_lds(once, (const void*)cbwd3_kernel<MAXS, NTW, GEO, WL>));
  hipLaunchKernelGGL((cbwd3_kernel<MAXS, NTW, GEO, WL>), L.grid, dim3(512), L.smem + (WL ? CBWD_WTAB(NTW) : 0), L.s, P);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}

// bsed_conv_bwd3 (plan == null: pointer and G checks and the launch) and its plan after ONE prepare step
static int bsed_run_conv_bwd(const BsedWgradDesc* desc, void* stream, BsedContractPlan* plan) {
  CbwdParams P;
  size_t smem;
  const int rc = cbwd_prepare(desc, P, smem);
  if (rc != BSED_OK) return rc;
  const BsedWgradDesc& d = P.d;
  const CbwdPlan pl = cbwd_plan(P);
  BsedLaunch L;
  if (plan) L = bsed_plan_begin(plan, cbwd_auto_g(P, pl), P.ntiles, 0);
  else {
    const char* who = "bsed_conv_bwd3";
    BSED_CHECK_ARG(d.in && d.dy && d.part && d.bn_y && d.bn_coef && d.bn_mean && d.w3s && d.d_in, "%s: null tensor", who);
    BSED_CHECK_ARG(!d.a_scale && !d.a_shift && !d.dy_out, "%s: no input affine and no dy_out (d_y stays on the chip)", who);
    BSED_CHECK_ARG(d.d_in != d.in && d.d_in != d.dy && d.d_in != d.bn_y, "%s: d_in must not alias in, dy or bn_y "
                   "(other workgroups still read them)", who);
    BSED_CHECK_ARG(d.G > 0 && d.G <= P.ntiles, "%s: G (%d) must be in 1..%d tiles", who, d.G, P.ntiles);
    L = BsedLaunch{dim3((unsigned)d.G), smem, (hipStream_t)stream, nullptr};
  }
  // the 16 -> 32 form keeps the data gradient's 36 KB of weight fragments in LDS (97 + 36 KB); 64 output channels leave
  // no room for their 72 KB
  if (pl.geo) return pl.ntw == 1 ? launch_cbwd<2, 1, 1, 1>(P, L) : launch_cbwd<5, 2, 1, 0>(P, L);
  if (pl.ntw == 1) return launch_cbwd<3, 1, 0, 0>(P, L);
  return pl.maxs == 3 ? launch_cbwd<3, 2, 0, 0>(P, L) : launch_cbwd<5, 2, 0, 0>(P, L);
}
extern "C" int bsed_conv_bwd_plan(const BsedWgradDesc* desc, BsedContractPlan* out) {
  BSED_CHECK_ARG(desc && out, "bsed_conv_bwd_plan: null argument");
  return bsed_run_conv_bwd(desc, nullptr, out);
}
extern "C" int bsed_conv_bwd3(const BsedWgradDesc* desc, void* stream) { return bsed_run_conv_bwd(desc, stream, nullptr); }
