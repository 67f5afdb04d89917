// Shared device/host helpers for the bsed HIP library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include "../../include/bsed.h"

#define BSED_OK 0
#define BSED_ERR_ARG (-1)
#define BSED_ERR_HIP (-2)
#define BSED_ERR_STATE (-3)

void bsed_set_error(const char* fmt, ...);
// device-resident step state (capi.hip): null in eager mode
const uint64_t* bsed_seed_add_ptr();
const int* bsed_step_add_ptr();
const float* bsed_lr_ptr();

#define BSED_CHECK_ARG(cond, ...)                 \
  do {                                            \
    if (!(cond)) {                                \
      bsed_set_error(__VA_ARGS__);                \
      return BSED_ERR_ARG;                        \
    }                                             \
  } while (0)

#define BSED_LAUNCH_CHECK()                                                         \
  do {                                                                              \
    hipError_t e__ = hipGetLastError();                                             \
    if (e__ != hipSuccess) {                                                        \
      bsed_set_error("%s:%d HIP launch error: %s", __FILE__, __LINE__,              \
                     hipGetErrorString(e__));                                       \
      return BSED_ERR_HIP;                                                          \
    }                                                                               \
  } while (0)

#define BSED_HIP(call)                                                              \
  do {                                                                              \
    hipError_t e__ = (call);                                                        \
    if (e__ != hipSuccess) {                                                        \
      bsed_set_error("%s:%d %s: %s", __FILE__, __LINE__, #call,                     \
                     hipGetErrorString(e__));                                       \
      return BSED_ERR_HIP;                                                          \
    }                                                                               \
  } while (0)

// Kernels that need more than 64 KB of dynamic LDS have hipFuncAttributeMaxDynamicSharedMemorySize raised once per
// (kernel, DEVICE): the attribute is per device, so the guard is a per-kernel atomic bitmask indexed by the current
// device, not a process-wide flag (a second GPU in the same process, or two host threads, stay correct; setting
// the attribute twice in a race is harmless).
#include <atomic>
struct BsedLdsOnce { std::atomic<uint64_t> mask{0}; };
static inline hipError_t bsed_max_lds(BsedLdsOnce& once, const void* fn, int bytes = 160 * 1024) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = 1ull << (dev & 63);
  if (once.mask.load(std::memory_order_acquire) & bit) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) once.mask.fetch_or(bit, std::memory_order_release);
  return e;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bsed_bf16x2 __attribute__((ext_vector_type(2)));

// Split-fp32 operands: x = hi + lo with hi = bf16(x), lo = bf16(x - hi), both round-to-nearest-even.  gfx950 converts
// two floats to a packed bf16 pair in ONE instruction (v_cvt_pk_bf16_f32); the integer-arithmetic rounding used before
// cost ~11 VALU instructions per element and made the staging loops of the split-fp32 kernels issue-bound.
//   hi / lo : packed pairs, element a in the low half
__device__ __forceinline__ void bsed_split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  const f32x2 v = {a, b};
  hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bsed_bf16x2));
  const f32x2 r = {a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xFFFF0000u)};
  lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bsed_bf16x2));
}
typedef float f32x16 __attribute__((ext_vector_type(16)));

// The tile of the fp32-core contraction (igemm.hip) and of the weight gradients (wgrad.hip): 128 output positions, staged
// by 256 threads in the forward kernel
#define IG_THREADS 256
#define IG_TILE_M 128

#if defined(__HIPCC__)
// row of accumulator register r in the C layout of a 32 x 32 MFMA (lh = lane >> 5; pinned on hardware by bsed_selftest_mfma)
__device__ __forceinline__ int crow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// ----------------------------------------------------------------------------------------------
// Activation storage of a kernel instance: ABF = 0 fp32, ABF = 1 bf16 (the "bf16" throughput mode of BASELINE
// configs[1-2]: conv outputs, pooled outputs and their gradients are bf16 in HBM; accumulation, BatchNorm statistics,
// master weights and the optimizer stay fp32).  The C ABI keeps `float*` parameter types; with act_bf16 set they
// point to bf16 tensors.
// ----------------------------------------------------------------------------------------------
typedef uint32_t bsed_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float bsed_bf2f(uint32_t h16) { return __uint_as_float(h16 << 16); }
template <int ABF> __device__ __forceinline__ float act_ld(const float* base, size_t i) {
  if (ABF) return bsed_bf2f(reinterpret_cast<const unsigned short*>(base)[i]);
  return base[i];
}
// two-phase form for groups of per-element loads: act_ld_raw issues the load and returns its bits untouched, act_cvt
// turns them into the value LATER.  (With the conversion next to the load hipcc placed every bf16 load's shift -- and
// so an s_waitcnt vmcnt(0) -- directly behind it: one load in flight at a time, the bf16 GLU backward 40 % slower than
// the fp32 one.)  Put __builtin_amdgcn_sched_barrier(0) between the load group and the first act_cvt.
template <int ABF> __device__ __forceinline__ uint32_t act_ld_raw(const float* base, size_t i) {
  if (ABF) return reinterpret_cast<const unsigned short*>(base)[i];
  return __float_as_uint(base[i]);
}
template <int ABF> __device__ __forceinline__ float act_cvt(uint32_t raw) {
  return __uint_as_float(ABF ? raw << 16 : raw);
}
template <int ABF> __device__ __forceinline__ void act_st(float* base, size_t i, float v) {
  if (ABF) reinterpret_cast<__bf16*>(base)[i] = (__bf16)v;   // round to nearest even
  else base[i] = v;
}
// 8 consecutive elements starting at element i (i a multiple of 8): one 16-byte load (bf16) or two (fp32)
template <int ABF> __device__ __forceinline__ void act_ld8(const float* base, size_t i, float* v) {
  if (ABF) {
    const bsed_u32x4 r = *reinterpret_cast<const bsed_u32x4*>(reinterpret_cast<const unsigned short*>(base) + i);
#pragma unroll
    for (int q = 0; q < 4; ++q) { v[2 * q] = __uint_as_float(r[q] << 16); v[2 * q + 1] = __uint_as_float(r[q] & 0xFFFF0000u); }
  } else {
    const f32x4 a = *reinterpret_cast<const f32x4*>(base + i), b = *reinterpret_cast<const f32x4*>(base + i + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
  }
}
// 4 consecutive elements starting at element i (i a multiple of 4)
template <int ABF> __device__ __forceinline__ f32x4 act_ld4(const float* base, size_t i) {
  if (ABF) {
    const uint2 r = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(base) + i);
    return f32x4{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xFFFF0000u), __uint_as_float(r.y << 16),
                 __uint_as_float(r.y & 0xFFFF0000u)};
  }
  return *reinterpret_cast<const f32x4*>(base + i);
}
template <int ABF> __device__ __forceinline__ void act_st4(float* base, size_t i, f32x4 v) {
  if (ABF) {
    const f32x2 a = {v[0], v[1]}, b = {v[2], v[3]};
    uint2 r;
    r.x = __builtin_bit_cast(uint32_t, __builtin_convertvector(a, bsed_bf16x2));
    r.y = __builtin_bit_cast(uint32_t, __builtin_convertvector(b, bsed_bf16x2));
    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(base) + i) = r;
  } else {
    *reinterpret_cast<f32x4*>(base + i) = v;
  }
}

// ----------------------------------------------------------------------------------------------
// Split-fp32 operand images of the weight-gradient family (wgrad.hip, conv_bwd.hip): position-major bf16 hi / lo planes
// in LDS, read as MFMA fragments through gfx950's transposing LDS read (the layout and its swizzle: wgrad.hip).
// ----------------------------------------------------------------------------------------------
typedef short w3_bf16x8 __attribute__((ext_vector_type(8)));
typedef short w3_bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) unsigned short w3_lds_u16;
typedef __attribute__((address_space(3))) w3_bf16x4 w3_lds_v4;
typedef uint32_t w3_u32x2 __attribute__((ext_vector_type(2)));
typedef float w3_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) w3_u32x2 w3_lds_u2;

// physical 32-channel chunk of logical chunk `ch` in the row of position / patch column pc (nch = chunks per row: 1, 2
// or 4): 4 consecutive pc x 64 B then tile the 64 banks
__device__ __forceinline__ int w3_chunk(int ch, int pc, int nch) {
  return ch ^ ((nch == 2 ? (pc >> 1) : pc) & (nch - 1));
}

// 8 consecutive positions of this lane's channel: two transposing reads of 4 rows each.  a0 / a1 are LDS BYTE
// addresses (plane base included, so that no base add is left in the K loop)
__device__ __forceinline__ w3_bf16x8 w3_frag(uint32_t a0, uint32_t a1) {
  const w3_bf16x4 u = __builtin_amdgcn_ds_read_tr16_b64_v4i16((w3_lds_v4*)(uintptr_t)a0);
  const w3_bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((w3_lds_v4*)(uintptr_t)a1);
  return __builtin_shufflevector(u, v, 0, 1, 2, 3, 4, 5, 6, 7);
}

// 4 channels of one position -> the two planes (ABF, the bf16 mode: the hi plane alone)
template <int ABF = 0>
__device__ __forceinline__ void w3_store4(w3_lds_u16* hi_plane, w3_lds_u16* lo_plane, int o, const float4& v) {
  w3_u32x2 hi, lo;
  uint32_t h0, l0, h1, l1;
  bsed_split2(v.x, v.y, h0, l0);
  bsed_split2(v.z, v.w, h1, l1);
  hi[0] = h0; hi[1] = h1; lo[0] = l0; lo[1] = l1;
  *(w3_lds_u2*)(hi_plane + o) = hi;
  if (!ABF) *(w3_lds_u2*)(lo_plane + o) = lo;
}
// activation loads / stores through a pointer computed in ELEMENTS from the tensor base (ABF: the tensor is bf16)
template <int ABF> __device__ __forceinline__ float4 w3_ld4(const float* base, const float* q) {
  const f32x4 t = act_ld4<ABF>(base, (size_t)(q - base));
  return make_float4(t[0], t[1], t[2], t[3]);
}
template <int ABF> __device__ __forceinline__ void w3_st4(float* base, float* q, const float4& v) {
  act_st4<ABF>(base, (size_t)(q - base), f32x4{v.x, v.y, v.z, v.w});
}
template <int ABF>
__device__ __forceinline__ f32x16 w3_mfma(const w3_bf16x8& a_hi, const w3_bf16x8& a_lo, const w3_bf16x8& b_hi,
                                          const w3_bf16x8& b_lo, f32x16 acc) {
  if (!ABF) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, acc, 0, 0, 0);
  }
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc, 0, 0, 0);
}
#endif

static inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// log2 of a power of two, -1 for anything else
static inline int ilog2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

// Host side of every tiled contraction (bsed_igemm, bsed_igemm3, bsed_igemm3s, bsed_igemm3n, bsed_wgrad*): checks the
// shape, tile, tap, input-pitch and padding fields that BsedIgemmDesc and BsedWgradDesc share (P.d, already copied
// from the caller's descriptor) and fills the geometry the kernels derive their addresses from: P.lgTW, d.tilesH,
// d.tilesW, P.PW / PH / PP (the tile plus its halo) and P.pw_magic (pos / PW == (pos * pw_magic) >> 20 for every
// position of the patch, verified here).  `who` = the entry point, for the messages; cin_mult = what CIN must be a
// multiple of; pitch_align = what in_pitch must be a multiple of (elements).  Returns the number of position tiles
// (below 2^31) or BSED_ERR_ARG; makes no HIP call.
template <class Params>
static int bsed_tile_geometry(Params& P, const char* who, int cin_mult, int pitch_align) {
  auto& d = P.d;
  BSED_CHECK_ARG(d.NB > 0 && d.H > 0 && d.W > 0 && d.CIN > 0 && d.N > 0, "%s: bad shape", who);
  BSED_CHECK_ARG(d.CIN % cin_mult == 0, "%s: CIN must be a multiple of %d", who, cin_mult);
  BSED_CHECK_ARG(d.TH * d.TW == 128, "%s: TH*TW must be 128 (got %dx%d)", who, d.TH, d.TW);
  P.lgTW = ilog2_exact(d.TW);
  BSED_CHECK_ARG(P.lgTW >= 0, "%s: TW must be a power of two", who);
  BSED_CHECK_ARG(d.W % d.TW == 0, "%s: TW must divide W", who);
  BSED_CHECK_ARG(d.ntaps >= 1 && d.ntaps <= 9, "%s: ntaps must be in 1..9", who);
  for (int t = 0; t < d.ntaps; ++t)
    BSED_CHECK_ARG(abs(d.dh[t]) <= d.hh && abs(d.dw[t]) <= d.hw, "%s: tap %d outside the halo", who, t);
  BSED_CHECK_ARG(d.in_pitch >= d.CIN && d.in_pitch % pitch_align == 0, "%s: bad pitch", who);
  BSED_CHECK_ARG(d.NP % 32 == 0 && d.NP >= d.N, "%s: NP must be N rounded up to 32", who);
  d.tilesH = ceil_div(d.H, d.TH);
  d.tilesW = d.W / d.TW;
  P.PW = d.TW + 2 * d.hw;
  P.PH = d.TH + 2 * d.hh;
  P.PP = P.PW * P.PH;
  P.pw_magic = ((1 << 20) + P.PW - 1) / P.PW;
  for (int pos = 0; pos < P.PP; ++pos)
    BSED_CHECK_ARG(((pos * P.pw_magic) >> 20) == pos / P.PW, "%s: internal: magic division fails for PW=%d", who, P.PW);
  const long ntiles = (long)d.NB * d.tilesH * d.tilesW;
  BSED_CHECK_ARG(ntiles < (1L << 31), "%s: too many tiles", who);
  return (int)ntiles;
}

// ----------------------------------------------------------------------------------------------
// Host side of the six contraction entry points (BsedContractPlan, include/bsed.h).  Each kernel has ONE function
// bsed_run_*(desc, stream, plan): its prepare step (shape checks, geometry, LDS bytes, grid), then either the pointer / G
// checks and the launch (plan == null: the entry point) or the plan's numbers and the label (capi.hip's queries).
// ----------------------------------------------------------------------------------------------
int bsed_run_igemm(const BsedIgemmDesc* desc, void* stream, BsedContractPlan* plan);
int bsed_run_igemm3(const BsedIgemmDesc* desc, void* stream, BsedContractPlan* plan);
int bsed_run_igemm3s(const BsedIgemmDesc* desc, void* stream, BsedContractPlan* plan);
int bsed_run_igemm3n(const BsedIgemmDesc* desc, void* stream, BsedContractPlan* plan);
int bsed_run_wgrad(const BsedWgradDesc* desc, int mode3, void* stream, BsedContractPlan* plan);
// What a template dispatch of the family is handed: a launch or, with `label` set, the request to NAME the instance
// instead of launching it.  Every leaf launcher opens with BSED_LABEL_ONLY(L, "kernel<%d, ...>", its own template
// arguments): the label is spelled from the constants the launch below it is instantiated with, as rocprofv3 prints them.
struct BsedLaunch { dim3 grid; size_t smem; hipStream_t s; char* label; };
#define BSED_LABEL_ONLY(L, ...) \
  do { if ((L).label) { snprintf((L).label, sizeof(BsedContractPlan::label), __VA_ARGS__); return BSED_OK; } } while (0)
static inline BsedLaunch bsed_plan_begin(BsedContractPlan* out, int G, int max_G, int stats_rows) {
  out->G = G; out->max_G = max_G; out->stats_rows = stats_rows; out->label[0] = 0;
  return BsedLaunch{dim3(), 0, nullptr, out->label};
}
// output channels per workgroup of bsed_igemm, bsed_igemm3 and bsed_igemm3n: the widest of 128 / 64 / 32 dividing NP
static inline int bsed_contract_bn(int NP) { return NP % 128 == 0 ? 128 : (NP % 64 == 0 ? 64 : 32); }
// what the prepare steps of bsed_igemm3, bsed_igemm3s and bsed_igemm3n begin with (returns the tile count) ...
template <class Params>
static int bsed_igemm3_front(const BsedIgemmDesc* desc, Params& P, const char* who, int cin_mult, int pitch_align) {
  BSED_CHECK_ARG(desc, "%s: null descriptor", who);
  P.d = *desc;
  BSED_CHECK_ARG(P.d.epilogue == BSED_EPI_PLAIN || P.d.epilogue == BSED_EPI_STATS, "%s: PLAIN / STATS epilogues only", who);
  const int ntiles = bsed_tile_geometry(P, who, cin_mult, pitch_align);
  if (ntiles >= 0) BSED_CHECK_ARG(P.d.out_pitch >= P.d.N, "%s: bad pitch", who);
  return ntiles;
}
// ... and the pointer checks their entry points add
static inline int bsed_igemm3_pointers(const BsedIgemmDesc& d, const char* who) {
  BSED_CHECK_ARG(d.in && d.w && d.out, "%s: null tensor", who);
  BSED_CHECK_ARG(d.epilogue != BSED_EPI_STATS || d.stats, "%s: STATS needs a stats buffer", who);
  return BSED_OK;
}

// ----------------------------------------------------------------------------------------------
// Host side of the eight GLU / first-block entry points (BsedGluDesc, include/bsed.h).  No HIP call is made here.
// ----------------------------------------------------------------------------------------------
// What bsed_glu_plan answers, for the entry point `kernel` (BSED_GLU_*) and the shape fields of d: every shape check of
// the family (the stricter one where the former per-file copies differed) and every grid size, slab count and template
// choice, with the measurements behind them.  The entry points launch what this returns.
static inline const char* bsed_glu_name(int kernel) {   // the entry point of a BSED_GLU_* id, for the messages
  static const char* const names[] = {"bsed_glu16_fwd", "bsed_glu16_bwd", "bsed_block0_fwd", "bsed_block0_bwd",
                                      "bsed_glu_bwd_fused", "bsed_glu_fwd3", "bsed_glu_bwd3", "bsed_glu_bwd3n"};
  return kernel >= 0 && kernel < 8 ? names[kernel] : nullptr;
}
static inline int bsed_glu_plan_for(const BsedGluDesc& d, int kernel, BsedGluPlan& p) {
  const char* who = bsed_glu_name(kernel);
  BSED_CHECK_ARG(who, "bsed_glu_plan: unknown kernel %d", kernel);
  const bool tiled = kernel >= BSED_GLU_BWD_FUSED, glu3 = kernel >= BSED_GLU_FWD3;
  const bool block0 = kernel == BSED_GLU_BLOCK0_FWD || kernel == BSED_GLU_BLOCK0_BWD;
  const int C = d.C;
  BSED_CHECK_ARG(d.NB > 0 && d.H > 0 && d.W > 0, "%s: bad shape", who);
  BSED_CHECK_ARG((d.ph == 1 || d.ph == 2) && (d.pw == 1 || d.pw == 2), "%s: pooling windows must be 1 or 2", who);
  BSED_CHECK_ARG(d.act_bf16 == 0 || (d.act_bf16 == 1 && (glu3 || block0)), "%s: no bf16 activations (act_bf16 = %d)",
                 who, d.act_bf16);
  if (!tiled) BSED_CHECK_ARG(C == 16, "%s: built for 16 channels (got %d)", who, C);
  else if (kernel == BSED_GLU_BWD3) BSED_CHECK_ARG(C == 32 || C == 64, "%s: built for C in {32,64} (got %d)", who, C);
  else if (kernel == BSED_GLU_BWD3N) BSED_CHECK_ARG(C == 128, "%s: built for C = 128 (got %d)", who, C);
  else BSED_CHECK_ARG(C == 32 || C == 64 || C == 128, "%s: built for C in {32,64,128} (got %d)", who, C);
  const long positions = (long)d.NB * d.H * d.W;
  p.dw_rows = 0; p.variant = 0; p.table_bytes = 0;
  if (!tiled) {
    BSED_CHECK_ARG(d.TH == 0 && d.TW == 0, "%s: a streaming kernel without a tile: TH = TW = 0 (got %dx%d)", who, d.TH,
                   d.TW);
    BSED_CHECK_ARG(d.W % d.pw == 0 && d.H >= d.ph, "%s: bad shape (W %% pw == 0, H >= ph)", who);
    BSED_CHECK_ARG(!block0 || positions < (1L << 31), "%s: too many positions", who);
    const long rows = (long)d.NB * (d.H / d.ph);   // pooled rows: the work items of the forward kernels
    long items = rows, g = std::min<long>(rows, 8192);
    if (kernel == BSED_GLU_16_BWD) {               // items: (row, 64-column chunk)
      items = (long)d.NB * d.H * ((d.W + 63) / 64);
      g = std::min<long>(2048, (long)d.NB * d.H);
    } else if (kernel == BSED_GLU_BLOCK0_FWD) {    // items: (pooled row, 128-column chunk)
      items = rows * ((d.W + 127) / 128);
      g = std::min<long>(items, 8192);
    } else if (kernel == BSED_GLU_BLOCK0_BWD) {    // items: (pooled row, 64-column chunk)
      items = rows * ((d.W + 63) / 64);
      g = std::min<long>(8192, rows);              // 2048 / 4096 / 8192 workgroups: 0.983 / 0.966 / 0.957 ms
    }
    BSED_CHECK_ARG(items < (1L << 30), "%s: too many rows", who);   // item + G stays an int in the prefetching loops
    p.G = (int)g; p.max_G = (int)items;
    if (kernel == BSED_GLU_16_BWD || kernel == BSED_GLU_BLOCK0_BWD) p.dw_rows = p.G;
    // block0 SMALL: fewer than 2^28 positions (every tensor below 4 GB, element counters below 2^32): 32-bit offsets;
    // the bf16 forward is built without it
    if (block0) p.variant = d.ph | (positions < (1L << 28) && !(d.act_bf16 && kernel == BSED_GLU_BLOCK0_FWD) ? 16 : 0);
    return BSED_OK;
  }
  BSED_CHECK_ARG(d.TH * d.TW == 128, "%s: TH*TW must be 128 (got %dx%d)", who, d.TH, d.TW);
  const int lgTW = ilog2_exact(d.TW);
  BSED_CHECK_ARG(lgTW >= 0, "%s: TW must be a power of two", who);
  BSED_CHECK_ARG(d.W % d.TW == 0, "%s: TW must divide W", who);
  const long ntiles = (long)d.NB * ceil_div(d.H, d.TH) * (d.W / d.TW);
  BSED_CHECK_ARG(ntiles < (1L << 31), "%s: too many tiles", who);
  BSED_CHECK_ARG(!glu3 || positions * C < (1L << 32),
                 "%s: activation tensor beyond the 32-bit element offsets of this kernel", who);
  // persistent kernels: G = the workgroups of one resident round (LDS- and register-limited occupancy x 256 CUs)
  int round = 0, slabs = 0;
  if (kernel == BSED_GLU_BWD_FUSED) {
    round = C == 128 ? 256 : (C == 64 ? 512 : 768);
    slabs = C == 128 ? 1 : (C == 64 ? 2 : 4);      // waves that share one dW row-tile split the positions (KSPLIT)
    p.variant = C == 128 ? 8 : 4;                  // NW
  } else if (kernel == BSED_GLU_FWD3) {
    // measured (B = 256): C = 32: 512 / 768 / 1024 / 1536 workgroups 0.447 / 0.367 / 0.412 / 0.350 ms; C = 64: 0.180 / 0.160 / 0.167 / 0.155;
    // C = 128 (64 KB of weight fragments in LDS, two per CU): 256 / 512 / 768 / 1024 0.514 / 0.422 / 0.454 / 0.435
    round = C == 128 ? 512 : 1536;
  } else if (kernel == BSED_GLU_BWD3) {
    round = C == 32 ? 768 : 512;
    slabs = 4;                                     // one per wave
  } else {
    round = 256;                                   // 8-wave workgroups take two tiles at a time
    p.table_bytes = (size_t)2 * 4 * 8 * 2 * 64 * 16;   // both weight operands pre-split into fragment order
  }
  p.max_G = (int)(kernel == BSED_GLU_BWD3N ? (ntiles + 1) / 2 : ntiles);
  p.G = std::min(p.max_G, round);
  p.dw_rows = p.G * slabs;
  // glu_fwd3 / glu_bwd3 are also built with the tile width of the wide maps (16) as a compile-time constant
  if (kernel == BSED_GLU_FWD3 || kernel == BSED_GLU_BWD3) p.variant = lgTW == 4 ? 4 : -1;
  return BSED_OK;
}

// The argument check of an entry point: the plan's shape checks, then `reads` = the pointer fields it wants (bit i =
// the i-th pointer of BsedGluDesc in declaration order; every other one must be null) and G in 1..max_G.  seed_add
// receives the device-resident seed addend of the step state (capi.hip) -- the family's one read of it.
static inline int bsed_glu_args(const BsedGluDesc* desc, int kernel, unsigned reads, BsedGluPlan& plan,
                                const uint64_t*& seed_add) {
  const char* who = bsed_glu_name(kernel);
  BSED_CHECK_ARG(desc, "%s: null descriptor", who);
  const BsedGluDesc& d = *desc;
  const int rc = bsed_glu_plan_for(d, kernel, plan);
  if (rc) return rc;
  static const char* const names[] = {"x", "y", "cw", "cb", "scale", "shift", "w", "wfwd", "bias", "dpool", "pooled", "g",
                                      "dlin", "part_dw", "part_db", "part_st", "part_gx", "frag_table"};
  const void* const ptrs[] = {d.x, d.y, d.cw, d.cb, d.scale, d.shift, d.w, d.wfwd, d.bias, d.dpool, d.pooled, d.g,
                              d.dlin, d.part_dw, d.part_db, d.part_st, d.part_gx, d.frag_table};
  for (int i = 0; i < 18; ++i) {
    const bool wants = (reads >> i) & 1;
    BSED_CHECK_ARG(wants == (ptrs[i] != nullptr), wants ? "%s: null tensor %s" : "%s: does not read %s: it must be null",
                   who, names[i]);
  }
  BSED_CHECK_ARG(d.G > 0 && d.G <= plan.max_G, "%s: G must be in 1..%d (got %d)", who, plan.max_G, d.G);
  seed_add = bsed_seed_add_ptr();
  return BSED_OK;
}
enum : unsigned {   // `reads` of bsed_glu_args
  GLU_X = 1u << 0, GLU_Y = 1u << 1, GLU_CONV = 3u << 2 /* cw, cb */, GLU_BN = 3u << 4 /* scale, shift */, GLU_W = 1u << 6,
  GLU_WFWD = 1u << 7, GLU_BIAS = 1u << 8, GLU_DPOOL = 1u << 9, GLU_POOLED = 1u << 10, GLU_G = 1u << 11,
  GLU_DLIN = 1u << 12, GLU_PART_DW = 1u << 13, GLU_PART_B = 3u << 14 /* part_db, part_st */, GLU_PART_GX = 1u << 16,
  GLU_FRAG = 1u << 17,
  GLU_LIN = GLU_BN | GLU_W | GLU_BIAS   // BatchNorm apply + the Linear layer
};

// bsed_glu_args for the tiled kernels (glu3.hip, glu_bwd.hip), then the fields Glu3Params and GluBwdParams share by
// name: the descriptor's tensors, the tile geometry, the pooled extent, the dropout fields and the seed addend.  The
// caller sets the tensors only one of the structs has.
template <class Params>
static int bsed_glu_geometry(Params& P, const BsedGluDesc* desc, int kernel, unsigned reads, BsedGluPlan& plan) {
  const int rc = bsed_glu_args(desc, kernel, reads, plan, P.seed_add);
  if (rc) return rc;
  const BsedGluDesc& d = *desc;
  P.y = d.y; P.scale = d.scale; P.shift = d.shift; P.bias = d.bias; P.dpool = d.dpool;
  P.g = d.g; P.part_dw = d.part_dw; P.part_db = d.part_db; P.part_st = d.part_st;
  P.NB = d.NB; P.H = d.H; P.W = d.W; P.TH = d.TH; P.TW = d.TW;
  P.lgTW = ilog2_exact(d.TW);
  P.tilesH = ceil_div(d.H, d.TH); P.tilesW = d.W / d.TW;
  P.ntiles = d.NB * P.tilesH * P.tilesW;
  P.ph = d.ph; P.pw = d.pw; P.Hp = d.H / d.ph; P.Wp = d.W / d.pw;
  P.drop_p = d.drop_p; P.rng_stream = d.rng_stream; P.seed = d.seed;
  return BSED_OK;
}

#if defined(__HIPCC__)
// ----------------------------------------------------------------------------------------------
// Philox4x32-10 counter RNG: stateless, keyed on (seed, stream) with a 64-bit element counter, so
// forward and backward regenerate identical dropout masks without storing them.
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox4x32(uint64_t counter, uint32_t stream, uint64_t seed) {
  uint32_t c0 = (uint32_t)counter, c1 = (uint32_t)(counter >> 32), c2 = stream, c3 = 0x5eed5eedu;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

// keep-mask for one element: element index e -> 32-bit word (e & 3) of philox(e >> 2)
__device__ __forceinline__ float dropout_scale(uint64_t e, uint32_t stream, uint64_t seed, float p) {
  if (p <= 0.f) return 1.f;
  uint4 r = philox4x32(e >> 2, stream, seed);
  uint32_t w = (e & 3) == 0 ? r.x : (e & 3) == 1 ? r.y : (e & 3) == 2 ? r.z : r.w;
  // uniform in [0,1): keep if u >= p
  float u = (float)(w >> 8) * (1.0f / 16777216.0f);
  return u >= p ? 1.0f / (1.0f - p) : 0.f;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// v_exp_f32 + v_rcp_f32 (1 ulp each): relative error <= ~|x| * 6e-8, used in the streaming epilogues
__device__ __forceinline__ float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// ----------------------------------------------------------------------------------------------
// Dropout masks for the fused epilogues: a 32-bit mix hash ("lowbias32") of the element index keyed on
// (seed, layer stream).  ~8 VALU instructions per element instead of ~100 for Philox, stateless, identical
// in forward and backward.  (Philox stays for the Gaussian SNR noise.)
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t drop_key(uint32_t stream, uint64_t seed) {
  return mix32((uint32_t)seed ^ (stream * 0x9E3779B9u)) + mix32((uint32_t)(seed >> 32) ^ 0x85ebca6bu);
}
__device__ __forceinline__ uint32_t drop_threshold(float p) { return (uint32_t)(p * 16777216.0f); }
__device__ __forceinline__ float drop_mul(uint64_t e, uint32_t key, uint32_t thr, float scale) {
  const uint32_t h = mix32((uint32_t)e * 0x9E3779B1u + key + (uint32_t)(e >> 32) * 0x85ebca6bu);
  return (h >> 8) >= thr ? scale : 0.f;
}

// Two keep-multipliers from ONE hash (the first CNN block, whose per-element work is what bounds its kernels): the
// elements e (even) and e + 1 take the low / high 16 bits of the hash of e >> 1 against a 16-bit threshold.  The keep
// probability is 1 - floor(65536 p) / 65536: within 1.6e-5 of 1 - p for any p, exact for p = 0.5.
__device__ __forceinline__ uint32_t drop_threshold16(float p) { return (uint32_t)(p * 65536.0f); }
__device__ __forceinline__ void drop_mul2(uint64_t e_even, uint32_t key, uint32_t thr16, float scale, float& m0,
                                          float& m1) {
  const uint64_t e = e_even >> 1;
  const uint32_t h = mix32((uint32_t)e * 0x9E3779B1u + key + (uint32_t)(e >> 32) * 0x85ebca6bu);
  m0 = (h & 0xFFFFu) >= thr16 ? scale : 0.f;
  m1 = (h >> 16) >= thr16 ? scale : 0.f;
}

// the same two multipliers for element indices below 2^32 (the (e >> 32) term of drop_mul2 is zero there): 32-bit
// index arithmetic only
__device__ __forceinline__ void drop_mul2_32(uint32_t e_even, uint32_t key, uint32_t thr16, float scale, float& m0,
                                             float& m1) {
  const uint32_t h = mix32((e_even >> 1) * 0x9E3779B1u + key);
  m0 = (h & 0xFFFFu) >= thr16 ? scale : 0.f;
  m1 = (h >> 16) >= thr16 ? scale : 0.f;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
#endif
