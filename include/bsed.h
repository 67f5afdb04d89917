/* bsed.h -- C ABI of libbsed.so, the MI355X (gfx950) drop-in for the mel + CRNN train-step hot path
 * of fumchin/bird-sound-event-detecion.
 *
 * The reference is pure Python/PyTorch and has no FFI of its own: the drop-in
 * boundary is its Python API (CRNN / Predictor / preprocess / train_mt / update_ema_variables /
 * get_predictions).  The package `bird-sound-event-detecion_amd` mirrors that API and binds THIS
 * library with ctypes; each entry point below names the reference code it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller unless the
 *     comment says "host";  tensors are contiguous fp32 unless a pitch is given.
 *   - activations are NHWC: (N, H=time, W=freq, C).  A reference (B,1,T,F) input is the same bytes.
 *   - every call is asynchronous on `stream` (a hipStream_t; NULL = default stream); nothing
 *     allocates, frees or synchronises except the *_create / *_destroy pairs.
 *   - return 0 on success, <0 on failure; bsed_last_error() returns a thread-local message.
 */
#ifndef BSED_H
#define BSED_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* bsed_last_error(void);
/* "gfx950" build tag + ABI version, for the loader's sanity check */
const char* bsed_build_info(void);
int bsed_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Mel front end.   replaces preprocess()  (reference src/data/preprocess.py:18-45,
 * src/synth_data/synth_data_preprocess.py:15-42) and the DataLoader transforms
 * AugmentGaussianNoise / ApplyLog / PadOrTrunc (src/data/Transforms.py:74-86,89-139,155-196).
 * ---------------------------------------------------------------------------------------------- */
typedef struct BsedMelCfg {
  int sr;      /* 32000 (reference) or 22050 (BASELINE measurement config) */
  int n_fft;   /* 2048 */
  int hop;     /* 255 */
  int n_mels;  /* 128 */
  float fmin;  /* 0 */
  float fmax;  /* 16000 (must be <= sr/2) */
} BsedMelCfg;

int bsed_mel_plan_create(const BsedMelCfg* cfg /*host*/, void** plan /*host out*/);
int bsed_mel_plan_destroy(void* plan);
int bsed_mel_plan_nnz(const void* plan);                    /* non-zeros of the filterbank */
int bsed_mel_plan_frames_per_wave(const void* plan);        /* 2: bsed_mel_linear runs stft_mel2_kernel (two frames per wave), 1: stft_mel_kernel */
int bsed_mel_num_frames(const void* plan, int n_samples);   /* 1 + n_samples / hop */
/* wav (B, n_samples) -> LINEAR mel amplitude (B, T, n_mels) == preprocess(audio).  Also emits the
 * per-clip max (B) and the per-(clip, band) sum over time of x^2 (B, n_mels), which the dB clamp and
 * the SNR noise need, so neither costs another pass over HBM.  scratch: bsed_mel_scratch_floats(plan, B, n_samples)
 * floats (per-workgroup partial sums of squares, added in fixed order: the result is bitwise repeatable). */
long bsed_mel_scratch_floats(const void* plan, int B, int n_samples);
int bsed_mel_linear(const void* plan, const float* wav, int B, int n_samples, float* mel_lin,
                    float* clip_max, float* bin_sumsq, float* scratch, void* stream);
/* the same two statistics for features that arrive as linear mel (the reference's wav/<name>.npy files) */
int bsed_mel_stats(const float* mel_lin, int B, int T, int n_mels, float* clip_max, float* bin_sumsq, void* stream);
/* noisy = mel + N(0,1) * sqrt(mean_t(mel^2) * 10^(-snr/10))  (AugmentGaussianNoise.gaussian_noise).
 * unit_noise (B,T,n_mels) may inject the N(0,1) draws (parity tests); NULL = Philox(seed). */
int bsed_mel_noise(const float* mel_lin, const float* bin_sumsq, const float* unit_noise, int B, int T,
                   int n_mels, float snr_db, uint64_t seed, float* noisy, float* clip_max_noisy,
                   void* stream);
/* librosa.amplitude_to_db(x, ref=1, amin=1e-5, top_db) per clip + zero pad / truncate to T_out
 * -> (B, T_out, n_mels), i.e. the (B,1,T_out,n_mels) CRNN input. */
int bsed_mel_db(const float* mel_lin, const float* clip_max, int B, int T, int T_out, int n_mels,
                float top_db, float* out_db, void* stream);
/* bsed_mel_db plus the two rolled views of the ISP shift-consistency step from one read of the linear mel:
 * out_db as bsed_mel_db writes it; out_db_tshift[b] = torch.roll(out_db[b], shift_frames[b], time);
 * out_db_fshift[b] = torch.roll(out_db[b], shift_bins[b], frequency)   (src/main_scmt_ada_weak.py:234-248).
 * The rolls act on the padded / truncated (T_out, n_mels) tensor; shifts (device int32, B each) of any sign or size
 * are taken modulo the axis length.  Three distinct (B, T_out, n_mels) outputs, bitwise bsed_mel_db + bsed_roll. */
int bsed_mel_db_views(const float* mel_lin, const float* clip_max, int B, int T, int T_out, int n_mels,
                      float top_db, const int* shift_frames, const int* shift_bins, float* out_db,
                      float* out_db_tshift, float* out_db_fshift, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dataset scaler (ABI 10; csrc/scaler.hip, csrc/mel.hip).   replaces Scaler.means / Scaler.normalize
 * (reference src/utilities/Scaler.py:38-110) and the Normalize(scaler) transform (src/data/Transforms.py:230-250).
 * ---------------------------------------------------------------------------------------------- */
/* acc (2, n_mels) float64 += per-band [sum of x, sum of x^2] of a batch, x being the dB feature bsed_mel_db would write
 * for T_out frames per clip, computed on the fly from LINEAR mel (B, T, n_mels) and clip_max (B): no dB tensor is
 * written.  Frames T <= t < T_out are 0 dB pad rows (they add nothing), frames t >= T_out are dropped.  x^2 is a float32
 * product, widened (the reference squares a float32 array); both sums accumulate in float64.  Every workgroup writes a
 * partial into scratch (bsed_scaler_scratch_doubles doubles) and a second kernel adds them to acc in a fixed order: no
 * floating-point atomics, bitwise repeatable.  n_mels 1..256 (full-width loads at 128), B <= 65535. */
long bsed_scaler_scratch_doubles(int B, int T, int T_out, int n_mels);
int bsed_scaler_accum(const float* mel_lin, const float* clip_max, int B, int T, int T_out, int n_mels,
                      float top_db, double* acc, double* scratch, void* stream);
/* the same from a dB tensor (B, T_out, n_mels) (features that are already transformed); scratch as for T = T_out */
int bsed_scaler_accum_db(const float* x_db, int B, int T_out, int n_mels, double* acc, double* scratch,
                         void* stream);
/* out = float32((float64(x) - mean[m]) / stdev[m]) over n_rows rows of n_mels bands: Scaler.normalize followed by
 * torch.Tensor(...).  mean, stdev: (n_mels) float64.  out may be x. */
int bsed_scaler_normalize(const float* x_db, long long n_rows, int n_mels, const double* mean, const double* stdev,
                          float* out, void* stream);
/* bsed_mel_db / bsed_mel_db_views with that normalisation as the epilogue: every element is
 * float32((float64(v) - mean[m]) / stdev[m]) with v bitwise what the unnormalised entry point writes (a pad row becomes
 * -mean / stdev).  In the views form the values are normalised BEFORE the rolls, as the reference rolls the normalised
 * batch: the frequency-rolled view carries each source band's statistics with it. */
int bsed_mel_db_norm(const float* mel_lin, const float* clip_max, int B, int T, int T_out, int n_mels,
                     float top_db, const double* mean, const double* stdev, float* out_db, void* stream);
int bsed_mel_db_views_norm(const float* mel_lin, const float* clip_max, int B, int T, int T_out, int n_mels,
                           float top_db, const int* shift_frames, const int* shift_bins, const double* mean,
                           const double* stdev, float* out_db, float* out_db_tshift, float* out_db_fshift,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM contraction on the fp32 matrix cores (v_mfma_f32_32x32x2_f32; csrc/igemm.hip).
 *   out[p][n] = sum_{tap,k} in[p + (dh,dw)(tap)][k] * w[tap][k][n]      zero padding outside (H,W)
 * One body, selected by `epilogue`, replaces the stock ATen/cuDNN ops the reference reaches through
 *   nn.Conv2d 3x3 + train-mode BatchNorm2d statistics   (src/models/CNN.py:46-49)       BSED_EPI_STATS
 *   GLU = Linear(C,C)(bn(x)) * sigmoid(bn(x)), Dropout, AvgPool2d (CNN.py:5-16,59-67)  BSED_EPI_GLU_POOL
 *   their backward passes                                                BSED_EPI_GLU_BWD / _ADD_STATS2
 *   nn.GRU input projections x @ W_ih^T and data gradients (src/models/RNN.py:12)      BSED_EPI_PLAIN
 * ---------------------------------------------------------------------------------------------- */
enum {
  BSED_EPI_PLAIN = 0,      /* out = acc + bias                                                        */
  BSED_EPI_STATS = 1,      /* + per-tile (sum, sum of squares) per channel -> stats[tile][2][N]        */
  BSED_EPI_GLU_POOL = 2,   /* out = avgpool(dropout((acc+bias) * sigmoid(e_src*e_scale+e_shift)))      */
  BSED_EPI_GLU_BWD = 3,    /* out = d_lin, out2 = d_res*lin*sig*(1-sig); stats[tile][0][N] = sum d_lin */
  BSED_EPI_ADD_STATS2 = 4  /* out = acc + out2; stats = (sum g, sum g*e_src)                           */
};

typedef struct BsedIgemmDesc {
  const float* in;       /* (NB,H,W,in_pitch) NHWC; CIN <= in_pitch                                    */
  const float* w;        /* packed (ntaps, CIN, NP) by bsed_pack_weight                                */
  const float* bias;     /* (N) or NULL                                                                */
  float* out;            /* (NB,H,W,out_pitch)  [GLU_POOL: (NB,Hp,Wp,out_pitch)]                       */
  float* out2;           /* GLU_BWD: second output; ADD_STATS2: residual input (may alias out)         */
  float* stats;          /* (num_tiles, 2, N) per-tile partial sums                                    */
  const float* a_scale;  /* optional per-CIN affine applied while loading `in` (BatchNorm apply)       */
  const float* a_shift;
  const float* e_src;    /* epilogue side input (NB,H,W,e_pitch): pre-BN conv output                   */
  const float* e_scale;  /* (N) BatchNorm scale/shift of the gate branch                               */
  const float* e_shift;
  const float* e_dpool;  /* GLU_BWD: gradient w.r.t. the pooled output (NB,Hp,Wp,N)                    */
  int in_pitch, out_pitch, e_pitch;
  int NB, H, W, CIN, N, NP;   /* NP = N rounded up to a multiple of 32 (weight row stride)            */
  int TH, TW;                 /* spatial tile, TH*TW == 128, TW a power of two dividing W             */
  int tilesH, tilesW;         /* filled by the library                                                 */
  int hh, hw;                 /* halo rows / cols = max |dh| / |dw|                                    */
  int ntaps, dh[9], dw[9];
  int ph, pw, Hp, Wp;         /* pooling window and pooled extent (floor)                              */
  int epilogue;
  float drop_p;               /* dropout probability of the GLU epilogues (0 = off)                    */
  uint32_t rng_stream;        /* Philox stream id (layer id)                                           */
  uint64_t seed;
  int valid_h, valid_w;       /* 0 = H, W.  Otherwise only output positions (h < valid_h, w < valid_w) are stored and
                               * enter the STATS sums ("valid" convolutions computed on a padded grid: the stride-2
                               * discriminator layers run as 2x2 stride-1 convolutions over space-to-depth input,
                               * whose last row / column of the grid is not an output).  PLAIN / STATS epilogues. */
  int act_bf16;               /* bsed_igemm3n / bsed_igemm3s: 1 = `in` and `out` are bf16 tensors ("bf16" throughput mode:
                               * one bf16 MFMA per product, fp32 accumulation, bias and statistics); 0 = fp32 */
  int G;                      /* bsed_igemm3s: workgroups per 32 output channels, BsedContractPlan.G or any value in
                               * 1..max_G; the other entry points ignore it */
} BsedIgemmDesc;

/* What the library would launch for a contraction descriptor (ABI 12): one answer for the six entry points below. */
enum { BSED_CONTRACT_IGEMM = 0, BSED_CONTRACT_IGEMM3 = 1, BSED_CONTRACT_IGEMM3S = 2, BSED_CONTRACT_IGEMM3N = 3,
       BSED_CONTRACT_WGRAD = 4, BSED_CONTRACT_WGRAD3 = 5 };
typedef struct BsedContractPlan {
  int G;           /* recommended workgroups along grid.x: igemm3s / wgrad* the persistent-grid size, else the tile count */
  int max_G;       /* largest G the entry point accepts (position tiles) */
  int stats_rows;  /* rows of (2, N) the STATS-type epilogues write at that G; 0 for the weight gradients */
  char label[96];  /* the template instance the entry point would launch now, spelled as rocprofv3 prints it */
} BsedContractPlan;
/* Both queries run every shape check of the entry point `kernel` names, with its messages, and return BSED_ERR_ARG
 * where the launch would; they make no HIP call.  Pointers and G are ignored, except that a BsedWgradDesc with bn_y set
 * is planned as the BatchNorm-backward-on-load form it asks for.  `label` follows the bsed_igemm3n_set_* hooks and
 * BSED_WGRAD3_NOPIPE as they stand at the call. */
int bsed_igemm_plan(const BsedIgemmDesc* desc /*host*/, int kernel /*0..3*/, BsedContractPlan* out /*host*/);

int bsed_igemm(const BsedIgemmDesc* desc /*host*/, void* stream);

/* Same contraction with split-fp32 operands on the bf16 matrix cores ("bf16x3": a*b ~ a_hi*b_hi + a_hi*b_lo +
 * a_lo*b_hi, fp32 accumulate, ~1e-5 relative; csrc/igemm3.hip).  BSED_EPI_PLAIN / BSED_EPI_STATS only, CIN a
 * multiple of 32; desc->w must come from bsed_pack_weight3 (bf16 hi/lo planes, (ntaps, CIN/32, NP, 64) uint16). */
int bsed_igemm3(const BsedIgemmDesc* desc /*host*/, void* stream);
int bsed_pack_weight3(const float* src, void* dst, int ntaps, int K, int N, int NP, long s_tap, long s_k, long s_n,
                      void* stream);
/* CIN = 16 / 32 variant (the 16 -> 32 channel convolution, data gradients of 32-channel layers): weights of all taps
 * stay in LDS, CIN/16 MFMA K steps per tap,
 * persistent grid of desc->G workgroups per 32 output channels (bsed_igemm_plan); desc as for bsed_igemm3 with
 * w = bsed_pack_weight3s table ((NP/32) * ntaps * (K/16) * 2 * 64 * 16 bytes); STATS writes G partial rows (one per workgroup). */
int bsed_pack_weight3s(const float* src, void* dst, int ntaps, int K, int N, int NP, long s_tap, long s_k, long s_n,
                       void* stream);
/* several bsed_pack_weight3 (kind 0) / bsed_pack_weight3s (kind 1) re-layouts in one launch: the weights of a train step
 * are constant until its optimizer update, so every packed copy the step needs can be made at its start (same bits as the
 * single-job entries; the reference has no counterpart: its convolutions read the PyTorch weight tensors directly,
 * src/models/CNN.py:46-47) */
#define BSED_PACK_MAX_JOBS 32
typedef struct BsedPackJob {
  const float* src; void* dst;
  int kind, ntaps, K, N, NP;
  long s_tap, s_k, s_n;
} BsedPackJob;
int bsed_pack_weights_batch(const BsedPackJob* jobs /*host*/, int njobs, void* stream);
int bsed_igemm3s(const BsedIgemmDesc* desc /*host*/, void* stream);
/* The same contraction as bsed_igemm3 (same reference layers: src/models/CNN.py:46-47, the seven nn.Conv2d; GRU input
 * projections src/models/RNN.py:7-16) in the round-3 structure (csrc/igemm3n.hip): a wave owns 32 output channels and
 * fetches their weight fragments straight from global memory (w = bsed_pack_weight3s table, K any multiple of 32), the
 * activation patch is double-buffered in LDS, one barrier per 32-channel chunk.  `out` is bit-identical to
 * bsed_igemm3's; STATS writes BsedContractPlan.stats_rows partial rows of (2, N): 4 / NWN per tile. */
int bsed_igemm3n(const BsedIgemmDesc* desc /*host*/, void* stream);
void bsed_igemm3n_set_wpe(int knob);  /* test hook: 2 / 3 = the BN = 128 build for that many waves per SIMD whatever the
                                       * shape, + 8 = no raised wave priority outside the MFMA loop, 0 = default */
void bsed_igemm3n_set_shape(int shape); /* test hook: MFMA shape of the nine-tap instances, 16 = v_mfma_f32_16x16x32_bf16 (default with
                                         * fp32 activations), 32 = v_mfma_f32_32x32x16_bf16 (default with bf16 activations, and
                                         * bit-identical to bsed_igemm3); 0 = defaults */

/* Weight gradients (csrc/wgrad.hip).  dW[tap][k][n] = sum_p in[p + (dh,dw)(tap)][k] * dy[p][n]: persistent workgroups
 * over position tiles write partial slabs part[G][ntaps][CINP][NP]; bsed_reduce_partials sums them into the gradient. */
typedef struct BsedWgradDesc {
  const float* in;       /* (NB,H,W,in_pitch) */
  const float* dy;       /* (NB,H,W,dy_pitch) */
  float* part;           /* (G, ntaps, CINP, NP) */
  const float* a_scale;  /* optional per-CIN affine on `in` */
  const float* a_shift;
  int in_pitch, dy_pitch;
  int NB, H, W, CIN, CINP, N, NP, G;
  int TH, TW, tilesH, tilesW, hh, hw;
  int ntaps, dh[9], dw[9];
  /* BatchNorm backward applied on load (bsed_wgrad3 only; all four NULL = plain dy).  With bn_y set, `dy` holds
   * g = dL/d(BatchNorm output) and the contraction runs on d_y = A g + B (bn_y - mean) + C, bn_coef = (3,N) [A|B|C] from
   * bsed_bn_bwd, bn_y / dy_out laid out like dy.  dy_out (optional) receives d_y, written once per element, for the
   * data-gradient convolution that follows: the separate apply pass over g and y (3 tensor passes) is gone. */
  const float* bn_y;
  const float* bn_coef;
  const float* bn_mean;
  float* dy_out;
  int act_bf16;          /* bsed_wgrad3: 1 = in, dy, bn_y and dy_out are bf16 tensors ("bf16" mode: one bf16 MFMA per product,
                          * the BatchNorm-backward map and the accumulation in fp32); 0 = fp32 */
  /* bsed_conv_bwd3 only (ABI 14; the other entry points ignore the three): the data gradient of the same convolution */
  const void* w3s;       /* bsed_pack_weight3s table of the TRANSPOSED weight (K = N, N = CIN, the layer's nine taps) */
  float* d_in;           /* (NB,H,W,din_pitch): dL/d(in) */
  int din_pitch;
} BsedWgradDesc;

/* BsedContractPlan of bsed_wgrad (BSED_CONTRACT_WGRAD) / bsed_wgrad3 (BSED_CONTRACT_WGRAD3): G = the recommended number
 * of partial slabs, label = wgrad_kernel / wgrad3_kernel / wgrad3p_kernel / wgrad1_kernel with its template arguments */
int bsed_wgrad_plan(const BsedWgradDesc* desc /*host*/, int kernel /*4, 5*/, BsedContractPlan* out /*host*/);
int bsed_wgrad(const BsedWgradDesc* desc /*host*/, void* stream);
/* the same contraction with split-fp32 operands on the bf16 matrix cores (bf16x3, ~1e-5 relative): both tiles stay
 * position-major in LDS (bf16 hi / lo planes) and the operand fragments come out of transposing LDS reads; multi-tap
 * shapes whose two tile buffers fit in LDS run the producer/consumer kernel (wgrad3p_kernel).  Same descriptor, same
 * partial-slab layout; G should come from bsed_wgrad_plan (the recommendation differs between the kernels).
 * BSED_WGRAD3_NOPIPE=1 in the environment forces wgrad3_kernel (tests). */
int bsed_wgrad3(const BsedWgradDesc* desc /*host*/, void* stream);
/* Both gradients of a 3 x 3 / pad 1 convolution under a train-mode BatchNorm in ONE pass (ABI 14; csrc/conv_bwd.hip;
 * nn.Conv2d + nn.BatchNorm2d backward, reference src/models/CNN.py:46-49): the partial slabs of bsed_wgrad3 with BatchNorm
 * backward applied on load (bn_y, bn_coef, bn_mean required) AND d_in = conv^T(d_y, w) -- what bsed_wgrad3 with dy_out
 * followed by bsed_igemm3n computes -- without d_y ever leaving the chip: a persistent producer / consumer workgroup per
 * CU forms d_y for a 128-position tile plus its one-position ring (zeros outside the image) in LDS and runs both
 * contractions from it.  Split-fp32 mode, fp32 activations, the nine taps in row-major order, TW <= 16, CIN <= 32 (a
 * multiple of 4), N = 32 or 64, no a_scale / dy_out; two tile buffers must fit 160 KB of LDS (BSED_ERR_ARG otherwise).
 * Per slab the products are added in bsed_wgrad3's order, and at the plan's G a slab holds the tiles bsed_wgrad3's slab
 * holds; per d_in element in the order of the data-gradient kernel the two-kernel route runs (16 -> 32 channels:
 * bsed_igemm3s's 16 x 16 x 32 form; N = 64: bsed_igemm3n's 32 x 32 x 16 form): the routed layer keeps that route's bits.
 * bsed_conv_bwd_plan: every shape check, no HIP call; G = the recommended number of slabs, or 0 where the kernel takes
 * the shape but the two-kernel route measured faster (the caller then keeps it); max_G, label as for bsed_wgrad_plan. */
int bsed_conv_bwd_plan(const BsedWgradDesc* desc /*host*/, BsedContractPlan* out /*host*/);
int bsed_conv_bwd3(const BsedWgradDesc* desc /*host*/, void* stream);
/* The slab reducers (csrc/reduce.hip; one summation order and one split rule behind both entry points: an immediate and
 * a batched reduction give the same bits).  dst[tap*s_tap + k*s_k + n*s_n] (+)= sum_g part[g][tap][k][n]   (k < K, n < N) */
int bsed_reduce_partials(const float* part, int G, int ntaps, int KP, int NP, int K, int N, float* dst,
                         long s_tap, long s_k, long s_n, int accumulate, void* stream);
/* several bsed_reduce_partials in one launch (the host queues the reductions whose results only the optimizer needs
 * and flushes them together): same arithmetic contract per job, jobs of one call must write distinct destinations */
#define BSED_REDUCE_MAX_JOBS 40
typedef struct BsedReduceJob {
  const float* part; float* dst;
  int G, ntaps, KP, NP, K, N, accumulate;
  long s_tap, s_k, s_n;
} BsedReduceJob;
int bsed_reduce_partials_batch(const BsedReduceJob* jobs /*host*/, int njobs, void* stream);
/* the weight layout of bsed_igemm (csrc/igemm.hip): dst[tap][k][n] = src[tap*s_tap + k*s_k + n*s_n], zero for N <= n < NP */
int bsed_pack_weight(const float* src, float* dst, int ntaps, int K, int N, int NP, long s_tap, long s_k,
                     long s_n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming CNN pieces (csrc/cnn_ops.hip)
 * ---------------------------------------------------------------------------------------------- */
/* first conv, Cin = 1 (src/models/CNN.py:46-47 with i = 0): x (NB,H,W) -> y (NB,H,W,CO); w is the
 * PyTorch (CO,1,3,3) tensor; stats (bsed_conv0_num_tiles, 2, CO) per-tile (sum, sumsq) or NULL. */
int bsed_conv0_fwd(const float* x, const float* w, const float* bias, float* y, float* stats, int NB, int H,
                   int W, int CO, void* stream);
int bsed_conv0_num_tiles(int NB, int H, int W);
/* dW of the first conv: part (G, 9, CO) partial slabs for bsed_reduce_partials.  With y / coef / mean (together or
 * all NULL) dy is the gradient w.r.t. the BatchNorm OUTPUT and BatchNorm's backward (coef from bsed_bn_bwd in
 * coefficients-only mode) is applied on load: the first block's d_y never touches HBM. */
int bsed_conv0_wgrad(const float* x, const float* dy, const float* y, const float* coef, const float* mean,
                     float* part, int G, int NB, int H, int W, int CO, void* stream);
/* fp64 scratch needed by the statistics reductions below (not to be shared by calls running concurrently on two
 * streams) */
size_t bsed_stats_scratch_bytes(int C);
/* BatchNorm2d(eps, momentum) in train mode (src/models/CNN.py:49): per-tile partials -> batch mean /
 * invstd, scale = gamma*invstd, shift = beta - mean*scale; running stats (unbiased var) and
 * num_batches_tracked are updated in place when given. count = NB*H*W. */
int bsed_bn_finalize(const float* partial, long ntiles, int C, double count, float eps, float momentum,
                     const float* gamma, const float* beta, float* running_mean, float* running_var,
                     long long* num_batches_tracked, float* mean, float* invstd, float* scale, float* shift,
                     void* scratch, void* stream);
/* eval mode: scale/shift from the running statistics */
int bsed_bn_eval(int C, float eps, const float* gamma, const float* beta, const float* running_mean,
                 const float* running_var, float* scale, float* shift, void* stream);
/* the same for every BatchNorm layer of an eval-mode forward in one launch */
#define BSED_BN_EVAL_MAX_JOBS 16
typedef struct BsedBnEvalJob {
  const float *gamma, *beta, *running_mean, *running_var;
  float *scale, *shift;
  int C;
} BsedBnEvalJob;
int bsed_bn_eval_batch(const BsedBnEvalJob* jobs /*host*/, int njobs, float eps, void* stream);
/* BatchNorm backward: partial = per-tile (sum g, sum g*y); writes dgamma/dbeta and turns g (n_elems,
 * NHWC, in place) into d_y = A g + B (y - mean) + C;  coef (3,C) receives [A | B | C].  g_inout = y = NULL:
 * coefficients only (the consumer applies the map on load). */
int bsed_bn_bwd(const float* partial, long ntiles, int C, double count, const float* gamma, const float* mean,
                const float* invstd, float* dgamma, float* dbeta, int accumulate, float* g_inout, const float* y,
                long n_elems, float* coef, void* scratch, void* stream);
/* dst[c] (+)= sum_tiles partial[tile][which][c] */
int bsed_stats_to_grad(const float* partial, long ntiles, int C, int which, float* dst, int accumulate,
                       void* scratch, void* stream);
/* dst[c] (+)= sum_r in[r*pitch + c], r < M; part holds G*2*C floats */
int bsed_colsum(const float* in, long M, int C, int pitch, float* part, int G, float* dst, int accumulate,
                void* scratch, void* stream);
/* first stage of bsed_colsum alone: part (G, 2, C), G <= M, slot 0 = per-workgroup column sums (second stage: a
 * bsed_reduce_partials_batch job with KP = 2, K = 1) */
int bsed_colsum_part(const float* in, long M, int C, int pitch, float* part, int G, void* stream);
/* nn.Dropout(p) with a stateless Philox mask: out = in * keep/(1-p); the same call is its backward */
int bsed_dropout(const float* in, float* out, long n, float p, uint32_t rng_stream, uint64_t seed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GLU half of a CNN block (BatchNorm apply -> Linear -> sigmoid gate -> Dropout -> AvgPool2d, src/models/CNN.py:5-16,
 * 59-67, and its autograd) and the fused first block: eight entry points, one descriptor, one plan query.
 * A field an entry point does not read must be NULL / 0 for it (checked); all eight read NB, H, W, C, ph, pw (pooling
 * windows of 1 or 2), drop_p, rng_stream, seed and G.  The tiled kernels also read TH, TW (TH*TW == 128, TW a power of
 * two dividing W); the streaming kernels (glu16, block0) have no tile and want W % pw == 0 and H >= ph.
 *   entry point          tensors read                                        tensors written
 *   bsed_glu16_fwd       y scale shift w bias                                pooled
 *   bsed_glu16_bwd       y scale shift w bias dpool                          g part_dw part_db part_st
 *   bsed_block0_fwd      x cw cb scale shift w bias              [act_bf16]  pooled
 *   bsed_block0_bwd      x cw cb scale shift w bias dpool        [act_bf16]  part_dw part_db part_st part_gx
 *   bsed_glu_bwd_fused   y scale shift w wfwd bias dpool                     g part_dw part_db part_st
 *   bsed_glu_fwd3        y scale shift w bias                    [act_bf16]  pooled
 *   bsed_glu_bwd3        y scale shift w bias dpool              [act_bf16]  g part_dw part_db part_st
 *   bsed_glu_bwd3n       y scale shift w bias dpool              [act_bf16]  g dlin part_db part_st frag_table
 * ---------------------------------------------------------------------------------------------- */
typedef struct BsedGluDesc {
  const float* x;        /* block0: the input map (NB,H,W)                                             */
  const float* y;        /* pre-BatchNorm conv output (NB,H,W,C)                                       */
  const float *cw, *cb;  /* block0: the (16,1,3,3) conv weight and its bias                            */
  const float *scale, *shift;   /* (C) BatchNorm apply                                                 */
  const float* w;        /* the (C,C) Linear weight itself, [n][c]                                     */
  const float* wfwd;     /* bsed_glu_bwd_fused: bsed_pack_weight'ed W^T, [c][n]                        */
  const float* bias;     /* (C) Linear bias                                                            */
  const float* dpool;    /* gradient w.r.t. the pooled output (NB,H/ph,W/pw,C)                         */
  float* pooled;         /* forward output (NB,H/ph,W/pw,C)                                            */
  float* g;              /* dL/d(BatchNorm output) (NB,H,W,C)                                          */
  float* dlin;           /* bsed_glu_bwd3n: d_lin (NB,H,W,C) for the separate weight-gradient pass      */
  float* part_dw;        /* (BsedGluPlan.dw_rows, C, C) per-workgroup partial slabs of dW              */
  float *part_db, *part_st;     /* (G,2,C): slot 0 = sum d_lin; (sum g, sum g*y) for bsed_bn_bwd       */
  float* part_gx;        /* block0: (G,9,16) partial sums of g x_tap for bsed_block0_wgrad_finish      */
  void* frag_table;      /* bsed_glu_bwd3n: BsedGluPlan.table_bytes of device scratch, filled by the call */
  int NB, H, W, C;
  int TH, TW;            /* spatial tile of the tiled kernels; 0, 0 for the streaming ones             */
  int ph, pw;            /* pooling window                                                             */
  float drop_p;          /* dropout probability (0 = off)                                              */
  uint32_t rng_stream;   /* stream id of the mask (layer id)                                           */
  uint64_t seed;
  int act_bf16;          /* 1: y, dpool, g, dlin, pooled are bf16 tensors ("bf16" throughput mode); 0 = fp32 */
  int G;                 /* workgroups to launch: BsedGluPlan.G, or any value in 1..max_G              */
} BsedGluDesc;

enum {                   /* one value per entry point, for bsed_glu_plan                               */
  BSED_GLU_16_FWD = 0, BSED_GLU_16_BWD = 1, BSED_GLU_BLOCK0_FWD = 2, BSED_GLU_BLOCK0_BWD = 3,
  BSED_GLU_BWD_FUSED = 4, BSED_GLU_FWD3 = 5, BSED_GLU_BWD3 = 6, BSED_GLU_BWD3N = 7
};
typedef struct BsedGluPlan {
  int G;                 /* workgroups the library recommends (one resident round of a persistent kernel) */
  int max_G;             /* the largest G the entry point accepts (its work items)                      */
  int dw_rows;           /* rows of part_dw at that G: G * slabs per workgroup (0: no part_dw)          */
  int variant;           /* template arguments the library picks beyond C and act_bf16 (labels of profiles and bench
                          * lines): glu_fwd3 / glu_bwd3 the compile-time log2 tile width (4, or -1 = run time);
                          * glu_bwd_fused NW (waves per workgroup); block0 PH | SMALL << 4; 0 otherwise */
  size_t table_bytes;    /* size of frag_table (0: none)                                                */
} BsedGluPlan;
/* checks the shape fields of desc (pointers and G are ignored) and fills *out; makes no HIP call.  The entry points
 * run the same checks, then want every tensor of their row above and G in 1..max_G. */
int bsed_glu_plan(const BsedGluDesc* desc /*host*/, int kernel, BsedGluPlan* out);

/* GLU stage of a 16-channel block as HBM-bound streaming kernels (csrc/glu_small.hip): same math as
 * bsed_igemm(BSED_EPI_GLU_POOL) / the GLU backward chain, one pass over y. */
int bsed_glu16_fwd(const BsedGluDesc* desc /*host*/, void* stream);
int bsed_glu16_bwd(const BsedGluDesc* desc /*host*/, void* stream);

/* The whole first CNN block (conv3x3 1->16, BatchNorm, GLU, dropout, avg-pool: src/models/CNN.py:46-67, i = 0) WITHOUT
 * its conv output and gradient tensors in HBM (csrc/block0.hip): y0 is a 9-tap stencil of the input and is recomputed
 * where it is needed; BatchNorm's batch statistics come from x alone; conv0's weight gradient is assembled from
 * Gx = sum g x_tap (taken by the backward kernel) and the input's tap correlations R / Sx (taken with the statistics).
 *   stats : x (NB,H,W) -> stats (G,2,16) per-workgroup (sum y, sum y^2) for bsed_bn_finalize; xr_part (G,54) scratch;
 *           xr64 (54) fp64 totals [Sx (9) | R upper triangle (45)] for bsed_block0_wgrad_finish
 *   fwd   : x -> pooled (B,H/ph,W/pw,16), same values (bit for bit) as bsed_conv0_fwd + bsed_glu16_fwd
 *   bwd   : x, dpool -> per-workgroup partials part_dw (G,16,16), part_db (G,2,16) [slot 0], part_st (G,2,16) =
 *           (sum g, sum g*y) for bsed_bn_bwd (coefficients only), part_gx (G,9,16)
 *   wgrad_finish : dst (16,1,3,3) (+)= A Gx + B (Yx - mean Sx) + C Sx with coef = [A|B|C] of bsed_bn_bwd */
int bsed_block0_stats(const float* x, const float* cw_t /* the (16,1,3,3) weight transposed: [tap][channel] */,
                      const float* cb, float* stats, float* xr_part, double* xr64,
                      int G, int NB, int H, int W, int CO, void* stream);
int bsed_block0_fwd(const BsedGluDesc* desc /*host*/, void* stream);
int bsed_block0_bwd(const BsedGluDesc* desc /*host*/, void* stream);
int bsed_block0_wgrad_finish(const float* part_gx, int G, const double* xr64, const float* coef, const float* mean,
                             const float* cw, const float* cb, float* dst, int accumulate, int CO, void* stream);

/* Fused GLU backward for C in {32,64,128} (csrc/glu_bwd.hip): y, d_pooled -> g in one pass, with the three
 * contractions (lin recompute, g, dW) chained on chip on the fp32 matrix cores. */
int bsed_glu_bwd_fused(const BsedGluDesc* desc /*host*/, void* stream);
/* The same fused GLU backward in the split-fp32 ("bf16x3") contraction mode for C in {32,64} (csrc/glu3.hip): all
 * three contractions on the bf16 matrix cores, activations never staged through LDS. */
int bsed_glu_bwd3(const BsedGluDesc* desc /*host*/, void* stream);
/* C = 128 in the split-fp32 mode: g, db and BatchNorm partials as above, but d_lin is written out and the Linear
 * weight gradient is a separate 1-tap bsed_wgrad3(in = y with a_scale/a_shift, dy = d_lin). */
int bsed_glu_bwd3n(const BsedGluDesc* desc /*host*/, void* stream);
/* Forward of the same stage in the split-fp32 mode, C in {32,64,128}; replaces bsed_igemm(BSED_EPI_GLU_POOL).
 * Vertical pooling (ph = 2) is supported for tile widths TW in {2,8,16}. */
int bsed_glu_fwd3(const BsedGluDesc* desc /*host*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Clip-level domain discriminator glue (csrc/disc.hip); replaces Clip_Discriminator.forward
 * (src/models/CRNN_GRL.py:16-53), GradientReverseFunction (src/DA/grl.py:12-22) and the BCE of
 * ConditionalDomainAdversarialLoss.forward (src/DA/cdan_frame.py:89-119).  The 3x3 / stride-2 / pad-0
 * convolutions run as im2col + bsed_igemm / bsed_wgrad; images are (N, H = time, W = feature, C).
 * ---------------------------------------------------------------------------------------------- */
/* Frame-level discriminator glue (csrc/disc.hip; reference Frame_Discriminator, src/models/CRNN_GRL.py:116-140).
 *   bsed_leaky_dropout_fwd/bwd: out = LeakyReLU_slope(a) * dropout mask; d_a = d_out * mask * LeakyReLU'(a) (n % 4 == 0;
 *     the mask is a counter hash of (seed, rng_stream, element index), regenerated in backward);
 *   bsed_frame_head_fwd: d (M) = sigmoid(x (M,32) . w (32) + b);
 *   bsed_frame_head_bwd: dx (M,32) and part (G,2,32): row 0 = partial dw, row 1 column 0 = partial db (sum over G). */
int bsed_leaky_dropout_fwd(const float* a, float* out, long n, float slope, float drop_p, uint32_t rng_stream,
                           uint64_t seed, void* stream);
int bsed_leaky_dropout_bwd(const float* d_out, const float* a, float* d_a, long n, float slope, float drop_p,
                           uint32_t rng_stream, uint64_t seed, void* stream);
int bsed_frame_head_fwd(const float* x, const float* w, const float* b, float* d, long M, int K, void* stream);
int bsed_frame_head_bwd(const float* x, const float* w, const float* d, const float* d_out, float* dx, float* part, int G,
                        long M, int K, void* stream);

/* Space-to-depth glue of the direct stride-2 convolutions (csrc/disc.hip): a 3x3 / stride-2 / pad-0 convolution over
 * A (Hi,Wi,C) equals a 2x2 / stride-1 convolution over X'[p][q][(a*2+b)*C + c] = A[2p+a][2q+b][c] (4C channels, taps
 * (dp,dq) in {0,1}^2, weight slot (dp,dq,a,b) = W[2dp+a][2dq+b] or zero), which the implicit-GEMM kernels run without
 * an im2col matrix.
 *   bsed_s2d_fwd: X' (N,Hp,Wp,4C), Hp = ceil(Hi/2), Wp = ceil(Wi/2), from y (N,Ha,Wa,C) (allocated extent >= valid
 *                 extent Hi x Wi) with BatchNorm apply + LeakyReLU(0.2) fused (scale/shift NULL: identity); pixels
 *                 beyond Hi x Wi are zero.
 *   bsed_s2d_bwd: g (N,Ha,Wa,C) = dX' gathered back * LeakyReLU'(y*scale+shift) on the valid extent, zero elsewhere, and
 *                 per-block partial sums (sum g, sum g*y) for the BatchNorm backward: stats (bsed_s2d_num_blocks, 2, C). */
int bsed_s2d_fwd(const float* y, const float* scale, const float* shift, float* xp, int N, int Ha, int Wa, int Hi, int Wi,
                 int C, void* stream);
int bsed_s2d_num_blocks(int N, int Ha, int Wa, int C);
int bsed_s2d_bwd(const float* dxp, const float* y, const float* scale, const float* shift, float* g, float* stats, int N,
                 int Ha, int Wa, int Hi, int Wi, int C, void* stream);

/* col[(n,ho,wo)][(dw*3+dh)*CP + c] = leaky_relu_0.2(act*scale+shift) (identity when scale == NULL);
 * C == 1 writes 16 columns (9 taps + zeros).  Ho = (Hi-3)/2+1, Wo = (Wi-3)/2+1. */
int bsed_im2col_s2(const float* act, const float* scale, const float* shift, float* col, int N, int Hi, int Wi,
                   int C, int CP, void* stream);
/* adjoint gather.  C > 1: out = d_act * leaky'(y*scale+shift), stats (bsed_col2im_s2_num_blocks, 2, C) =
 * per-block (sum g, sum g*y) for bsed_bn_bwd.  C == 1: out = d_act * out_scale (GRL: out_scale = -lambda). */
int bsed_col2im_s2(const float* dcol, const float* y, const float* scale, const float* shift, float* out,
                   float* stats, int N, int Hi, int Wi, int C, int CP, float out_scale, void* stream);
int bsed_col2im_s2_num_blocks(int N, int Hi, int Wi, int C);
/* BN5 + LeakyReLU + AdaptiveAvgPool2d((2,1)) + Linear(16,1) + sigmoid (+ BCE vs label 1 for n < Ns else 0,
 * mean over N, and the backward to g5 = dL/d(BN5 output) with per-sample partials) */
int bsed_disc_head(const float* y5, const float* scale, const float* shift, const float* wl, const float* bl, int N,
                   int Ns, int H5, int W5, int C5, int train, float* d_out, float* g5, float* stats, float* dwl_part,
                   float* dbl_part, float* loss_part, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Feature-pyramid glue of CRNN_fpn (csrc/fpn.hip); replaces nn.Upsample((T_out,1), mode='bilinear',
 * align_corners=True) on width-1 maps (src/models/CRNN_GRL.py:333-336,378-384) and its backward.
 * Tensors are (B, T, C) with a row pitch, so the output can be the right half of a concatenation buffer.
 * ---------------------------------------------------------------------------------------------- */
int bsed_upsample_time_fwd(const float* in, float* out, int B, int T_in, int T_out, int C, int in_pitch, int out_pitch,
                           void* stream);
int bsed_upsample_time_bwd(const float* dout, float* din, int B, int T_in, int T_out, int C, int dout_pitch,
                           int din_pitch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bidirectional GRU recurrence (csrc/gru.hip); replaces nn.GRU of src/models/RNN.py:7-16.
 *   xp    (B,T,768)  x @ [W_ih; W_ih_reverse]^T + b_ih   (from bsed_igemm), [dir*384 + gate*128 + k]
 *   w_hh  (2,384,128), b_hh (2,384)                       gate order r,z,n
 *   out   (B,T,256)  [dir*128 + k];  gates (B,T,2,4,128) r,z,n,(W_hn h + b_hn) saved for backward
 *   rows_per_wg  batch rows per workgroup of the fp32 register kernels: 1 or 2, at both entries; any other value
 *                returns BSED_ERR_ARG before anything is launched.  gates may be NULL in the forward entries (inference).
 * ---------------------------------------------------------------------------------------------- */
int bsed_gru_fwd(const float* xp, const float* w_hh, const float* b_hh, float* out, float* gates, int B, int T,
                 int rows_per_wg, void* stream);
/* BPTT: dxp = d(x-side pre-activations) (B,T,768), dgh = d(h-side pre-activations) (B,T,768) */
int bsed_gru_bwd(const float* dout, const float* out, const float* gates, const float* w_hh, float* dxp,
                 float* dgh, int B, int T, int rows_per_wg, void* stream);
/* The same recurrence with h @ W_hh^T of every step on the bf16 matrix cores with split-fp32 operands (4 batch rows
 * per workgroup; the default in the bf16x3 contraction mode).  Same tensors, same layouts, same reference lines. */
int bsed_gru_fwd3(const float* xp, const float* w_hh, const float* b_hh, float* out, float* gates, int B, int T,
                  void* stream);
/* part_bih / part_bhh (nullable, together): (bsed_gru_bwd3_rows(B), 768) per-batch-row partial sums over time of
 * dxp / dgh, i.e. the bias gradients before the final column sum (bsed_colsum over those few rows). */
int bsed_gru_bwd3(const float* dout, const float* out, const float* gates, const float* w_hh, float* dxp,
                  float* dgh, float* part_bih, float* part_bhh, int B, int T, void* stream);
int bsed_gru_bwd3_rows(int B);

/* ------------------------------------------------------------------------------------------------
 * Predictor head + losses (csrc/head.hip); replaces Predictor.forward (src/models/CRNN_GRL.py:441-460)
 * and the BCE / MSE loss assembly of train_mt (src/main_baseline.py:431-498).
 *   w (2C,K): rows 0..C-1 = dense.weight, rows C..2C-1 = dense_softmax.weight; b (2C) likewise.
 * ---------------------------------------------------------------------------------------------- */
/* out (B,C) = max over time of y (B,T,C): the clip-level targets the train loop derives from the strong ones
 * (src/main_baseline.py train_mt: target_weak = target.max(-2)[0]) */
int bsed_max_over_time(const float* y, float* out, int B, int T, int C, void* stream);
/* The head kernels split each clip's frames over S = bsed_head_splits(B, T) workgroups.  bsed_head_fwd needs a
 * (B,S,2,C) scratch buffer `part` when S > 1; bsed_head_bwd writes S rows per clip into its partial outputs
 * (dw_part (B*S,2C,K), db_part (B*S,2C), loss_part (B*S,6)): sum over the leading dimension as before. */
int bsed_head_splits(int B, int T);
/* K = 256 and 1 <= C <= BSED_HEAD_MAX_CLASSES (ABI 8; the width of the label set that bsed_tag_masks fixes): anything
 * else is BSED_ERR_ARG before any HIP call, here and in bsed_head_bwd.  bsed_head_lds_bytes: the dynamic LDS in bytes
 * that the forward (backward = 0) or backward launch for C classes requests, negative for an unsupported C; host only. */
#define BSED_HEAD_MAX_CLASSES 64
int bsed_head_lds_bytes(int C, int backward);
int bsed_head_fwd(const float* x, const float* w, const float* b, float* strong, float* sof_raw, float* weak,
                  float* den, float* part, int B, int T, int K, int C, int attention, void* stream);

/* CNN-only tagging head (csrc/tag.hip); replaces the tail of CRNN_pred.forward (src/models/CRNN_GRL.py:252-290):
 * strong = sigmoid(x), sof = clamp(softmax_class(logits), 1e-7, 1), weak = sum_t strong*sof / sum_t sof.
 *   x, logits, strong (B,T,C); weak (B,C); part: (B, bsed_tag_splits(B,T), 2, C) scratch.  C = 128. */
int bsed_tag_splits(int B, int T);
int bsed_tag_head_fwd(const float* x, const float* logits, float* strong, float* weak, float* part, int B, int T, int C,
                      void* stream);

/* get_predictions post-processing (src/evaluation_measures.py:188-205): out = median_filter(strong > threshold,
 * size=(win,1)) with scipy.ndimage's window origin and 'reflect' boundary; (B,T,C) float 0/1 mask */
int bsed_binarize_median(const float* strong, float* out, int B, int T, int C, float threshold, int win,
                         void* stream);

/* Contiguous-region decode + frames -> seconds on the GPU (ManyHotEncoder.decode_strong, src/utilities/ManyHotEncoder.py:
 * 148-164, and src/evaluation_measures.py:205-209).  mask (B,T,C) 0/1 from bsed_binarize_median.
 *   bsed_decode_count: counts (B*C) = number of on-runs per (clip, class) column;
 *   bsed_decode_write: offsets (B*C) = exclusive prefix sum of counts (caller's), E = total; writes ev_clip (E),
 *     ev_class (E), ev_frames (E,2) [onset, offset) and ev_seconds (E,2) = clip(frame * scale, 0, max_len) in float64,
 *     ordered by clip, class, time -- the reference's row order. */
int bsed_decode_count(const float* mask, int B, int T, int C, int* counts, void* stream);
int bsed_decode_write(const float* mask, const int* offsets, int B, int T, int C, double scale, double max_len,
                      int* ev_clip, int* ev_class, int* ev_frames, double* ev_seconds, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Recording-level detection (csrc/detect.hip): one long waveform -> overlapping clip-sized windows -> the clip path ->
 * window probabilities stitched onto the recording's frame grid -> events.  One output frame is frame_samples =
 * hop * pooling_time_ratio samples (1020); window starts are given in OUTPUT FRAMES so that local frame j of a window
 * that starts at frame s is frame s + j of the recording.
 * ---------------------------------------------------------------------------------------------- */
/* wave (n) + starts (W, int32 output frames) -> out (W, win): out[w] = wave[starts[w] * frame_samples : ... + win], bit
 * for bit, in one launch.  win and frame_samples must be multiples of 4 and wave / out 16-byte aligned (rows move as
 * 16-byte pieces; any other geometry is refused).  A window that does not lie inside the recording is zero-filled. */
int bsed_gather_windows(const float* wave, long n, const int* starts, int W, int win, int frame_samples, float* out,
                        void* stream);

#define BSED_STITCH_UNIFORM 0
#define BSED_STITCH_TRIANGULAR 1
/* p (W, Tp, C) window probabilities + starts (W, int32 output frames) -> out (T_total, C): the weighted mean over the
 * windows that cover a frame, summed in ascending window order (no atomics: bitwise repeatable); a frame covered by
 * one window is copied.  weighting: BSED_STITCH_UNIFORM, or BSED_STITCH_TRIANGULAR wgt(j) = min(j + 1, Tp - j).
 * Contract: starts[w] = w * hop_frames for w < W - 1, 1 <= hop_frames <= Tp; the last window may instead be aligned to
 * the end of the recording, (W - 2) * hop_frames < starts[W - 1] <= (W - 1) * hop_frames; T_total = starts[W - 1] + Tp. */
int bsed_stitch_windows(const float* p, const int* starts, int W, int Tp, int C, int hop_frames, int T_total,
                        int weighting, float* out, void* stream);

/* Contiguous-region decode of ONE (T, C) 0/1 mask with a long time axis, parallel over time: chunks of
 * BSED_DECODE_LONG_FRAMES frames, nchunks = ceil(T / BSED_DECODE_LONG_FRAMES).
 *   bsed_decode_long_count: counts (C * nchunks), counts[c * nchunks + k] = regions of class c that start in chunk k;
 *   bsed_decode_long_write: offsets (C * nchunks) = exclusive prefix sum of counts (caller's), E = total; writes
 *     ev_class (E), ev_frames (E,2) [onset, offset) and ev_seconds (E,2) = clip(frame * scale, 0, max_len) in float64,
 *     ordered by class, then time -- what bsed_decode_write gives for one clip.  C <= 512. */
#define BSED_DECODE_LONG_FRAMES 64
int bsed_decode_long_count(const float* mask, int T, int C, int* counts, void* stream);
int bsed_decode_long_write(const float* mask, const int* offsets, int T, int C, double scale, double max_len,
                           int* ev_class, int* ev_frames, double* ev_seconds, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Validation (csrc/metrics.hip, ABI 6): the event lists of S thresholds from one launch, and the collar-based event
 * counts behind the reference's model-selection F1 (compute_metrics -> sed_eval EventBasedMetrics, t_collar 0.2 s,
 * percentage_of_length 0.2; src/main_baseline.py:1010-1032).
 * ---------------------------------------------------------------------------------------------- */
/* Threshold sweep.  strong (B,T,C); thresholds (S) float32 on the DEVICE; windows (C) int32 on the device, the median
 * window of each class, 0 (or less) = the class yields no events (learned_post's classes beyond its list).
 *   bsed_sweep_count: counts (S,B,C) = number of events per (threshold, clip, class);
 *   bsed_sweep_write: offsets (S*B*C, or S*B*C + 1 with the total last: only the first S*B*C are read) = exclusive prefix
 *     sum of counts (caller's), E = total; writes ev_frames (E,2) int32 [onset, offset) and ev_seconds (E,2) float64 =
 *     clip(frame * scale, 0, max_len), ordered by threshold, clip, class, time.
 * The events of threshold s are bit for bit those of bsed_binarize_median(thresholds[s], windows[c]) ->
 * bsed_decode_count / bsed_decode_write, for every T and every window (win > T and win > 2T included).  Each clip's
 * tile is read from HBM once per launch and staged in LDS; a tile above 160 KB (T * C > 40960) is walked in global
 * memory instead, with the same results.  Refused before any launch: null pointers, a non-positive size, and geometry
 * whose worst-case event total S * B * C * ceil(T / 2) exceeds 2^31 - 1. */
int bsed_sweep_count(const float* strong, const float* thresholds, const int* windows, int S, int B, int T, int C,
                     int* counts, void* stream);
int bsed_sweep_write(const float* strong, const float* thresholds, const int* windows, const int* offsets, int S, int B,
                     int T, int C, double scale, double max_len, int* ev_frames, double* ev_seconds, void* stream);

/* Event matching.  est_offsets (S*B*C + 1) int32: exclusive prefix of the estimated lists, grouped by (threshold, clip,
 * class), the total last; est_seconds (E,2) float64 [onset, offset].  ref_offsets (B*C + 1) and ref_seconds (R,2): the
 * reference events grouped by (clip, class).  The lists need not come from bsed_sweep_write and may overlap.  Hit rule, in
 * float64:  fabs(ref_on - est_on) <= t_collar  and
 *           fabs(ref_off - est_off) <= fmax(t_collar, percentage_of_length * (ref_off - ref_on)).
 * acc (S,C,3) int64 += (Ntp, Nsys, Nref) summed over the clips: Ntp the size of a MAXIMUM bipartite matching of the hit
 * graph of each (threshold, clip, class), Nsys / Nref the list lengths.  Integer atomics: the accumulator persists
 * across calls (zero it first) and repeated runs give the same bits.
 * Contract (the CALLER's check, the offsets live on the device): at most BSED_MATCH_MAX_REF reference events per
 * (clip, class); events beyond that are counted in Nref but never matched.  B <= 524280 per call. */
#define BSED_MATCH_MAX_REF 64
int bsed_event_match(const int* est_offsets, const double* est_seconds, const int* ref_offsets, const double* ref_seconds,
                     int S, int B, int C, double t_collar, double percentage_of_length, long long* acc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Intersection-based counts (csrc/intersect.hip, ABI 13): what psds_eval's macro F1 with a cross-trigger matrix
 * (PSDSEval(0.5, 0.5, 0.3).compute_macro_f_score, reference src/evaluation_measures.py:518-526) and its PSDS
 * (:287-316, :505-510) are computed from.  psds_eval is not installed where this project is developed: the rules below
 * are psds_eval's AS THIS PROJECT STATES THEM, parity with psds_eval not pinned; the integer counts are the primary
 * result, the F1 / rates / PSDS arithmetic on them is float64 numpy on the host (evaluation/intersection.py).
 *
 * Everything is per (threshold s, clip b) over C classes; est[s][b][j] and ref[b][k] are the lists of the layout of
 * bsed_event_match (est_offsets (S*B*C + 1), est_seconds (E,2), ref_offsets (B*C + 1), ref_seconds (R,2), float64
 * [onset, offset], list order).  The totals E and R are read from the offsets on the device.
 *   pair intersection   it = fmin(off_e, off_r) - fmax(on_e, on_r); a pair counts only when it > 0, so touching or
 *                       zero-length events contribute nothing and nothing divides by zero
 *   pair ratios         det_precision = it / (off_e - on_e),   gt_coverage = it / (off_r - on_r)
 * All sums are float64, sequential, left to right in the list order of the OTHER side, one division per pair; a host that
 * loops the same way gets the same bits, so the counts are compared with ==, no tolerance.
 *   DTC   an estimated event of class j passes when the sum of det_precision over ref[b][j] is >= dtc
 *   GTC   a reference event of class k is a true positive when the sum of gt_coverage over the DTC-PASSING events of
 *         est[s][b][k] is >= gtc (a failing detection adds no coverage)
 *   FP    an estimated event that fails DTC is a false positive of its class (a passing one is neither TP nor FP)
 *   CTTC  a DTC-FAILING estimated event of class j and every class k != j: when the sum of its det_precision over
 *         ref[b][k] is >= cttc, ct[k][j] += 1 -- once per (event, k), however many reference events contributed; a
 *         DTC-passing event never cross-triggers
 * evaluated: (B) uint8 on the device, or NULL = every clip; a clip with evaluated[b] == 0 is skipped whole, both sides.
 * Outputs, integer atomics, persistent across calls (zero them first), two runs give the same bits:
 *   acc (S,C,4) int64 += (Ntp, Nfp, Nsys, Nref);   ct (S,C,C) int64, [reference class k][estimated class j], zero diagonal.
 * dtc_flags: caller-owned scratch of max(E, 1) bytes (1 = the event passed DTC), written by the first launch and read by
 * the second.  No cap on the length of a list on either side (no matching is involved); lists may overlap and need not
 * come from bsed_sweep_write.  Two launches, no host sync.  Refused before any launch: null pointers (evaluated may be
 * NULL), non-positive S, B or C, dtc / gtc / cttc outside (0, 1], S*C*C or S*B*C beyond int32.
 * ---------------------------------------------------------------------------------------------- */
int bsed_intersection_counts(const int* est_offsets, const double* est_seconds, const int* ref_offsets,
                             const double* ref_seconds, const uint8_t* evaluated, int S, int B, int C, double dtc,
                             double gtc, double cttc, uint8_t* dtc_flags, long long* acc, long long* ct, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Segment-based counts (csrc/segment_metrics.hip, ABI 16): what sed_eval's SegmentBasedMetrics -- the second metric of
 * the reference's compute_sed_eval_metrics (src/evaluation_measures.py:87-120, :318-325; time_resolution 1.0, no
 * evaluated length) -- computes its F1 and error rate from.  sed_eval is not installed where this project is developed:
 * the rules below are sed_eval's SegmentBasedMetrics AS THIS PROJECT STATES THEM, parity with sed_eval not pinned; the
 * integer counts are the primary result, the arithmetic on them is float64 numpy on the host (segment_metrics.py).
 *
 * The lists are those of bsed_event_match and bsed_intersection_counts: est_offsets (S*B*C + 1), est_seconds (E,2),
 * ref_offsets (B*C + 1), ref_seconds (R,2), float64 [onset, offset] (finite); they may overlap and need not be sorted.
 *   segments an event covers   [max(0, floor(onset / resolution)), ceil(offset / resolution)), each quotient ONE float64
 *                       division; when the upper end is not above the lower end the event is active nowhere: a
 *                       zero-length event exactly on a boundary covers nothing, [1.0, 2.0] at resolution 1 covers
 *                       segment 1 only, a negative onset starts in segment 0
 *   segments of (s, b)  length_seconds > 0: ceil(length_seconds / resolution) for every clip, activity beyond it is cut
 *                       off;  length_seconds == 0: the largest ceil(offset / resolution) over ALL events of both sides of
 *                       that (threshold, clip), all classes, 0 when both sides are empty (how the reference calls
 *                       sed_eval: no evaluated length)
 * With A[t] / E[t] the sets of classes active in segment t in the reference / in the estimate, over the segments of the
 * evaluated clips:
 *   class_acc (S,C,4) int64 += (Ntp, Nfp, Nfn, Ntn): c in both / in E[t] only / in A[t] only / in neither -- the order of
 *                       bsed_tag_counts
 *   overall (S,4) int64 += (sum Sub, sum Del, sum Ins, number of segments), per segment with Nref = |A[t]|, Nsys = |E[t]|,
 *                       Ntp = |A[t] & E[t]|:  Sub = min(Nref, Nsys) - Ntp,  Del = max(0, Nref - Nsys),
 *                       Ins = max(0, Nsys - Nref)
 * evaluated: (B) uint8 on the device, or NULL = every clip; a clip with evaluated[b] == 0 is skipped whole, both sides.
 * Integer atomics, at most one 64-bit add per workgroup per (s, c, kind): the accumulators persist across calls (zero
 * them first), two runs give the same bits.  expected_seconds is a host-side HINT (the list lengths are device data): it
 * only sizes the grid's dimension over tiles of segments, which the workgroups walk with a grid stride, so every value
 * gives the same counts; pass the length of a typical clip.  No cap on the length of a list or of a clip.  One launch, no
 * host sync, no workspace.  Refused before any launch: null pointers (evaluated may be NULL), non-positive S, B or C,
 * C > BSED_SEGMENT_MAX_CLASSES, a resolution or expected_seconds that is not a positive finite number, a negative or
 * non-finite length_seconds, S*B*C beyond int32, ceil(length_seconds / resolution) beyond int32.
 * ---------------------------------------------------------------------------------------------- */
#define BSED_SEGMENT_MAX_CLASSES 64
int bsed_segment_counts(const int* est_offsets, const double* est_seconds, const int* ref_offsets,
                        const double* ref_seconds, const uint8_t* evaluated, int S, int B, int C, double resolution,
                        double length_seconds, double expected_seconds, long long* class_acc, long long* overall,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * All-pairs statistics of an embedding (csrc/pair_stats.hip, ABI 17): what the domain gap between two sets of
 * recordings is computed from -- the silhouette of the synth / real labelling (the number src/visualize.py prints, there
 * on a t-SNE projection), the leave-one-out nearest-neighbour domain accuracy and the multi-kernel MMD^2
 * (domain_gap.py does that arithmetic in float64 numpy).  The definitions are this project's own; parity with sklearn is
 * shown only through the float64 restatement of tests/domain_gap_reference.py.
 *
 * x (N,D) float32, rows x_pitch >= D elements apart, base on any 4-byte boundary;  group (N) int32: a label in [0, G)
 * or anything else = MASKED: such a point is summed into nothing and is nobody's neighbour, its own row is still
 * produced (no label is used as an index before it is range-checked);  scale (S) float32.
 *   d2(i,j)           = sum_k (x_ik - x_jk)^2: each difference rounded once to float32, accumulated in float32 in any
 *                       order, FMA allowed.  The direct-difference form, NOT |x|^2 + |y|^2 - 2 x.y: embeddings of one
 *                       model lie close together, and the cancellation of the Gram form has no bound in terms of d2
 *   d(i,j)            = the correctly rounded float32 square root of d2(i,j)
 *   dist_sum (N,G) float64      [i][g]    = sum over j != i with group[j] == g of (double)d(i,j)
 *   kern_sum (N,G,S) float64    [i][g][s] = the same sum of (double)expf(-(d2(i,j) * scale[s])); not touched when S == 0
 *   nn_d2 (N) float32, nn_index (N) int32 = the smallest d2(i,j) over the unmasked j != i and its j, the smallest j on an
 *                       exact tie; +infinity and -1 when there is no candidate
 * All sums over j are float64, in an order fixed by (N, D, G, S, splits): two launches with the same arguments give the
 * same bits; no floating-point atomics.  The grid is (tiles of 64 rows) x splits: a workgroup walks its own contiguous
 * range of the tiles of 64 columns and writes its partial sums to the workspace, a second launch adds them in split
 * order.  splits == 0: the library's choice, bsed_pair_stats_splits(N, D) (>= 1); another value gives the same results
 * to float64 round-off.  workspace: caller-owned device memory of at least bsed_pair_stats_workspace(N, G, S, splits)
 * bytes (0 for arguments bsed_pair_stats would refuse; splits == 0 sizes it for the automatic choice), 8-byte aligned,
 * contents irrelevant before and after.  Two launches, no host synchronisation.
 * Refused before any HIP call, with a message that starts "bsed_pair_stats:": null pointers (scale and kern_sum may be
 * NULL only when S == 0); N < 1 or above 2^30; D < 1; G outside 1..BSED_PAIR_MAX_GROUPS; S outside
 * 0..BSED_PAIR_MAX_SCALES; x_pitch < D; splits < 0 or above 65535; a workspace smaller than the query says or not
 * 8-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
#define BSED_PAIR_MAX_GROUPS 8
#define BSED_PAIR_MAX_SCALES 8
int bsed_pair_stats_splits(int N, int D);
size_t bsed_pair_stats_workspace(int N, int G, int S, int splits);
int bsed_pair_stats(const float* x, long long x_pitch, int N, int D, const int* group, int G, const float* scale,
                    int S, int splits, double* dist_sum, double* kern_sum, float* nn_d2, int* nn_index,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exact t-SNE of an embedding at two components (csrc/tsne.hip, ABI 19): the map src/visualize.py draws of the synth and
 * the real embeddings, by the rules of sklearn 1.7's TSNE(method="exact") -- the algorithm its default Barnes-Hut method
 * approximates; the tree is not rebuilt.  tsne.py drives the three entry points; tests/tsne_reference.py restates them in
 * float64 and is pinned to sklearn's own functions.  No atomics; every sum has an order fixed by the arguments, so the
 * same arguments give the same bits.  Every entry point refuses bad arguments before any HIP call with a message that
 * starts with its own name, and makes no host synchronisation.
 *
 * bsed_tsne_affinities: x (N,D) float32, rows x_pitch >= D elements apart, base on any 4-byte boundary -> P (N,N)
 * float32 dense, beta (N) float32, sum_p one float64.  Four launches.
 *   d2(i,j)   exactly as bsed_pair_stats defines it (direct differences in float32, the same chain over k: the same
 *             bits); symmetric bit for bit, 0 on the diagonal.  It is written to P first.
 *   search    per row i over the N - 1 other points, sklearn's _binary_search_perplexity in float64 (d2 converted):
 *             beta starts at 1 with no lower and no upper bound; at most 100 steps; a step evaluates
 *             sum = SUM_j exp(-d2 beta) (a sum of exactly 0 is read as 1e-8, rounded to float32 as sklearn's constant is)
 *             and H = log(sum) + beta SUM_j d2 exp(-d2 beta) / sum; it stops when |H - log(perplexity)| <= 1e-5 (the
 *             float32 value of 1e-5, likewise); otherwise, H too large: beta becomes the lower bound and is doubled
 *             while the upper bound is infinite, else replaced by its mean with the upper bound; H too small: beta becomes
 *             the upper bound and is halved while the lower bound is infinite, else replaced by its mean with the lower
 *             bound.  p(j|i) = exp(-d2 beta_i) / sum at the last beta that was EVALUATED (after 100 steps that is not
 *             the beta of the 101st), rounded to float32; beta[i] is that beta_i rounded to float32.
 *   P_ij      = p(j|i) + p(i|j) in float32 (commutative: symmetric bit for bit), 0 on the diagonal, in place.  It is NOT
 *             divided by its sum: sum_p = SUM_ij P_ij in float64 in a fixed order, and the gradient takes 1 / sum_p.
 *             sklearn also clamps P_ij / sum_p from below at 2.2e-16; that is left out.
 * The sums over a row are float64 in a fixed order (256 strided partials, a fixed tree); the row of d2 stays in LDS up to
 * N = 32768 and is re-read from P beyond.  workspace: bsed_tsne_affinities_workspace(N) bytes (0 for an N that is
 * refused), 8-byte aligned, caller-owned, contents irrelevant before and after.
 * Refused: null pointers; N < 2 or N > BSED_TSNE_MAX_POINTS; D < 1; x_pitch < D; a perplexity outside (0, N); x, P or
 * beta off a 4-byte boundary, sum_p or the workspace off an 8-byte one; a workspace smaller than the query says.
 *
 * bsed_tsne_gradient: sklearn's _kl_divergence at one degree of freedom.  y (N,2) float32, P as above ->
 * grad (N,2) float32, stats three float64.  Three launches, five with want_error.
 *   w_ij   = 1 / (1 + |y_i - y_j|^2) (float32 per pair),  Z = SUM_{i != j} w_ij,
 *   grad_i = 4 SUM_j (exaggeration inv_sum_p P_ij - w_ij / Z) w_ij (y_i - y_j), formed as
 *            4 (exaggeration inv_sum_p SUM_j P_ij w_ij (y_i - y_j) - (1 / Z) SUM_j w_ij^2 (y_i - y_j)): the products per
 *            pair in float32, the four columns a thread owns added in float32, everything above that in float64;
 *   stats[0] = Z;  stats[1] = |grad|^2, the float64 sum of the squares of the float32 values returned;
 *   stats[2] = with want_error = 1: KL = SUM_{i != j} p log(max(p, 2.2e-16) / max(q, 2.2e-16)), q = w_ij / Z,
 *            p = exaggeration inv_sum_p P_ij (the exaggerated P while exaggeration is not 1, as sklearn reports it), in
 *            float64 throughout, by a second pass over P once Z is known; the logarithm is evaluated on such a launch
 *            only.  With want_error = 0: NaN (what sklearn returns).
 *   sklearn clamps q from below at 2.2e-16 inside the gradient too; that is left out: a gradient element differs by at
 *   most 4 * 2.2e-16 * SUM_j w_ij |y_i - y_j| from the clamped one.
 * The grid is (tiles of 64 rows) x splits; a workgroup streams its contiguous range of the tiles of 64 columns of P once
 * and writes per-row partials (attraction, repulsion, sum of w) to the workspace; a second launch adds them in split
 * order, a third forms Z in row order, the gradient and the stats.  splits == 0: the library's choice,
 * bsed_tsne_gradient_splits(N); any other value gives the same results to float64 round-off.  workspace:
 * bsed_tsne_gradient_workspace(N, splits) bytes (0 for arguments that are refused), 8-byte aligned.
 * Refused: null pointers; N < 2 or N > BSED_TSNE_MAX_POINTS; inv_sum_p or exaggeration not positive and finite;
 * want_error outside {0, 1}; splits < 0 or above 65535; misaligned pointers; a workspace too small or off an 8-byte
 * boundary.
 *
 * bsed_tsne_update: sklearn's _gradient_descent step on n = 2 N elements, every operation rounded to float32 on its own
 * (no fused multiply-add), bit for bit what numpy computes:
 *   inc = update * grad < 0;  gains = inc ? gains + 0.2f : gains * 0.8f;  gains = gains < min_gain ? min_gain : gains;
 *   update = momentum * update - learning_rate * (grad * gains);  y = y + update.        grad is left as it is.
 * Refused: null pointers; n < 1 or n > 2 * BSED_TSNE_MAX_POINTS; a pointer off a 4-byte boundary.
 * ---------------------------------------------------------------------------------------------- */
#define BSED_TSNE_MAX_POINTS 65536
size_t bsed_tsne_affinities_workspace(int N);
int bsed_tsne_affinities(const float* x, long long x_pitch, int N, int D, float perplexity, float* P, float* beta,
                         double* sum_p, void* workspace, size_t workspace_bytes, void* stream);
int bsed_tsne_gradient_splits(int N);
size_t bsed_tsne_gradient_workspace(int N, int splits);
int bsed_tsne_gradient(const float* y, const float* P, int N, double inv_sum_p, double exaggeration, int want_error,
                       int splits, float* grad, double* stats, void* workspace, size_t workspace_bytes, void* stream);
int bsed_tsne_update(float* y, const float* grad, float* update, float* gains, long n, float momentum,
                     float learning_rate, float min_gain, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Domain classifier (csrc/svc.hip, ABI 20): the cross-validated RBF support vector classifier of src/visualize.py
 * (svm_classfication: cross_val_score(SVC(), features, target, cv=5)) by the rules of libsvm's C-SVC Solver as sklearn
 * 1.7 runs it, restated below; shrinking is left out (it changes the path, not the optimum).  svc.py drives the three
 * entry points; tests/svc_reference.py restates them in float64 and is pinned to sklearn.  No floating-point atomics;
 * every sum and every choice has an order fixed by the arguments, so the same arguments give the same bits.  Every entry
 * point refuses bad arguments before any HIP call with a message that starts with its own name, and makes no host
 * synchronisation.  All pointers are device pointers except gamma, which is read on the HOST (that is where it is
 * checked) and handed to the kernels by value.
 *
 * bsed_svc_d2: x (N,D) float32, rows x_pitch >= D elements apart, base on any 4-byte boundary -> d2 (N,N) float32
 * dense: exactly the d2(i,j) bsed_pair_stats defines (direct differences, each rounded once to float32, one float32
 * chain over k; not the Gram form) -- the device code bsed_tsne_affinities starts with (csrc/d2_tile.h): symmetric bit
 * for bit, 0 on the diagonal.  One launch.
 * Refused: null pointers; N < 1 or N > BSED_SVC_MAX_POINTS (1 GiB of d2); D < 1; x_pitch < D; x or d2 off a 4-byte
 * boundary.
 *
 * bsed_svc_solve: P independent C-SVC duals  min 1/2 a^T Q a - SUM a,  0 <= a_t <= C,  SUM y_t a_t = 0,
 * Q_ts = y_t y_s K(t,s), in ONE launch, one workgroup of 256 threads per problem.  Problem p trains on the points
 * train_index[train_offsets[p] .. train_offsets[p+1]) (global point numbers in [0, N), any order, gaps allowed; a
 * position t below is a place in that list); y (N) int32 holds the label +1 / -1 of every global point.
 *   kernel    K(i,j) = (double)expf(-(gamma[p] * d2(i,j))): product and expf in float32, evaluated on the fly for the
 *             two rows an iteration needs (nothing of K is stored); so K(i,i) = 1.
 *   state     alpha and the gradient G = Q alpha - 1 are float64; alpha starts at 0 and G at -1.
 *   sets      I_up = {t: y_t = +1 and alpha_t < C, or y_t = -1 and alpha_t > 0};
 *             I_low = {t: y_t = +1 and alpha_t > 0, or y_t = -1 and alpha_t < C}  (libsvm's).
 *   i         = argmax over I_up of -y_t G_t; Gmax is that maximum.  Gmax2 = max over I_low of y_t G_t.
 *   stop      converged (BSED_SVC_CONVERGED) when Gmax + Gmax2 < tol; that sum, at the last evaluation, is gap[p].
 *             Otherwise, after max_iter pair updates: BSED_SVC_NOT_CONVERGED.  info[p] = {pair updates made, status}.
 *   j         = argmin over the t of I_low with b_t = Gmax + y_t G_t > 0 of -b_t^2 / a_t, a_t = 2 - 2 K(i,t), replaced
 *             by TAU = 1e-12 when not positive (second-order working-set selection).
 *   ties      in both choices go to the smallest position t.  This is this project's rule: libsvm's loops keep the
 *             first maximum for i and the LAST minimum for j, and the path is not pinned to that.
 *   update    libsvm's: with q = 2 - 2 K(i,j) (TAU when not positive); y_i != y_j: delta = (-G_i - G_j) / q, both alphas
 *             plus delta, then clipped to the box along alpha_i - alpha_j = const; y_i == y_j: delta = (G_i - G_j) / q,
 *             alpha_i minus and alpha_j plus delta, clipped along alpha_i + alpha_j = const -- the four clipping cases
 *             of each in libsvm's order.  Then G_t += Q_ti dalpha_i + Q_tj dalpha_j for every t.
 *   rho       libsvm's calculate_rho: the mean of y_t G_t over the free points (0 < alpha_t < C), summed in a fixed
 *             order; without a free point (ub + lb) / 2, ub = the minimum of y_t G_t over {alpha_t = C, y_t = -1} and
 *             {alpha_t = 0, y_t = +1}, lb = the maximum over {alpha_t = C, y_t = +1} and {alpha_t = 0, y_t = -1}.
 *   alpha     (total_train) float64, in the order of train_index.
 * Bad problems.  No offset or index is used as an address before it is range-checked.  A problem whose offsets do not
 * satisfy 0 <= begin <= end <= total_train and end - begin <= max_train (BSED_SVC_BAD_OFFSETS), with an index outside
 * [0, N) (BSED_SVC_BAD_INDEX), with a label that is not +1 / -1 (BSED_SVC_BAD_LABEL) or with one class only
 * (BSED_SVC_ONE_CLASS; an empty list is one) writes info[p] = {0, status} and rho[p] = NaN and touches nothing else: not
 * its alpha, not gap[p].  The other problems of the launch are unaffected.
 * The loop is bounded by max_iter; a workgroup waits for nothing but its own barriers.
 * Memory: alpha, G and the (index, label) of every position live in LDS while max_train <= BSED_SVC_LDS_POINTS (20 bytes
 * a point: 120 KB of the 160 KB) and in global memory beyond (alpha in its output, the rest in the workspace); the
 * arithmetic is the same, and so are the bits.  workspace: bsed_svc_solve_workspace(P, total_train) bytes (0 for
 * arguments that are refused), 8-byte aligned, caller-owned, contents irrelevant before and after; it is asked for
 * whatever max_train is and written only beyond BSED_SVC_LDS_POINTS.
 * Refused: null pointers; N < 2 or N > BSED_SVC_MAX_POINTS; P outside 1..BSED_SVC_MAX_PROBLEMS; total_train outside
 * 1..P * BSED_SVC_MAX_POINTS; max_train outside 1..BSED_SVC_MAX_POINTS; C, tol or a gamma[p] not positive and finite;
 * max_iter outside 1..10 000 000; d2, y, the offsets, the indices, gamma or info off a 4-byte boundary; alpha, rho, gap
 * or the workspace off an 8-byte one; a workspace smaller than the query says.
 *
 * bsed_svc_decision: for every entry e of test_index (total_test of them; problem p owns test_offsets[p] ..
 * test_offsets[p+1]) the float64 decision value of its problem,
 *   dec[e] = SUM_j alpha_j y_j K(test_index[e], train_index[j]) - rho[p]   over the training list of p,
 * with the same K; the sum has a fixed order (64 partial sums over the positions j = lane, lane + 64, ..., folded by a
 * fixed tree).  One launch for all problems, one wavefront per entry.  alpha, rho and info are bsed_svc_solve's.  NaN for
 * an entry of a problem that solve marked bad (status above BSED_SVC_NOT_CONVERGED), of a problem whose training offsets
 * or indices are out of range, for a test index outside [0, N) and for an entry no problem owns; no index is used as an
 * address before it is range-checked.
 * Refused: null pointers; N < 2 or N > BSED_SVC_MAX_POINTS; P outside 1..BSED_SVC_MAX_PROBLEMS; total_train or
 * total_test outside 1..P * BSED_SVC_MAX_POINTS; a gamma[p] not positive and finite; misaligned pointers as above (dec
 * on an 8-byte boundary).
 * ---------------------------------------------------------------------------------------------- */
#define BSED_SVC_MAX_POINTS 16384
#define BSED_SVC_MAX_PROBLEMS 64
#define BSED_SVC_LDS_POINTS 6144
#define BSED_SVC_MAX_ITER 10000000
enum { BSED_SVC_CONVERGED = 0, BSED_SVC_NOT_CONVERGED = 1, BSED_SVC_BAD_INDEX = 2, BSED_SVC_BAD_LABEL = 3,
       BSED_SVC_ONE_CLASS = 4, BSED_SVC_BAD_OFFSETS = 5 };
int bsed_svc_d2(const float* x, long long x_pitch, int N, int D, float* d2, void* stream);
size_t bsed_svc_solve_workspace(int P, int total_train);
int bsed_svc_solve(const float* d2, int N, const int* y, const int* train_offsets, const int* train_index, int P,
                   int total_train, int max_train, const float* gamma, double C, double tol, int max_iter, double* alpha,
                   double* rho, double* gap, int* info, void* workspace, size_t workspace_bytes, void* stream);
int bsed_svc_decision(const float* d2, int N, const int* y, const int* train_offsets, const int* train_index,
                      const int* test_offsets, const int* test_index, int P, int total_train, int total_test,
                      const float* gamma, const double* alpha, const double* rho, const int* info, double* dec,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Clip-level tagging (csrc/tagging.hip, ABI 7): the counts behind the reference's per-class weak F1
 * (get_f_measure_by_class, src/evaluation_measures.py:346-427, intermediate_at_measures :430-446) for a whole threshold
 * sweep, and the pseudo weak labels of a batch (src/audio_tagging_inference.py:289-316).
 * ---------------------------------------------------------------------------------------------- */
/* scores (B,C) with T_scores = 0, or (B,T_scores,C), reduced by its maximum over time (:390-392); targets (B,C) with
 * T_targets = 0, used as given, or (B,T_targets,C), reduced by its maximum over time and binarised with `> 0.5`
 * (:394-398).  Both maxima propagate NaN as numpy's do.  thresholds: (S) float32 on the DEVICE, or (S,C) with
 * per_class = 1.  est = score > threshold (strict; a NaN score or threshold gives est = 0).
 * counts (S,C,4) int64 += (tp, fp, fn, tn) over the B clips, as intermediate_at_measures writes them, evaluated in
 * float64 on the target value:  est + ref == 2,  est - ref == 1,  ref - est == 1,  est + ref == 0  -- a target of -1
 * (encode_weak("empty")) is an fp where est = 0 and a tn where est = 1.  Integer atomics, at most one 64-bit add per
 * workgroup per (s, c, kind): the accumulator persists across calls (zero it first), repeated runs give the same bits.
 * Every score and target element is read from HBM once per call whatever S is (the reduced rows of a workgroup's clips
 * are staged in LDS); when even one clip's two rows do not fit (C > 8192) the thresholds read global memory instead,
 * with the same results.  B = 0 returns 0 and launches nothing.  Refused before any launch: null pointers (B > 0), a
 * non-positive S or C, a negative B or T, per_class outside {0, 1}, T * C > (2^31 - 1) / 2, S * C > (2^31 - 1) / 4. */
int bsed_tag_counts(const float* scores, int T_scores, const float* targets, int T_targets, const float* thresholds,
                    int per_class, int S, int B, int C, long long* counts, void* stream);
/* scores as above -> masks[row_offset + b] (uint64, a device buffer of N rows): bit c set when score[b][c] >
 * class_thresholds[c] ((C) float32 on the device) or, with class_thresholds = NULL, > threshold.  *nonempty (device
 * int64) += the number of clips of the batch with a non-zero mask.  C <= 64; rows row_offset .. row_offset + B must lie
 * inside the buffer; B = 0 returns 0 and launches nothing. */
int bsed_tag_masks(const float* scores, int T_scores, const float* class_thresholds, float threshold, int B, int C,
                   long row_offset, long N, uint64_t* masks, long long* nonempty, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Resampling (csrc/resample.hip).  stands in for librosa.load(path, sr=cfg.sr)'s mono mix + resampling
 * (reference src/data/preprocess.py:182); the filter is this project's own (features.resample_filter), NOT
 * librosa's / soxr's: no bit parity with them is claimed.
 * ---------------------------------------------------------------------------------------------- */
#define BSED_PCM_F32 0
#define BSED_PCM_S16 1
/* in: n_in interleaved frames of `channels` samples, float32 (BSED_PCM_F32) or int16 (BSED_PCM_S16) -> out (n_out) mono
 * float32,   out[m] = sum_j x[j] * taps[m * down - j * up + half_len]   over 0 <= j < n_in and tap indices in
 * 0 .. 2 * half_len (zero outside the signal; zero-phase: out[m] sits at input time m * down / up), with the mono mix
 * made while the frames are loaded, in fp32:
 *   BSED_PCM_S16:  x[j] = (float)(s[j][0] + s[j][1] + ... as int32) * (float)(1.0 / (32768.0 * channels))
 *   BSED_PCM_F32:  x[j] = (((s[j][0] + s[j][1]) + s[j][2]) + ...)   * (float)(1.0 / channels)
 * table: the taps by output residue.  With P = (2 * half_len) / up + 1 taps per phase, a(c) = (c * down + half_len) / up
 * and r(c) = (c * down + half_len) % up (integer division), row c = m % up of the (up, P) table is
 *   table[c * P + i] = taps[r(c) + i * up], 0 where r(c) + i * up > 2 * half_len,
 * and out[k * up + c] = fmaf chain over i = 0 .. P - 1, in that order, of x[k * down + a(c) - i] * table[c * P + i]: one
 * fp32 sum per output in a fixed order, no atomics, independent of the launch partition, bitwise repeatable.
 * up = down = 1, half_len = 0, table = {1.0f} converts and mixes only.
 * Refused before any launch: null pointers; n_in < 1; channels outside 1..64; an unknown format; up or down < 1 or
 * not coprime; n_out != ceil(n_in * up / down); in and out overlapping; a filter whose 64 (or `up`, if fewer) table
 * rows plus the samples of 1024 outputs do not fit the 160 KB of LDS (4 * (65 * P + 15 * down + (63 * down) / up + 1 + P) bytes for up > 32). */
int bsed_resample_poly(const void* in, int format, long n_in, int channels, const float* table, int up, int down,
                       int half_len, float* out, long n_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Soundscape synthesis (csrc/synth.hip).  stands in for the reference's offline desed / scaper generation of the SYN set
 * (src/synth_data/synth_data_preprocess.py:116-188): strongly labelled clips are mixed on the device from a resident bank
 * of event snippets and backgrounds.  The sampling is this project's own (synth.py): no parity with desed's draws is
 * claimed.  The gains come from the items' RMS or from their integrated loudness (bsed_loudness below), as the caller
 * of synth.py chooses.
 * ---------------------------------------------------------------------------------------------- */
#define BSED_SYNTH_MAX_EVENTS 16
/* bank: (bank_len) float32, every snippet and background back to back -> out (B, n) float32.  Clip b has a background
 * (bg_off[b], bg_len[b], bg_phase[b]: int64, bank offset / length / start phase in samples; bg_gain[b]: float32) and
 * n_ev[b] (int32, clamped to 0..K) events; event k of clip b is row-major entry [b * K + k] of src (int64: bank offset of
 * its first sample), on (int64: clip sample of its first sample), len (int64: samples), g and inv_fade (float32).
 * Sample j of clip b, in fp32 and in exactly this order:
 *   acc = bank[bg_off + (bg_phase + j) % bg_len] * bg_gain                          (0 when bg_len <= 0: silence)
 *   for k = 0 .. n_ev - 1, if on <= j < on + len, with i = j - on:
 *     w   = fminf(fminf(1, (float)(i + 1) * inv_fade), fminf(1, (float)(len - i) * inv_fade))
 *     acc = fmaf(bank[src + i] * w, g, acc)
 *   out[b][j] = acc
 * one fp32 sum per output in a fixed order, no atomics, independent of the launch partition and of B, bitwise
 * repeatable.  (% is the non-negative remainder.)  The tables are device memory and are not validated (synth.py validates
 * a plan before it uploads it); whatever they hold, no bank index outside 0 .. bank_len - 1 is dereferenced -- such a
 * sample reads as 0 -- and nothing outside out is written.
 * Refused before any launch: null pointers; B < 1; n < 1; K outside 0..BSED_SYNTH_MAX_EVENTS; bank_len < 1; out not
 * 16-byte aligned; a table not aligned to its element size. */
int bsed_synth_mix(const float* bank, long bank_len, const long* bg_off, const long* bg_len, const long* bg_phase,
                   const float* bg_gain, const int* n_ev, const long* src, const long* on, const long* len,
                   const float* g, const float* inv_fade, int B, long n, int K, float* out, void* stream);
/* the targets of such a batch.  n_ev (B) and cls, on_f, off_f (B, K), all int32: class, first frame and end frame of
 * every event -> strong (B, T, C): 1 where some event k < n_ev[b] of class c has on_f <= t < off_f, else 0; weak (B, C):
 * the maximum of strong over t.  Every element is written, in one launch.  An event with off_f <= on_f, or with a class
 * outside 0..C-1, contributes nothing; frames outside 0..T-1 are clipped.
 * Refused before any launch: null pointers; B, T or C < 1; K outside 0..BSED_SYNTH_MAX_EVENTS; misaligned pointers. */
int bsed_synth_targets(const int* n_ev, const int* cls, const int* on_f, const int* off_f, int B, int K, int T, int C,
                       float* strong, float* weak, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Integrated loudness (ABI 15; csrc/loudness.hip).  ITU-R BS.1770-4 for one channel: what scaper (through pyloudnorm)
 * levels the reference's SYN set by (ref_db and the SNR range of src/synth_data/data_config.py:5 are LUFS there).  The
 * rules below are the whole definition; neither pyloudnorm nor scaper was at hand when this was written, so parity with
 * their values is not pinned.
 *
 * Coefficients, on the host in double, from sr, with K = tan(pi * f0 / sr):
 *   stage 1 (shelf):      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196,
 *                         Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2,
 *                         b = (Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0,
 *                         a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0
 *   stage 2 (high-pass):  f0 = 38.13547087602444, Q = 0.5003270373238773, b = 1, -2, 1, a1 and a2 as above from this K, Q
 * (at 48 kHz the table of BS.1770-4 to its printed digits).  bsed_kweight_coefs writes b0 b1 b2 a1 a2 of stage 1, then
 * of stage 2, to out (HOST, 10 doubles); it makes no HIP call and refuses sr outside 1000..384000.
 *
 * Signal of segment s = (seg_off[s], seg_len[s]) of the flat float32 buffer x (x_len samples), len = min(seg_len[s],
 * max_len), half = (sr + 1) / 2:  n_eff = len if len >= half, else len * ceil(half / len) -- a short snippet is measured
 * over whole repetitions of itself up to at least 0.5 s, scaper's practice for events shorter than a block;
 * v[i] = (double)x[seg_off + i % len], 0 where that index lies outside 0 .. x_len - 1; filter state zero at i = 0; stage 1
 * then stage 2, each   y[i] = b0 v[i] + b1 v[i-1] + b2 v[i-2] - a1 y[i-1] - a2 y[i-2]   in double.
 * Blocks: l_j = (j * sr) / 10 in 64-bit integer division; block j is [l_j, l_(j+4)) and exists while l_(j+4) <= n_eff;
 * z_j = the mean of y^2 over the block's own length (for rates divisible by 10: 400 ms at 75 % overlap).
 * Gates: L_j = -0.691 + 10 log10 z_j;  A = {j : L_j > -70};  A empty: the result is -infinity; otherwise
 * Gamma = -0.691 + 10 log10(mean_A z) - 10,  G = {j in A : L_j > Gamma},  loud = -0.691 + 10 log10(mean_G z).
 * A segment with seg_len < 1 gives -infinity and zero counts.
 * -> loud (S) float64;  counts (S, 3) int32 or NULL: the number of blocks, |A|, |G|.
 *
 * Accuracy: the result is not bitwise-defined (the kernel splits a segment, and how depends on S and max_len).  It is
 * within 1e-6 LU of the sequential recurrence above for every segment whose L_j all lie more than 1e-3 LU from both
 * gates, and counts are equal for those segments.  Inside a workgroup the split is exact (a scan of the 4-value filter
 * state); across workgroups a piece starts ceil(50 / -ln r) samples early from zero state, r the largest pole radius
 * (0.21 s at every rate), which leaves less than e^-50 times its length of the input's size behind: below double
 * round-off for anything a float32 input can hold.  Repeatability: bitwise from launch to launch for the same arguments;
 * every sum has a fixed order and there are no floating-point atomics.
 *
 * seg_off and seg_len are DEVICE int64 tables and are not validated: whatever they hold, no index outside
 * 0 .. x_len - 1 is dereferenced and nothing outside loud, counts and the workspace is written.  ws: caller-owned device
 * memory of at least bsed_loudness_ws_bytes(S, max_len, sr) bytes (the per-hop sums of y^2: 8 * S * the hops of the
 * longest effective length; -1 for arguments bsed_loudness would refuse), 8-byte aligned, contents irrelevant before and
 * after.  Two launches, no host synchronisation.
 * Refused before any HIP call: null pointers (counts may be NULL); S < 1; x_len < 1; max_len < 1 (either above 2^40);
 * sr outside 1000..384000, or below 3364 (the shelf's centre frequency would lie above sr / 2, where the recurrence is
 * not stable); ws_bytes too small; a pointer not aligned to its element size.
 * ---------------------------------------------------------------------------------------------- */
int bsed_kweight_coefs(int sr, double* out /*host: 10*/);
long bsed_loudness_ws_bytes(int S, long max_len, int sr);
int bsed_loudness(const float* x, long x_len, const long* seg_off, const long* seg_len, int S, long max_len, int sr,
                  void* ws, long ws_bytes, double* loud, int* counts, void* stream);

typedef struct BsedHeadBwdDesc {
  const float* x;            /* (B,T,K) encoder output */
  const float* w;            /* (2C,K) */
  const float* strong;       /* (B,T,C) saved by bsed_head_fwd */
  const float* sof_raw;      /* (B,T,C) unclamped softmax */
  const float* weak;         /* (B,C) */
  const float* den;          /* (B,C) sum_t clamp(softmax) */
  const float* y_strong;     /* (B,T,C) or NULL: BCE(strong, y) * w_strong */
  const float* y_weak;       /* (B,C)   or NULL: BCE(weak, y)   * w_weak */
  const float* ema_strong;   /* (B,T,C) or NULL: MSE(strong, ema) * w_cons_s */
  const float* ema_weak;     /* (B,C)   or NULL: MSE(weak, ema)   * w_cons_w */
  const float* ema_strong2;  /* (B,T,C) or NULL: second MSE target on strong * w_cons_s2 (ISP shift consistency) */
  const float* g_strong_ext; /* (B,T,C) or NULL: upstream dL/dstrong (autograd drop-in path) */
  const float* g_weak_ext;   /* (B,C)   or NULL */
  float w_strong, w_weak, w_cons_s, w_cons_w, w_cons_s2;
  float inv_n_strong, inv_n_weak; /* 1/(B*T*C), 1/(B*C): reduction='mean' */
  float* dx;                 /* (B,T,K) */
  float* dw_part;            /* (B,2C,K) per-clip partials for bsed_reduce_partials */
  float* db_part;            /* (B,2C) */
  float* loss_part;          /* (B,6): plain sums of BCE_strong, BCE_weak, SE_strong, SE_weak, SE_strong2, 0 */
  int B, T, K, C, attention;
} BsedHeadBwdDesc;

int bsed_head_bwd(const BsedHeadBwdDesc* desc /*host*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Flat-arena optimizer / EMA (csrc/optim.hip)
 * ---------------------------------------------------------------------------------------------- */
/* torch.optim.Adam step (src/main_baseline.py:861-867); grad_scale multiplies g first (1/world_size) */
int bsed_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, long step, float grad_scale, void* stream);
/* torch.optim.SGD(momentum, nesterov, weight_decay) step (src/main_scmt_ada_weak.py:854-866) */
int bsed_sgd_step(float* p, const float* g, float* buf, long n, float lr, float momentum, float weight_decay,
                  int first_step, int nesterov, float grad_scale, void* stream);
/* update_ema_variables (src/main_baseline.py:91-105): ema = ema*alpha + p*(1-alpha) */
int bsed_ema_update(float* ema, const float* p, long n, float alpha, void* stream);
int bsed_ema_update_i64(long long* ema, const long long* p, int n, float alpha, void* stream);
int bsed_scale(float* x, long n, float s, void* stream);
/* per-sample circular shift (torch.roll) of a (B,H,W) tensor: out[b][h][w] = in[b][(h-sh[b]) mod H][(w-sw[b]) mod W];
 * sh / sw are DEVICE int32 arrays (B) or NULL.  Reference src/main_baseline.py:229-277,374-401 (ISP views). */
int bsed_roll(const float* in, float* out, int B, int H, int W, const int* sh, const int* sw, void* stream);
/* Row mixing for interpolation consistency training, "mixup" (csrc/mix.hip).  replaces mixup_data_sup / mixup_data of
 * the reference (src/main.py:127-137,143-156; called at :387,427,460), whose mixup_data takes its three tensors to the
 * host and back.  One launch serves njobs (1..BSED_MIX_MAX_JOBS) jobs; job i mixes the rows of one (rows[i], row_len[i])
 * tensor with the rows a permutation names:
 *   out[r][j] = fl32( fl32(lam * in[r][j]) + fl32(oml * in[perm[r]][j]) )      r < rows, j < row_len
 * The two products are rounded separately, then the sum -- no fused multiply-add, which would round once and give other
 * bits.  With lam = (float)l and oml = (float)(1.0 - l), the subtraction in double, this is bit for bit what
 * `l * x + (1 - l) * x[index, :]` gives in torch and numpy float32 on the host.  Every element of out is written once;
 * bitwise repeatable and independent of the launch partition.
 * The job table is seven parallel HOST arrays of njobs entries, copied into the kernel's arguments (no device allocation,
 * no host synchronisation): in / out / perm hold DEVICE pointers (const float*, float*, const int*), perm[i] an int32
 * array of rows[i] entries.  A job whose in, out and row_len * 4 are all multiples of 16 bytes moves 16 bytes per load
 * and store, any other one 4; both give the same bits.
 * perm is not validated on the device: whatever it holds, an entry outside 0 .. rows - 1 is clamped into that range, so
 * nothing outside the job's in is dereferenced and nothing outside its out is written.
 * Refused before any HIP call: a null table or a null pointer in a job; njobs outside 1..BSED_MIX_MAX_JOBS; rows < 1 or
 * row_len < 1; rows * ceil(row_len / 4) of 2^31 or more; a pointer not aligned to 4 bytes; in == out or overlapping in /
 * out ranges within a job (the gather makes mixing in place a race). */
#define BSED_MIX_MAX_JOBS 8
int bsed_mix_rows(const void* in /*host*/, const void* out /*host*/, const void* perm /*host*/, const float* lam /*host*/,
                  const float* oml /*host*/, const int* rows /*host*/, const long* row_len /*host*/, int njobs,
                  void* stream);
/* y += a * x  (sums the class-loss and domain-loss gradients at the encoder output) */
int bsed_axpy(float* y, const float* x, long n, float a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Self tests (used by tests/ only)
 * ---------------------------------------------------------------------------------------------- */
/* C(32,32) = A(32,K) @ B(K,32) through one wave of v_mfma_f32_32x32x2_f32: pins the fragment maps */
int bsed_selftest_mfma(const float* A, const float* B, float* C, int K, void* stream);
/* the same through v_mfma_f32_32x32x16_bf16 with bf16x3 split operands (K a multiple of 16) */
int bsed_selftest_mfma_bf16x3(const float* A, const float* B, float* C, int K, void* stream);

/* Device-resident step state for HIP-graph replays of a train step (csrc/capi.hip).  In a launch made while it is set,
 * the dropout kernels of the plain train step -- bsed_dropout, bsed_block0_fwd / _bwd, bsed_glu_fwd3, bsed_glu_bwd3,
 * bsed_glu_bwd3n, bsed_glu16_fwd / _bwd, bsed_glu_bwd_fused and the GLU_POOL / GLU_BWD epilogues of bsed_igemm -- add
 * *seed_add_dev (uint64) to their seed, and bsed_adam_step adds *step_add_dev (int) to its step count and uses *lr_dev
 * (float) in place of its lr argument.  bsed_leaky_dropout_fwd / _bwd and bsed_mel_noise do not read it.
 * bsed_step_state_advance is the graph node that bumps the two addends after a step.  The state belongs to the calling
 * thread and is read on the host when a kernel is launched: set it immediately before a stream capture and clear it
 * immediately after, on the capturing thread.  A captured graph carries the pointers it was captured with and never
 * consults the library again; the memory behind them must outlive the graph.  All three NULL = eager mode (the
 * default); a mix of NULL and non-NULL is refused. */
int bsed_set_step_state(const void* seed_add_dev, const void* step_add_dev, const void* lr_dev);
int bsed_step_state_advance(void* seed_add_dev, void* step_add_dev, uint64_t seed_inc, int step_inc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BSED_H */
