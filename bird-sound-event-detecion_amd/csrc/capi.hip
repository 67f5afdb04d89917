// Error plumbing + build info of libbsed.so.
#include "bsed_common.h"
#include "../../include/bsed.h"
#include <stdarg.h>

static thread_local char g_err[512] = "";

void bsed_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* bsed_last_error(void) { return g_err; }
extern "C" const char* bsed_build_info(void) { return "libbsed gfx950: fp32 storage/accumulation, split-fp32 (bf16x3) contractions on v_mfma_f32_32x32x16_bf16 by default, "
         "exact-fp32 v_mfma_f32_32x32x2_f32 kernels selectable (hand-written HIP)"; }
extern "C" int bsed_abi_version(void) { return 20; }   // 20: the domain classifier, an RBF C-SVC by libsvm's rules, bsed_svc_d2 / bsed_svc_solve / bsed_svc_decision and bsed_svc_solve_workspace (csrc/svc.hip); 19: exact t-SNE of an embedding, bsed_tsne_affinities / bsed_tsne_gradient / bsed_tsne_update and their workspace queries (csrc/tsne.hip); 18: row mixing for interpolation consistency training, bsed_mix_rows (csrc/mix.hip); 17: all-pairs statistics of an embedding for the domain gap, bsed_pair_stats / bsed_pair_stats_splits / bsed_pair_stats_workspace (csrc/pair_stats.hip); 16: segment-based counts for sed_eval's segment F1 and error rate, bsed_segment_counts (csrc/segment_metrics.hip); 15: integrated loudness in LUFS, bsed_loudness / bsed_loudness_ws_bytes / bsed_kweight_coefs (csrc/loudness.hip); 14: both gradients of the HBM-bound 3 x 3 convolutions in one pass, bsed_conv_bwd3 / bsed_conv_bwd_plan, BsedWgradDesc.w3s / d_in / din_pitch (csrc/conv_bwd.hip); 13: intersection-based counts for psds_eval's macro F1 and PSDS (csrc/intersect.hip); 12: BsedContractPlan + bsed_igemm_plan / bsed_wgrad_plan for the six contraction entry points, BsedIgemmDesc.G (csrc/igemm*.hip); 11: BsedGluDesc + bsed_glu_plan for the GLU / first-block entry points (csrc/glu*.hip, csrc/block0.hip); 10: dataset scaler statistics + normalised dB kernels (csrc/scaler.hip, csrc/mel.hip); 9: soundscape synthesis (csrc/synth.hip); 8: Predictor head for 1..64 classes + bsed_head_lds_bytes (csrc/head.hip); 7: clip-level tagging counts + pseudo-label masks (csrc/tagging.hip); 6: threshold sweep + event F1 counts (csrc/metrics.hip); 5: resampling (csrc/resample.hip); 4: recording-level detection (csrc/detect.hip)

// the plan of a GLU / first-block entry point (bsed_common.h): the query the callers size their buffers with
extern "C" int bsed_glu_plan(const BsedGluDesc* desc, int kernel, BsedGluPlan* out) {
  BSED_CHECK_ARG(desc && out, "bsed_glu_plan: null argument");
  return bsed_glu_plan_for(*desc, kernel, *out);
}
// the plan of a contraction entry point: the kernel's own prepare step and template dispatch answer (csrc/igemm*.hip)
extern "C" int bsed_igemm_plan(const BsedIgemmDesc* desc, int kernel, BsedContractPlan* out) {
  static int (*const run[])(const BsedIgemmDesc*, void*, BsedContractPlan*) = {bsed_run_igemm, bsed_run_igemm3,
                                                                                bsed_run_igemm3s, bsed_run_igemm3n};
  BSED_CHECK_ARG(desc && out && kernel >= BSED_CONTRACT_IGEMM && kernel <= BSED_CONTRACT_IGEMM3N,
                 "bsed_igemm_plan: null argument or unknown kernel %d", kernel);
  return run[kernel](desc, nullptr, out);
}
extern "C" int bsed_wgrad_plan(const BsedWgradDesc* desc, int kernel, BsedContractPlan* out) {
  BSED_CHECK_ARG(desc && out && (kernel == BSED_CONTRACT_WGRAD || kernel == BSED_CONTRACT_WGRAD3),
                 "bsed_wgrad_plan: null argument or unknown kernel %d", kernel);
  return bsed_run_wgrad(desc, kernel == BSED_CONTRACT_WGRAD3, nullptr, out);
}

// ----------------------------------------------------------------------------------------------
// Device-resident step state (HIP-graph replays of a train step, engine.SEDTrainer.capture_step): a captured launch
// bakes its scalar arguments, so what changes from step to step -- the dropout seed, the optimizer's step count and the
// learning rate -- is ALSO read from device memory.  For a launch made while the pointers are set,
//   - the dropout kernels of the plain train step add *seed_add to their seed: bsed_dropout, the eight BsedGluDesc
//     entry points (bsed_glu16_*, bsed_block0_fwd / _bwd, bsed_glu_bwd_fused, bsed_glu_fwd3 / _bwd3 / _bwd3n: one read,
//     in bsed_glu_args of bsed_common.h) and the GLU_POOL / GLU_BWD epilogues of bsed_igemm.  bsed_leaky_dropout_fwd /
//     _bwd (discriminator) and bsed_mel_noise (mean teacher) do NOT: no step that can be captured reaches them;
//   - bsed_adam_step adds *step_add to its step count and takes *lr instead of its lr argument;
//   - bsed_step_state_advance (a node of the graph) bumps the two addends.
// Null pointers = eager mode (the default): the host scalars alone, the same arithmetic, the same bits.  The pointers
// are read on the host at launch time and are meant to be set only for the duration of a stream capture, on the
// capturing thread (they are thread_local: launches of other threads never see them): the captured nodes carry the
// pointers they were captured with, so a replay does not consult the library, and the memory behind them must outlive
// the graph.
// ----------------------------------------------------------------------------------------------
static thread_local const uint64_t* g_seed_add = nullptr;
static thread_local const int* g_step_add = nullptr;
static thread_local const float* g_lr = nullptr;
const uint64_t* bsed_seed_add_ptr() { return g_seed_add; }
const int* bsed_step_add_ptr() { return g_step_add; }
const float* bsed_lr_ptr() { return g_lr; }
extern "C" int bsed_set_step_state(const void* seed_add_dev, const void* step_add_dev, const void* lr_dev) {
  BSED_CHECK_ARG((seed_add_dev != nullptr) == (step_add_dev != nullptr) && (seed_add_dev != nullptr) == (lr_dev != nullptr),
                 "bsed_set_step_state: the three pointers are set together or cleared together");
  g_seed_add = (const uint64_t*)seed_add_dev;
  g_step_add = (const int*)step_add_dev;
  g_lr = (const float*)lr_dev;
  return BSED_OK;
}
__global__ void step_state_advance_kernel(uint64_t* seed_add, int* step_add, uint64_t seed_inc, int step_inc) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { *seed_add += seed_inc; *step_add += step_inc; }
}
extern "C" int bsed_step_state_advance(void* seed_add_dev, void* step_add_dev, uint64_t seed_inc, int step_inc, void* stream) {
  BSED_CHECK_ARG(seed_add_dev && step_add_dev, "bsed_step_state_advance: null state");
  hipLaunchKernelGGL(step_state_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint64_t*)seed_add_dev,
                     (int*)step_add_dev, seed_inc, step_inc);
  BSED_LAUNCH_CHECK();
  return BSED_OK;
}
