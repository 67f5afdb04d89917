#!/bin/bash
# Build libbsed.so for gfx950 in-tree (the .so travels to the GPU box with the snapshot).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result"
mkdir -p obj
# an object is stale when its source or ANY header (csrc/*.h, the C ABI) is newer
newer_header() { local h; for h in *.h ../../include/bsed.h; do [ "$h" -nt "$1" ] && return 0; done; return 1; }
pids=()
objs=()
for f in *.hip; do
  o=obj/${f%.hip}.o
  objs+=("$o")
  if [ ! -f "$o" ] || [ "$f" -nt "$o" ] || newer_header "$o"; then
    # mel.hip: the SLP vectorizer packs the FFT's scalar fp32 arithmetic into v_pk_* with op_sel swizzles, whose
    # destination-forwarding hazards cost ~90 s_nop per frame: 0.635 -> 0.599 ms without it (A/B on MI355X).
    # The GCN register-pressure trackers let the scheduler see stft_mel2_kernel's real pressure: without them the
    # default max-occupancy scheduler fills all 256 registers and the allocator spills 16-49 dwords (their reloads sit
    # behind the prefetched global loads in vmcnt order: 0.655 ms against 0.603 ms spill-free)
    extra=""; [ "$f" = "mel.hip" ] && extra="-fno-slp-vectorize -mllvm -amdgpu-use-amdgpu-trackers=1"
    # glu3.hip / head.hip: no SLP vectorizer either.  (1) Speed: the packed v_pk_* forms it makes of the epilogues'
    # per-element fp32 arithmetic are SLOWER here (GLU backward family 2.14 -> 1.91 ms per step at B = 256, same-box
    # A/B; igemm.hip and wgrad.hip -- one file when that was measured --, block0.hip and gru.hip lose without it and keep
    # it, as does reduce.hip: all three build with the default flags).  (2) Repeatability: with the vectorizer on, a
    # build of glu_bwd3n_kernel whose tile width is a compile-time constant is not bitwise repeatable (the pool /
    # dropout mask of one element class flips in lanes 48..63 from launch to launch; no wait state, scheduling fence or
    # s_waitcnt changes it -- tools/asm_variant.sh experiments).  Cause not identified; masked by
    # -fno-slp-vectorize; see ADVICE.md.  tests/test_glu_repeat_gpu.py checks every built instance over repeated launches.
    { [ "$f" = "glu3.hip" ] || [ "$f" = "head.hip" ]; } && extra="-fno-slp-vectorize"
    $HIPCC $FLAGS $extra -c "$f" -o "$o" &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../libbsed.so "${objs[@]}"
echo "built $(realpath ../libbsed.so)"
