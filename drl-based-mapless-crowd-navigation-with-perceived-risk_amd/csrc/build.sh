#!/bin/bash
# Builds libcrowdnav.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
#   build.sh                the product library
#   build.sh timing         ONLY the profiling sibling libcrowdnav_timing.so (stage time stamps, and crowdnav_debug.hip: PMC calibration
#                           kernels, device-math test kernels; never loaded by the product)
#   build.sh all            both
#   build.sh objects DIR    only compile the product's units into DIR/<object>.o (tools/profc/build.sh links them with its own unit 1:
#                           CN_SKIP_UNIT=k1 leaves that one out)
#   -ffp-contract=off : no implicit FMA contraction; every fma() in the sources is explicit, which is
#                       what makes the simulator bit-reproducible against the CPU oracle
# One file per subsystem, and UNITS below is the only list of them: the compile loop and the link line both come from it.
# crowdnav_kernel.hip (the environment's step, sequence and policy kernels) is compiled as five units (-DCN_TU=n).  Which kernel is
# defined in which unit is a column of the kernel table, crowdnav_variants.h: unit 1 holds every one-step kernel, units 2-5 the sequence
# and policy kernels (their rows name the unit), compiled with -mllvm -disable-machine-licm: see the note above the kernel definitions.
# The units only spread the compile over processes and flags.  crowdnav_step_group.hip includes the same file for its group-only
# section (cn_step_group_*'s kernels: one launch for several handles), so unit 1 compiles what it always did.  crowdnav_stages.h is the one table of the step kernel's stage stamps
# (timing slots, the FAIR kernels' s_setprio levels; the profiling tools parse it).  crowdnav_lds.h holds every size of an environment's LDS working
# set once: the kernels carve with them, crowdnav_abi.hip sizes the launches from cn_lds_map, which composes them.  crowdnav_abi.hip is the environment's host side; the other files each
# hold a subsystem's kernels next to the host code that launches them: the TD3 actor and the population's actors, the tabular
# learners, the population's recorder (its bodies, crowdnav_record.h, are shared with crowdnav_replay.hip's kernels: one learner's
# replay writes and episode log, and with crowdnav_nstep.hip's, the recorder of n-step rows; crowdnav_record_host.h holds the members' checks of both recorders; crowdnav_eval.hip, the evaluator of many jobs, instantiates the episode log's body a third time), a learner's
# state as one blob (crowdnav_state.hip: one copy kernel; crowdnav_state.h is what it asks of a learner's unit), and the fused learners, a unit each -- crowdnav_td3.hip (with the population), crowdnav_ddpg.hip,
# crowdnav_dqn.hip, crowdnav_sac.hip -- around crowdnav_gemm.hip, the only unit that defines the GEMM and prep kernels they all
# launch: it exports host launchers (crowdnav_learner.h, with the learners' host scaffold; crowdnav_learner_device.h holds the
# device helpers that more than one of these units inlines).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../lib"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-builtin-pow -Wall -Wno-unused-function"
WHAT="${1:-product}"
UNITS=(         # object, source, flags of its own
  "k1    crowdnav_kernel.hip      -DCN_TU=1"
  "k2    crowdnav_kernel.hip      -DCN_TU=2 -mllvm -disable-machine-licm"
  "k3    crowdnav_kernel.hip      -DCN_TU=3 -mllvm -disable-machine-licm"
  "k4    crowdnav_kernel.hip      -DCN_TU=4 -mllvm -disable-machine-licm"
  "k5    crowdnav_kernel.hip      -DCN_TU=5 -mllvm -disable-machine-licm"
  "kgrp  crowdnav_step_group.hip"
  "abi   crowdnav_abi.hip"
  "actor crowdnav_actor.hip"
  "gemm  crowdnav_gemm.hip"
  "td3   crowdnav_td3.hip"
  "ddpg  crowdnav_ddpg.hip"
  "dqn   crowdnav_dqn.hip"
  "sac   crowdnav_sac.hip"
  "replay crowdnav_replay.hip"
  "tab   crowdnav_tab.hip"
  "rec   crowdnav_pop_record.hip"
  "nstep crowdnav_nstep.hip"
  "eval  crowdnav_eval.hip"
  "state crowdnav_state.hip"
)
TIMING_UNITS=("debug crowdnav_debug.hip")      # build.sh timing adds these
compile_units() {   # $1 = directory for the objects, $2.. = extra flags: every unit of LIST, in parallel; OBJS = the objects, in LIST's order
  local dir="$1" pids=() failed=0 pid unit obj src own; shift
  OBJS=()
  for unit in "${LIST[@]}"; do
    read -r obj src own <<< "$unit"
    [ "$obj" = "${CN_SKIP_UNIT:-}" ] && continue
    "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" $own -c -o "$dir/$obj.o" "$HERE/$src" & pids+=($!)
    OBJS+=("$dir/$obj.o")
  done
  for pid in "${pids[@]}"; do wait "$pid" || failed=1; done     # a bare `wait` returns 0 whatever the jobs returned
  if [ "$failed" != 0 ]; then echo "build.sh: a compile failed" >&2; return 1; fi
}
build_lib() {   # $1 = output name, $2.. = extra flags
  local name="$1"; shift
  local T; T="$(mktemp -d)"
  trap 'rm -rf "$T"' RETURN
  mkdir -p "$OUT"
  compile_units "$T" "$@"
  # link next to the target and rename: a process that already mapped the old file keeps it, nobody maps a partial one
  "$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$OUT/.$name.$$" "${OBJS[@]}"
  mv -f "$OUT/.$name.$$" "$OUT/$name"
}
LIST=("${UNITS[@]}")
if [ "$WHAT" = "objects" ]; then compile_units "$2"; fi
if [ "$WHAT" = "product" ] || [ "$WHAT" = "all" ]; then
  build_lib libcrowdnav.so
  echo "built $OUT/libcrowdnav.so"
fi
if [ "$WHAT" = "timing" ] || [ "$WHAT" = "all" ]; then
  LIST+=("${TIMING_UNITS[@]}")
  build_lib libcrowdnav_timing.so -DCN_TIMING
  echo "built $OUT/libcrowdnav_timing.so (stage time stamps; profiling only)"
fi
