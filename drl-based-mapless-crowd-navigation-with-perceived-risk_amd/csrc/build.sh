#!/bin/bash
# Builds libcrowdnav.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
#   build.sh            the product library
#   build.sh timing     ONLY the profiling sibling libcrowdnav_timing.so (stage time stamps, PMC calibration kernels,
#                       device-math test kernels; never loaded by the product)
#   build.sh all        both
#   -ffp-contract=off : no implicit FMA contraction; every fma() in the sources is explicit, which is
#                       what makes the simulator bit-reproducible against the CPU oracle
# crowdnav_kernel.hip is compiled as six units (-DCN_TU=n).  Which kernel is defined in which unit is a column of the kernel table,
# crowdnav_variants.h: unit 1 holds every one-step kernel, units 2-5 the sequence and policy kernels (their rows name the unit) --
# compiled with -mllvm -disable-machine-licm: see the note above the kernel definitions -- and unit 6 the population's actor
# kernels (cn_actor_pop_*: apart, so that unit 1's kernels keep their instruction streams).  The units only spread the compile
# over processes and flags; the file also compiles as one unit with CN_TU unset.
# crowdnav_pop_record.hip holds the population recorder's two kernels (cn_pop_record); their bodies, crowdnav_record.h, are the ones
# crowdnav_td3.hip's cn_replay_write / cn_episode_log_add kernels are made of.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../lib"
mkdir -p "$OUT"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-builtin-pow -Wall -Wno-unused-function"
WHAT="${1:-product}"
build_lib() {   # $1 = output name, $2.. = extra flags
  local name="$1"; shift
  local T; T="$(mktemp -d)"
  trap 'rm -rf "$T"' RETURN
  local pids=()
  "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" -DCN_TU=1 -c -o "$T/k1.o" "$HERE/crowdnav_kernel.hip" & pids+=($!)
  "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" -DCN_TU=2 -mllvm -disable-machine-licm -c -o "$T/k2.o" "$HERE/crowdnav_kernel.hip" & pids+=($!)
  "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" -DCN_TU=3 -mllvm -disable-machine-licm -c -o "$T/k3.o" "$HERE/crowdnav_kernel.hip" & pids+=($!)
  "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" -DCN_TU=4 -mllvm -disable-machine-licm -c -o "$T/k4.o" "$HERE/crowdnav_kernel.hip" & pids+=($!)
  "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" -DCN_TU=5 -mllvm -disable-machine-licm -c -o "$T/k5.o" "$HERE/crowdnav_kernel.hip" & pids+=($!)
  "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" -DCN_TU=6 -c -o "$T/k6.o" "$HERE/crowdnav_kernel.hip" & pids+=($!)
  "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" -c -o "$T/abi.o" "$HERE/crowdnav_abi.hip" & pids+=($!)
  "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" -c -o "$T/td3.o" "$HERE/crowdnav_td3.hip" & pids+=($!)
  "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" -c -o "$T/tab.o" "$HERE/crowdnav_tab.hip" & pids+=($!)
  "$HIPCC" $FLAGS ${CN_EXTRA_FLAGS:-} "$@" -c -o "$T/rec.o" "$HERE/crowdnav_pop_record.hip" & pids+=($!)
  local failed=0 pid
  for pid in "${pids[@]}"; do wait "$pid" || failed=1; done     # a bare `wait` returns 0 whatever the jobs returned
  if [ "$failed" != 0 ]; then echo "build.sh: a compile of $name failed" >&2; return 1; fi
  # link next to the target and rename: a process that already mapped the old file keeps it, nobody maps a partial one
  "$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$OUT/.$name.$$" "$T/k1.o" "$T/k2.o" "$T/k3.o" "$T/k4.o" "$T/k5.o" "$T/k6.o" "$T/abi.o" "$T/td3.o" "$T/tab.o" "$T/rec.o"
  mv -f "$OUT/.$name.$$" "$OUT/$name"
}
if [ "$WHAT" = "product" ] || [ "$WHAT" = "all" ]; then
  build_lib libcrowdnav.so
  echo "built $OUT/libcrowdnav.so"
fi
if [ "$WHAT" = "timing" ] || [ "$WHAT" = "all" ]; then
  build_lib libcrowdnav_timing.so -DCN_TIMING
  echo "built $OUT/libcrowdnav_timing.so (stage time stamps; profiling only)"
fi
