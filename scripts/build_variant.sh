#!/bin/bash
# A/B helper: a variant library that differs from csrc/libfmj_hip.so in ONE step-kernel unit, the register row length the measured
# model runs (default 20, the salamander; MAXD=<n> names another).  That unit is compiled with the extra flags, every other object is
# the one build() left in csrc/_obj, so a full build() of this tree must come first.
#   scripts/build_variant.sh <name> [hipcc flags...]      -> csrc/libfmj_hip_<name>.so, for FMJ_SO (scripts/ab.sh) or FMJ_STAMPS_SO
#   e.g. scripts/build_variant.sh b -DFMJ_DUAL_PRIO_PHASE=2;  scripts/build_variant.sh stamps_b -DFMJ_STAMPS -DFMJ_DUAL_PRIO_PHASE=2
# The host object is not rebuilt: what fmj_dual_build_info reports about the priority policy is the default build's.
set -euo pipefail
name=$1; shift
maxd=${MAXD:-20}
csrc=$(cd "$(dirname "$0")/../farms_mujoco_amd/csrc" && pwd)
[ -f "$csrc/_obj/host.o" ] || { echo "no objects in $csrc/_obj: run build() first" >&2; exit 1; }
mkdir -p "$csrc/_obj_variants"
obj=$csrc/_obj_variants/${name}_k$maxd.o
hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize -mllvm -pragma-unroll-threshold=131072 -fPIC "$@" -DFMJ_TU_MAXD=$maxd -c "$csrc/fmj_hip.hip" -o "$obj"
others=$(ls "$csrc"/_obj/*.o | grep -v "/k$maxd\.o$")
hipcc --offload-arch=gfx950 -shared -fPIC $others "$obj" -o "$csrc/libfmj_hip_$name.so"
ls -la "$csrc/libfmj_hip_$name.so"
