#!/bin/bash
# Device assembly of every translation unit of libfmj_hip.so, and one sha256 per unit: the gate of a refactor that must not
# change the generated code. Two trees that print the same 29 digests compile to the same kernels.
#   scripts/device_listing.sh [TREE] [OUTDIR]
# TREE is a source tree holding farms_mujoco_amd/csrc and include/ (default: this checkout; for a revision,
# `git archive REV farms_mujoco_amd/csrc include | tar -x -C DIR`), OUTDIR receives <unit>.s (default: a fresh temporary directory).
# Flags are those of farms_mujoco_amd/_lib.py build() plus --cuda-device-only -S; the digest is taken over the listing without
# its .file / .ident lines (they name the path and the compiler build) and with the hash in the __hip_cuid_<hash> symbol blanked
# (hipcc derives it from the source path). MAX_JOBS caps the parallel compiles.
# A change that adds a kernel to a unit moves that unit's digest; scripts/kernel_body_digest.py then compares the kernels that were
# already there one by one, from the two listings in OUTDIR.
set -euo pipefail
tree=$(cd "${1:-$(dirname "$0")/..}" && pwd)
out=${2:-$(mktemp -d /tmp/fmj_listing_XXXX)}
mkdir -p "$out"
flags="--offload-arch=gfx950 -O3 -fno-slp-vectorize -mllvm -pragma-unroll-threshold=131072 -fPIC --cuda-device-only -S -Wno-unused-command-line-argument"
units="host:"
for n in $(seq 4 4 64); do units+=" k$n:-DFMJ_TU_MAXD=$n"; done
units+=" kw32:-DFMJ_TU_WIDE=32 kw64:-DFMJ_TU_WIDE=64 kf64:-DFMJ_TU_F64 kf64l:-DFMJ_TU_F64=2 kf64r:-DFMJ_TU_F64=3 kf64c:-DFMJ_TU_F64=4 kf64t:-DFMJ_TU_F64=5 kf64e:-DFMJ_TU_F64=6 kf64m:-DFMJ_TU_F64=7 kf64me:-DFMJ_TU_F64=8 kf64tr:-DFMJ_TU_F64=9 kf64er:-DFMJ_TU_F64=10"
jobs=${MAX_JOBS:-$(nproc)}
# run from the tree with a relative source path: the listing then holds no absolute path of the tree
cd "$tree"
printf '%s\n' $units | xargs -P "$jobs" -I{} sh -c 'u={}; hipcc '"$flags"' ${u#*:} farms_mujoco_amd/csrc/fmj_hip.hip -o "'"$out"'/${u%%:*}.s"'
for u in $units; do
  u=${u%%:*}
  printf '%s  %s\n' "$(grep -v -e '^[[:space:]]*\.file' -e '^[[:space:]]*\.ident' "$out/$u.s" | sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_/g' | sha256sum | cut -d' ' -f1)" "$u"
done
echo "listings in $out" >&2
