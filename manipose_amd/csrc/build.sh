#!/bin/bash
# Build libmanipose_hip.so for gfx950 (MI355X) in-tree.  Usage: manipose_amd/csrc/build.sh
# MP_DIAG=1: the diagnostics build (-DMP_GEMM_DIAG: per-tile time stamps / start stagger in the persistent GEMMs) -> libmanipose_hip_diag.so,
# loaded through MANIPOSE_HIP_LIB by tools/gemm_stamps.py; never the product library.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../libmanipose_hip.so"
OBJ="$HERE/_obj"
EXTRA=""
if [ "${MP_DIAG:-0}" = "1" ]; then OUT="$HERE/../libmanipose_hip_diag.so"; OBJ="$HERE/_obj_diag"; EXTRA="-DMP_GEMM_DIAG"; fi
mkdir -p "$OBJ"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
# -fno-slp-vectorize and -packed-fp32-ops: no v_pk_*_f32 in the device code.  Two round-3 wrong-result defects sat at SLP-made packed ops with op_sel (cause: common.h, "packed-fp32 guard"; reproduced in round 5, profiles/r05_defect_isa/)
# (DESIGN sections 2 and 5), and packed fp32 is slower than the plain instructions it replaces on this chip (same-box A/B of the whole
# library: 171.6 / 170.9 -> 170.2 / 169.9 ms per step).  The feature flag also reaches the host pass, which says it does not know it: filtered.
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -fno-slp-vectorize -Xclang -target-feature -Xclang -packed-fp32-ops -Wall -Wno-unused-function $EXTRA"
pids=()
objs=()
for f in "$HERE"/*.hip; do
  o="$OBJ/$(basename "${f%.hip}").o"
  objs+=("$o")                 # the link takes the objects of the sources that are present, not a stale one of a deleted source
  if [ ! -f "$o" ] || [ "$f" -nt "$o" ] || [ "$HERE/common.h" -nt "$o" ] || [ "$HERE/kernels.h" -nt "$o" ] || [ "$HERE/hazard.h" -nt "$o" ] || [ "$HERE/kloop_asm.inc" -nt "$o" ] || [ "$HERE/lift_common.h" -nt "$o" ] || [ "$HERE/lift_geom.h" -nt "$o" ] || [ "$HERE/lift_skeleton.h" -nt "$o" ] || [ "$HERE/../../include/manipose_hip.h" -nt "$o" ]; then
    $HIPCC $FLAGS -c "$f" -o "$o" 2> >(grep -v "is not a recognized feature for this target" >&2) &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT" "${objs[@]}"
echo "built $OUT"
