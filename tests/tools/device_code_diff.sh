#!/bin/bash
# Developer check (no GPU needed): is the device code of two source trees the same, byte for byte?
#   bash tests/tools/device_code_diff.sh <old tree> <new tree> [workdir]
# Every .hip file of the Makefile's KERNEL_SRC is compiled for the device only (hipcc --cuda-device-only -S) with the Makefile's
# HIPFLAGS, once as the product and once with -DUVRT_DEV_VARIANTS, in both trees, and the assembly is compared.  The one
# symbol that depends on where a tree lies (__hip_cuid_<hash of the path>) is masked.  One line per file and build, then
# the verdict; exit status 0 only when nothing differs.  What a host-only change must show.
set -e
OLD=$(cd "$1" && pwd); NEW=$(cd "$2" && pwd); WORK=${3:-$(mktemp -d)}
PKG=small-project-uv-robot-ray-tracer_amd
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize -Wall -Wno-unused-result"
SRC=$(sed -n '/^KERNEL_SRC/,/[^\\]$/p' "$NEW/$PKG/Makefile" | tr -d '\\' | tr ' ' '\n' | grep '\.hip$')
for side in old new; do
  if [ $side = old ]; then T=$OLD; else T=$NEW; fi
  mkdir -p "$WORK/$side"
  for f in $SRC; do
    b=$(basename $f .hip)
    ( cd "$T/$PKG" && $HIPCC $FLAGS --cuda-device-only -S -o "$WORK/$side/$b.product.s" $f 2>/dev/null ) &
    ( cd "$T/$PKG" && $HIPCC $FLAGS -DUVRT_DEV_VARIANTS --cuda-device-only -S -o "$WORK/$side/$b.dev.s" $f 2>/dev/null ) &
  done
  wait
  sed -i -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_MASKED/g' "$WORK/$side"/*.s
done
bad=0
for f in "$WORK"/new/*.s; do
  b=$(basename $f)
  if cmp -s "$WORK/old/$b" "$f"; then echo "identical  $b  ($(wc -l < $f) lines)"; else echo "DIFFERENT  $b"; bad=$((bad+1)); fi
done
n=$(ls "$WORK"/new/*.s | wc -l)
echo "$n files compared, $bad differ"
[ $bad -eq 0 ]
