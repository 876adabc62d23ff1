#!/bin/bash
# Build experiment variants of the render library: tools/_var/<name>/librt_amd.so, one per
# "name=-DFLAG ..." argument (depth <= RT_MAX_B, default 3 = the c1..c5 kernels; the per-depth translation units
# of a variant compile in parallel).  Run them with tools/ab_variants.sh or tools/ab_libs.py on the GPU.
# The kernel objects are the Makefile's own list (its `kobjs` target: every unit of the device half, the per-depth
# render, adaptive and lens objects), built into the variant's directory with the variant's flags.
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=$ROOT/ray_tracer_fragment_shader_amd/csrc
LIB=$ROOT/ray_tracer_fragment_shader_amd/lib
make -C "$SRC" -s ../lib/rt_host.o ../lib/rt_screen.o ../lib/rt_group.o ../lib/rt_group_plan.o
for spec in "$@"; do
  name=${spec%%=*}; flags=${spec#*=}
  d=$ROOT/tools/_var/$name; mkdir -p "$d"
  make -C "$SRC" -s -j8 OUT="$d" EXTRA="-DRT_MAX_B=${RT_MAX_B:-3} $flags" ${KERNARG_PRELOAD:+KERNARG_PRELOAD=$KERNARG_PRELOAD} kobjs
  /opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o "$d/librt_amd.so" "$d"/*.o "$LIB/rt_host.o" "$LIB/rt_screen.o" \
      "$LIB/rt_group.o" "$LIB/rt_group_plan.o" -L/opt/rocm/lib -lrccl -lhsa-runtime64
  rm -f "$d"/*.o
  echo "built $name"
done
