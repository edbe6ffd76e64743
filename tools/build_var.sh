#!/bin/bash
# Variant builds of the library for A/B timing on the GPU box (RAOCP_HIP_LIB=build/var/<name>.so):
#   tools/build_var.sh <name> "<-D flags for raocp_capi.hip>" [<name> "<flags>" ...]
# Each variant recompiles the capi translation unit (the L / L^T kernels live there) and links
# it with the current objects of the other translation units (the Makefile's unit list, so a
# variant links what the library links); the builds run in parallel.
# VAR_ALL=1: every translation unit with the variant's flags (e.g. -DRAOCP_DIAG).
# VAR_UNIT=<u> (dynr, cp4, cp5, or any unit but capi): only that unit with the flags, linked
# with the current objects of the others (capi included): a one-minute build.
set -e
cd "$(dirname "$0")/../raocp-toolbox_amd"
mkdir -p ../build/var
units=$(make -s units)
pids=()
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  ( # the units compiled with the variant's flags; every other unit's current object is linked
    if [ "${VAR_ALL:-0}" = 1 ]; then mine=$units; else mine=${VAR_UNIT:-capi}; fi
    objs=""
    for u in $units; do
      if [[ " $mine " == *" $u "* ]]; then
        /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $flags \
          -c csrc/raocp_$u.hip -o ../build/var/${u}_$name.o > ../build/var/$name.$u.build.txt 2>&1 || exit 1
        objs="$objs ../build/var/${u}_$name.o"
      else
        objs="$objs ../build/obj/raocp_$u.o"
      fi
    done
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared $objs -o ../build/var/$name.so && echo "variant $name built" ) &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
