#!/bin/bash
# build a variant of libivx_hip.so with extra -D flags for the region probe (ivx_regions_route.hip, ivx_regions_probe.hip):
# tools/variant.sh <name> <flags...>
set -eo pipefail
cd "$(dirname "$0")/../datafusion-bio-functions_amd"
N=$1; shift
for f in route probe; do
hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -I../include "$@" -c csrc/ivx_regions_$f.hip -o /tmp/jr_${f}_$N.o -Rpass-analysis=kernel-resource-usage 2>&1 | grep -A8 "k_probe_regionsILi1" | grep -E "VGPRs:|ScratchSize|LDS Size" || true
done
OBJS=$(ls build/*.o | grep -v ivx_regions_)
hipcc --offload-arch=gfx950 -shared -fPIC -o lib/lib_$N.so $OBJS /tmp/jr_route_$N.o /tmp/jr_probe_$N.o
echo built lib/lib_$N.so
