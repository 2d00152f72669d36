#!/bin/bash
# Build an experiment variant of the modem library with extra compile flags:
#   tools/build_variant.sh NAME "-DOFDM_RX_NOFFT ..."  ->  abtest/libofdm_NAME.so
# (timing experiments only; the product is c-ofdm_amd/lib/libofdm_mi355x.so).
# abtest/ travels to the GPU box (git-ignored); delete it after an experiment.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
FLAGS="$*"
SRC=${SRC:-$R}  # source tree (e.g. an exported older commit)
B=$R/abtest/build_$NAME
mkdir -p $B $R/abtest
H="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -munsafe-fp-atomics -I$SRC/include $FLAGS"
# every device source of the tree being built (an older commit may have fewer)
pids=()
for f in $SRC/c-ofdm_amd/csrc/*.hip; do
  $H -c $f -o $B/$(basename $f .hip).o & pids+=($!)
done
# and every host source (ofdm_capi.cpp alone in older trees)
for f in $SRC/c-ofdm_amd/csrc/*.cpp; do
  $H -x hip -c $f -o $B/$(basename $f .cpp).o & pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o $R/abtest/libofdm_$NAME.so $B/*.o -ldl
rm -rf $B
echo built abtest/libofdm_$NAME.so
