#!/bin/bash
# A/B library builds of the tile kernel's r layout and of the fused field write, for scripts/ab_so.sh:
# lib/libnngp_both.so (the default build), lib/libnngp_p1.so (chain-major r, epilogue kernel kept:
# capi.hip with -DNNGP_NO_FUSED_FIELD), lib/libnngp_p2.so (fused field write, interleaved r:
# tiles.hip with -DNNGP_TILE_R_INTERLEAVED).  A parent build goes to lib/libnngp_parent.so by hand.
cd "$(dirname "$0")/../improving-performances-of-mcmc-for-nearest-neighbor-gaussian-process-models-with-full-data-augmentat_amd/csrc" || exit 1
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-pass-failed -Wno-unused-value -Wno-unused-result"
L="-L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib"
make -j4 || exit 1
/opt/rocm/bin/hipcc $F -DNNGP_NO_FUSED_FIELD -c capi.hip -o build/capi_nofuse.o &
/opt/rocm/bin/hipcc $F -DNNGP_TILE_R_INTERLEAVED -c tiles.hip -o build/tiles_il.o &
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../lib/libnngp_p1.so build/graph_prep.o build/kernels.o build/tiles.o build/capi_nofuse.o $L &&
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../lib/libnngp_p2.so build/graph_prep.o build/kernels.o build/tiles_il.o build/capi.o $L &&
cp ../../lib/libnngp.so ../../lib/libnngp_both.so
