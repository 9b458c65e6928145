#!/bin/bash
# instrumented build (cycle sections printed by block 1 of the index sort, the index match, the index parse, the emit and the entropy decode kernels)
cd "$(dirname "$0")/.." && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -fvisibility=hidden -DSQZ_STATS -Iinclude \
  -o sqz_amd/lib/libsqz_amd_stats.so sqz_amd/csrc/*.hip
