#!/bin/bash
# Fast register/ISA check of the stencil unit of one degree:
#   tools/kstat.sh [P] [extra hipcc flags]   -> /tmp/kstat.s + resource usage
P=${1:-5}; shift
SRC=$(cd "$(dirname "$0")/../dealii-galerkin-difference-methods_amd/csrc" && pwd)/gdm_stencil.hip
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -Wno-unused-function --cuda-device-only -S \
  -DGDM_PART=$P "$@" $SRC -o /tmp/kstat.s -Rpass-analysis=kernel-resource-usage 2>&1 |
  grep -E "error|Function Name|VGPRs:|SGPRs:|Spill|Occupancy" | grep -A6 "stencil8" | sed 's/.*remark: //'
