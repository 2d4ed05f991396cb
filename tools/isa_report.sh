#!/bin/bash
# Registers, scratch, LDS and occupancy of every kernel of every translation unit as compiled for gfx950 (no GPU needed):
# tools/isa_report.sh > profiles/rNN/isa_resources.txt
# Extra arguments go to hipcc (e.g. -DCHROMA_HYBRID_RENDER=0).
set -e
here=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d)
# (one assembly file per translation unit that holds kernels, compiled side by side; bvh_device.hip and wide_device.hip, the
#  tree builders, were never part of this table)
for unit in chroma_hip geometry kernel_calls daq_calls steps_calls seed_calls dirseed_calls comm; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math \
    -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero -Wno-unused-value -Wno-unused-result \
    "$@" -S --cuda-device-only -o $tmp/$unit.s $here/chroma_amd/csrc/$unit.hip 2>/dev/null &
done
wait
for unit in chroma_hip geometry kernel_calls daq_calls steps_calls seed_calls dirseed_calls comm; do test -s $tmp/$unit.s; done
echo "# kernel, VGPRs, SGPRs, scratch bytes, LDS bytes, waves/SIMD, code bytes   (hipcc -O3, gfx950; flags of chroma_amd/csrc/Makefile)"
awk '
/^[_A-Za-z0-9]+:.*; @/ { name=$1; sub(":","",name) }
/; codeLenInByte/ { code=$4 }
/; TotalNumSgprs:/ { s=$3 }
/; NumVgprs:/ { v=$3 }
/; ScratchSize:/ { sc=$3 }
/; LDSByteSize:/ { l=$3 }
/; Occupancy:/ { printf "%s, %s, %s, %s, %s, %s, %s\n", name, v, s, sc, l, $3, code }
' $tmp/*.s | while IFS= read -r line; do n=${line%%,*}; d=$(echo "$n" | c++filt | sed 's/(.*//'); echo "$d,${line#*,}"; done | sort
rm -rf $tmp
