#!/bin/bash
# Build libfmcw.so and one library per build-time alternative of the device tracker's kernel
# (csrc/tws_dev_kernel.hpp: FMCW_TWS_WAVEMIN, FMCW_TWS_WAVES, FMCW_TWS_PREFETCH), for measurement:
#   lib/libfmcw_tws_walk.so        intended-mode association by a scalar walk of the candidate ballot
#   lib/libfmcw_tws_waves4.so      four waves (streams) per workgroup
#   lib/libfmcw_tws_noprefetch.so  a scan's records loaded when the scan begins
# Then, on an MI355X:  FMCW_LIB=$PWD/fpga-fmcw-radar-processor_amd/lib/libfmcw_tws_walk.so python tools/tws_dev_bench.py
set -euo pipefail
cd "$(dirname "$0")/../fpga-fmcw-radar-processor_amd"
make -j"${JOBS:-8}"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -fvisibility=hidden -Wall -Wno-unused-result -Wno-unused-value"
OTHERS=$(ls build/*.o | grep -v 'fmcw_tws_dev')
for v in "walk:-DFMCW_TWS_WAVEMIN=0" "waves4:-DFMCW_TWS_WAVES=4" "noprefetch:-DFMCW_TWS_PREFETCH=0"; do
  name=${v%%:*}
  $HIPCC $FLAGS ${v#*:} -c -o build/fmcw_tws_dev_$name.o csrc/fmcw_tws_dev.hip
  $HIPCC $FLAGS -shared -o lib/libfmcw_tws_$name.so $OTHERS build/fmcw_tws_dev_$name.o -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
  rm -f lib/libfmcw_tws_$name.so.[0-9]*
  echo "built lib/libfmcw_tws_$name.so"
done
