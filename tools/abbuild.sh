#!/bin/bash
# A/B builds (diagnostic): tools/abbuild.sh <name> [-DMACRO=...]...
# builds cndp_amd/lib/libcndp_gpu_<name>.so from the same sources with extra
# defines; select it at run time with CNDP_GPU_LIB=<path>.
set -e
cd "$(dirname "$0")/.."
name=$1
shift
obj=cndp_amd/build/ab_$name
mkdir -p "$obj"
objs=""
for f in rib fib fib_near node pcb fwd tx tcb tcpout; do
    gcc -O3 -fPIC -std=gnu11 -c cndp_amd/csrc/$f.c -o "$obj/$f.o"
    objs="$objs $obj/$f.o"
done
# the other device modules take no A/B defines: the default build's objects
devs=$(ls cndp_amd/build/cndp_l4.o cndp_amd/build/cndp_tcp.o cndp_amd/build/cndp_tcb.o cndp_amd/build/cndp_fwd.o cndp_amd/build/cndp_tx.o)
/opt/rocm/bin/hipcc -O3 -fPIC -std=c++17 --offload-arch=gfx950 -w "$@" -c cndp_amd/csrc/cndp_gpu.hip -o "$obj/cndp_gpu.o"
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -Wl,--version-script=cndp_amd/csrc/exports.map \
    -o "cndp_amd/lib/libcndp_gpu_$name.so" $objs "$obj/cndp_gpu.o" $devs -lpthread
echo "built cndp_amd/lib/libcndp_gpu_$name.so"
