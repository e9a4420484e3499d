#!/bin/sh
# A/B and mutation builds: build/exp/NAME/libvqcpc_hip.so = the current objects with ONE translation unit recompiled.
# usage: tools/build_variant.sh NAME "-DXD_GSPLIT=8 ..." [UNIT [SOURCE]]
#   UNIT    the translation unit to recompile, without .hip (default ar_xcd: the A/B builds of the per-XCD decoder)
#   SOURCE  the file to compile in its place (default csrc/UNIT.hip), e.g. a copy with one line changed, to show that a test
#           file notices the fault; such copies and libraries live under build/ and are never committed
# then: python tools/ab_libs.py build/exp/A/libvqcpc_hip.so build/exp/B/libvqcpc_hip.so
# Build the library first (make -C vectorquantizedcpc_amd/csrc): the other units are linked from its objects (the Makefile's OBJS).
set -e
cd "$(dirname "$0")/.."
C=vectorquantizedcpc_amd/csrc
U=${3:-ar_xcd}
SRC=${4:-$C/$U.hip}
mkdir -p build/exp/$1
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -I$C $2 -c $SRC -o build/exp/$1/$U.o
OBJS=
for o in $(sed -n 's/^OBJS *= *//p' $C/Makefile | sed 's/\.o//g'); do
    if [ $o = $U ]; then OBJS="$OBJS build/exp/$1/$U.o"; else OBJS="$OBJS $C/$o.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/exp/$1/libvqcpc_hip.so $OBJS
