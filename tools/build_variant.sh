#!/bin/sh
# A/B builds of the per-XCD decoder: build/exp/NAME/libvqcpc_hip.so = the current objects with ar_xcd.hip recompiled with extra defines.
# usage: tools/build_variant.sh NAME "-DXD_GSPLIT=8 ..."   (then: python tools/ab_libs.py build/exp/A/libvqcpc_hip.so build/exp/B/libvqcpc_hip.so)
set -e
cd "$(dirname "$0")/.."
C=vectorquantizedcpc_amd/csrc
mkdir -p build/exp/$1
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off $2 -c $C/ar_xcd.hip -o build/exp/$1/ar_xcd.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/exp/$1/libvqcpc_hip.so $C/runtime.o $C/gemm_chain.o $C/encoder.o $C/encoder_host.o $C/codebook.o $C/vocoder.o $C/vocoder_host.o $C/vocoder_plan.o $C/vocoder_stream.o $C/nll.o $C/scan.o build/exp/$1/ar_xcd.o $C/ar_xcm.o $C/melfront.o $C/loudness.o $C/resample.o $C/cpc.o $C/cpc_grad.o $C/abx.o $C/gate_probe.o
