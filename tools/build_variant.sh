#!/bin/bash
# development: build libvechat_hip.so with extra -D flags into vechat_amd/lib/variants/ for A/B runs on the GPU box
#   tools/build_variant.sh NAME [-DVC_TILE=1 ...];  run with VECHAT_HIP_LIB=vechat_amd/lib/variants/libvechat_hip_NAME.so
#   VC_PLAIN_CFG=1 tools/build_variant.sh plain     the library WITHOUT -structurizecfg-skip-uniform-regions (tools/gpu_flag_parity.sh)
# The flags are build()'s (__graft_entry__.py): only vc_api.hip takes the structurizecfg option, vc_align.hip and vc_large.hip are plain.
# In a checkout of another commit (git worktree) it builds that commit's library: tools/gpu_poa_rate.py --graph --parent-lib.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p vechat_amd/lib/variants
obj=$(mktemp -d)
trap 'rm -rf "$obj"' EXIT
FAST="-mllvm -structurizecfg-skip-uniform-regions"
[ "$VC_PLAIN_CFG" = "1" ] && FAST=""
CC="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -I include"
$CC $FAST "$@" -c vechat_amd/csrc/vc_api.hip -o "$obj/vc_api.o" &
$CC "$@" -c vechat_amd/csrc/vc_align.hip -o "$obj/vc_align.o"
$CC "$@" -c vechat_amd/csrc/vc_large.hip -o "$obj/vc_large.o"
wait %1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I include "$obj/vc_api.o" "$obj/vc_align.o" "$obj/vc_large.o" \
  vechat_amd/csrc/vc_host.cpp vechat_amd/csrc/vc_windows.cpp vechat_amd/csrc/vc_io.cpp \
  -lpthread -lz -o vechat_amd/lib/variants/libvechat_hip_$name.so
echo built $name
