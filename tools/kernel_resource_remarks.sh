#!/bin/bash
# The compiler's resource-usage remarks of every kernel in one translation unit, without the
# source positions (they move with every edit), to diff two commits' kernels:
#   tools/kernel_resource_remarks.sh csrc/heartbeat.hip > after.txt    (from go-libp2p-pubsub_amd/)
set -euo pipefail
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
o=$(mktemp --suffix=.o)
trap 'rm -f "$o"' EXIT
"$HIPCC" --offload-arch="${ARCH:-gfx950}" -O3 -std=c++17 -fPIC -ffp-contract=off -I../include -Icsrc \
    -Rpass-analysis=kernel-resource-usage -c "$1" -o "$o" 2>&1 |
    grep "remark:" | sed -E 's/^[^ ]+: remark: //; s/ \[-Rpass-analysis=kernel-resource-usage\]//'
