#!/bin/bash
# The memory instructions and vmcnt waits of one kernel, in emitted order, with the
# labels and branches between them: how many dependent round trips a path takes.
#   tools/kernel_mem_listing.sh csrc/deliver.hip _ZN4gsim9k_send_tmILi512ELb0ELb0ELb0ELb0EEEvNS_9RoundArgsE
# (from go-libp2p-pubsub_amd/; extra arguments go to the compiler, e.g. -DGSIM_TM_P=4)
set -euo pipefail
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
src=$1; kern=$2; shift 2
s=$(mktemp --suffix=.s)
trap 'rm -f "$s"' EXIT
"$HIPCC" --offload-arch="${ARCH:-gfx950}" -O3 -std=c++17 -fPIC -ffp-contract=off -I../include -Icsrc \
    -S --cuda-device-only "$@" "$src" -o "$s" 2>/dev/null
awk -v k="$kern" '
    $0 ~ "^" k ":" { on = 1 }
    on && /^\.Lfunc_end/ { exit }
    on && (/^\.LBB/ || /global_(load|atomic|store)/ || /scratch_(load|store)/ || /s_waitcnt.*vmcnt/ ||
           /s_cbranch|s_branch/ || /s_barrier/) { sub(/^[ \t]+/, "  "); sub(/[ \t]*;.*$/, ""); print }
' "$s"
