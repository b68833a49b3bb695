#!/usr/bin/env bash
# device_asm_diff.sh — is the gfx950 device code of the row, merge and slice (multi-vector, SDDMM) kinds the same in two
# source trees?
#
#   scripts/device_asm_diff.sh emit <csrc dir> <out dir>     one <unit>.s per translation unit, with the Makefile's flags
#   scripts/device_asm_diff.sh diff <out dir A> <out dir B>  compares them, one line per unit; exit 1 if any differs
#
# A refactor of xwindow.hpp / row_launch.hpp / slice_cut.hpp or of a file that includes them is checked this way instead
# of being timed: `emit` on a checkout of the parent and on the working tree, then `diff`.  Comments, .file / .loc /
# .ident lines and debug sections are dropped before the comparison, and the compilation unit's id (a hash of its path)
# is blanked.  UNITS="a b" in the environment limits both commands to those units.
set -euo pipefail

UNITS=${UNITS:-"csr_vector csr_vector_f64 csr_vector_h16 light_rows light_rows_f64 merge_path_f32 merge_path_f64 merge_path_i32 merge_path_pattern rows_plan multi_f32 multi_f64 multi_i32 multi_h16 sddmm multi_perm_f32 multi_perm_f64 multi_perm attention attention_bwd"}
unit_flags() {  # what the Makefile adds for one unit
    case "$1" in multi_*) echo -DMI355_MULTI_SPLIT_UNITS ;; esac
}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
HIPFLAGS=${HIPFLAGS:--O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function}
JOBS=${JOBS:-4}

strip_asm() {   # comments, file / line records, debug sections, blank lines; the unit id is a hash of the file's path
    sed -e 's/[[:space:]]*;.*$//' -e 's/__hip_cuid_[0-9a-f]*/__hip_cuid/g' -e '/^[[:space:]]*\.\(file\|loc\|ident\)[[:space:]]/d' "$1" |
        awk '/^[[:space:]]*\.section[[:space:]]+\.debug/ { skip = 1; next }
             /^[[:space:]]*\.(section|text|data|rodata|amdgpu_metadata)/ { skip = 0 }
             !skip && NF'
}

case "${1:-}" in
emit)
    src=$(cd "$2" && pwd)
    mkdir -p "$3"
    out=$(cd "$3" && pwd)
    cd "$src"
    # shellcheck disable=SC2086
    for u in $UNITS; do echo "$(unit_flags "$u") --cuda-device-only -S $u.hip -o $out/$u.s"; done |
        xargs -P "$JOBS" -L1 $HIPCC $HIPFLAGS
    ;;
diff)
    status=0
    for u in $UNITS; do
        if cmp -s <(strip_asm "$2/$u.s") <(strip_asm "$3/$u.s"); then
            echo "$u: identical ($(strip_asm "$2/$u.s" | wc -l) lines)"
        else
            echo "$u: DIFFERS ($(diff <(strip_asm "$2/$u.s") <(strip_asm "$3/$u.s") | grep -c '^[<>]' || true) diff lines)"
            status=1
        fi
    done
    exit $status
    ;;
*)
    sed -n '2,11p' "$0"
    exit 2
    ;;
esac
