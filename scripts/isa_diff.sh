#!/bin/bash
# Is the generated code of the kernels the same as at another revision?  (no GPU needed)
#   scripts/isa_diff.sh [-m MAP] [REV] [FILE.hip ...]   REV: default HEAD~1; files: default every file of build.py's HIP_SRC
# MAP: a file of `old-symbol new-symbol` lines (mangled names; # starts a comment) for kernels that a change renames, as
# dropping a template parameter does: REV's assembly has each old symbol replaced by the new one before the comparison.
# Exports REV's grtcode_amd/csrc and include, compiles each file of both trees device-only to assembly with build.py's
# HIPFLAGS and prints one line per function: file, name, instruction lines before and after, `same` or `DIFF`.  Labels and
# instructions are compared as text, comments stripped; `(descriptors)` stands for everything outside the function
# bodies -- kernel descriptors with their register counts, metadata, data.  The __hip_cuid_* symbol, a hash of the
# source text, is the one difference let through.  Exit status 1 if anything differs.
set -euo pipefail
map=
if [ "${1-}" = -m ]; then map=$(realpath "$2"); shift 2; fi     # (relative to the caller's directory)
cd "$(dirname "$0")/.."
rev=HEAD~1
if [ $# -gt 0 ] && [[ $1 != *.hip ]]; then rev=$1; shift; fi
root=$(pwd)
flags=$(python3 -c "from grtcode_amd.build import HIPFLAGS, ROOT; print(' '.join(f.replace(ROOT, '@ROOT@') for f in HIPFLAGS))")
if [ $# -gt 0 ]; then files=$(for f in "$@"; do basename "$f"; done)
else files=$(python3 -c "from grtcode_amd.build import HIP_SRC; print(' '.join(HIP_SRC))"); fi
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/old" "$tmp/new"
git archive "$rev" grtcode_amd/csrc include | tar -x -C "$tmp/old"
ln -s "$root/grtcode_amd" "$root/include" "$tmp/new/"

for f in $files; do
    for side in old new; do
        # (the compiler's warnings are the build's to show; here only a failure speaks)
        echo "hipcc ${flags//@ROOT@/$tmp/$side} --cuda-device-only -S $tmp/$side/grtcode_amd/csrc/hip/$f -o $tmp/$side/${f%.hip}.s 2>$tmp/$side/${f%.hip}.log || { cat $tmp/$side/${f%.hip}.log >&2; exit 255; }"
    done
done | xargs -P "${GRT_BUILD_JOBS:-4}" -I{} sh -c {}

# one file per function (labels and instructions), one for the rest
split() {
    mkdir -p "$2"
    sed -e 's/__hip_cuid_[0-9a-f]*/__hip_cuid_/g' -e 's/[ \t]*;.*$//' -e '/^[ \t]*$/d' "$1" | sed -f "$3" | awk -v dir="$2" '
        /^\t\.type\t.*,@function/ { name = $2; sub(/,@function$/, "", name); next }
        name != "" && $0 == name ":" { out = dir "/" name; print name > dir "/order"; next }
        /^\.Lfunc_end[0-9]+:/ { out = ""; name = ""; next }
        out != "" { print > out; next }
        { print > (dir "/(descriptors)") }'
}
count() { if [ -f "$1" ]; then grep -c -v -E '^(\.|[A-Za-z_])[^ \t]*:$|^[ \t]*\.' "$1" || true; else echo -; fi; }

# (the map as a sed script for the old side; mangled names are letters, digits and underscores)
: > "$tmp/none.sed"
: > "$tmp/map.sed"
if [ -n "$map" ]; then awk '!/^#/ && NF == 2 { print "s/\\<" $1 "\\>/" $2 "/g" }' "$map" > "$tmp/map.sed"; fi

status=0
for f in $files; do
    split "$tmp/old/${f%.hip}.s" "$tmp/old/${f%.hip}" "$tmp/map.sed"
    split "$tmp/new/${f%.hip}.s" "$tmp/new/${f%.hip}" "$tmp/none.sed"
    for name in $(cat "$tmp/old/${f%.hip}/order" "$tmp/new/${f%.hip}/order" | awk '!seen[$0]++') "(descriptors)"; do
        a="$tmp/old/${f%.hip}/$name"; b="$tmp/new/${f%.hip}/$name"
        if cmp -s "$a" "$b"; then verdict=same; else verdict=DIFF; status=1; fi
        if [ "$name" = "(descriptors)" ]; then
            printf '%-24s %-100s %19s %s\n' "$f" "$name" "" "$verdict"
        else
            printf '%-24s %-100s %9s %9s %s\n' "$f" "$(echo "$name" | c++filt -p)" "$(count "$a")" "$(count "$b")" "$verdict"
        fi
    done
done
exit $status
