#!/bin/bash
# Is the generated code of the kernels the same as at another revision?  (no GPU needed)
#   scripts/isa_diff.sh [-u] [-m MAP] [REV] [FILE.hip ...]   REV: default HEAD~1; files: default every file of build.py's HIP_SRC
# MAP: a file of `old-symbol new-symbol` lines (mangled names; # starts a comment) for kernels that a change renames, as
# dropping a template parameter does: REV's assembly has each old symbol replaced by the new one before the comparison.
# Exports REV's grtcode_amd/csrc and include, compiles each file of both trees device-only to assembly with build.py's
# HIPFLAGS and prints one line per function: file, name, instruction lines before and after, `same` or `DIFF`.  Labels and
# instructions are compared as text, comments stripped; `(descriptors)` stands for everything outside the function
# bodies -- kernel descriptors with their register counts, metadata, data.  The __hip_cuid_* symbol, a hash of the
# source text, is the one difference let through.  Exit status 1 if anything differs.
# -u: compare independently of the order of the functions in the file, which follows the order in which the host code names
# the instances of a template.  The compiler numbers a function's block labels (.LBB<n>_<m>) and its end label by the
# function's place in the file; -u drops that index, and takes out of `(descriptors)`, under the function's name, what
# belongs to one function: `(descriptor)` -- its section, linkage and size directives, its resource symbols and its
# .amdhsa_kernel ... .end_amdhsa_kernel block -- and `(metadata)`, its entry under amdhsa.kernels.  A symbol that one side
# alone has is a DIFF as without -u, and what remains of `(descriptors)` is compared in place.  So a change that only
# moves launch sites shows `same` throughout, and no source file has to be arranged around the listing's label numbers.
set -euo pipefail
map=
unordered=0
while [ "${1-}" = -m ] || [ "${1-}" = -u ]; do
    if [ "$1" = -u ]; then unordered=1; shift; else map=$(realpath "$2"); shift 2; fi     # (relative to the caller's directory)
done
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

# one file per function (labels and instructions), one for the rest; -u: two more per function, NAME.kd and NAME.meta
split() {
    mkdir -p "$2"
    sed -e 's/__hip_cuid_[0-9a-f]*/__hip_cuid_/g' -e 's/[ \t]*;.*$//' -e '/^[ \t]*$/d' "$1" | sed -f "$3" |
    if [ $unordered = 1 ]; then sed -E 's/\.(LBB|LJTI|LCPI|Lfunc_begin|Lfunc_end)[0-9]+/.\1/g'; else cat; fi | awk -v dir="$2" -v u=$unordered '
        function flush(dest,   i) { for (i = 0; i < nbuf; i++) print buf[i] > dest; nbuf = 0 }
        function flush_entry(   i, dest) {
            dest = ename != "" ? dir "/" ename ".meta" : rest
            for (i = 0; i < nent; i++) print ent[i] > dest
            nent = 0; ename = ""
        }
        BEGIN { rest = dir "/(descriptors)" }
        /^\t\.type\t.*,@function/ {
            name = $2; sub(/,@function$/, "", name)
            if (u) { kd = dir "/" name ".kd"; flush(kd); print > kd; tail = "" }
            next
        }
        name != "" && $0 == name ":" { out = dir "/" name; print name > dir "/order"; next }
        /^\.Lfunc_end[0-9]*:/ { out = ""; name = ""; if (u) tail = kd; next }
        # (inside a body: the kernel descriptor, from its .rodata section back to the text)
        out != "" && u && /^\t\.section\t\.rodata/ { inkd = 1 }
        out != "" && inkd { print > kd; if (/^\t\.section\t\.text/) inkd = 0; next }
        out != "" { print > out; next }
        # (between the bodies: what follows a function is its own up to the next section, and a section with its linkage
        # directives belongs to the function whose .type line comes next)
        u && /^\t\.section\t/ && !/\.AMDGPU\.csdata/ { flush(rest); tail = ""; buf[nbuf++] = $0; next }
        u && nbuf > 0 && /^\t\.(globl|weak|protected|hidden|p2align)/ { buf[nbuf++] = $0; next }
        u && nbuf > 0 { flush(rest) }
        u && tail != "" { print > tail; next }
        # (the metadata: one entry per kernel, named by its .name line)
        u && /^amdhsa\.kernels:/ { meta = 1; print > rest; next }
        meta && /^[^ ]/ { flush_entry(); meta = 0 }
        meta && /^  - / { flush_entry() }
        meta { if ($1 == ".name:") ename = $2; ent[nent++] = $0; next }
        { print > rest }
        END { flush(rest) }'
}
count() { if [ -f "$1" ]; then grep -c -v -E '^(\.|[A-Za-z_])[^ \t]*:$|^[ \t]*\.' "$1" || true; else echo -; fi; }

# (the map as a sed script for the old side; mangled names are letters, digits and underscores)
: > "$tmp/none.sed"
: > "$tmp/map.sed"
if [ -n "$map" ]; then awk '!/^#/ && NF == 2 { print "s/\\<" $1 "\\>/" $2 "/g" }' "$map" > "$tmp/map.sed"; fi

status=0
line() {    # file, label, old, new
    if cmp -s "$3" "$4"; then verdict=same; else verdict=DIFF; status=1; fi
    printf '%-24s %-100s %9s %9s %s\n' "$1" "$2" "$(count "$3")" "$(count "$4")" "$verdict"
}
for f in $files; do
    split "$tmp/old/${f%.hip}.s" "$tmp/old/${f%.hip}" "$tmp/map.sed"
    split "$tmp/new/${f%.hip}.s" "$tmp/new/${f%.hip}" "$tmp/none.sed"
    for name in $(cat "$tmp/old/${f%.hip}/order" "$tmp/new/${f%.hip}/order" | awk '!seen[$0]++'); do
        a="$tmp/old/${f%.hip}/$name"; b="$tmp/new/${f%.hip}/$name"
        line "$f" "$(echo "$name" | c++filt -p)" "$a" "$b"
        for part in kd:descriptor meta:metadata; do
            if [ -f "$a.${part%:*}" ] || [ -f "$b.${part%:*}" ]; then
                line "$f" "$(echo "$name" | c++filt -p) (${part#*:})" "$a.${part%:*}" "$b.${part%:*}"
            fi
        done
    done
    if cmp -s "$tmp/old/${f%.hip}/(descriptors)" "$tmp/new/${f%.hip}/(descriptors)"; then verdict=same; else verdict=DIFF; status=1; fi
    printf '%-24s %-100s %19s %s\n' "$f" "(descriptors)" "" "$verdict"
done
exit $status
