#!/bin/bash
# Did a change touch device code?  The compiler's account of every kernel (tools/resource_usage.py) and the device assembly of the named
# units, of a commit and of the working tree, compared with diff.  No GPU needed.  From the repository's root:
#
#     tools/listing_diff.sh <commit> <unit> ... > profiles/<name>_listing_diff.txt      e.g.  tools/listing_diff.sh HEAD~1 cov sdust bgrun
#
# A unit is csrc/<unit>.hip, built with the flags of cornetto_amd/Makefile.  Every unit's assembly names a symbol __hip_cuid_<hash of the
# source text>: a hunk that only renames it is left out (diff -I).  Under every diff its exit status: 0 = nothing else differs.
set -u
[ $# -ge 1 ] || { echo "usage: tools/listing_diff.sh <commit> [unit ...]" >&2; exit 2; }
commit=$1
shift
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -Wno-inline-asm -ffp-contract=off"
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir -p "$tmp/a/tree" "$tmp/b"
git archive "$commit" | tar -x -C "$tmp/a/tree" || exit 1

echo "\$ diff <(python tools/resource_usage.py <tree of $(git rev-parse --short "$commit")>) <(python tools/resource_usage.py)"
python tools/resource_usage.py "$tmp/a/tree" > "$tmp/a/usage.txt"
python tools/resource_usage.py > "$tmp/b/usage.txt"
diff "$tmp/a/usage.txt" "$tmp/b/usage.txt"
echo "(exit status $?; $(($(wc -l < "$tmp/b/usage.txt") - 1)) kernels)"

for u in "$@"; do
    (cd "$tmp/a/tree/cornetto_amd" && $HIPCC $FLAGS --cuda-device-only -S "csrc/$u.hip" -o "$tmp/a/$u.s") 2> /dev/null &
    (cd cornetto_amd && $HIPCC $FLAGS --cuda-device-only -S "csrc/$u.hip" -o "$tmp/b/$u.s") 2> /dev/null &
done
wait
for u in "$@"; do
    echo
    echo "\$ diff -I __hip_cuid_ <($HIPCC $FLAGS --cuda-device-only -S csrc/$u.hip -o -, tree of $(git rev-parse --short "$commit")) <(the same here)"
    [ -s "$tmp/a/$u.s" ] && [ -s "$tmp/b/$u.s" ] || { echo "(csrc/$u.hip did not compile in one of the trees)"; continue; }
    diff -I __hip_cuid_ "$tmp/a/$u.s" "$tmp/b/$u.s"
    echo "(exit status $?; $(wc -l < "$tmp/b/$u.s") lines)"
done
