#!/bin/bash
# Are the EMA = false instantiations of adam_kernel / sgd_momentum_kernel the instructions of an older tree?  No GPU needed.
#   scripts/isa_diff_optim.sh <older tree>      (a checkout of the commit before the EMA flag: kernels templated on CLIP alone)
# Cross-compiles pp_optim.hip of both trees for gfx950 to assembly, cuts the four kernels out, drops comments and replaces
# mangled names and basic-block / function numbers, and diffs.  Prints one line per kernel; exit status 1 on any difference.
set -o pipefail
HERE=$(cd "$(dirname "$0")/.." && pwd)
OLD=${1:?usage: scripts/isa_diff_optim.sh <older tree>}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
for t in old new; do
  dir=$OLD; [ $t = new ] && dir=$HERE
  ${HIPCC:-hipcc} --offload-arch=${ARCH:-gfx950} -O3 -fPIC -std=c++17 -I"$dir/include" -I"$dir/pacingpseudo_amd/csrc" --cuda-device-only -S \
    "$dir/pacingpseudo_amd/csrc/pp_optim.hip" -o "$TMP/$t.s" 2>/dev/null || { echo "compiling $dir failed"; exit 2; }
done
body() {  # file, start of the mangled name
  awk -v k="$2" 'index($0, k) == 1 && /:/ {on = 1} on {print} on && /^\.Lfunc_end/ {on = 0}' "$1" |
    sed -E 's/;.*//; s/_Z[A-Za-z0-9_]+/SYM/g; s/BB[0-9]+_/BB_/g; s/func_end[0-9]+/func_end/; s/[ \t]+$//'
}
rc=0
for pair in "_Z11adam_kernelILb0EE _Z11adam_kernelILb0ELb0EJEE" "_Z11adam_kernelILb1EE _Z11adam_kernelILb1ELb0EJEE" \
            "_Z19sgd_momentum_kernelILb0EE _Z19sgd_momentum_kernelILb0ELb0EJEE" "_Z19sgd_momentum_kernelILb1EE _Z19sgd_momentum_kernelILb1ELb0EJEE"; do
  set -- $pair
  body "$TMP/old.s" "$1" > "$TMP/a"; body "$TMP/new.s" "$2" > "$TMP/b"
  n=$(wc -l < "$TMP/a")
  if [ "$n" -gt 50 ] && diff "$TMP/a" "$TMP/b" > "$TMP/d"; then echo "$1 -> $2: $n lines, identical"
  else echo "$1 -> $2: DIFFERENT ($n lines in the older kernel)"; head -20 "$TMP/d"; rc=1; fi
done
exit $rc
