#!/bin/bash
# Hash of the device assembly of every library source, to show that a host-side change left the kernels alone:
#   tools/device_code_hashes.sh [csrc directory] > after.txt     (and the same in a checkout of the commit before)
# Each csrc/*.hip is compiled for the device only with the Makefile's flags; the one thing that differs between two
# compilations of the same device code, the translation unit's __hip_cuid_<hash>, is masked before hashing.
set -euo pipefail
csrc=${1:-$(dirname "$0")/../bayesian-inference_amd/csrc}
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
cd "$csrc"
flags=$(make -pn | sed -n 's/^CXXFLAGS := //p')
for f in *.hip; do
  hipcc $flags --offload-device-only -S "$f" -o "$tmp/$f.s" 2>/dev/null &
done
wait
for f in *.hip; do
  printf '%-18s %s\n' "$f" "$(sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$tmp/$f.s" | sha256sum | cut -d' ' -f1)"
done
