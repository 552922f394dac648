#!/bin/bash
# usage: tools/build_variant.sh <name> [extra hipcc flags...]   -> build/exp/lib<name>.so
# Developer A/B builds of the same library (loaded through FLATE_HIP_LIB); never shipped.
# The sources are build.py's SOURCES: one list for the product library and its variants.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
C=moonbit-flate_amd/csrc
srcs=$(python3 -c "import sys; sys.path.insert(0, 'moonbit-flate_amd'); import build; print(' '.join('$C/' + s for s in build.SOURCES))")
mkdir -p build/exp
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared -Iinclude -I$C "$@" \
  $srcs -o build/exp/lib$name.so -lpthread -ldl
echo build/exp/lib$name.so
