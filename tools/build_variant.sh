#!/bin/bash
# tools/build_variant.sh NAME "<extra hipcc flags>"  ->  build_variants/libhrcore_NAME.so  (A/B experiments; load with HRCORE_LIB)
# The units and the flags are the Makefile's (SRCS, print-flags); the objects go to a directory of their own.
set -e
name="$1"; extra="$2"
root="$(cd "$(dirname "$0")/.." && pwd)"
csrc="$root/heatray_amd/csrc"
tmp="$(mktemp -d)"; mkdir -p "$root/build_variants"
FLAGS="$(make -s -C "$csrc" print-flags EXTRA="$extra")"
srcs="$(sed -n 's/^SRCS := //p' "$csrc/Makefile")"
cd "$csrc"
pids=""
for f in $srcs; do
  /opt/rocm/bin/hipcc $FLAGS -c "$f" -o "$tmp/${f%.hip}.o" & pids="$pids $!"
done
for p in $pids; do wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$root/build_variants/libhrcore_$name.so" "$tmp"/*.o
rm -rf "$tmp"; echo "built build_variants/libhrcore_$name.so"
