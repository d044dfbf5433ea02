#!/bin/sh
# Builds the library's sources with AddressSanitizer + UBSan on the HOST side only (the device code is compiled as always) together with
# arg_checks.cpp into ONE stand-alone program and runs it: the host-side argument checks and index arithmetic of the C ABI under the
# sanitizers, on a machine without a GPU. Nothing here is loaded into Python and nothing runs on a device.
#   sh tools/host_asan/run.sh        (objects and the program go to build/host_asan/, which git ignores)
set -eu
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT="$ROOT/build/host_asan"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
mkdir -p "$OUT"
ls "$ROOT"/f3d-gaus_amd/csrc/*.hip | xargs -P 4 -I{} sh -c \
    "$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-gpu-rdc $SAN -c {} -o $OUT/\$(basename {} .hip).o"
$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -fno-gpu-rdc $SAN -I"$ROOT/include" -x hip "$ROOT/tools/host_asan/arg_checks.cpp" -c -o "$OUT/arg_checks.o"
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined "$OUT"/*.o -o "$OUT/arg_checks"
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/arg_checks"
