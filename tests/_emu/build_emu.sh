#!/bin/sh
# TEST-ONLY: builds the fibre-emulated copy of libzkhip (same kernel sources, g++, -DZK_EMU) so that
# kernel indexing / LDS / barrier logic runs under `pytest -m "not gpu"`.  Never shipped, never a fallback.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
SRC="$HERE/../../zokrates_amd/csrc"
FLAGS="-U_FORTIFY_SOURCE -O2 -g -std=c++17 -fPIC -DZK_EMU ${EMU_FLAGS:-} -x c++ -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-unused-variable -Wno-restrict"
mkdir -p "$HERE/obj"
# One build at a time: the suite's worker processes each find a stale library and come here together; unserialised they wrote the same
# object files and relinked the library under each other's link steps (undefined references in the executable's link, now and then).
# The results are moved into place whole, so a process that links or loads the old ones meanwhile never sees half a file.
# (without the flock program the build runs as it always did, unserialised)
exec 9>"$HERE/.build.lock"
if command -v flock >/dev/null 2>&1; then flock 9; fi
# every unit's own exit status: a bare `wait` answers 0 whatever the compilers did, and an object of an earlier build would be linked
pids=""
for f in curve_bn254 curve_bls381 bn254_g1 bn254_g2 bls381_g1 bls381_g2 zkhip_api ingest; do
  rm -f "$HERE/obj/$f.o"
  g++ $FLAGS -c "$SRC/$f.hip" -o "$HERE/obj/$f.o" &
  pids="$pids $!"
done
failed=0
for p in $pids; do wait "$p" || failed=1; done
if [ "$failed" != 0 ]; then echo "build_emu.sh: a translation unit did not compile" >&2; exit 1; fi
g++ -shared -o "$HERE/libzkhip_emu.so.tmp" "$HERE"/obj/*.o
mv -f "$HERE/libzkhip_emu.so.tmp" "$HERE/libzkhip_emu.so"
# the compiled host side (csrc/host) against the emulator library: the same executable the product ships, for CPU tests
g++ -O2 -std=c++17 -Wall -pthread "$SRC/host/backend.cpp" "$SRC/host/verify.cpp" "$SRC/host/cli_main.cpp" -L"$HERE" -lzkhip_emu -Wl,-rpath,'$ORIGIN' -o "$HERE/zkhip-cli-emu.tmp"
mv -f "$HERE/zkhip-cli-emu.tmp" "$HERE/zkhip-cli-emu"
