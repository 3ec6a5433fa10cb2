#!/bin/bash
# AddressSanitizer pass over the HOST code (CPU only; GPU ASan is not available on the pool): the .cpp sources of
# the product library (C ABI, host builders) and the oracle are rebuilt with -fsanitize=address and the
# CPU test suite runs against them.  Usage: tools/asan_cpu.sh [pytest args]; outputs under /tmp/nnbvh_asan.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=/tmp/nnbvh_asan
LLVM=/opt/rocm/lib/llvm
RT=$(ls $LLVM/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so | head -1)
mkdir -p $OUT
cd $ROOT
python -c "from nn_bvh_amd import build; build.build()" >/dev/null
SAN="-fsanitize=address -shared-libasan -fno-omit-frame-pointer -g"
# the host sources are the .cpp entries of the build's own list; the device objects come from the product build
HOST=$(python -c "from nn_bvh_amd import build; print(' '.join(s[:-4] for s in build.SOURCES if s.endswith('.cpp')))")
objs=""
for f in $HOST; do
  /opt/rocm/bin/hipcc -O1 $SAN -ffp-contract=off -fPIC -std=c++17 -I$ROOT/include -c $ROOT/nn_bvh_amd/csrc/$f.cpp -o $OUT/$f.o
  objs="$objs $OUT/$f.o"
done
for o in $ROOT/nn_bvh_amd/_obj/product/*.o; do
  case " $HOST " in *" $(basename $o .o) "*) ;; *) objs="$objs $o";; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $SAN -o $ROOT/nn_bvh_amd/libnnbvh_hip_asan.so $objs
$LLVM/bin/clang -O1 $SAN -std=gnu11 -fPIC -ffp-contract=off -mfma -shared -o $OUT/libnnbvh_oracle_asan.so $ROOT/oracle/nnbvh_oracle.c -lm -lpthread
LD_PRELOAD=$RT ASAN_OPTIONS=detect_leaks=0:abort_on_error=1:symbolize=1 ASAN_SYMBOLIZER_PATH=$LLVM/bin/llvm-symbolizer \
  NNBVH_LIB=libnnbvh_hip_asan.so NNBVH_ORACLE_LIB=$OUT/libnnbvh_oracle_asan.so \
  python -m pytest tests -x -q -m "not gpu" -p no:cacheprovider "$@"
rm -f $ROOT/nn_bvh_amd/libnnbvh_hip_asan.so
