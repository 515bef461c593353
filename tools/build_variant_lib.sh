#!/bin/bash
# A/B variant of the library: bash tools/build_variant_lib.sh <name> <-Dflags...>
#   e.g. tools/build_variant_lib.sh nomfma -DPCS_ABLATE5=2
# -> openpcseg_amd/lib/dbg/<name>.so: every conv*.hip recompiled with the flags (conv_common.h switches reach the launch
# shape code too), the other objects of the product build linked as they are; select it with PCS_LIB_PATH.
# Variant builds are never loaded by default and are removed before a round ends (they must not travel as product).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
python -m openpcseg_amd.build > /dev/null
mkdir -p $ROOT/openpcseg_amd/lib/dbg /tmp/pcsvar_$name
rm -f /tmp/pcsvar_$name/*.o
# compile lines = openpcseg_amd/build.py: FLAGS + the file's EXTRA_FLAGS
flags() { python -c "import sys; from openpcseg_amd import build as b; print(' '.join([b.HIPCC] + b.FLAGS + b.EXTRA_FLAGS.get(sys.argv[1], [])))" $1; }
cd $ROOT
for f in $ROOT/openpcseg_amd/csrc/conv*.hip; do
  $(flags $(basename $f)) "$@" -c $f -o /tmp/pcsvar_$name/$(basename $f).o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC /tmp/pcsvar_$name/*.o \
  $(ls $ROOT/openpcseg_amd/lib/*.hip.o | grep -v "/conv") -o $ROOT/openpcseg_amd/lib/dbg/$name.so
echo $ROOT/openpcseg_amd/lib/dbg/$name.so
