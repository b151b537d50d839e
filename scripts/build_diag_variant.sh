#!/bin/bash
# Diagnostic library variant: some translation units recompiled with extra defines, linked with
# the default objects of every other unit (build/obj). Same flags as quad-periodic-mpc_amd/build.py.
# A unit is named by its source, or where one source has several units (build.py's UNITS: the builds
# of the wide template, the per-instance hooks) by its object's name in build/obj without the .o,
# e.g. cmpc_wide_unit.hip_CMPC_UNIT_WIDE-96,1,1,0; the unit's own defines are kept.
# usage: build_diag_variant.sh <out.so> <unit> -DX=1 ...            (one unit)
#        build_diag_variant.sh <out.so> "unit1:-DX=1 -DY=2" "unit2:-DZ=3"   (several)
set -e
cd "$(dirname "$0")/.."
OUT=$1; shift
FLAGS=$(python3 -c "import importlib,sys; sys.path.insert(0,'.'); print(' '.join(importlib.import_module('quad-periodic-mpc_amd.build').FLAGS))")
# one line per unit: its default object, its source, its own defines
UNITS=$(python3 -c "
import importlib, sys
sys.path.insert(0, '.')
b = importlib.import_module('quad-periodic-mpc_amd.build')
for src, defs in b.UNITS:
    print(b._obj(src, defs), src, *['-D' + d for d in defs])")
specs=()
if [[ "$1" == *:* ]]; then specs=("$@"); else specs=("$1:${*:2}"); fi
objs=$(echo "$UNITS" | cut -d' ' -f1)
extra=""
for sp in "${specs[@]}"; do
  TU=${sp%%:*}; DEFS=${sp#*:}
  line=$(echo "$UNITS" | grep -F "/$TU.o " || true)
  if [ "$(echo "$line" | grep -c .)" != 1 ]; then echo "no single unit named $TU" >&2; exit 2; fi
  read -r dflt src udefs <<< "$line"
  o=/tmp/diag_$(basename $OUT)_$TU.o
  X=""; [[ "$src" == *.cpp ]] && X="-x hip"
  /opt/rocm/bin/hipcc $X --offload-arch=gfx950 $FLAGS $udefs $DEFS -c quad-periodic-mpc_amd/csrc/$src -o $o
  objs=$(echo "$objs" | grep -vxF "$dflt")
  extra="$extra $o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" $objs $extra
echo "$OUT"
