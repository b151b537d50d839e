#!/bin/bash
# A/B helper: link a library one of whose translation units is compiled from its source at git
# revision <rev> (with the current headers and the unit's own defines), every other unit from
# build/obj (the current tree). A unit is named as for build_diag_variant.sh: by its source, or by
# its object's name in build/obj without the .o where one source has several units.
# usage: build_rev_variant.sh <rev> <unit> <out.so>
set -e
cd "$(dirname "$0")/.."
REV=$1; TU=$2; OUT=$3
FLAGS=$(python3 -c "import importlib,sys; sys.path.insert(0,'.'); print(' '.join(importlib.import_module('quad-periodic-mpc_amd.build').FLAGS))")
UNITS=$(python3 -c "
import importlib, sys
sys.path.insert(0, '.')
b = importlib.import_module('quad-periodic-mpc_amd.build')
for src, defs in b.UNITS:
    print(b._obj(src, defs), src, *['-D' + d for d in defs])")
line=$(echo "$UNITS" | grep -F "/$TU.o " || true)
if [ "$(echo "$line" | grep -c .)" != 1 ]; then echo "no single unit named $TU" >&2; exit 2; fi
read -r dflt src udefs <<< "$line"
TMP=quad-periodic-mpc_amd/csrc/_rev_${src}
git show "$REV:quad-periodic-mpc_amd/csrc/$src" > "$TMP"
X=""; [[ "$src" == *.cpp ]] && X="-x hip"
/opt/rocm/bin/hipcc $X --offload-arch=gfx950 $FLAGS $udefs -c "$TMP" -o /tmp/rev_$$.o
rm -f "$TMP"
objs=$(echo "$UNITS" | cut -d' ' -f1 | grep -vxF "$dflt")
mkdir -p "$(dirname "$OUT")"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" $objs /tmp/rev_$$.o
echo "$OUT"
