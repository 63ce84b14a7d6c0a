#!/bin/bash
# tools/build_variant.sh <name> <file.hip> "<extra -D flags>": links lib/variants/libsylph_<name>.so with one translation
# unit rebuilt under -DSYLPH_ABLATE + extra defines (kernel ablations / A-B builds; select with SYLPH_LIB_PATH).
# The object list and the unit's compile command come from csrc/Makefile.
set -e
NAME=$1; SRC=$2; FLAGS=$3
cd "$(dirname "$0")/../sylph-few-shot-detection_amd/csrc"
BASE=$(basename "$SRC" .hip)
make -s -j16
mkdir -p ../lib/variants
OBJ=/tmp/variant_${NAME}_${BASE}.o
CMD=$(make -s -n -B "$BASE.o")
${CMD% -o *} -DSYLPH_ABLATE $FLAGS -o "$OBJ"
OBJS=""
for o in $(make -s --eval='print-objs: ; @echo $(OBJS)' print-objs); do
  if [ "$o" == "$BASE.o" ]; then OBJS="$OBJS $OBJ"; else OBJS="$OBJS $o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS -ldl -o ../lib/variants/libsylph_${NAME}.so
echo built ../lib/variants/libsylph_${NAME}.so
