#!/bin/bash
# lib/variants/libsylph_hq.so: the product objects + conv_hpipe.hip rebuilt with the dispatch to the four-wave probe kernel
# (tools/probes/conv_hpipe4.hip, SYLPH_CONV_HQ=1 selects it at run time).  Measurement only.
set -e
cd "$(dirname "$0")/../../sylph-few-shot-detection_amd/csrc"
mkdir -p ../lib/variants
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -DSYLPH_ABLATE -DSYLPH_HQ_PROBE"
/opt/rocm/bin/hipcc $F -c conv_hpipe.hip -o /tmp/hq_conv_hpipe.o
/opt/rocm/bin/hipcc $F -c ../../tools/probes/conv_hpipe4.hip -o /tmp/hq_conv_hpipe4.o
make -s -j16
OBJS=""
for o in $(make -s --eval='print-objs: ; @echo $(OBJS)' print-objs); do [ "$o" == conv_hpipe.o ] || OBJS="$OBJS $o"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS /tmp/hq_conv_hpipe.o /tmp/hq_conv_hpipe4.o -ldl -o ../lib/variants/libsylph_hq.so
echo built ../lib/variants/libsylph_hq.so
