#!/bin/bash
# A variant of the library built from the same sources with extra compiler flags, for A/B runs on one box:
#   bash tools/buildvar.sh <name> <flags ...>      -> build/libswmarlin_<name>.so   (select it with SWM_LIB_PATH)
# e.g. bash tools/buildvar.sh p0 -DSWM_LIGHT_PRIO=0 -DSWM_TAIL_PRIO=0   (the library without issue priorities: collect_profiles.sh)
# Built by csrc/Makefile (its units, its flags plus EXTRA) into an object directory and an output of its own: the in-tree
# csrc/build/ and libswmarlin.so are not touched.
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
d=$root/build/var_$name; mkdir -p $d
make -C $root/simpleworks_amd/csrc -j${MAX_JOBS:-8} BUILD=$d OUT=$root/build/libswmarlin_$name.so EXTRA="$*" && rm -rf $d && echo built $name
