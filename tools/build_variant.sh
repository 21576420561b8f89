#!/bin/bash
# Experiment build for an on-box A/B of one or more units of the library:
#   tools/build_variant.sh NAME UNIT[,UNIT...] [hipcc -D flags...]
#     -> dealii-galerkin-difference-methods_amd/lib/ab/NAME/libgdm_hip.so
# UNIT is an object of csrc/Makefile without its suffix (gdm_stencil_p5,
# gdm_mass3_p5, gdm_mass3_rk_p5, gdm_mass, gdm_capi, ...).  The named units are
# rebuilt by the Makefile's own rules with the flags added; every other object
# comes from the in-tree build (lib/obj), by the Makefile's own list.  Select the
# result with GDM_HIP_LIB (tools/gpu_ab.sh, tools/time_apply.py) and delete
# lib/ab/NAME when the experiment is recorded.
set -e
[ $# -ge 2 ] || { echo "usage: $0 NAME UNIT[,UNIT...] [hipcc -D flags...]" >&2; exit 2; }
NAME=$1; UNITS=${2//,/ }; shift 2
PKG=$(cd "$(dirname "$0")/../dealii-galerkin-difference-methods_amd" && pwd)
C=$PKG/csrc
O=$PKG/lib/ab/$NAME
mkdir -p "$O/obj"
OBJS=$(make -s -C "$C" print-objs)  # relative to csrc
VARIANT=""
for u in $UNITS; do
  case " $OBJS " in *"/$u.o "*) ;; *) echo "$0: no unit $u in the library" >&2; exit 2 ;; esac
  VARIANT="$VARIANT $O/obj/$u.o"
  OBJS=$(echo " $OBJS " | sed "s# [^ ]*/$u\.o # #")
done
make -C "$C" GDM_OBJ="$O/obj" GDM_VARIANT_FLAGS="$*" $VARIANT
(cd "$C" && /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-z,defs -o "$O/libgdm_hip.so" $VARIANT $OBJS)
rm -rf "$O/obj"
echo "built $O"
