#!/bin/bash
# Builds library variants for A/B timing: tools/ab_build.sh name "<extra hipcc flags>" ...
# -> tools/ab/ab_<name>.so (same C ABI; select with PIXO_HIP_LIB=...; kept OUT of the package directory and out of git —
# delete the variants after the call that measured them: everything under tools/ab/ is pushed to the GPU box).  Only the
# files named by AB_SRC (default jpeg_kernels.hip; several separated by blanks, e.g. AB_SRC="png_deflate.hip png_encode_api.cpp")
# are recompiled per variant; the other translation units, the lists of pixo_amd/csrc/Makefile, are compiled once into
# /tmp/pixo_ab_obj.
#   AB_REV=<git revision> tools/ab_build.sh name     the whole library of another revision, built by its own Makefile
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p "$ROOT/tools/ab"
if [ -n "$AB_REV" ]; then
  T=$(mktemp -d /tmp/pixo_ab_rev_XXXXXX)
  trap 'rm -rf "$T"' EXIT
  git -C "$ROOT" archive "$AB_REV" | tar -x -C "$T"
  make -C "$T/pixo_amd/csrc" -j16 > /dev/null
  cp "$T/pixo_amd/libpixo_hip.so" "$ROOT/tools/ab/ab_$1.so"
  echo "built ab_$1.so (revision $AB_REV)"
  exit 0
fi
cd "$ROOT/pixo_amd/csrc"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize"
OBJ=/tmp/pixo_ab_obj; mkdir -p $OBJ
SRC=${AB_SRC:-jpeg_kernels.hip}
ALL="$(sed -n 's/^KERNELS *= *//p' Makefile) $(sed -n 's/^HOST *= *//p' Makefile)"
# (the shipped build's flag for the coefficient kernels, see the Makefile; a variant may override it with its own -mllvm option)
PRELOAD="-mllvm -amdgpu-kernarg-preload-count=14"
preload() { { [ $1 = jpeg_kernels.hip ] || [ $1 = jpeg_pixels_code.hip ]; } && echo "$PRELOAD" || true; }
for f in $ALL; do
  o=$OBJ/$f.o   # (the whole name: png_inflate.hip and png_inflate.cpp share a stem)
  if [ ! -f $o ] || [ $f -nt $o ] || [ -n "$(find . ../../include -name '*.h*' -newer $o | head -1)" ]; then /opt/rocm/bin/hipcc $FLAGS $(preload $f) -c $f -o $o & fi
done
wait
while [ $# -ge 2 ]; do
  OBJS=""
  for f in $ALL; do
    case " $SRC " in
      *" $f "*)
        case "$2" in *NO_PRELOAD*) P="";; *) P="$(preload $f)";; esac
        /opt/rocm/bin/hipcc $FLAGS $P $2 -c $f -o $OBJ/${f}_$1.o
        OBJS="$OBJS $OBJ/${f}_$1.o";;
      *) OBJS="$OBJS $OBJ/$f.o";;
    esac
  done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o ../../tools/ab/ab_$1.so $OBJS
  echo "built ab_$1.so ($2)"
  shift 2
done
