#!/bin/bash
# Build variants of one kernel file with -D switches (the numeric knobs: NSD_P_SLEEP, NSD_X4_KP, NSD_BX4_CHD, ...) and time them all in
# ONE visit to the GPU (box-to-box variation is ~1-5 %).
#   tools/sweep.sh nsd_lstm2_fwd48.hip "-DNSD_P_SLEEP=1 -DNSD_S_SLEEP=2" "-DNSD_P_SLEEP=3" ...
# Writes libnsd_hip_v<i>.so next to the shipped library and prints the command to run: one kbench run per library, each under its own
# time limit, chained so that nothing starts after a run that failed.
set -e
cd "$(dirname "$0")/../neural-speech-decoding_amd/csrc"
src=$1; shift
make -s -j4 >/dev/null 2>&1
# the library's objects and flags are the Makefile's (SRCS / FLAGS), not a copy of them
objs=$(make -s -pn | sed -n 's/^OBJS := //p')
flags0=$(make -s -pn | sed -n 's/^FLAGS = //p' | sed 's/\$(ARCH)/gfx950/')
case " $objs " in *" ${src%.hip}.o "*) ;; *) echo "$src is not one of the Makefile's SRCS" >&2; exit 1;; esac
tmp=$(mktemp -d)
i=0
libs="libnsd_hip.so"
for flags in "$@"; do
    /opt/rocm/bin/hipcc $flags0 $flags -c $src -o $tmp/sweep_$i.o
    o=$(echo " $objs " | sed "s# ${src%.hip}.o # $tmp/sweep_$i.o #")
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libnsd_hip_v$i.so $o
    echo "v$i: $flags"
    libs="$libs libnsd_hip_v$i.so"
    i=$((i+1))
done
rm -rf "$tmp"
cmd=""
for l in $libs libnsd_hip.so; do
    cmd="$cmd${cmd:+ && }echo $l && NSD_LIB=$l timeout -k 10 120 python tools/kbench.py | grep ablate="
done
echo "run (from the repository root): set -o pipefail; $cmd"
