#!/bin/bash
# Lists every kernel of the library that uses scratch (private) memory: tools/check_scratch.sh [--table] [file.hip ...]
# (device-only -S of each csrc/*.hip, in parallel; CPU only, a few minutes).  Expected in air_gemm.hip: the 28-byte tables of
# the legacy fp32 / round-1 GEMM kernels (gemm_f32_kernel, gemm_bf16_kernel: every tile but 1 x 1), and six lean bf16 kernels:
# 36 bytes in gemm_bf16v2_kernel<1, 1, false, {0, 3, 4, 5}> and <2, 4, false, 0>, 20 bytes in <1, 1, true, 0>
# (profiles/gemm_parts_resources.txt).  Any other hot kernel that shows up here has an array the compiler could not keep in
# registers (HIP vector structs carried across barriers) or ran out of its register budget
# (wgrad_grouped_bf16_kernel sits at exactly 168).
# --table: one line per kernel of the given files instead, sorted by demangled name -- VGPRs (arch + acc), scratch bytes,
# static LDS bytes, occupancy (waves per SIMD) and code bytes, from the assembly's own per-kernel comments.  Two such
# tables (before / after a change to a kernel body) diff line by line: DESIGN.md section 23.
table=0; [ "$1" = "--table" ] && { table=1; shift; }
root=$(cd "$(dirname "$0")/.." && pwd)
src=$root/tf-attend-infer-repeat_amd/csrc
files=("$@"); [ ${#files[@]} -eq 0 ] && files=($src/*.hip)
tmp=$(mktemp -d)
for f in "${files[@]}"; do
  ( /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I$root/include -I$src --cuda-device-only -S "$f" -o $tmp/$(basename $f).s 2>/dev/null ) &
done
wait
if [ $table = 1 ]; then
  for s in $tmp/*.s; do
    awk -v f=$(basename $s .s) '/^\t\.amdhsa_kernel /{name=$2} /^; codeLenInByte = /{c=$4} /^; TotalNumVgprs:/{v=$3} /^; ScratchSize:/{sc=$3}
      /^; LDSByteSize:/{l=$3} /^; Occupancy:/{if (name != "") printf "%s\t%s\tvgpr %s scratch %s lds %s occupancy %s code %s\n", name, f, v, sc, l, $3, c; name=""}' $s
  done | c++filt | sed 's/(anonymous namespace):://; s/^void //' | sort
else
  for s in $tmp/*.s; do
    awk -v f=$(basename $s .s) '/^_Z.*:/{name=$1} /; NumVgprs:/{v=$3} /; ScratchSize: [1-9]/{printf "%s  %s scratch %s bytes, %s VGPRs\n", f, name, $3, v}' $s
  done | c++filt | sed 's/(anonymous namespace):://'
fi
rm -rf $tmp
