#!/bin/bash
# Registers, scratch and LDS of every kernel, as the compiler reports them (no GPU needed):
#   tools/kernel_resources.sh > profiles/rNN_kernel_resources.txt
#   tools/kernel_resources.sh oslam_arbitrate > profiles/rNN_kernel_resources_arbitrate.txt   (the named units only)
# Each translation unit with the flags the Makefile builds it with; EXTRA="-D..." adds to them, as in the Makefile.
# For the two units with the vote kernels it also prints float_denorm_mode_32 of every vote kernel's descriptor: the
# vote addresses are computed on denormal floats (VoteRegs::vote) and need 3 there, denormals kept in and out.
cd "$(dirname "$0")/../objective-slam_amd/csrc"
units="$*"
[ -z "$units" ] && units="$(ls *.hip | sed 's/\.hip$//')"      # every kernel unit
for f in $units; do
  fl=""; [ $f = oslam_vote_wide ] && fl="-mllvm -disable-machine-licm"
  echo "== $f.hip $fl"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -ffp-contract=off -fno-fast-math -I../../include -I. $EXTRA $fl \
      -Rpass-analysis=kernel-resource-usage -c $f.hip -o /tmp/kr_$$.o 2>&1 \
    | grep -E "Function Name|TotalSGPRs|VGPRs:|AGPRs:|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size" | sed 's/.*remark: *//; s/ \[-Rpass.*//'
  case $f in oslam_vote|oslam_vote_wide)
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -ffp-contract=off -fno-fast-math -I../../include -I. $EXTRA $fl \
        --offload-device-only -S $f.hip -o - 2>/dev/null \
      | awk '/^[ \t]*\.amdhsa_kernel /{k=$2} /\.amdhsa_float_denorm_mode_32/ && k ~ /^_Z[0-9]+k_vote/ {print "float_denorm_mode_32 " $2 "  " k}' ;;
  esac
done
rm -f /tmp/kr_$$.o
