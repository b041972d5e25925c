#!/bin/bash
# Register / occupancy summary of one replay unit: tools/regs.sh <KIND> [NPASS] [extra hipcc flags]
case "${2:-1}" in 1|2|4) ;; *) echo "usage: tools/regs.sh <KIND> [NPASS: 1, 2 or 4] [extra hipcc flags]" >&2; exit 2 ;; esac
cd "$(dirname "$0")/.."
F=$(python -c "from funsearch_kubernetes_simulator_amd.ops.build import _hip_flags; print(' '.join(_hip_flags()))")
/opt/rocm/bin/hipcc $F -DFKS_KIND=${1:-3} -DFKS_NPASS=${2:-1} "${@:3}" -c csrc/hip/replay_kernels.hip -o /dev/null \
  -Rpass-analysis=kernel-resource-usage 2>&1 | python3 tools/regs_summary.py
