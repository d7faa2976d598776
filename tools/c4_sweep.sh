#!/bin/bash
# C4 global-label kernel sweep (one GPU): slots per CU
set -e
cd "$(dirname "$0")/.."
for slots in 1 2 4; do
  SHD_SSSP_SLOTS=$slots timeout -k 10 120 python -u tools/c4_probe.py 0 4096 3,1
done
