#!/usr/bin/env python3
"""The three sizing exports of the gap-index candidates over a grid of valid arguments, one line per tuple, without a
GPU: run against two builds (TVZ_LIB selects one) and compared with diff, it shows that a change to the workspace layout
left every byte count as it was.
   TVZ_LIB=PARENT/tvidz_amd/libtvz.so python3 profiles/gap_candidates_sizes.py > parent.txt
   python3 profiles/gap_candidates_sizes.py > branch.txt && diff parent.txt branch.txt && wc -l branch.txt"""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tvidz_amd import _lib  # noqa: E402

lib = _lib.load()
for Q, L, explicit, cap, C in itertools.product((0, 1, 16, 70, 65535), (0, 4, 514, 4095), (False, True), (1, 17, 4096), (1, 64)):
    if cap < C:
        continue
    keys = Q * L // 2 + 3 if explicit else 0
    print("plain", Q, L, keys, cap, C, lib.tvz_align_candidates_workspace_bytes(Q, L, keys, cap, C))
    for R in (1, 3, 8):
        if Q * R <= 65535:
            print("rates", Q, L, keys, R, cap, C, lib.tvz_align_candidates_rates_workspace_bytes(Q, L, keys, R, cap, C))
    for n_ranks in (0, 1, 16):
        print("sharded", Q, L, keys, cap, C, n_ranks, lib.tvz_align_candidates_sharded_workspace_bytes(Q, L, keys, cap, C, n_ranks))
