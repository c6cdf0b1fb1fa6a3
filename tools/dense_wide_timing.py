#!/usr/bin/env python3
"""Times ops.dense_xty beyond 64 columns (odil_dense_block_xty_wide) as the Schur route calls it: D^T [D | r] of a
float64 matrix of `rows` x (p + 1), HIP events, one warm-up call, median of --reps, beside the time that reading both
operands ONCE at --hbm TB/s would take.

    python tools/dense_wide_timing.py --case 131072 97 --case 131072 141
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from odil_amd import ops  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--case", type=int, nargs=2, action="append", metavar=("ROWS", "P"), required=True)
    parser.add_argument("--reps", type=int, default=11)
    parser.add_argument("--hbm", type=float, default=6.3, help="achievable HBM rate, TB/s")
    args = parser.parse_args()
    dev = torch.device("cuda:0")
    for rows, p in args.case:
        daug = torch.empty((rows, p + 1), dtype=torch.float64, device=dev).uniform_(-1, 1)
        ops.dense_xty(daug[:, :p], daug)  # warm-up: workspace, code object
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            ops.dense_xty(daug[:, :p], daug)
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_time(stop))
        nbytes = 2 * daug.numel() * daug.element_size()  # X and Y, each read once (here they share their memory)
        floor = nbytes / (args.hbm * 1e12) * 1e3
        med = statistics.median(times)
        print(json.dumps(dict(rows=rows, p=p, dtype="float64", operand_bytes=nbytes // 2, reps=args.reps,
                              median_ms=round(med, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4),
                              read_both_once_ms=round(floor, 4), ratio=round(med / floor, 2))), flush=True)
        del daug
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
