#!/usr/bin/env python3
"""Kernel time of the TN contraction kernels and their second stage from a rocprofv3 kernel_stats.csv, per family: total ms of the
profiled run and launches.  Usage: tn_groups.py kernel_stats.csv"""
import csv
import re
import sys

FAMILIES = [("gemm_tn_kernel", r"gemm_tn_kernel"), ("gemm_tn_bf16s_kernel", r"gemm_tn_bf16s_kernel"), ("gemm_tn_f16s_kernel", r"gemm_tn_f16s_kernel"),
            ("gemm_tn_f16s8_kernel", r"gemm_tn_f16s8_kernel"), ("s16_tn_kernel", r"s16_tn_kernel"), ("tn_reduce_kernel", r"[^_]tn_reduce_kernel"),
            ("tn_reduce_lanes_kernel", r"[^_]tn_reduce_lanes_kernel"), ("tn_reduce_oihw_kernel", r"[^_]tn_reduce_oihw_kernel"),
            ("s16_tn_reduce_kernel", r"s16_tn_reduce_kernel")]
tot = {f: [0.0, 0] for f, _ in FAMILIES}
for r in csv.DictReader(open(sys.argv[1])):
    for f, pat in FAMILIES:
        if re.search(pat, r["Name"]):
            tot[f][0] += float(r["TotalDurationNs"]) / 1e6
            tot[f][1] += int(r["Calls"])
            break
print(" ".join(f"{f}={t:.2f}ms/{n}" for f, (t, n) in tot.items() if n))
