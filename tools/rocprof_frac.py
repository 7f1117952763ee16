#!/usr/bin/env python3
"""The projection-GEMM roofline fraction on rocprofv3's clock, next to the one bench.py printed in the SAME run.

    python tools/rocprof_frac.py <kernel_stats.csv> <bench_under_rocprof.json> [out.json]

kernel_stats.csv: the `rocprofv3 --kernel-trace --stats` summary of `python3 bench.py --steps K --warmup W --full ...` (every step of
the command: warm-up, timed, sparse-probe and dense-probe passes — all the same step); the json: the line that command printed.
Output: steps the trace covers (GEMM calls / launches per step), GEMM ms per step (sum of the gemm4w_k / gemm4w_sk_k /
gemm_sk_256 rows / steps), frac_rocprof = the line's GEMM FLOPs per step / that time / the MFMA peak, the sum of ALL kernel
durations per step against the line's ms_per_step (the rocprof durations tile the step when the two agree), the per-family
non-GEMM times, and the ratio line-frac / frac_rocprof that the round-4 verdict asked to hold within 1 %."""
import csv
import json
import sys

GEMM = ("gemm4w_k", "gemm4w_sk_k", "gemm_sk_256", "fewrows_partial_k", "fewrows_finish_k")
GEMM_SECOND = ("fewrows_finish_k",)        # second kernel of a projection (gemm_fewrows.hip): its time counts, its calls do not
FAMILIES = (("attention", ("attn_",)), ("rmsnorm", ("rmsnorm_",)))


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    line = json.loads([ln for ln in open(sys.argv[2]).read().splitlines() if ln.startswith("{")][-1])
    roof = line["roofline"]
    lps = roof["launches_per_step"]
    flops_step = roof["avg_flops_per_launch"] * lps
    is_gemm = lambda r: any(g in r["Name"] for g in GEMM)
    calls = sum(int(r["Calls"]) for r in rows if is_gemm(r) and not any(g in r["Name"] for g in GEMM_SECOND))
    steps = calls / lps
    gemm_ms = sum(float(r["TotalDurationNs"]) for r in rows if is_gemm(r)) / 1e6 / steps
    # this library's kernels are all named *_k; everything else in the trace is torch (the closed-form weight generator and the
    # packing of model construction — one-time, not part of a step — plus a handful of scalar ops per step)
    is_lib = lambda r: is_gemm(r) or "_k<" in r["Name"] or "_k(" in r["Name"]
    all_ms = sum(float(r["TotalDurationNs"]) for r in rows if is_lib(r)) / 1e6 / steps
    torch_ms = sum(float(r["TotalDurationNs"]) for r in rows if not is_lib(r)) / 1e6 / steps
    fam = {}
    for name, keys in FAMILIES:
        fam[name] = sum(float(r["TotalDurationNs"]) for r in rows if is_lib(r) and any(k in r["Name"] for k in keys)) / 1e6 / steps
    fam["other_library_kernels"] = all_ms - gemm_ms - sum(fam.values())
    fam["torch_kernels_incl_one_time_model_construction"] = torch_ms
    per = {}
    for r in rows:
        if is_gemm(r):
            per[r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]] = {
                "calls_per_step": int(r["Calls"]) / steps, "avg_us": float(r["AverageNs"]) / 1e3}
    peak = roof["peak"] * 1e12
    frac_rocprof = flops_step / (gemm_ms * 1e-3) / peak
    out = {"steps_in_trace": steps, "gemm_launches_per_step": lps, "gemm_ms_per_step_rocprof": gemm_ms,
           "avg_launch_us_rocprof": gemm_ms * 1e3 / lps, "frac_rocprof": frac_rocprof,
           "frac_bench_line": roof["frac"], "line_over_rocprof": roof["frac"] / frac_rocprof,
           "gemm_ms_per_step_bench_line": roof["gemm_ms_per_step"],
           "sum_of_library_kernel_ms_per_step": all_ms, "ms_per_step_bench_line": line["ms_per_step"],
           "kernel_time_over_step": all_ms / line["ms_per_step"], "gemm_share_of_kernel_time": gemm_ms / all_ms,
           "non_gemm_ms_per_step": fam, "step_roofline_frac_bench_line": line["step_roofline"]["frac"],
           "per_gemm_kernel": per}
    txt = json.dumps(out, indent=1)
    print(txt)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
