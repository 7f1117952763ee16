#!/usr/bin/env python3
"""What does a token step of the decode cost between the LM head and the next RMSNorm, and how long is the device idle per token?
Reads a rocprofv3 --kernel-trace CSV of `tools/eval_bench.py` (greedy_decode, or --generate / --stop_eos) and prints, over the
window from the first to the last one-row attention launch (attn_decode): the tokens in it (attention launches / layers), per
token the span, the summed kernel time and the idle time, the time of the token-step kernel (decode_next_k) and the summed time
of the framework's own kernels (at::native…: the index / argmax / gather glue of greedy_decode), and the idle time next to the
token step: from the end of the LM head's launch to the start of the next token's first RMSNorm, less the kernels in between
(what the host-side stop check of `generate`, or the glue's launches in `greedy_decode`, leave the device waiting for).
usage: python tools/decode_trace.py <..._kernel_trace.csv> <n_layers>"""
import csv
import sys


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    L = int(sys.argv[2])
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    at = [i for i, r in enumerate(rows) if "attn_decode" in r["Kernel_Name"]]
    if not at:
        raise SystemExit("no attn_decode launch in the trace")
    seg = rows[at[0]:at[-1] + 1]
    tokens = len(at) / L
    dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])      # noqa: E731
    span = int(seg[-1]["End_Timestamp"]) - int(seg[0]["Start_Timestamp"])
    busy = sum(dur(r) for r in seg)
    step = [dur(r) for r in seg if "decode_next_k" in r["Kernel_Name"]]
    glue = [dur(r) for r in seg if "at::native" in r["Kernel_Name"] or "at_cuda_detail" in r["Kernel_Name"]]
    print(f"{len(seg)} kernels over {tokens:.1f} token steps of {L} layers: per token span {span / tokens / 1e3:8.1f} us, "
          f"kernels {busy / tokens / 1e3:8.1f} us, idle {(span - busy) / tokens / 1e3:7.1f} us")
    if step:
        print(f"decode_next_k: {len(step)} launches, {sum(step) / len(step) / 1e3:6.2f} us each "
              f"({sum(step) / tokens / 1e3:6.2f} us per token)")
    first = [i for i, r in enumerate(seg) if "attn_decode" in r["Kernel_Name"]][::L]      # each token's first attention launch
    turn = []
    for a in first[1:]:
        j = a
        while j > 0 and "rmsnorm" not in seg[j]["Kernel_Name"].lower():
            j -= 1                                          # the token's first RMSNorm
        k = j - 1
        while k > 0 and ("decode_next_k" in seg[k]["Kernel_Name"] or "at::native" in seg[k]["Kernel_Name"]
                         or "at_cuda_detail" in seg[k]["Kernel_Name"]):
            k -= 1                                          # the LM head's last launch
        between = sum(dur(r) for r in seg[k + 1:j])
        turn.append(int(seg[j]["Start_Timestamp"]) - int(seg[k]["End_Timestamp"]) - between)
    if turn:
        turn.sort()
        print(f"idle at the token step (LM head end -> next RMSNorm start, less the kernels between): median "
              f"{turn[len(turn) // 2] / 1e3:6.2f} us, mean {sum(turn) / len(turn) / 1e3:6.2f} us, max {turn[-1] / 1e3:6.2f} us "
              f"over {len(turn)} steps")
    print(f"framework kernels: {len(glue)} launches = {len(glue) / tokens:5.1f} per token, "
          f"{sum(glue) / tokens / 1e3:6.2f} us per token")


if __name__ == "__main__":
    main()
