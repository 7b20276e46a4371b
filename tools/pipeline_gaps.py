#!/usr/bin/env python
"""How much of the decoder the slot pipeline hides, from a rocprofv3 kernel trace of bench.py
(`rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python bench.py --steps 32 --warmup 8`):

    python tools/pipeline_gaps.py DIR/.../t_kernel_trace.csv --launches 4

Encoder-class kernels are the kernels of the queues that carry the encoder attention (attn_enc*): the two encoder streams.  A
decoder launch is the run of kernels on one of the other queues that ends with the head (head_rows_kernel / pair_verdict_kernel).
The timed region is taken as the last --launches decoder launches (steps / group of the bench command): from the first encoder
kernel that starts behind the head before them to the end of the last kernel.  Printed: the time in the region during which no
encoder-class kernel runs, and per decoder launch its span and the share of it that encoder kernels overlap."""
import argparse
import collections
import csv


def union(iv):
    """sorted disjoint union of [a, b) intervals"""
    out = []
    for a, b in sorted(iv):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def covered(u, a, b):
    """length of [a, b) covered by the disjoint union u"""
    return sum(max(0, min(b, y) - max(a, x)) for x, y in u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--launches", type=int, required=True, help="decoder launches in the timed region (bench: steps / group)")
    args = ap.parse_args()
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), r["Kernel_Name"]) for r in csv.DictReader(open(args.trace))]
    rows.sort()
    enc_q = {q for _, _, q, n in rows if "attn_enc" in n}
    heads = [r for r in rows if "head_rows_kernel" in r[3] or "pair_verdict_kernel" in r[3]]
    if len(heads) <= args.launches or not enc_q:
        raise SystemExit(f"{len(heads)} decoder launches and {len(enc_q)} encoder queues in the trace: nothing to cut a region of {args.launches} from")
    before = heads[-args.launches - 1][1]                      # end of the last head in front of the region
    enc = [r for r in rows if r[2] in enc_q and r[0] >= before]
    t0, t1 = enc[0][0], max(r[1] for r in rows)
    u = union([(a, b) for a, b, _, _ in enc])
    busy = covered(u, t0, t1)
    print(f"timed region: {(t1 - t0) / 1e6:.3f} ms, {args.launches} launch sequences, encoder queues {sorted(enc_q)}")
    print(f"no encoder-class kernel running: {(t1 - t0 - busy) / 1e6:.3f} ms ({(t1 - t0 - busy) / (t1 - t0) * 100:.1f} % of the region)")
    # decoder launches: per non-encoder queue, the kernels between two heads
    dec = collections.defaultdict(list)
    for r in rows:
        if r[2] not in enc_q and r[0] >= t0 and "copyBuffer" not in r[3] and "fillBuffer" not in r[3]:
            dec[r[2]].append(r)
    spans = []
    for q, rs in dec.items():
        first = None
        for a, b, _, n in rs:
            first = a if first is None else first
            if "head_rows_kernel" in n or "pair_verdict_kernel" in n:
                spans.append((first, b, q))
                first = None
    tot_span = tot_hid = 0
    for i, (a, b, q) in enumerate(sorted(spans)):
        hid = covered(u, a, b)
        tot_span += b - a
        tot_hid += hid
        print(f"decoder launch {i} (queue {q}): span {(b - a) / 1e6:.3f} ms at +{(a - t0) / 1e6:.3f} ms, {hid / (b - a) * 100:5.1f} % under encoder kernels")
    if tot_span:
        print(f"decoder spans in all: {tot_span / 1e6:.3f} ms, {tot_hid / tot_span * 100:.1f} % under encoder kernels, {(tot_span - tot_hid) / 1e6:.3f} ms exposed")


if __name__ == "__main__":
    main()
