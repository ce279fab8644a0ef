#!/usr/bin/env python3
"""The two measurements of profiles/NOTES_dup.md that the tool (tools/bammarkdup_bench.cpp) does not make, on one input (scripts/make_bench_bam.py --shuffled --pairs):
  sig_vs_stats   k_dup_sig against slx_stats_add_device on the same 64 MiB batch in HBM, alternating, from the units' own device-event counters
  sorter_route   reader -> sorter -> [slx_dup_mark_sorter] -> slx_sort_finish -> GPU BGZF writer, wall time from a full sorter to the closed file, with and
                 without marking, alternating
One JSON line per measurement.

    python scripts/dup_measure.py in.bam out_prefix [reps]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (before the library: bench.py's order)

if torch.cuda.is_available():
    torch.cuda.init()
from seqlib_amd import bamio, dupio, sortio, statsio  # noqa: E402


def batches(rd, max_bytes=64 << 20):
    while True:
        b = bamio.Batch()
        bamio._ffi.check(bamio.lib().slx_bam_next(rd.h, max_bytes, C.byref(b)))
        if b.n_records == 0:
            return
        yield b


def sig_vs_stats(path, reps):
    rd = bamio.Reader(path)
    text = rd.header()[0]
    b = next(batches(rd))
    m, s = dupio.Marker(header_text=text), statsio.Stats()
    sig, add = [], []
    for k in range(reps + 1):
        m.clear()
        a0, s0 = m.counter("us_sig"), s.counter("us_add")
        m.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
        s.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
        if k:          # (the first round warms up)
            sig.append(m.counter("us_sig") - a0)
            add.append(s.counter("us_add") - s0)
    out = dict(what="sig_vs_stats", records=b.n_records, bytes=b.n_bytes, us_k_dup_sig=sig, us_stats_add=add, median_sig=statistics.median(sig), median_stats=statistics.median(add),
               gb_per_s_sig=b.n_bytes / statistics.median(sig) / 1e3, us_place=m.counter("us_place"), us_commit=m.counter("us_commit"), long_records=m.counter("long_records"))
    print(json.dumps(out), flush=True)


def sorter_route(path, prefix, reps):
    times = {False: [], True: []}
    info = {}
    for k in range(2 * (reps + 1)):
        mark = bool(k & 1)
        rd = bamio.Reader(path)
        text = rd.header()[0]
        s = sortio.Sorter()
        for b in batches(rd):
            s.add_device(b.d_stream, b.n_bytes, b.d_rec_off, b.n_records)
        out = "%s.sorted.bam" % prefix
        w = bamio.Writer(out)
        m = dupio.Marker(header_text=text) if mark else None
        t0 = time.perf_counter()
        if mark:
            m.mark_sorter(s.h)
        s.finish(w)
        w.close()
        dt = time.perf_counter() - t0
        if k >= 2:
            times[mark].append(dt)
        if mark:
            info = {c: m.counter(c) for c in ("records", "pairs", "duplicates", "us_sig", "us_place", "us_commit", "us_join", "us_pairs", "us_group", "us_apply", "held_bytes")}
            m.close()
        s.close()
        rd.close()
        os.remove(out)
    print(json.dumps(dict(what="sorter_route", unit="s", without_marking=times[False], with_marking=times[True], median_without=statistics.median(times[False]),
                          median_with=statistics.median(times[True]), **info)), flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    sig_vs_stats(sys.argv[1], reps)
    sorter_route(sys.argv[1], sys.argv[2], reps)
