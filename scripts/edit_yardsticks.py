"""The record editor's gather against two yardsticks on the SAME batch (profiles/NOTES_edit.md): one reader batch is held in HBM, and on it

    identity     the editor's kernels under the empty plan: every byte moves once through a 2 KiB tile in LDS ("us_size", "us_scan", "us_gather")
    drop2_addRG  the plan of tools/bamedit_bench.cpp: drop XA and SA, add a constant RG:Z
    sorter       slx_sort_add_device + slx_sort_to_host of those bytes: the sorter's "us_gather" (the same tile shape, sources in sorted order)
    d2d_copy     a device-to-device copy of n_bytes, timed with events

    python scripts/edit_yardsticks.py <mapped.bam>          (scripts/make_bench_bam.py --sorted)

Every figure is the median of 7 runs after a warm-up, in microseconds; GB/s count the bytes read plus the bytes written, 2 x n_bytes.  One JSON line per measurement.
Needs a GPU and torch (for the copy; torch initialises the GPU before the library loads, the order bench.py uses).
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RUNS = 7


def main():
    import torch
    torch.cuda.init()
    from seqlib_amd import bamio, editio, sortio
    rd = bamio.Reader(sys.argv[1])
    _, b = rd.next(1 << 30)
    n, nb = b.n_records, b.n_bytes
    print(json.dumps({"what": "batch", "records": n, "bytes": nb}))
    rate = lambda us: round(2 * nb / us / 1e3, 1)
    e = editio.Editor()

    def apply():
        e.apply_device(b.d_stream, nb, b.d_rec_off, n)
        return e.counter("us_size"), e.counter("us_scan"), e.counter("us_gather")

    def editor(what):
        runs = [apply() for _ in range(RUNS + 1)][1:]
        size, scan, gather = (statistics.median(r[k] for r in runs) for k in range(3))
        print(json.dumps({"what": what, "us_size": size, "us_scan": scan, "us_gather": gather, "gather_min": min(r[2] for r in runs), "gather_max": max(r[2] for r in runs),
                          "gather_GB_per_s": rate(gather), "bytes_out": e.counter("bytes_out"), "long_records": e.counter("long_records")}))
        return gather

    identity = editor("identity")
    e.drop_tag(b"XA")
    e.drop_tag(b"SA")
    e.add_z(b"RG", b"bench.group")
    editor("drop2_addRG")
    e.close()

    gathers = []
    for _ in range(RUNS + 1):
        s = sortio.Sorter()
        s.add_device(b.d_stream, nb, b.d_rec_off, n)
        s.to_host()
        gathers.append(s.counter("us_gather"))
        s.close()
    sorter = statistics.median(gathers[1:])
    print(json.dumps({"what": "sorter", "us_gather": sorter, "gather_min": min(gathers[1:]), "gather_max": max(gathers[1:]), "gather_GB_per_s": rate(sorter),
                      "editor_identity_over_sorter": round(identity / sorter, 2)}))

    src = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def copy():
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) * 1000

    times = [copy() for _ in range(RUNS + 1)][1:]
    c = statistics.median(times)
    print(json.dumps({"what": "d2d_copy", "us": round(c, 1), "min": round(min(times), 1), "max": round(max(times), 1), "GB_per_s": rate(c), "editor_identity_over_copy": round(identity / c, 2)}))
    rd.close()


if __name__ == "__main__":
    main()
