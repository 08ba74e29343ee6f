#!/usr/bin/env python3
"""What the depth profile files cost from files: `dut-coverage coverage` on the chr21-shaped 30x BAM of tools/e2e_bench.py
(same generator and seed), with and without --depth-dist / --depth-windows --window 500 / --depth-summary,
DUT_CLI_FOREGROUND=1 (one process: the caller waits for everything), alternating runs, wall time of the command.

    python tools/depth_files_bench.py [--length 46709983] [--depth 30] [--reps 5] [--dir DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from decodingustools_amd import build as _b, synth  # noqa: E402
import e2e_bench_lib as EL  # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v), "all": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=46_709_983)
    ap.add_argument("--depth", type=float, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_depth_files.json"))
    a = ap.parse_args()
    out = a.dir or tempfile.mkdtemp()
    os.makedirs(out, exist_ok=True)
    L = a.length
    seed = synth.seed_for(2, 20)
    rec = synth.short_read_contig(L, a.depth, seed)
    ref = synth.make_reference(L, seed)
    bam, fa = os.path.join(out, "s.bam"), os.path.join(out, "s.fa")
    EL.write_bam_native(out, bam, "chr21", L, rec, threads=16)
    EL.write_fasta(fa, "chr21", ref)
    n_reads = int(rec.n)
    del rec, ref
    flags = ["--depth-dist", "d.tsv", "--depth-windows", "w.tsv", "--window", "500", "--depth-summary", "s.tsv"]
    env = dict(os.environ, DUT_CLI_FOREGROUND="1")
    times = {"plain": [], "depth": []}
    sizes = {}

    def run(kind):
        d = os.path.join(out, kind)
        os.makedirs(d, exist_ok=True)
        t0 = time.perf_counter()
        r = subprocess.run([_b.CLI, "coverage", bam, "-r", fa, "-o", "g.bed", "-s", "r.html"] + (flags if kind == "depth" else []),
                           cwd=d, env=env, capture_output=True, text=True, timeout=300)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            sys.exit(f"{kind}: exit {r.returncode}: {r.stderr[-2000:]}")
        return dt

    run("plain")                                               # warm: page cache, code objects
    for _ in range(a.reps):
        for kind in ("plain", "depth"):
            times[kind].append(run(kind))
    for f in ("d.tsv", "w.tsv", "s.tsv"):
        sizes[f] = os.path.getsize(os.path.join(out, "depth", f))
    same = open(os.path.join(out, "plain", "g.bed"), "rb").read() == open(os.path.join(out, "depth", "g.bed"), "rb").read()
    res = {"workload": f"dut-coverage coverage s.bam -r s.fa -o g.bed -s r.html, {L} bp, {a.depth}x, {n_reads} reads, "
                       f"{os.path.getsize(bam)} bytes of BAM, DUT_CLI_FOREGROUND=1, wall seconds of the command",
           "measured_against": "the same command without the depth flags, alternating, same process tree and files",
           "depth_flags": " ".join(flags), "without_flags_s": spread(times["plain"]), "with_flags_s": spread(times["depth"]),
           "added_s_median": statistics.median(times["depth"]) - statistics.median(times["plain"]),
           "depth_file_bytes": sizes, "bed_identical": same}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
