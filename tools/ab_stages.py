#!/usr/bin/env python3
"""Same-box A/B of the engine's host stages (push, upload) for two builds of the library, the way tools/ab_bench.sh
compares kernels: child processes alternate between the two builds through DUT_CALLABLE_LIB with DUT_TIMING=1, each
runs the contig three times on one engine (the first, cold pass is dropped), and the stage times are read from stderr.
Contigs: the one bench.py uses for its single-GPU figure (chr21-sized, 30x short reads, pass-bit form), and with
DUT_QUAL_FORM=bytes an 8 Mb long-read contig (run table) and a 10 Mb short-read contig (records).  Per stage: medians,
maxima, and `ok` = this build's median is not above the parent's largest value.

    python tools/ab_stages.py <parent lib.so> <new lib.so> <out.json> [rounds = 4]
"""
import json, os, re, statistics, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decodingustools_amd import synth                     # (pure numpy: the parent never loads the library or opens the GPU)

LINE = re.compile(r"engine: (.+?)\s+([0-9.]+) ms$")
PASSES = 3                                                 # per child: the first one is cold and dropped


def child(lib, form, rec, ref, L, tid, log_path):
    os.environ["DUT_CALLABLE_LIB"] = lib
    os.environ["DUT_TIMING"] = "1"
    if form == "bytes":
        os.environ["DUT_QUAL_FORM"] = "bytes"
    else:
        os.environ.pop("DUT_QUAL_FORM", None)
    fd = os.open(log_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 2)
    from decodingustools_amd import CallableOptions, CallableProfiler, ContigProfiler, Engine, process_single_contig
    opt = CallableOptions()
    bed = os.path.join(tempfile.gettempdir(), "ab_stages_%d.bed" % os.getpid())
    with Engine(opt, 0) as eng:
        for k in range(PASSES):
            os.write(2, b"##pass %d\n" % k)
            counter = CallableProfiler(bed)
            process_single_contig(eng, counter, ContigProfiler("c", L), opt, tid, rec, ref)
            counter.close()
    os.write(2, b"##end\n")
    os.remove(bed)
    os._exit(0)


def parse(log_path):
    passes, cur = [], None
    for ln in open(log_path, errors="replace"):
        ln = ln.rstrip()
        if ln.startswith("##pass"):
            cur = {}; passes.append(cur)
        elif ln.startswith("##end"):
            cur = None
        elif cur is not None:
            m = LINE.search(ln)
            if m:
                cur[m.group(1).strip()] = cur.get(m.group(1).strip(), 0.0) + float(m.group(2))
    return passes[1:]


def main():
    lib_a, lib_b, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]), sys.argv[3]
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    configs = []
    t0 = time.time()
    L = 46_709_983; seed = synth.seed_for(2, 20)
    configs.append(("chr21_30x_short_bits", "bits", synth.short_read_contig(L, 30.0, seed), synth.make_reference(L, seed), L, 20))
    print("chr21 generated", round(time.time() - t0, 1), "s", flush=True)
    L2 = 8_000_000; seed2 = synth.seed_for(3, 23)
    configs.append(("long_8mb_30x_bytes", "bytes", synth.long_read_contig(L2, 30, seed2), synth.make_reference(L2, seed2), L2, 23))
    L3 = 10_000_000; seed3 = synth.seed_for(2, 21)
    configs.append(("short_10mb_30x_bytes", "bytes", synth.short_read_contig(L3, 30.0, seed3), synth.make_reference(L3, seed3), L3, 21))
    print("all generated", round(time.time() - t0, 1), "s", flush=True)
    result = {}
    for name, form, rec, ref, Lc, tid in configs:
        samples = {"parent": {}, "new": {}}
        for r in range(rounds):
            for tag, lib in (("parent", lib_a), ("new", lib_b)):
                log_path = os.path.join(os.path.dirname(out), f"ab_{name}_{tag}_{r}.log")
                pid = os.fork()
                if pid == 0:
                    try:
                        child(lib, form, rec, ref, Lc, tid, log_path)
                    finally:
                        os._exit(3)
                _, status = os.waitpid(pid, 0)
                if status != 0:
                    print("child failed", name, tag, r, status, flush=True)
                    sys.exit(1)                                  # nothing more is started
                for p in parse(log_path):
                    for k, v in p.items():
                        samples[tag].setdefault(k, []).append(v)
            print(name, "round", r, "done", round(time.time() - t0, 1), "s", flush=True)
        table = {}
        for k in sorted(set(samples["parent"]) | set(samples["new"])):
            a, b = samples["parent"].get(k, []), samples["new"].get(k, [])
            if not a or not b or not (k.startswith("push:") or k.startswith("upload:")):
                continue
            table[k] = dict(parent_median=round(statistics.median(a), 2), parent_max=round(max(a), 2), new_median=round(statistics.median(b), 2),
                            new_max=round(max(b), 2), n=len(b), ok=statistics.median(b) <= max(a))
        result[name] = dict(reads=int(rec.n), length=Lc, qual_form=form, samples_per_build=len(next(iter(samples["new"].values()))), stages_ms=table)
        for k, v in table.items():
            print(f"  {k:40s} parent med {v['parent_median']:8.2f} max {v['parent_max']:8.2f} | new med {v['new_median']:8.2f}  {'ok' if v['ok'] else 'SLOWER'}", flush=True)
    json.dump(result, open(out, "w"), indent=1)


main()
