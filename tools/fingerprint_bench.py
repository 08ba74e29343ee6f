#!/usr/bin/env python3
"""`fingerprint` throughput on one GPU.

  1. Device-resident hashing: synthetic 150-bp reads from a seed, pushed as BAM 4-bit codes; the hash kernel's
     time from device events -> G k-mers/s, at k = 31, 21 and 51 (scaled 1000).
  2. End to end: the same reads written to a BAM, `dut_fp_files` on it with DUT_TIMING=1 -- per batch the host
     decode time beside the device time (decode of batch i+1 runs while batch i is on the device).
  3. The hash kernels' VGPRs, LDS, scratch and spills (tools/isa_stats.py).

    python tools/fingerprint_bench.py [--reads 2000000] [--e2e-reads 2000000] [--out DIR]
"""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from decodingustools_amd import build as _b  # noqa: E402
from decodingustools_amd.fingerprint import Fingerprint, fingerprint_file  # noqa: E402


def reads_seq4(n, L, seed):
    """n reads of L bases (ACGT, 0.1 % N) as BAM 4-bit codes and base offsets."""
    rng = np.random.default_rng(seed)
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, size=n * L)]
    codes[rng.random(codes.size) < 0.001] = 15
    if codes.size % 2:
        codes = np.concatenate([codes, np.zeros(1, np.uint8)])
    return ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8), np.arange(n + 1, dtype=np.uint64) * np.uint64(L)


def write_bam(path, seq4, n, L):
    """Unmapped records of L bases (L even), BGZF level 1, blocks compressed on 16 threads."""
    assert L % 2 == 0
    name = b"r\0"
    body = 32 + len(name) + L // 2 + L
    rec = np.zeros((n, 4 + body), np.uint8)
    hdr = struct.pack("<IiiBBHHHIiii", body, -1, -1, len(name), 0, 4680, 0, 4, L, -1, -1, 0) + name
    rec[:, :len(hdr)] = np.frombuffer(hdr, np.uint8)
    rec[:, len(hdr):len(hdr) + L // 2] = seq4.reshape(n, L // 2)
    rec[:, len(hdr) + L // 2:] = 30
    raw = rec.tobytes()
    text = b"@HD\tVN:1.6\n"
    head = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", 0)

    def block(data):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z = c.compress(data) + c.flush()
        return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(z) + 25) + z +
                struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))

    step = 60000
    chunks = [head] + [raw[i:i + step] for i in range(0, len(raw), step)]
    with ThreadPoolExecutor(16) as ex, open(path, "wb") as f:
        for b in ex.map(block, chunks):
            f.write(b)
        f.write(block(b""))


def device_rate(seq4, off, k, reps=3):
    with Fingerprint(k, 1000) as fp:
        fp.push((seq4, off))                                  # warm-up: code objects, buffers
        s0 = fp.stats()
        t0 = time.perf_counter()
        for _ in range(reps):
            fp.push((seq4, off))
        wall = time.perf_counter() - t0
        s1 = fp.stats()
        r = fp.finish()
    win = s1["n_windows"] - s0["n_windows"]
    hash_ms = s1["hash_ms"] - s0["hash_ms"]
    return {"k": k, "windows": win, "batches": s1["n_batches"] - s0["n_batches"], "hash_ms": round(hash_ms, 3),
            "h2d_ms": round(s1["h2d_ms"] - s0["h2d_ms"], 3), "reduce_ms": round(s1["reduce_ms"] - s0["reduce_ms"], 3),
            "gkmers_per_s_kernel": round(win / hash_ms / 1e6, 2), "push_wall_s": round(wall, 3),
            "gkmers_per_s_push": round(win / wall / 1e9, 2), "n_distinct": r.n_distinct}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--e2e-reads", type=int, default=2_000_000)
    ap.add_argument("--out", default=".", help="directory for fingerprint_bench.json (the generated BAM goes to a temporary directory)")
    a = ap.parse_args()
    _b.build()
    os.makedirs(a.out, exist_ok=True)
    L = 150
    seq4, off = reads_seq4(a.reads, L, seed=2024)
    res = {"reads": a.reads, "read_len": L, "scaled": 1000, "device": []}
    for k in (31, 21, 51):
        r = device_rate(seq4, off, k)
        res["device"].append(r)
        print(json.dumps(r), flush=True)
    # end to end from a BAM
    tmp = tempfile.TemporaryDirectory()
    bam = os.path.join(tmp.name, "fp_bench.bam")
    s4e, offe = (seq4, off) if a.e2e_reads == a.reads else reads_seq4(a.e2e_reads, L, seed=2024)
    t0 = time.perf_counter()
    write_bam(bam, s4e, a.e2e_reads, L)
    print(f"wrote {bam}: {os.path.getsize(bam) / 1e6:.1f} MB in {time.perf_counter() - t0:.1f} s", flush=True)
    env = dict(os.environ, DUT_TIMING="1")
    fingerprint_file(bam)                                     # page cache warm
    t0 = time.perf_counter()
    p = subprocess.run([_b.CLI, "fingerprint", bam], capture_output=True, text=True, env=env)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr
    rows = [tuple(float(x) for x in m.groups()) for m in
            re.finditer(r"host decode ([\d.]+) ms, device ([\d.]+) ms \(push call ([\d.]+) ms\)", p.stderr)]
    dec = sum(r[0] for r in rows)
    dev = sum(r[1] for r in rows)
    res["e2e"] = {"reads": a.e2e_reads, "bases": a.e2e_reads * L, "wall_s": round(wall, 3), "batches": len(rows),
                  "host_decode_ms_total": round(dec, 1), "device_ms_total": round(dev, 1),
                  "push_ms_total": round(sum(r[2] for r in rows), 1), "stdout": p.stdout.strip().splitlines(),
                  "per_batch_decode_vs_device_ms": [[r[0], r[1]] for r in rows[:8]]}
    print(json.dumps(res["e2e"]), flush=True)
    isa = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), "k_fp_hash"], capture_output=True, text=True)
    res["isa"] = isa.stdout
    print(isa.stdout)
    with open(os.path.join(a.out, "fingerprint_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    tmp.cleanup()


if __name__ == "__main__":
    main()
