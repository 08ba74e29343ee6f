"""The host side of `consensus`, without a device: the composed rule in plain C++ against the independent reference
tests/cons_ref.py, the assembler and both writers against the hand-derived cases of tests/golden/cons_kat.json, the CLI's
argument checks; and the reference's own vectorised rule against its rule in exact fractions."""
import json
import os
import subprocess

import numpy as np
import pytest

import cons_ref as K
from decodingustools_amd import CallableOptions, EngineError, build as _b, variants as V
from decodingustools_amd.callable_loci import INS_CANDIDATE, INS_OBS, ConsResult, HostStage, InsResult

DOC = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cons_kat.json")))
KAT, P = DOC["cases"], DOC["params"]
PARAMS = [(1, 1, 1), (10, 3, 7000), (3, 2, 2500), (4, 1, 10000)]
REFS = "ACGTNacgtn"


def small_counts(total):
    """Every (a, c, g, t, rest, del) with sum <= total."""
    for a in range(total + 1):
        for c in range(total + 1 - a):
            for g in range(total + 1 - a - c):
                for t in range(total + 1 - a - c - g):
                    for rest in range(total + 1 - a - c - g - t):
                        for d in range(total + 1 - a - c - g - t - rest):
                            yield a, c, g, t, rest, d


def test_rule_equals_the_reference_over_all_small_counts():
    """All 18 564 count tuples with sum <= 12: the C++ rule, the reference's rule in fractions and its vectorised form
    agree in class and byte, under four parameter sets and a reference byte that cycles through ACGTN in both cases."""
    tuples = list(small_counts(12))
    assert len(tuples) == 18_564
    acgt = np.array([x[:4] for x in tuples], np.int64)
    depth = acgt.sum(1) + np.array([x[4] for x in tuples], np.int64)
    dels = np.array([x[5] for x in tuples], np.int64)
    ref = np.frombuffer("".join(REFS[i % len(REFS)] for i in range(len(tuples))).encode(), np.uint8)
    seen = set()
    for prm in PARAMS:
        vec = K.reduce(acgt, depth, dels, ref, len(tuples), *prm, 0, len(tuples))
        n = [0] * 5
        for i, (a, c, g, t, rest, d) in enumerate(tuples):
            want = K.classify(a, c, g, t, depth[i], d, ref[i], *prm)
            got = V.cons_classify_counts(a, c, g, t, int(depth[i]), d, *prm, int(ref[i]))
            assert got == want == (int(vec["cls"][i]), chr(vec["cons"][i])), (tuples[i], chr(ref[i]), prm, got, want)
            n[got[0]] += 1
            seen.add(got)
        assert tuple(n) == vec["counts"]
    assert {s[1] for s in seen} == set("n-ACGTN") and {s[0] for s in seen} == set(range(5))


def test_rule_at_the_seven_tenths_and_per_10k_edges_of_large_counts():
    ref = ord("A")
    for depth in (10, 1000, 999_999, 1 << 20, (1 << 31) + 7, (1 << 32) - 1):
        m = -(-7 * depth // 10)                                         # the smallest count with 10 m >= 7 depth
        for base, at in (("A", 0), ("C", 1), ("G", 2), ("T", 3)):
            cnt = [0, 0, 0, 0]
            cnt[at] = m
            got = V.cons_classify_counts(*cnt, depth, 0, 1, 1, 1, ref)
            assert got == (K.REF if base == "A" else K.ALT, base) == K.classify(*cnt, depth, 0, ref, 1, 1, 1), (depth, base)
            cnt[at] = m - 1
            got = V.cons_classify_counts(*cnt, depth, 0, 1, 1, 1, ref)
            assert got == (K.NO_CALL, "N") == K.classify(*cnt, depth, 0, ref, 1, 1, 1), (depth, base)
    # 10000 * del == per_10k * span exactly and one below, where the product is past 2^32 and the span past it too
    for span, per in ((1 << 20, 4500), (10_000, 1), (30_000, 3333), ((1 << 32) + 10_000, 7000), ((1 << 33) - 2, 5000), (7, 10000)):
        d = -(-per * span // 10000)
        for n_del, cls in ((d, K.DELETED), (d - 1, None)):
            depth = span - n_del
            if depth >= 1 << 32 or n_del >= 1 << 32 or n_del < 0:
                continue
            got = V.cons_classify_counts(depth, 0, 0, 0, depth, n_del, 1, 1, per, ref)
            assert got == K.classify(depth, 0, 0, 0, depth, n_del, ref, 1, 1, per), (span, per, n_del)
            assert cls is None or got == (cls, "-")
            assert cls is not None or got[0] != K.DELETED or n_del == 0
    # the first among equals; a reference byte that is no base gives alt; the order of the table
    assert V.cons_classify_counts(5, 5, 0, 0, 10, 0, 1, 1, 1, ref) == (K.NO_CALL, "N")
    assert V.cons_classify_counts(7, 0, 0, 0, 10, 0, 1, 1, 1, ord("n")) == (K.ALT, "A")
    assert V.cons_classify_counts(7, 0, 0, 0, 10, 0, 1, 1, 1, ord("a")) == (K.REF, "A")
    assert V.cons_classify_counts(0, 0, 0, 0, 0, 9, 10, 1, 1, ref) == (K.LOW_DEPTH, "n")         # span below min_depth comes first
    assert V.cons_classify_counts(0, 0, 0, 0, 0, 10, 10, 1, 1, ref) == (K.DELETED, "-")
    assert V.cons_classify_counts(4, 0, 0, 0, 4, 6, 10, 7, 7000, ref) == (K.LOW_DEPTH, "n")      # spanned, the deletion not called
    assert V.cons_classify_counts(0, 0, 0, 0, 8, 0, 1, 1, 1, ref) == (K.NO_CALL, "N")            # N holds all of the depth
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 10001)):
        with pytest.raises(EngineError):
            V.cons_classify_counts(1, 0, 0, 0, 1, 0, *bad, ref)
    with pytest.raises(EngineError):
        V.cons_classify_counts(3, 3, 0, 0, 5, 0, 1, 1, 1, ref)                                  # a + c > depth


def kat_insertions(case):
    """The InsResult and the reference's list for the insertion rows of a case: one allele per listed insertion."""
    rows = [c for c in case["changes"] if c[2].startswith("ins")]
    cand = np.zeros(len(rows), INS_CANDIDATE)
    obs = []
    for i, (pos, _end, _kind, ref, seq, count, depth, _note) in enumerate(rows):
        cand[i]["pos"], cand[i]["ref"], cand[i]["ins"], cand[i]["depth"] = pos, ord(ref), count, depth
        key = [0, 0]
        for j, b in enumerate(seq):
            key[j // 16] |= "=ACMGRSVTWYHKDBN".index(b) << (60 - 4 * (j % 16))
        obs += [(pos, len(seq), key, 0, 0)] * count
    res = InsResult(start=0, end=case["contig_len"], low_depth=0, kept=case["contig_len"] - len(rows), inserted=len(rows), candidates=cand,
                    observations=np.array(obs, INS_OBS) if obs else np.zeros(0, INS_OBS))
    ref_list = [(pos, depth, [dict(pos=pos, len=len(seq), seq=seq, count=count)]) for pos, _e, _k, _r, seq, count, depth, _n in rows]
    return res, ref_list


@pytest.mark.parametrize("case", KAT, ids=[c["name"] for c in KAT])
def test_assembler_and_writers_on_the_hand_derived_cases(case, tmp_path):
    L = case["contig_len"]
    ref = np.frombuffer(case["ref"].encode(), np.uint8)
    cons = np.frombuffer(case["cons"].encode(), np.uint8)
    assert len(cons) == L and sum(case["counts"]) == L
    ins, ref_list = kat_insertions(case)
    want_changes = [tuple(c) for c in case["changes"]]
    # the reference's assembler reproduces the hand-derived FASTA and change list ...
    seq, changes = K.assemble(cons, ref, 0, ref_list, P["min_ins_count"], P["min_ins_per_10k"], case["fill"])
    assert K.expected_fasta("k", seq, 0, L, True) == case["fasta"] and changes == want_changes
    # ... and so does the library's
    asm = V.cons_assemble(cons, ref, 0, ins, P["min_depth"], P["min_ins_count"], P["min_ins_per_10k"], case["fill"])
    assert asm.seq == seq
    got = [(c["pos"], c["end"], c["kind"], c["ref"], c["cons"], c["count"] if c["kind"].startswith("ins") else None,
            c["depth"] if c["kind"].startswith("ins") else None, c["note"]) for c in asm.changes]
    assert got == want_changes
    fa, tsv = str(tmp_path / "o.fa"), str(tmp_path / "o.tsv")
    V.write_consensus(fa, "k", asm, 0, L, whole_contig=True)
    assert open(fa).read() == case["fasta"]
    n = case["counts"]
    res = ConsResult(start=0, end=L, low_depth=n[0], deleted=n[1], no_call=n[2], ref=n[3], alt=n[4], cons=cons)
    V.write_consensus_changes(tsv, "k", res, asm, P["min_depth"], P["min_quality"], P["min_del_count"], P["min_del_per_10k"], P["min_ins_count"],
                              P["min_ins_per_10k"], None, 0, case["fill"])
    assert open(tsv).read() == K.expected_changes("k", n, seq, want_changes, 0, L, P["min_depth"], P["min_quality"], None, 0, P["min_del_per_10k"],
                                                  P["min_del_count"], P["min_ins_per_10k"], P["min_ins_count"], case["fill"])


def one_allele(pos, seq_codes, count, depth, length=None):
    length = len(seq_codes) if length is None else length
    cand = np.zeros(1, INS_CANDIDATE)
    cand[0]["pos"], cand[0]["ref"], cand[0]["ins"], cand[0]["depth"] = pos, ord("A"), count, depth
    key = [0, 0]
    for j, c in enumerate(seq_codes[:32]):
        key[j // 16] |= c << (60 - 4 * (j % 16))
    obs = np.array([(pos, length, key, 0, 0)] * count, INS_OBS)
    return InsResult(start=0, end=10, low_depth=0, kept=9, inserted=1, candidates=cand, observations=obs)


def test_assembler_skips_long_and_unsupported_alleles_and_writes_other_codes_as_n():
    ref = np.frombuffer(b"ACGTACGTAC", np.uint8)
    cons = ref.copy()
    # 33 bases: too long for the key; 32 bases are spliced
    asm = V.cons_assemble(cons, ref, 0, one_allele(3, [1] * 32, 5, 5, length=33), 3, 3, 7000)
    assert asm.seq == "ACGTACGTAC" and [(c["kind"], c["note"]) for c in asm.changes] == [("ins_skipped", "too_long")] and asm.insertions_skipped == 1
    asm = V.cons_assemble(cons, ref, 0, one_allele(3, [1] * 32, 5, 5), 3, 3, 7000)
    assert asm.seq == "ACG" + "A" * 32 + "TACGTAC" and asm.insertions == 1 and asm.changes[0]["count"] == 5
    # the position is called (ins 5 of depth 6) but its top allele has 3 of them: 3 / 6 is below 0.7
    res = one_allele(3, [2, 4], 3, 6)
    other = one_allele(3, [8], 2, 6)
    res.candidates["ins"] = 5
    res.observations = np.concatenate([res.observations, other.observations])
    asm = V.cons_assemble(cons, ref, 0, res, 3, 3, 7000)
    assert asm.seq == "ACGTACGTAC" and [(c["kind"], c["note"], c["cons"], c["count"]) for c in asm.changes] == [("ins_skipped", "no_allele", "CG", 3)]
    assert K.assemble(cons, ref, 0, [(3, 6, [dict(len=2, seq="CG", count=3)])], 3, 7000)[1] == [(3, 3, "ins_skipped", "G", "CG", 3, 6, "no_allele")]
    # codes outside A C G T become N: = (0), N (15), R (5)
    asm = V.cons_assemble(cons, ref, 0, one_allele(10, [0, 1, 15, 5, 8], 4, 4), 3, 3, 7000)
    assert asm.seq == "ACGTACGTAC" + "NANNT" and asm.changes[0]["cons"] == "NANNT"
    # a candidate outside the range, a byte outside the alphabet
    with pytest.raises(EngineError):
        V.cons_assemble(cons, ref, 0, one_allele(11, [1], 4, 4), 3, 3, 7000)
    with pytest.raises(EngineError):
        V.cons_assemble(np.frombuffer(b"ACGTXCGTAC", np.uint8), ref, 0)


def test_deletion_runs_regions_and_line_width(tmp_path):
    ref = np.frombuffer(("ACGT" * 40).encode(), np.uint8)
    text = "AC" + "-" * 64 + "GT" + "-" * 65 + "T" + "n" * 5 + "-"
    start = 17
    cons = np.frombuffer(text.encode(), np.uint8)
    asm = V.cons_assemble(cons, ref, start, fill="ref")
    seq, changes = K.assemble(cons, ref, start, fill="ref")
    assert asm.seq == seq and asm.deletions == 3 and len(seq) == 10
    got = [(c["pos"], c["end"], c["kind"], c["ref"], c["cons"]) for c in asm.changes]
    assert got == [c[:5] for c in changes]
    dels = [c for c in got if c[2] == "del"]
    assert [(d[0], d[1]) for d in dels] == [(start + 3, start + 66), (start + 69, start + 133), (start + 140, start + 140)]
    assert len(dels[0][3]) == 64 and dels[1][3] == "." and dels[2][3] == bytes(ref[start + 139:start + 140]).decode()
    fa = str(tmp_path / "o.fa")
    for width in (1, 3, 10, 60):
        V.write_consensus(fa, "chrM", asm, start, start + len(text), line_width=width)
        assert open(fa).read() == K.expected_fasta("chrM", seq, start, start + len(text), False, width)
    assert open(fa).read().startswith(f">chrM:{start + 1}-{start + len(text)}\n")
    V.write_consensus(fa, "chrM", asm, 0, 160, whole_contig=True)
    assert open(fa).read() == ">chrM\n" + seq + "\n"
    with pytest.raises(EngineError):
        V.write_consensus(fa, "chrM", asm, 0, 160, line_width=0)
    empty = V.cons_assemble(np.zeros(0, np.uint8), ref, 5)
    V.write_consensus(fa, "chrM", empty, 5, 5)
    assert empty.seq == "" and empty.changes == [] and open(fa).read() == ">chrM:6-5\n"


def cli(tmp_path, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="9999")                  # no device can be opened
    return subprocess.run([_b.CLI, "consensus", str(tmp_path / "none.bam"), "-r", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.fa")]
                          + list(args), capture_output=True, text=True, env=env)


@pytest.mark.parametrize("args,msg", [
    ([], "consensus needs '-L <CONTIG>'"),
    (["-L", "chrM", "--region", "5"], "invalid value '5' for '--region'"),
    (["-L", "chrM", "--region", "9-5"], "invalid value '9-5' for '--region'"),
    (["-L", "chrM", "--region", "a-b"], "for '--region'"),
    (["-L", "chrM", "--min-del-fraction", "0"], "invalid value '0' for '--min-del-fraction'"),
    (["-L", "chrM", "--min-del-fraction", "1.0001"], "invalid value '1.0001' for '--min-del-fraction'"),
    (["-L", "chrM", "--min-ins-fraction=1.5"], "invalid value '1.5' for '--min-ins-fraction'"),
    (["-L", "chrM", "--min-ins-fraction", "x"], "invalid value 'x' for '--min-ins-fraction'"),
    (["-L", "chrM", "--min-del-count", "0"], "invalid value '0' for '--min-del-count'"),
    (["-L", "chrM", "--min-ins-count=0"], "invalid value '0' for '--min-ins-count'"),
    (["-L", "chrM", "--fill", "n"], "invalid value 'n' for '--fill'"),
    (["-L", "chrM", "--fill=reference"], "invalid value 'reference' for '--fill'"),
    (["-L", "chrM", "--line-width", "0"], "invalid value '0' for '--line-width'"),
    (["-L", "chrM", "--line-width", "-3"], "invalid value '-3' for '--line-width'"),
    (["-L", "chrM", "--min-base-quality", "256"], "invalid value '256' for '--min-base-quality'"),
    (["-L", "chrM", "--min-base-quality", "q"], "invalid value 'q' for '--min-base-quality'"),
    (["-L", "chrM", "--exclude-flags", "0x10000"], "invalid value '0x10000' for '--exclude-flags'"),
    (["-L", "chrM", "--exclude-flags", "dup"], "invalid value 'dup' for '--exclude-flags'"),
    (["-L", "chrM", "--min-depth", "0"], "invalid value '0' for '--min-depth'"),
    (["-L", "chrM", "--min-del-per-strand", "2"], "unexpected argument '--min-del-per-strand'"),
])
def test_cli_argument_errors_exit_2_before_a_device_is_opened(tmp_path, args, msg):
    r = cli(tmp_path, *args)
    assert r.returncode == 2, r.stderr
    assert msg in r.stderr, r.stderr


def test_cli_accepts_well_formed_values_and_names_the_subcommand(tmp_path):
    """The argument check passes: the run then fails on the missing BAM with exit 1, not 2, still without a device."""
    for args in (["-L", "chrM"], ["-L", "chrM", "--fill", "ref", "--line-width=80", "--changes", str(tmp_path / "c.tsv")],
                 ["-L", "chrM", "--region=5-6", "--exclude-flags", "0x704", "--min-base-quality", "0", "--min-del-fraction=.0001", "--min-ins-fraction", "1",
                  "--min-del-count=1", "--min-ins-count", "7", "--fill=N"]):
        r = cli(tmp_path, *args)
        assert r.returncode == 1 and "invalid value" not in r.stderr, (args, r.stderr)
    r = subprocess.run([_b.CLI, "--help"], capture_output=True, text=True)
    assert "dut-coverage consensus" in r.stdout + r.stderr and "--fill N|ref" in r.stdout + r.stderr
    r = subprocess.run([_b.CLI, "consensus", "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "consensus" in r.stderr


def test_a_context_without_a_device_answers_a_device_error():
    with HostStage(CallableOptions()) as h:
        with pytest.raises(EngineError) as e:
            h.site_scan_consensus(20, 10, 3, 7000, np.frombuffer(b"ACGT", np.uint8))
        assert e.value.status == -2
