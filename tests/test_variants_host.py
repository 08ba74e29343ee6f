"""find-variants, the parts that need no GPU: the per-position classification in plain C++ (the f64 rule of
caller.rs:132-149, which the device's integer test `10 m >= 7 depth` is held against), the annotation of candidates
against a haplogroup tree, the TSV, the command line's argument errors and the refusal of a host-only context."""
import json
import os
import subprocess

import numpy as np
import pytest

from decodingustools_amd import build as _b, haplogroup as H, variants as V
from decodingustools_amd.callable_loci import SCAN_CANDIDATE, CallableOptions, EngineError, HostStage, ScanResult
from oracle import haplogroup_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CODE = O.CODE


def oracle_class(hist, ref_byte, min_depth):
    """The class of one position from oracle.haplogroup_oracle.call_sites (caller.rs:132-149) and the issue's definitions."""
    calls = O.call_sites([1], [True], [hist], min_depth)
    depth = int(sum(int(x) for x in hist))
    if depth < min_depth:
        return V.LOW_DEPTH, ""
    if 1 not in calls:
        return V.MIXED, ""
    base = calls[1][0]
    rb = chr(ref_byte).upper()
    if base not in "ACGT" or rb not in "ACGT":
        return V.UNCOMPARABLE, base
    return (V.MATCH if base == rb else V.VARIANT), base


def hist_of(**kw):
    h = np.zeros(16, np.uint32)
    for k, v in kw.items():
        h[CODE.index(k) if k != "EQ" else 0] = v
    return h


CRAFTED = [
    # the exact boundary: 7/10, 70/100, 2.8e9 / 4e9 are called
    (hist_of(G=7, A=3), "A", 10, V.VARIANT), (hist_of(G=70, A=30), "G", 10, V.MATCH),
    (hist_of(T=2_800_000_000, C=1_200_000_000), "C", 10, V.VARIANT),
    # one below and one above it
    (hist_of(C=699, A=301), "A", 10, V.MIXED), (hist_of(C=701, A=299), "A", 10, V.VARIANT),
    # the nearest neighbours of 7/10 at depth 2^32 - 1: ceil(0.7 * depth) = 3006477107 is called, one less is not
    (hist_of(A=3006477107, G=4294967295 - 3006477107), "G", 10, V.VARIANT),
    (hist_of(A=3006477106, G=4294967295 - 3006477106), "G", 10, V.MIXED),
    # depth == min_depth - 1, and just deep enough
    (hist_of(A=9), "C", 10, V.LOW_DEPTH), (hist_of(A=10), "C", 10, V.VARIANT), (hist_of(), "A", 1, V.LOW_DEPTH),
    # a majority of code 15 (N) and of code 0 (=): a call, but of nothing comparable
    (hist_of(N=9, A=1), "A", 10, V.UNCOMPARABLE), (hist_of(EQ=10), "A", 10, V.UNCOMPARABLE), (hist_of(M=8, A=2), "A", 10, V.UNCOMPARABLE),
    # codes outside A/C/G/T that share 0.7 between them: no call
    (hist_of(N=4, EQ=4, A=2), "A", 10, V.MIXED),
    # reference n / N / an IUPAC code: called, not comparable; lower-case acgt compares as upper case
    (hist_of(A=10), "n", 10, V.UNCOMPARABLE), (hist_of(A=10), "N", 10, V.UNCOMPARABLE), (hist_of(A=10), "R", 10, V.UNCOMPARABLE),
    (hist_of(A=10), "y", 10, V.UNCOMPARABLE), (hist_of(A=10), "a", 10, V.MATCH), (hist_of(T=10), "c", 10, V.VARIANT),
    (hist_of(G=10), "g", 10, V.MATCH), (hist_of(C=12, T=1), "t", 10, V.VARIANT),
]


@pytest.mark.parametrize("i", range(len(CRAFTED)))
def test_classify_crafted_histograms(i):
    hist, ref, min_depth, want = CRAFTED[i]
    exp = oracle_class(hist, ord(ref), min_depth)
    assert exp[0] == want, "the test's own expectation disagrees with the oracle"
    assert V.scan_classify(hist, ref, min_depth) == exp
    # the five counters say the same wherever they can say anything
    c5 = np.array([hist[1], hist[2], hist[4], hist[8], min(int(hist.sum()), 0xFFFFFFFF)], np.uint32)
    got5 = V.scan_classify_counts(c5, ref, min_depth)
    other = int(hist.sum()) - int(c5[:4].sum())
    if int(hist.sum()) >= min_depth and other / max(int(hist.sum()), 1) >= 0.7:
        assert got5 == (V.UNDETERMINED, "")
    else:
        assert got5 == exp


def test_integer_rule_equals_f64_rule():
    """10 * m >= 7 * depth (the device's test) against m as f64 / depth as f64 >= 0.7 (caller.rs:139-141, what
    dut_scan_classify and dut_call_sites compute) for 10 000 random pairs, the multiples of 10 around the boundary included."""
    rng = np.random.default_rng(17)
    depth = np.concatenate([rng.integers(1, 2 ** 32, 4000), rng.integers(1, 2000, 3000), rng.integers(1, 2 ** 32 // 10, 3000) * 10])
    m = np.empty_like(depth)
    near = rng.random(depth.shape[0]) < 0.7
    edge = -(-7 * depth // 10)                                   # ceil(0.7 depth): the smallest called count
    m[near] = np.clip(edge[near] + rng.integers(-2, 3, int(near.sum())), 0, depth[near])
    m[~near] = (rng.random(int((~near).sum())) * (depth[~near] + 1)).astype(np.int64)
    m = np.minimum(m, depth)
    n_called = 0
    for mi, di in zip(m.tolist(), depth.tolist()):
        integer = 10 * mi >= 7 * di
        assert integer == (mi / di >= 0.7), (mi, di)
        hist = np.zeros(16, np.uint32); hist[2] = mi; hist[8 if 2 * mi != di else 15] = di - mi
        if mi * 2 <= di:                                         # the other code is the larger one: its own ratio decides
            integer = 10 * (di - mi) >= 7 * di
        cls, _ = V.scan_classify(hist, "A", 1)
        assert (cls in (V.VARIANT, V.MATCH, V.UNCOMPARABLE)) == integer, (mi, di, cls)
        n_called += integer
    assert 2000 < n_called < 8000


def kat_tree():
    kat = json.load(open(os.path.join(GOLDEN, "haplogroup_kat.json")))
    return kat["tree"], kat["build_id"]


def cand(rows):
    c = np.zeros(len(rows), SCAN_CANDIDATE)
    for i, (pos, ref, alt, a, cc, g, t, depth) in enumerate(rows):
        c[i] = (pos, ord(ref), ord(alt), (0, 0), a, cc, g, t, depth)
    return c


def test_annotation_against_the_kat_tree():
    tree, build = kat_tree()
    # a second locus at position 100 (named to sort in front of a1) in another node
    tree = json.loads(json.dumps(tree))
    tree["allNodes"]["5"]["variants"].append({"variant": "Z0", "position": 100, "ancestral": "G", "derived": "T"})
    t = H.HaplogroupTree(json.dumps(tree))
    c = cand([(100, "A", "G", 0, 0, 20, 0, 20),          # a1 derived G; Z0 ancestral G
              (110, "T", "C", 0, 18, 0, 0, 18),          # a2: C is its ancestral allele
              (200, "G", "T", 0, 0, 0, 25, 25),          # b1 G>A: T is neither
              (205, "G", "T", 0, 0, 0, 25, 25),          # off the tree
              (400, "G", "T", 0, 0, 0, 12, 12)])         # x1 derived
    got = V.annotate_variants(t, build, "chrY", c)
    assert got == [(True, "Z0,a1", "ancestral,derived"), (True, "a2", "ancestral"), (True, "b1", "other"), (False, "", ""),
                   (True, "x1", "derived")]
    # the same candidates on another chromosome or another build: the tree knows none of them
    assert V.annotate_variants(t, build, "Y", c) == [(False, "", "")] * 5
    assert V.annotate_variants(t, "GRCh37", "chrY", c) == [(False, "", "")] * 5
    # agreement with the oracle's tree loader and its notion of "relevant" (collect_snps + the chromosome test)
    _, ot = O.load_tree(json.dumps(tree), "ftdna")
    sites, rel = O.sites_and_relevance(ot, build, "chrY")
    known = {p for p, r in zip(sites, rel) if r}
    assert [g[0] for g in got] == [int(p) in known for p in c["pos"]]
    # a DecodingUs tree: GRCh37 coordinates live on "Y", GRCh38 ones on "chrY"; an indel locus is not a SNP
    dus = [dict(name="R", parentName=None, variants=[], lastUpdated="x", isBackbone=True),
           dict(name="A", parentName="R", lastUpdated="x", isBackbone=False, variants=[
               dict(name="s1", variantType="SNP", coordinates={"CM000686.1": dict(start=100, stop=100, anc="A", der="G"),
                                                               "CM000686.2": dict(start=150, stop=150, anc="A", der="G")}),
               dict(name="i1", variantType="INDEL", coordinates={"CM000686.2": dict(start=205, stop=206, anc="G", der="T")})])]
    td = H.HaplogroupTree(json.dumps(dus), provider=H.DECODINGUS)
    assert [g[0] for g in V.annotate_variants(td, "GRCh37", "Y", c)] == [True, False, False, False, False]
    assert [g[0] for g in V.annotate_variants(td, "GRCh37", "chrY", c)] == [False] * 5
    assert [g[0] for g in V.annotate_variants(td, "GRCh38", "chrY", c)] == [False] * 5
    assert V.annotate_variants(td, "GRCh38", "chrY", cand([(150, "A", "G", 0, 0, 9, 0, 9)])) == [(True, "s1", "derived")]
    assert V.annotate_variants(t, build, "chrY", cand([])) == []


def hand_result():
    c = cand([(100, "A", "G", 1, 0, 19, 0, 20), (110, "T", "C", 0, 18, 0, 0, 18), (205, "G", "T", 2, 0, 1, 7, 10),
              (400, "G", "T", 0, 0, 3, 9, 13)])
    return ScanResult(start=50, end=450, low_depth=30, mixed=2, uncomparable=5, match=359, variant=4, candidates=c)


def test_tsv_byte_for_byte(tmp_path):
    tree, build = kat_tree()
    t = H.HaplogroupTree(json.dumps(tree))
    res = hand_result()
    assert res.low_depth + res.mixed + res.uncomparable + res.match + res.variant == res.end - res.start
    out = str(tmp_path / "v.tsv")
    V.write_variants(out, "chrY", res, 10, 20, tree=t, build_id=build)
    want = open(os.path.join(GOLDEN, "variants_kat.tsv"), "rb").read()
    assert open(out, "rb").read() == want
    # without a tree: the same lines with '.' in the last three columns
    V.write_variants(out, "chrY", res, 10, 20)
    lines = want.decode().split("\n")
    plain = [l if l.startswith("#") or not l else "\t".join(l.split("\t")[:10] + [".", ".", "."]) for l in lines]
    assert open(out).read() == "\n".join(plain)
    # the frequency column is alt count / depth in f64, four decimals
    assert [l.split("\t")[9] for l in lines if l and not l.startswith("#")] == ["%.4f" % f for f in (19 / 20, 18 / 18, 7 / 10, 9 / 13)]


def run(*args):
    return subprocess.run([_b.CLI] + list(args), capture_output=True, text=True)


ARGUMENT_ERRORS = {
    "no -L": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv"],
    "no -o": ["find-variants", "x.bam", "-r", "x.fa", "-L", "chrY"],
    "no -r": ["find-variants", "x.bam", "-o", "o.tsv", "-L", "chrY"],
    "region without a dash": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--region", "100"],
    "region not a number": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--region", "a-b"],
    "region negative": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--region=-5-10"],
    "region empty": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--region", "100-100"],
    "region backwards": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--region", "200-100"],
    "provider without tree": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--provider", "ftdna"],
    "tree type without tree": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--tree-type", "mt"],
    "bad provider": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--tree", "t.json", "--provider", "nope"],
    "min depth 0": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--min-depth", "0"],
    "min depth not a number": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--min-depth", "ten"],
    "min quality too large": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--min-quality", "256"],
    "unknown flag": ["find-variants", "x.bam", "-r", "x.fa", "-o", "o.tsv", "-L", "chrY", "--show-snps"],
}


@pytest.mark.parametrize("name", sorted(ARGUMENT_ERRORS))
def test_cli_argument_errors_leave_with_2_before_any_device(name):
    _b.build()
    r = run(*ARGUMENT_ERRORS[name])
    assert r.returncode == 2, (name, r.stderr)
    assert r.stderr.strip() and "hip" not in r.stderr.lower() and "device" not in r.stderr.lower().replace("--device", "")
    assert not os.path.exists("o.tsv")


def test_cli_usage_names_the_subcommand():
    _b.build()
    r = run("--help")
    assert r.returncode == 0 and "find-variants <BAM_FILE>" in r.stderr
    r = run("find-variants", "--help")
    assert r.returncode == 0 and "--region START-END" in r.stderr


def test_host_only_context_has_no_scan():
    ref = np.frombuffer(b"ACGTACGTAC", np.uint8)
    with HostStage(CallableOptions()) as h:
        with pytest.raises(EngineError) as e:
            h.site_scan(20, 10, ref)
        assert e.value.status == -2 and "host-only" in str(e.value)
        with pytest.raises(EngineError) as e:
            h.site_scan_counts(20, 0, 10)
        assert e.value.status == -2
