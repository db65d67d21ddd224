"""Golden vectors for complex-variant decomposition and the target selection that follows it (TEST INFRASTRUCTURE, CPU only).

Writes tests/golden/decompose_cases.json.  Never imported by the package, never run on a GPU machine.  Like the generators under
oracle/ (whose loaders it imports: nothing under oracle/ changes), it reads the reference's own TEXT at generation time and
executes it against an in-memory FASTA duck type:
  * the Variant class body (variant.pyx, via oracle/gen_variant_golden.load), so decompose_complex_variant runs as written;
  * findall_indels, make_insertion_first and merge_consecutive_gaps (oracle/gen_decoder_golden.function_text);
  * the target selection of VariantAlignment.__cinit__ (varaln.pyx:122-143), cut out between
    `self.target, second_target = target, target` and `self.bam = bam` and run with a plain object as `self`.
make_aligner / align are bound to the compiled reference (oracle/_ref/libssw_ref.so, built by oracle.build()) when it exists and
to the oracle's port otherwise; the file records which, and the gap pair of every alignment.  Every alignment made is checked to
have flag 0 and a CIGAR (the package's one defined deviation, a flag-1 traceback without CIGAR, cannot occur on these inputs).
Only data is written.

    python tools/gen_decompose_golden.py
"""
import collections
import json
import os
import sys
import textwrap
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O                                                      # noqa: E402
sys.path.append(os.path.join(ROOT, "oracle"))            # (the generators' loaders, imported as modules of their own)
from gen_decoder_golden import REF, function_text, strip_cython_types              # noqa: E402
from gen_variant_golden import Fasta, load as load_variant_text                    # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "decompose_cases.json")
Alignment = collections.namedtuple("Alignment", "CIGAR optimal_score sub_optimal_score reference_start reference_end read_start read_end")
DECOMPOSE_GAPS = [None, (3, 1), (5, 1)]                  # None: the method's defaults (4, 0)
TARGET_SETTINGS = [(True, 3, 1), (False, 3, 1), (False, 5, 1)]   # (auto_adjust_extension_penalty, gap_open, gap_ext)


class Aligners:
    """make_aligner / align of localn.pyx:464-472 on the compiled reference (or the port): SSW(match, mismatch) with setReference,
    setRead, align(gap_open, gap_extension) -- flag 1, filters 0, mask max(15, len // 2), score size 2 (sswpy.pyx:199-225)"""

    def __init__(self):
        O.build()
        self.kind = "reference" if O.have_reference() else "port"
        self.backend = O.Backend(self.kind)
        self.log = []

    def make_aligner(self, ref_seq, match_score, mismatch_penalty):
        return (ref_seq, O.dna_matrix(match_score, mismatch_penalty))

    def align(self, aligner, read_seq, gap_open_penalty, gap_extension_penalty):
        ref_seq, mat = aligner
        e = self.backend.align(O.encode(read_seq), O.encode(ref_seq), mat, gap_open_penalty, gap_extension_penalty)
        if e is None:
            raise ValueError("Problem Running alignment, see stdout")
        assert e["flag"] == 0 and e["cigar"] is not None, ("flag-1 traceback / no CIGAR on a decomposition job", read_seq, ref_seq, e)
        self.log.append([int(gap_open_penalty), int(gap_extension_penalty)])
        return Alignment(O.cigar_string(e["cigar"]), e["score1"], e["score2"], e["ref_begin1"], e["ref_end1"], e["read_begin1"], e["read_end1"])


def selection_function(ns):
    """varaln.pyx:122-143 as a function of (self, target, scoring, gaps); returns (target, second_target, is_complex_input)"""
    src = open(os.path.join(REF, "varaln.pyx")).read().split("\n")
    a = next(i for i, l in enumerate(src) if l.strip() == "self.target, second_target = target, target")
    b = next(i for i, l in enumerate(src) if i > a and l.strip() == "self.bam = bam")
    body = textwrap.indent(textwrap.dedent("\n".join(src[a:b])), "    ")
    text = ("def _select(self, target, match_score, mismatch_penalty, gap_open_penalty, gap_extension_penalty, auto_adjust_extension_penalty):\n"
            + body + "\n    return self.__target, second_target, is_complex_input\n")
    exec(compile(text, "<varaln:122-143>", "exec"), ns)
    return ns["_select"]


def vt(v):
    return [v.chrom, v.pos, v.ref, v.alt]


def synthetic_genome(rng, n):
    """upper-case random sequence with soft-masked (lower-case) stretches, N runs, a few IUPAC letters and short repeats"""
    g = list("".join("ACGT"[int(x)] for x in rng.integers(0, 4, n)))
    for _ in range(30):                                    # tandem repeats: indels that shift
        p = int(rng.integers(0, n - 40))
        unit = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(1, 4))))
        rep = unit * int(rng.integers(3, 9))
        g[p:p + len(rep)] = list(rep)
    masked = []
    for _ in range(25):                                    # soft-masked stretches
        p, L = int(rng.integers(0, n - 600)), int(rng.integers(150, 600))
        g[p:p + L] = [c.lower() for c in g[p:p + L]]
        masked.append((p, p + L))
    for _ in range(6):                                     # N runs
        p, L = int(rng.integers(400, n - 100)), int(rng.integers(5, 60))
        g[p:p + L] = ["N"] * L
    for _ in range(40):                                    # IUPAC letters
        g[int(rng.integers(0, n))] = "RYSWKMBDHV"[int(rng.integers(0, 10))]
    return "".join(g), masked


def main():
    ns = load_variant_text()                               # variant.pyx executed as text (oracle/gen_variant_golden.py)
    for n in ("merge_consecutive_gaps", "make_insertion_first"):
        exec(compile(strip_cython_types(function_text(os.path.join(REF, "utilities.pyx"), n)), "<utilities:%s>" % n, "exec"), ns)
    exec(compile(strip_cython_types(function_text(os.path.join(REF, "localn.pyx"), "findall_indels")), "<localn:findall_indels>", "exec"), ns)
    al = Aligners()
    ns["make_aligner"], ns["align"] = al.make_aligner, al.align
    select = selection_function(ns)
    Variant = ns["Variant"]

    rng = np.random.default_rng(20261016)
    genome, masked = synthetic_genome(rng, 24000)
    fa = Fasta({"chr1": genome})
    rs = lambda k: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, k))       # noqa: E731
    cases = []
    for k in range(330):
        if k % 15 == 0:
            pos = int(rng.integers(2, 110))                # within 110 bp of the contig start
        elif k % 3 == 0:
            a, b = masked[int(rng.integers(0, len(masked)))]
            pos = int(rng.integers(a + 2, b - 12))         # inside a soft-masked stretch
        else:
            pos = int(rng.integers(2, len(genome) - 200))
        kind = k % 10
        if kind < 6:                                       # complex indel: ref and alt of different lengths, unequal first bases
            r_len, a_len = int(rng.integers(1, 9)), int(rng.integers(1, 9))
            if r_len == a_len:
                a_len += 1
            ref = genome[pos - 1:pos - 1 + r_len]
            alt = rs(a_len)
        elif kind < 8:                                     # MNV
            n = int(rng.integers(2, 6))
            ref, alt = genome[pos - 1:pos - 1 + n], rs(n)
        elif kind == 8:                                    # SNV
            ref, alt = genome[pos - 1], rs(1)
        else:                                              # simple indel (non-complex: not aligned)
            base = genome[pos - 1]
            ref, alt = (base, base + rs(int(rng.integers(1, 5)))) if rng.random() < 0.5 else (genome[pos - 1:pos + int(rng.integers(1, 5))], base)
        if k % 3 == 0 and rng.random() < 0.7:
            alt = alt.upper()                              # upper-case alt over a soft-masked reference
        try:
            v = Variant("chr1", pos, ref, alt, fa)
        except ValueError:
            continue
        cases.append({"in": ["chr1", pos, ref, alt], "skip_validation": False})
    # inputs the per-variant code raises on, recorded with the exception type
    cases.append({"in": ["chr2", 500, "ACG", "T"], "skip_validation": True})         # unknown contig
    cases.append({"in": ["chr1", 3, genome[2:8], "G"], "skip_validation": False})    # a deletion at the contig start

    for c in cases:
        chrom, pos, ref, alt = c["in"]
        v = Variant(chrom, pos, ref, alt, fa, skip_validation=c["skip_validation"])
        c["decompose"], c["targets"], c["gaps_used"], c["target_gaps_used"] = [], [], [], []
        for gaps in DECOMPOSE_GAPS:
            del al.log[:]
            try:
                got = v.decompose_complex_variant() if gaps is None else v.decompose_complex_variant(3, 2, *gaps)
                c["decompose"].append({"out": [vt(x) for x in got]})
            except Exception as e:                         # (the type is what is pinned)
                c["decompose"].append({"raises": type(e).__name__})
            c["gaps_used"].append([list(g) for g in al.log])
        for auto, go, ge in TARGET_SETTINGS:
            del al.log[:]
            try:
                t, st, cx = select(types.SimpleNamespace(), v, 3, 2, go, ge, auto)
                c["targets"].append({"out": [vt(t), vt(st), bool(cx)]})
            except Exception as e:
                c["targets"].append({"raises": type(e).__name__})
            c["target_gaps_used"].append([list(g) for g in al.log])

    out = {"generator": "tools/gen_decompose_golden.py", "aligner": al.kind, "genome": {"chr1": genome},
           "scoring": [3, 2], "decompose_gaps": [list(g) if g else None for g in DECOMPOSE_GAPS],
           "target_settings": [list(s) for s in TARGET_SETTINGS], "cases": cases}
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    n_al = sum(len(g) for c in cases for g in c["gaps_used"] + c["target_gaps_used"])
    n_raise = sum("raises" in d for c in cases for d in c["decompose"] + c["targets"])
    print(len(cases), "cases,", n_al, "alignments on the", al.kind, "aligner,", n_raise, "raising calls,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
