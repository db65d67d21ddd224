"""Recorded results of the compiled reference for tests/test_oracle.py (TEST INFRASTRUCTURE, build container only).

Runs oracle/_ref/libssw_ref.so (the reference's ssw.c, built by oracle/Makefile) over
* the 600 random pairs of test_port_vs_compiled_reference_random (tests/test_oracle.py: random_pair_cases), every result kept, and
* the first 2000 reads of the SURVEY 8d dataset at (3,2,3,1) through the threaded harness (test_dataset_checksum_sample): the sums,
so that both tests hold the port against the reference on machines without that build.  Only inputs' seeds and outputs are written.

    python oracle/gen_reference_runs_golden.py        -> tests/golden/reference_runs.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O                   # noqa: E402
from tests.test_oracle import random_pair_cases  # noqa: E402


def main():
    O.build()
    if not O.have_reference():
        raise SystemExit("oracle/_ref/libssw_ref.so is not built (oracle/Makefile needs the reference sources)")
    ref = O.Backend("reference")
    seed, n = 7, 600
    expect = [ref.align(r, w, O.dna_matrix(ms, mm), go, ge) for r, w, ms, mm, go, ge in random_pair_cases(n, seed)]
    from indelpost_amd import synth
    jobs = synth.config2_jobs(2000)
    _, chk, ops = ref.cpu_baseline(jobs.reads, jobs.read_off, jobs.refs, jobs.ref_off, jobs.ref_id, jobs.gap_open, jobs.gap_ext,
                                   O.dna_matrix(3, 2), 4)
    out = {"source": "oracle/_ref/libssw_ref.so (the reference's ssw.c), oracle/gen_reference_runs_golden.py",
           "random_pairs": {"seed": seed, "n": n, "expect": expect},
           "checksum_sample": {"n": 2000, "scoring": [3, 2, 3, 1], "sum_score1": int(chk), "sum_cigar_len": int(ops)}}
    path = os.path.join(ROOT, "tests", "golden", "reference_runs.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
