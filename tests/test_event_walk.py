"""The event pass's per-job walk (indelpost_amd/csrc/ipx_events.h), compiled for the host with g++ (tests/events_host.py) -- the same
function the device kernels run -- against the reference's own decoders: the CIGAR rewrites and findall_indels vectors of
tests/golden/decoder_cases.json (oracle/gen_decoder_golden.py) and the letters known answer of the batched-decomposition issue."""
import json
import os

import numpy as np
import pytest

from indelpost_amd.cigar import cigar_tokens, findall_indels
from indelpost_amd.events import dicts_from_events
from tests import events_host as H
from tests.conftest import GOLDEN

@pytest.fixture(scope="module")
def decoder_cases():
    with open(os.path.join(GOLDEN, "decoder_cases.json")) as f:
        return json.load(f)


def _spans(cigarstring):
    toks = cigar_tokens(cigarstring)
    return sum(n for n, op in toks if op != "D"), sum(n for n, op in toks if op != "I")


def _aln(a):
    from indelpost_amd.sswpy import Alignment
    return Alignment(*a)


def test_cigar_rewrites_give_the_tokens_of_make_insertion_first(decoder_cases):
    cases = decoder_cases["cigar"]
    assert len(cases) == 300
    for c in cases:
        read_len, ref_len = _spans(c["cigar"])
        ev = H.walk(H.cigar_ops(c["cigar"]), 0, 0, None, None, read_len, ref_len)
        want, ri, qi = [], 0, 0
        for n, op in cigar_tokens(c["insertion_first"]):     # the reference's rewrite, walked as findall_indels walks it
            if op in "ID":
                want.append((op, n, ri, qi))
            if op == "I":
                qi += n
            elif op == "D":
                ri += n
            else:
                ri, qi = ri + n, qi + n
        got = [(k.decode(), n, r, q) for k, n, r, q in zip(ev["kind"].tolist(), ev["len"].tolist(), ev["ref_idx"].tolist(), ev["read_idx"].tolist())]
        assert got == want, c["cigar"]


def _read_end(aln):
    return aln.read_start + sum(n for n, op in cigar_tokens(aln.CIGAR) if op != "D")


def test_findall_indels_cases_rebuilt_from_events(decoder_cases):
    cases = decoder_cases["findall_indels"]
    assert len(cases) == 160
    for c in cases:
        aln = _aln(c["aln"])
        ops = H.cigar_ops(aln.CIGAR)
        ev = H.walk(ops, aln.reference_start, aln.read_start, c["read_seq"], c["ref_seq"])
        ev_indels = H.walk(ops, aln.reference_start, aln.read_start, None, None, len(c["read_seq"]), len(c["ref_seq"]))
        assert ev_indels.tolist() == ev[ev["kind"] != b"X"].tolist()
        args = (aln.reference_start, aln.read_start, _read_end(aln), c["genome_aln_pos"], c["ref_seq"], c["read_seq"])
        with_snvs = dicts_from_events(ev, *args, report_snvs=True, basequals=c["basequals"])
        without = dicts_from_events(ev_indels, *args, report_snvs=False, basequals=c["basequals"])
        expect = c["expect"]
        if c["report_snvs"]:
            assert [list(with_snvs[0]), list(with_snvs[1])] == expect
            assert without == expect[0]
        else:
            assert without == expect
            assert with_snvs[0] == expect
            # the snvs of a case recorded without them: the host decoder (pinned by the report_snvs cases of the same file)
            assert with_snvs[1] == findall_indels(aln, c["genome_aln_pos"], c["ref_seq"], c["read_seq"], True, c["basequals"])[1]
        for d in (with_snvs[0] + without):                    # key order as the reference builds the dicts
            assert list(d)[:3] == ["pos", "lt_ref", "lt_flank"] and list(d)[-2:] == ["lt_clipped", "rt_clipped"]


WINDOW = "acgtacgttgacctagcatgcatgcaatcgatcgtagctagctagcatcga"
READ = WINDOW[:20] + "GGTT" + WINDOW[23:]


def test_letters_known_answer():
    """soft-masked window, upper-case read: two of the four mismatches exist only because of case (the codes fold it)"""
    aln = _aln(["19M1I32M", 139, 0, 0, len(WINDOW) - 1, 0, len(READ) - 1])
    ev = H.walk(H.cigar_ops(aln.CIGAR), 0, 0, READ, WINDOW)
    assert [(k.decode(), r, q, n) for k, r, q, n in zip(ev["kind"].tolist(), ev["ref_idx"].tolist(), ev["read_idx"].tolist(), ev["len"].tolist())] == \
        [("I", 19, 19, 1), ("X", 19, 20, 1), ("X", 20, 21, 1), ("X", 21, 22, 1), ("X", 22, 23, 1)]
    indels, snvs = dicts_from_events(ev, 0, 0, len(READ), 1001 + aln.reference_start, WINDOW, READ, report_snvs=True)
    assert [(d["pos"], d["indel_type"], d["indel_seq"]) for d in indels] == [(1019, "I", "g")]
    assert [(s["pos"], s["ref"], s["alt"]) for s in snvs] == [(1020, "g", "G"), (1021, "c", "G"), (1022, "a", "T"), (1023, "t", "T")]
    assert (indels, snvs) == findall_indels(aln, 1001, WINDOW, READ, report_snvs=True)


def test_ops_other_than_gaps_advance_both_and_codes_above_8_read_as_m():
    rng = np.random.default_rng(5)
    ref = "".join("ACGTacgtNRU"[int(x)] for x in rng.integers(0, 11, 80))
    read = "".join("ACGTacgtNRU"[int(x)] for x in rng.integers(0, 11, 70))
    base = H.walk(H.cigar_ops("5M2I10M3D20M1D2I30M"), 3, 1, read, ref)
    for code in (3, 4, 5, 6, 7, 8, 9, 12, 15):                # N S H P = X and the codes above 8: all like M
        ops = H.cigar_ops("5M2I10M3D20M1D2I30M")
        m = [0, 2, 4, 7]                                      # the M tokens
        ops[m] = (ops[m] & ~np.uint32(15)) | np.uint32(code)
        assert H.walk(ops, 3, 1, read, ref).tolist() == base.tolist()


# ssw.c's banded traceback can return a CIGAR one base longer than the read it aligned (ssw.c:734-751): this pair, found by the
# GPU test of 30 000 random jobs, gives 8M43D4M7D7M28D23M from read index 1 -- 42 read bases of a 42-base read -- in the compiled
# reference, the oracle's port and the package alike
OVERRUN_READ = "YGYNCKTatNVAaWVGSDAYguGATAYUGYTCRAAGTGGWgC"
OVERRUN_WINDOW = ("MATNGatBHAcBUGnNtYVggDtDtGtNWATcnGBagCgBGBCttCCcaWgHTGGnTGYGangutcMVDCnAGBgaaGBTACGtuVGAVWtugRuRGHCRAtTMGTMMTYtYGANMBANCNNtNN"
                  "gBARKKNGCtuGgGTUaVYTAcgCnCAYHnRYRTgGTaBaACGAcAcaGDSGRGVgNKYNNcCYTWRUCUBAGBYutSaTTBAgNgcRCtTGHaNccYNARtRAACCGYSntaTCaDGAHgGaG"
                  "NtDGVccUDTBtTgcKVTTacSDgGNtTWMDRYACBTnSGMGTcNtHcgCATccCGYYTAVNctaGUTUCMNAGUTHgGNAnNcKHRnSAYTYWGYNGKTatNVAaWVGSguGATAYUGYTCRAAGTGGWgCMa")


def test_walk_past_the_end_follows_the_reference_slices(oracle_mod):
    from oracle.oracle import Backend, cigar_string, dna_matrix, encode
    e = Backend("port").align(encode(OVERRUN_READ), encode(OVERRUN_WINDOW), dna_matrix(3, 2), 3, 0)
    assert (cigar_string(e["cigar"]), e["read_begin1"], e["ref_begin1"]) == ("8M43D4M7D7M28D23M", 1, 252)
    aln = _aln([cigar_string(e["cigar"]), e["score1"], e["score2"], e["ref_begin1"], e["ref_end1"], e["read_begin1"], e["read_end1"]])
    assert _read_end(aln) == len(OVERRUN_READ) + 1
    ev = H.walk(H.cigar_ops(aln.CIGAR), aln.reference_start, aln.read_start, OVERRUN_READ, OVERRUN_WINDOW)
    got = dicts_from_events(ev, aln.reference_start, aln.read_start, _read_end(aln), 1000, OVERRUN_WINDOW, OVERRUN_READ, report_snvs=True)
    want = findall_indels(aln, 1000, OVERRUN_WINDOW, OVERRUN_READ, report_snvs=True)
    assert got == want and want[1][-1]["alt"] == ""                      # the last base compared with an empty slice
    # the same rule in small: a base against nothing differs, nothing against nothing does not
    for cig, read, ref, ri, qi in (("10M", "A" * 9, "A" * 20, 0, 0), ("6M", "ACGT", "ACG", 0, 0), ("5M2D3M", "AAAAAAA", "AAAAAAAAA", 1, 0),
                                   ("3M2I4M", "AAAAAAAA", "AAAAAA", 0, 1)):
        a = _aln([cig, 0, 0, ri, 0, qi, 0])
        ev = H.walk(H.cigar_ops(cig), ri, qi, read, ref)
        assert dicts_from_events(ev, ri, qi, _read_end(a), 50, ref, read, report_snvs=True) == findall_indels(a, 50, ref, read, True), cig


def test_a_walk_from_a_negative_index_is_an_error():
    with pytest.raises(H.OutsideError):
        H.walk(H.cigar_ops("10M"), -1, 0, "A" * 9, "A" * 20)
    with pytest.raises(H.OutsideError):
        H.walk(H.cigar_ops("5M"), 0, -1, None, None, 10, 20)
    assert len(H.walk(np.zeros(0, np.uint32), 0, 0, "", "")) == 0
