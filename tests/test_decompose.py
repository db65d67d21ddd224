"""Batched complex-variant decomposition on the CPU: decompose_complex_variants, the single-variant method and decomposed_targets
against tests/golden/decompose_cases.json (tools/gen_decompose_golden.py: the reference's own Variant class, findall_indels and
varaln.pyx:122-143 executed as text), with the alignments of the oracle's port and the events of the host build of the event walk
(tests/events_host.EventPortAligner patched in as the shared aligner, as tests/test_drivers.py patches PortAligner).
tests/test_gpu_events.py replays the same file through libindelpost_hip.so."""
import builtins
import json
import os

import pytest

from tests.conftest import GOLDEN


class Fasta:
    """the in-memory FASTA duck type the generator used (fetch clips negative coordinates at 0)"""

    def __init__(self, seqs):
        self.seqs, self.references, self.filename = seqs, list(seqs), None

    def fetch(self, chrom, start, end):
        return self.seqs[chrom][max(0, start):max(0, end)]

    def get_reference_length(self, chrom):
        return len(self.seqs[chrom])


def load_cases():
    with open(os.path.join(GOLDEN, "decompose_cases.json")) as f:
        d = json.load(f)
    from indelpost_amd import Variant
    fa = Fasta(d["genome"])
    vs = [Variant(*c["in"], fa, skip_validation=c["skip_validation"]) for c in d["cases"]]
    return d, vs


def vt(v):
    return [v.chrom, v.pos, v.ref, v.alt]


def check_one(expect, call):
    """expect: {"out": ...} or {"raises": type name}; call() -> the value to compare with "out" """
    if "raises" in expect:
        with pytest.raises(getattr(builtins, expect["raises"])):
            call()
    else:
        assert call() == expect["out"]


def _gap_args(gaps):
    return () if gaps is None else (3, 2) + tuple(gaps)


def replay_decompositions(d, vs, device=0):
    """every case under every gap setting: decompose_complex_variants case for case (the callable raising what the loop raises)
    and once as one call over every case that does not raise"""
    from indelpost_amd import decompose_complex_variants
    for j, gaps in enumerate(d["decompose_gaps"]):
        args = _gap_args(gaps)
        for c, v in zip(d["cases"], vs):
            check_one(c["decompose"][j], lambda: [vt(x) for x in decompose_complex_variants([v], *args, device=device)[0]])
        ok = [k for k, c in enumerate(d["cases"]) if "out" in c["decompose"][j]]
        got = decompose_complex_variants([vs[k] for k in ok], *args, device=device)
        assert [[vt(x) for x in g] for g in got] == [d["cases"][k]["decompose"][j]["out"] for k in ok]


def replay_targets(d, vs, device=0):
    from indelpost_amd import decomposed_targets
    for j, (auto, go, ge) in enumerate(d["target_settings"]):
        kw = dict(match_score=3, mismatch_penalty=2, gap_open_penalty=go, gap_extension_penalty=ge, auto_adjust_extension_penalty=auto,
                  device=device)
        for c, v in zip(d["cases"], vs):
            check_one(c["targets"][j], lambda: [[vt(t), vt(st), cx] for t, st, cx in decomposed_targets([v], **kw)][0])
        ok = [k for k, c in enumerate(d["cases"]) if "out" in c["targets"][j]]
        got = decomposed_targets([vs[k] for k in ok], **kw)
        assert [[vt(t), vt(st), cx] for t, st, cx in got] == [d["cases"][k]["targets"][j]["out"] for k in ok]


@pytest.fixture()
def port_events_as_gpu(oracle_mod, monkeypatch):
    from indelpost_amd import events, localn, retarget, sswpy
    from tests.events_host import EventPortAligner
    cache = {}

    def fake(device=0):
        if device not in cache:
            cache[device] = EventPortAligner(oracle_mod, device)
        return cache[device]
    for m in (sswpy, localn, retarget, events):
        monkeypatch.setattr(m, "_gpu", fake)
    return cache


@pytest.fixture(scope="module")
def cases():
    return load_cases()


def test_golden_file_shape(cases):
    d, vs = cases
    assert d["aligner"] == "reference" and len(vs) >= 300
    for c in d["cases"]:                                                      # every alignment under the gaps of its setting
        for gaps, used in zip(d["decompose_gaps"], c["gaps_used"]):
            assert all(u == (gaps or [4, 0]) for u in used)
    assert sum(v.pos <= 100 for v in vs) >= 10
    assert any(c["in"][2] != c["in"][2].upper() for c in d["cases"])          # soft-masked reference alleles
    assert {"IndexError", "KeyError"} <= {x["raises"] for c in d["cases"] for x in c["decompose"] + c["targets"] if "raises" in x}


def test_decompose_complex_variants_match_the_reference(cases, port_events_as_gpu):
    replay_decompositions(*cases)


def test_single_method_matches_the_reference(cases, port_events_as_gpu):
    d, vs = cases
    for j, gaps in enumerate(d["decompose_gaps"]):
        for c, v in zip(d["cases"], vs):
            check_one(c["decompose"][j], lambda: [vt(x) for x in v.decompose_complex_variant(*_gap_args(gaps))])


def test_decomposed_targets_match_the_reference(cases, port_events_as_gpu):
    replay_targets(*cases)


def test_one_batch_for_every_complex_variant(cases, port_events_as_gpu):
    from indelpost_amd import decompose_complex_variants
    d, vs = cases
    ok = [k for k, c in enumerate(d["cases"]) if "out" in c["decompose"][0]]
    decompose_complex_variants([vs[k] for k in ok])
    g = port_events_as_gpu[0]
    assert g.n_calls == 1 and g.n_event_calls == 1
    n_complex = sum(not vs[k].is_non_complex_indel() for k in ok)
    assert g.n_jobs == n_complex > 100


def test_mixed_call_keeps_input_order_and_raises_the_first_failure(cases, port_events_as_gpu):
    from indelpost_amd import decompose_complex_variants, decomposed_targets
    d, vs = cases
    cx = [k for k, c in enumerate(d["cases"]) if "out" in c["decompose"][0] and not vs[k].is_non_complex_indel() and len(c["decompose"][0]["out"]) > 1]
    simple = [k for k, c in enumerate(d["cases"]) if "out" in c["decompose"][0] and vs[k].is_indel and vs[k].is_non_complex_indel()]
    fail = [k for k, c in enumerate(d["cases"]) if "raises" in c["decompose"][0]]
    assert cx and simple and fail
    order = [cx[0], simple[0], cx[1], simple[1], cx[2]]
    got = decompose_complex_variants([vs[k] for k in order])
    assert [[vt(x) for x in g] for g in got] == [d["cases"][k]["decompose"][0]["out"] for k in order]
    assert got[1] == [vs[simple[0]]] and got[1][0] is vs[simple[0]]
    t = decomposed_targets([vs[k] for k in order])
    assert [[vt(a), vt(b), c] for a, b, c in t] == [d["cases"][k]["targets"][0]["out"] for k in order]
    # a failing variant among good ones: the call raises what the loop raises for it
    f = fail[0]
    with pytest.raises(getattr(builtins, d["cases"][f]["decompose"][0]["raises"])):
        decompose_complex_variants([vs[cx[0]], vs[simple[0]], vs[f], vs[cx[1]]])
    # two failures of different types (target selection: a decomposition without indels, an unknown contig): the first one in
    # input order wins
    kinds = {}
    for k, c in enumerate(d["cases"]):
        if "raises" in c["targets"][0]:
            kinds.setdefault(c["targets"][0]["raises"], k)
    assert len(kinds) >= 2
    (n1, k1), (n2, k2) = list(kinds.items())[:2]
    for a, b, name in ((k1, k2, n1), (k2, k1, n2)):
        with pytest.raises(getattr(builtins, name)):
            decomposed_targets([vs[cx[0]], vs[simple[0]], vs[a], vs[cx[1]], vs[b]])
