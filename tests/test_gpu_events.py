"""The event pass on the MI355X (ipx_find_events, csrc/ipx_events.h) and the batched decomposition built on it.

  * golden replays: the 160 findall_indels cases of tests/golden/decoder_cases.json through align_and_find_indels (alignments equal
    the recorded ones, results equal `expect`), and every case of tests/golden/decompose_cases.json through
    decompose_complex_variants and decomposed_targets -- no case left out;
  * the device's events against the host decoder (cigar.findall_indels, pinned by decoder_cases.json) on 30 000+ random jobs with
    lower case, U, N and IUPAC letters, read lengths mixed so that a MultiStreamAligner groups them by length and cuts four slices;
  * the pool and argument contract of the C entry point.
The random jobs hold CIGARs that ssw.c's banded traceback makes one base longer than their read (job 1648: 8M43D4M7D7M28D23M from
read index 1 of a 42-base read, the same in the compiled reference); the events of those follow the reference's string slicing
(tests/test_event_walk.py::test_walk_past_the_end_follows_the_reference_slices), so they too must equal findall_indels.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from indelpost_amd.cigar import cigar_tokens, findall_indels
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

GAP_PAIRS = [(3, 1), (3, 0), (5, 1), (4, 0), (1, 0), (0, 0)]      # oracle/gen_decoder_golden.py:119


def test_gpu_findall_indels_golden_replay():
    from indelpost_amd import align_and_find_indels
    from indelpost_amd.sswpy import Alignment
    with open(os.path.join(GOLDEN, "decoder_cases.json")) as f:
        cases = json.load(f)["findall_indels"]
    assert len(cases) == 160
    # decoder_cases.json does not record a case's gap pair: every case under each of its generator's pairs, the first pair that
    # reproduces the recorded alignment is the case's
    reads, refs = [c["read_seq"] for c in cases], [c["ref_seq"] for c in cases]
    starts = [c["genome_aln_pos"] - c["aln"][3] for c in cases]
    found = [None] * len(cases)
    for go, ge in GAP_PAIRS:
        for snv in (False, True):
            quals = [c["basequals"] for c in cases]
            alns, res = align_and_find_indels(reads, refs, starts, go, ge, 3, 2, report_snvs=snv, basequals=quals)
            for k, c in enumerate(cases):
                if found[k] is None and list(alns[k]) == c["aln"] and snv == c["report_snvs"]:
                    found[k] = (go, ge)
                    got = [list(res[k][0]), list(res[k][1])] if snv else res[k]
                    assert got == c["expect"], (k, go, ge)
    missing = [k for k, f in enumerate(found) if f is None]
    assert not missing, "cases no gap pair reproduces: %s" % missing
    by_pair = {p: sum(f == p for f in found) for p in GAP_PAIRS}
    print("gap pairs found:", by_pair)
    assert isinstance(alns[0], Alignment)


def test_gpu_letters_known_answer():
    """soft-masked window, upper-case read: alignment 19M1I32M score 139; the insertion 'g' at 1019 and four mismatches, two of them
    only because of case"""
    from indelpost_amd import align_and_find_indels
    window = "acgtacgttgacctagcatgcatgcaatcgatcgtagctagctagcatcga"
    read = window[:20] + "GGTT" + window[23:]
    alns, res = align_and_find_indels([read], [window], [1001], 4, 0, 3, 2, report_snvs=True)
    assert (alns[0].CIGAR, alns[0].optimal_score) == ("19M1I32M", 139)
    indels, snvs = res[0]
    assert [(d["pos"], d["indel_type"], d["indel_seq"]) for d in indels] == [(1019, "I", "g")]
    assert [(s["pos"], s["ref"], s["alt"]) for s in snvs] == [(1020, "g", "G"), (1021, "c", "G"), (1022, "a", "T"), (1023, "t", "T")]


def test_gpu_decompose_golden_replay():
    from tests.test_decompose import load_cases, replay_decompositions, replay_targets
    d, vs = load_cases()
    replay_decompositions(d, vs)
    replay_targets(d, vs)


LETTERS = np.frombuffer(b"ACGTACGTACGTacgtacgtNnUuRYSWKMBDHVN", np.uint8)


def _random_jobs(rng, n):
    """windows of 150-700 letters, reads cut from them and mutated (substitutions, indels), read lengths 40-300 with a few of
    505-900: every letter class of LETTERS appears in both"""
    n_win = n // 12
    wins = [LETTERS[rng.integers(0, len(LETTERS), int(rng.integers(150, 700)))] for _ in range(n_win)]
    long_wins = [LETTERS[rng.integers(0, len(LETTERS), int(rng.integers(1200, 2000)))] for _ in range(8)]
    wins += long_wins
    reads, rid = [], []
    for j in range(n):
        w = int(rng.integers(0, n_win)) if j % 500 else n_win + int(rng.integers(0, len(long_wins)))
        win = wins[w]
        L = int(rng.integers(505, 900)) if j % 500 == 0 else int(rng.choice([40, 60, 100, 150, 220, 300]))
        L = min(L, len(win) - 1)
        a = int(rng.integers(0, len(win) - L + 1))
        r = win[a:a + L].copy()
        m = rng.random(L)
        r[m < 0.04] = LETTERS[rng.integers(0, len(LETTERS), int((m < 0.04).sum()))]
        cut = sorted(rng.integers(0, L, int(rng.integers(0, 4))).tolist())
        parts, last = [], 0
        for p in cut:                                               # small insertions and deletions
            parts.append(r[last:p])
            if rng.random() < 0.5:
                parts.append(LETTERS[rng.integers(0, len(LETTERS), int(rng.integers(1, 6)))])
                last = p
            else:
                last = min(L, p + int(rng.integers(1, 6)))
        parts.append(r[last:])
        r = np.concatenate(parts)
        reads.append(r if len(r) else win[:10].copy())
        rid.append(w)
    return reads, wins, np.array(rid, np.int32)


def test_gpu_events_equal_the_host_decoder_on_30000_random_jobs():
    from indelpost_amd import JobTable, MultiStreamAligner
    from indelpost_amd.events import dicts_from_events
    from indelpost_amd.sswpy import alignments_from
    rng = np.random.default_rng(31337)
    n = 30000
    reads, wins, rid = _random_jobs(rng, n)
    rs, ws = [r.tobytes().decode() for r in reads], [w.tobytes().decode() for w in wins]
    go = rng.choice([3, 4, 5], n).astype(np.int64)
    ge = rng.choice([0, 1], n).astype(np.int64)
    jobs = JobTable.from_sequences(rs, ws, rid, go, ge, keep_text=True)
    assert max(len(r) for r in reads) >= 505
    with MultiStreamAligner(0, 3, 2, streams=4) as g:
        g.min_jobs_per_stream = 5000                                # four slices for 30 000 jobs
        g.group_by_length = True                                    # grouped by length on the way in: events must come home
        g.upload(jobs)
        assert len(g._active) == 4 and g._order is not None and not np.array_equal(g._order, np.arange(n))
        g.run()
        g.sync()
        res = g.download()
        off, cnt, ev = g.find_events(jobs.read_text, jobs.ref_text)
        off_i, cnt_i, ev_i = g.find_events()
    alns = alignments_from(res)
    n_x = n_gap = 0
    for k in range(n):
        a, e = alns[k], ev[off[k]:off[k] + cnt[k]]
        if a.CIGAR is None:                                         # (no CIGAR, nothing to decode: no events)
            assert cnt[k] == 0 and cnt_i[k] == 0
            continue
        ends = a.read_start + sum(t for t, op in cigar_tokens(a.CIGAR) if op != "D")
        pos = 1000 + 7 * k
        want = findall_indels(a, pos, ws[rid[k]], rs[k], report_snvs=True)
        assert dicts_from_events(e, a.reference_start, a.read_start, ends, pos, ws[rid[k]], rs[k], report_snvs=True) == want, k
        ei = ev_i[off_i[k]:off_i[k] + cnt_i[k]]
        assert ei.tolist() == e[e["kind"] != b"X"].tolist(), k
        n_x += int((e["kind"] == b"X").sum())
        n_gap += len(ei)
    print("jobs %d, gap events %d, mismatch events %d" % (n, n_gap, n_x))
    assert n_gap > 1000 and n_x > 10000


def test_gpu_event_pool_and_argument_contract():
    from indelpost_amd import GpuAligner, JobTable
    from indelpost_amd._lib import EVENT_DTYPE, IPX_ERR_ARG, IPX_ERR_EVENT_POOL
    rng = np.random.default_rng(7)
    win = "".join("ACGTacgt"[int(x)] for x in rng.integers(0, 8, 400))
    reads = [win[a:a + 80] + "TTGA" + win[a + 84:a + 160] for a in range(0, 200, 10)] + [win[5:9].upper()]
    jobs = JobTable.from_sequences(reads, [win], np.zeros(len(reads), np.int32), 4, 0, keep_text=True)
    g = GpuAligner(0, 3, 2)
    try:
        g.align(jobs)
        off, cnt, ev = g.find_events(jobs.read_text, jobs.ref_text)
        need = len(ev)
        assert need == int(cnt.sum()) > 0
        L, n = g._L, jobs.n_jobs
        o, c = np.full(n, -5, np.int64), np.full(n, -5, np.int32)
        e = np.zeros(need, EVENT_DTYPE)
        e["ref_idx"] = -9
        used = C.c_int64(0)
        rt, ft = jobs.read_text, jobs.ref_text
        rc = L.ipx_find_events(g._ctx, rt.ctypes.data, ft.ctypes.data, o.ctypes.data, c.ctypes.data, e.ctypes.data, need - 1, C.byref(used))
        assert rc == IPX_ERR_EVENT_POOL and used.value == need
        assert (o == -5).all() and (c == -5).all() and (e["ref_idx"] == -9).all()
        rc = L.ipx_find_events(g._ctx, rt.ctypes.data, None, o.ctypes.data, c.ctypes.data, e.ctypes.data, need, C.byref(used))
        assert rc == IPX_ERR_ARG
        rc = L.ipx_find_events(g._ctx, None, ft.ctypes.data, o.ctypes.data, c.ctypes.data, e.ctypes.data, need, C.byref(used))
        assert rc == IPX_ERR_ARG
        assert (o == -5).all() and (c == -5).all() and (e["ref_idx"] == -9).all()
        rc = L.ipx_find_events(g._ctx, rt.ctypes.data, ft.ctypes.data, o.ctypes.data, c.ctypes.data, e.ctypes.data, need, C.byref(used))
        assert rc == 0 and used.value == need
        assert o.tolist() == off.tolist() and c.tolist() == cnt.tolist()
        with pytest.raises(ValueError):
            g.find_events(jobs.read_text, None)
    finally:
        g.close()
