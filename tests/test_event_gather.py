"""MultiStreamAligner.find_events on the CPU: a batch cut into stream slices and grouped by read length on its way in must hand its
events back in the CALLER's job order, as download() does with the records.  The slices are tests.events_host.StagedEventPort (the
oracle's port for the alignments, the host build of the event walk for the events); the cutting, the grouping (the library's host
helper) and the gathering are the package's own."""
import functools

import numpy as np

from indelpost_amd.cigar import cigar_tokens, findall_indels


def _jobs(rng, n):
    letters = np.frombuffer(b"ACGTacgtNUuRY", np.uint8)
    wins = [letters[rng.integers(0, len(letters), int(rng.integers(120, 300)))] for _ in range(12)]
    reads, rid = [], []
    for j in range(n):
        w = int(rng.integers(0, len(wins)))
        L = int(rng.choice([20, 45, 70, 110]))
        a = int(rng.integers(0, len(wins[w]) - L))
        r = wins[w][a:a + L].copy()
        m = rng.random(L) < 0.06
        r[m] = letters[rng.integers(0, len(letters), int(m.sum()))]
        if j % 3 == 0:
            p = int(rng.integers(5, L - 5))
            r = np.concatenate([r[:p], letters[rng.integers(0, 4, 3)], r[p + (2 if j % 2 else 0):]])
        reads.append(r.tobytes().decode())
        rid.append(w)
    return reads, [w.tobytes().decode() for w in wins], np.array(rid, np.int32)


def test_multistream_events_come_home_in_the_callers_order(oracle_mod, hip_lib):
    from indelpost_amd import JobTable, MultiStreamAligner
    from indelpost_amd.events import dicts_from_events
    from indelpost_amd.sswpy import alignments_from
    from tests.events_host import StagedEventPort
    rng = np.random.default_rng(2024)
    n = 240
    reads, wins, rid = _jobs(rng, n)
    jobs = JobTable.from_sequences(reads, wins, rid, 4, 0, keep_text=True)
    g = MultiStreamAligner(0, 3, 2, streams=4, aligner_cls=functools.partial(StagedEventPort, oracle_mod=oracle_mod))
    g.min_jobs_per_stream = 50
    g.group_by_length = True
    g.upload(jobs)
    assert len(g._active) == 4 and not np.array_equal(g._order, np.arange(n))
    g.run()
    g.sync()
    alns = alignments_from(g.download())
    off, cnt, ev = g.find_events(jobs.read_text, jobs.ref_text)
    off_i, cnt_i, ev_i = g.find_events()
    for k in range(n):
        a = alns[k]
        e = ev[off[k]:off[k] + cnt[k]]
        end = a.read_start + sum(t for t, op in cigar_tokens(a.CIGAR) if op != "D")
        want = findall_indels(a, 500 + k, wins[rid[k]], reads[k], report_snvs=True)
        assert dicts_from_events(e, a.reference_start, a.read_start, end, 500 + k, wins[rid[k]], reads[k], report_snvs=True) == want, k
        assert ev_i[off_i[k]:off_i[k] + cnt_i[k]].tolist() == e[e["kind"] != b"X"].tolist(), k
    assert int((ev["kind"] == b"I").sum()) > 20 and int((ev["kind"] == b"X").sum()) > 200
