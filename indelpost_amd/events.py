"""findall_indels for a whole batch: one GPU alignment batch, one event pass, the dicts built on the host by slicing.

The reference decodes every alignment with findall_indels (localn.pyx:542-621): a Python loop over the CIGAR tokens after
make_insertion_first (utilities.pyx:384-401), and with report_snvs a comparison of every aligned base.  Here the library's event
pass (ipx_find_events, csrc/ipx_events.h) walks every job's CIGAR on the device, where the records and the CIGAR pool already
are, and hands back per job the indices of its indels and of its mismatching bases; Python only slices the strings at those
indices.  Bases are compared as LETTERS, byte for byte, as the reference compares strings: lower case (soft-masked FASTA), U and
IUPAC letters differ from their upper-case / folded codes.
"""
import numpy as np

from .batch import JobTable, dna_score_matrix
from .sswpy import _gpu, Alignment


def _read_ends(res):
    """per job: the read index after the walk -- read_start plus the length of every op but D (findall_indels' qi at the end)"""
    rec = res.records
    n = len(rec)
    out = rec["read_begin1"].astype(np.int64)
    cl = rec["cigar_len"].astype(np.int64)
    tot = int(cl.sum())
    if tot:
        at = np.repeat(rec["cigar_off"].astype(np.int64), cl) + (np.arange(tot) - np.repeat(np.cumsum(cl) - cl, cl))
        ops = np.asarray(res.cigar_pool)[at].astype(np.int64)
        adv = np.where((ops & 15) == 2, 0, ops >> 4)
        out = out + np.bincount(np.repeat(np.arange(n), cl), weights=adv.astype(np.float64), minlength=n).astype(np.int64)
    return out


def dicts_from_events(ev, reference_start, read_start, read_end, genome_aln_pos, ref_seq, read_seq, report_snvs=False, basequals=None):
    """What findall_indels(aln, genome_aln_pos, ref_seq, read_seq, report_snvs, basequals) returns, from the job's events (EVENT_DTYPE,
    walk order): same dicts, keys, key order and values.  read_end: the read index after the walk (findall_indels' final qi)."""
    pos0 = genome_aln_pos - 1 - reference_start          # findall_indels' pos - ri is constant along the walk
    indels, snvs = [], []
    for kind, ri, qi, n in zip(ev["kind"].tolist(), ev["ref_idx"].tolist(), ev["read_idx"].tolist(), ev["len"].tolist()):
        if kind == b"X":
            if report_snvs:
                snvs.append({"pos": pos0 + ri + 1, "ref": ref_seq[ri:ri + 1], "alt": read_seq[qi:qi + 1]})
            continue
        d = {"pos": pos0 + ri, "lt_ref": ref_seq[:ri], "lt_flank": read_seq[:qi]}
        if basequals:
            d["lt_qual"] = basequals[:qi]
        if kind == b"I":
            d["indel_type"] = "I"
            d["indel_seq"] = read_seq[qi:qi + n]
            d["rt_ref"] = ref_seq[ri:]
            d["rt_flank"] = read_seq[qi + n:]
        else:
            d["indel_type"] = "D"
            d["indel_seq"] = ""
            d["del_seq"] = ref_seq[ri:ri + n]
            d["rt_ref"] = ref_seq[ri + n:]
            d["rt_flank"] = read_seq[qi:]
        d["ref_idx"], d["read_idx"] = ri, qi
        if basequals:
            d["rt_qual"] = basequals[qi + n:] if kind == b"I" else basequals[qi:]
        indels.append(d)
    head, tail = read_seq[:read_start], read_seq[read_end:]
    for d in indels:
        d["lt_clipped"], d["rt_clipped"] = head, tail
    return (indels, snvs) if report_snvs else indels


def _check_letters(seqs, what):
    for s in seqs:
        if isinstance(s, str) and not s.isascii():
            raise ValueError("%s: letters must be ASCII (positions are byte positions)" % what)


def align_and_find_each(read_seqs, ref_seqs, window_starts, gap_opens, gap_exts, match_score, mismatch_penalty, report_snvs=False,
                        basequals=None, device=0):
    """align_and_find_indels job by job: per job either (alignment, findall_indels result) or the exception the reference's
    `aln = align(...)` / `findall_indels(aln, ...)` pair raises for it (ValueError: ssw_align returned NULL; TypeError: no CIGAR)."""
    read_seqs, ref_seqs = list(read_seqs), list(ref_seqs)
    n = len(read_seqs)
    if len(ref_seqs) != n or len(window_starts) != n:
        raise ValueError("read_seqs, ref_seqs and window_starts must have one entry per job")
    if basequals is not None and len(basequals) != n:
        raise ValueError("basequals must have one entry per job (or be None)")
    if n == 0:
        return []
    if report_snvs:
        _check_letters(read_seqs, "read_seqs")
        _check_letters(ref_seqs, "ref_seqs")
    jobs = JobTable.from_sequences(read_seqs, ref_seqs, np.arange(n, dtype=np.int32), gap_opens, gap_exts, keep_text=report_snvs)
    g = _gpu(device)
    g.set_scoring(matrix=dna_score_matrix(match_score, mismatch_penalty), flag=1, score_size=2)
    res = g.align(jobs)
    off, cnt, ev = g.find_events(jobs.read_text, jobs.ref_text) if report_snvs else g.find_events()
    rec = res.records
    cigars = res.cigar_strings()
    cols = [rec[f].tolist() for f in ("score1", "score2", "ref_begin1", "ref_end1", "read_begin1", "read_end1")]
    mode, ends = rec["mode"].tolist(), _read_ends(res).tolist()
    off, cnt = off.tolist(), cnt.tolist()
    out = []
    for k in range(n):
        if mode[k] == 2:                                         # reference: ssw_align returned NULL (sswpy.pyx:220-223)
            out.append(ValueError("Problem Running alignment, see stdout"))
            continue
        aln = Alignment(cigars[k], cols[0][k], cols[1][k], cols[2][k], cols[3][k], cols[4][k], cols[5][k])
        if aln.CIGAR is None:                                    # findall_indels cannot tokenise a missing CIGAR
            out.append(TypeError("expected string or bytes-like object, got 'NoneType'"))
            continue
        q = None if basequals is None else basequals[k]
        out.append((aln, dicts_from_events(ev[off[k]:off[k] + cnt[k]], aln.reference_start, aln.read_start, ends[k],
                                           window_starts[k] + aln.reference_start, ref_seqs[k], read_seqs[k], report_snvs, q)))
    return out


def align_and_find_indels(read_seqs, ref_seqs, window_starts, gap_opens, gap_exts, match_score, mismatch_penalty, report_snvs=False,
                          basequals=None, device=0):
    """Many `aln = align(make_aligner(ref_seqs[k], match_score, mismatch_penalty), read_seqs[k], gap_opens[k], gap_exts[k])` followed by
    `findall_indels(aln, window_starts[k] + aln.reference_start, ref_seqs[k], read_seqs[k], report_snvs, basequals[k])`
    (localn.pyx:464-472, 542-621) as ONE GPU alignment batch and one event pass.  gap_opens / gap_exts: one per job or one for all;
    basequals: None or one entry per job.  Returns (alignments, results), results[k] exactly what that findall_indels returns.
    Raises what the first job that fails would raise in the per-job loop."""
    got = align_and_find_each(read_seqs, ref_seqs, window_starts, gap_opens, gap_exts, match_score, mismatch_penalty, report_snvs,
                              basequals, device)
    for r in got:
        if isinstance(r, Exception):
            raise r
    return [r[0] for r in got], [r[1] for r in got]
