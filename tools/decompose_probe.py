"""Measurement of the batched complex-variant decomposition (profiles/r05_decompose.json).

Workload: 10 000 synthetic variants -- 70 % complex indels, the rest MNVs and SNVs -- on a 1 Mb synthetic genome with soft-masked
(lower-case) stretches and N runs, drawn from a fixed seed (every process builds the same one).
  parent loop  [v.decompose_complex_variant() for v in vs] with the PARENT commit's package (a `git archive` of it with its own
               library built, given by --parent): one alignment per variant
  new call     decompose_complex_variants(vs): one GPU alignment batch and one event pass, with its host / GPU split (wall time
               inside the aligner's align() and find_events(), the rest is host Python)
Each form runs in a fresh child process (the two packages share a name), three times each, alternating; every child first
decomposes 50 variants of its own to warm the context up.  The outputs of the forms are compared in full.  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats` run of one new-call child (--add-kernel-stats): the event pass is the k_events_*
kernels, the alignment pipeline every other kernel of that run.

    python tools/decompose_probe.py --drive --parent DIR --out FILE        (GPU: the six timed children)
    python tools/decompose_probe.py --child new --out FILE                 (one child; what rocprofv3 runs)
    python tools/decompose_probe.py --add-kernel-stats DIR --out FILE      (adds the kernel times of a rocprofv3 -d DIR run)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VARIANTS, GENOME_LEN, SEED = 10000, 1000000, 20261016


class Fasta:
    def __init__(self, seqs):
        self.seqs, self.references, self.filename = seqs, list(seqs), None

    def fetch(self, chrom, start, end):
        return self.seqs[chrom][max(0, start):max(0, end)]

    def get_reference_length(self, chrom):
        return len(self.seqs[chrom])


def workload(Variant, seed=SEED, n_variants=N_VARIANTS):
    rng = np.random.default_rng(seed)
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, GENOME_LEN)].copy()
    for _ in range(400):                                   # soft-masked stretches: about a third of the genome
        p, L = int(rng.integers(0, GENOME_LEN - 3000)), int(rng.integers(200, 1500))
        g[p:p + L] |= 32
    for _ in range(30):
        p, L = int(rng.integers(1000, GENOME_LEN - 1000)), int(rng.integers(10, 200))
        g[p:p + L] = ord("N")
    genome = g.tobytes().decode()
    fa = Fasta({"chr1": genome})
    rs = lambda k: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, k))       # noqa: E731
    vs = []
    while len(vs) < n_variants:
        pos = int(rng.integers(200, GENOME_LEN - 200))
        u = rng.random()
        if u < 0.7:                                        # complex indel
            r_len, a_len = int(rng.integers(1, 10)), int(rng.integers(1, 10))
            if r_len == a_len:
                a_len += 1
            ref, alt = genome[pos - 1:pos - 1 + r_len], rs(a_len)
        elif u < 0.85:                                     # MNV
            n = int(rng.integers(2, 6))
            ref, alt = genome[pos - 1:pos - 1 + n], rs(n)
        else:                                              # SNV
            ref, alt = genome[pos - 1], rs(1)
        try:
            v = Variant("chr1", pos, ref, alt, fa)
        except ValueError:
            continue
        if v.is_non_complex_indel():
            continue
        vs.append(v)
    return vs


def child(form, out):
    import indelpost_amd as ip
    vs = workload(ip.Variant)
    warm = workload(ip.Variant, SEED + 1, 50)              # the warm-up: 50 variants of another seed
    split = {}
    if form == "parent":
        [v.decompose_complex_variant() for v in warm]
        t0 = time.perf_counter()
        got = [v.decompose_complex_variant() for v in vs]
        wall = time.perf_counter() - t0
    else:
        from indelpost_amd import events
        real = events._gpu

        class Timed:                                       # wall time inside the aligner: the GPU side of the call
            def __init__(self, g):
                self.g, self.t_align, self.t_events = g, 0.0, 0.0

            def __getattr__(self, k):
                return getattr(self.g, k)

            def align(self, jobs):
                t = time.perf_counter()
                r = self.g.align(jobs)
                self.t_align += time.perf_counter() - t
                return r

            def find_events(self, *a):
                t = time.perf_counter()
                r = self.g.find_events(*a)
                self.t_events += time.perf_counter() - t
                return r
        ip.decompose_complex_variants(warm)
        timed = Timed(real(0))
        events._gpu = lambda device=0: timed
        t0 = time.perf_counter()
        got = ip.decompose_complex_variants(vs)
        wall = time.perf_counter() - t0
        events._gpu = real
        split = {"align_s": timed.t_align, "find_events_s": timed.t_events, "host_s": wall - timed.t_align - timed.t_events}
    res = {"form": form, "package": os.path.dirname(ip.__file__), "n_variants": len(vs), "wall_s": wall, "split": split,
           "n_out": sum(len(g) for g in got), "outputs": [[[x.chrom, x.pos, x.ref, x.alt] for x in g] for g in got]}
    with open(out, "w") as f:
        json.dump(res, f)


def drive(parent, out, reps=3, timeout=600):
    tmp = os.path.join(os.path.dirname(os.path.abspath(out)), "probe_children")
    os.makedirs(tmp, exist_ok=True)
    runs = {"parent": [], "new": []}
    outputs = {}
    for rep in range(reps):
        for form, pkg in (("parent", os.path.abspath(parent)), ("new", ROOT)):
            o = os.path.join(tmp, "%s_%d.json" % (form, rep))
            env = dict(os.environ, PYTHONPATH=pkg)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--out", o]
            subprocess.run(cmd, env=env, cwd=pkg, check=True, timeout=timeout)
            with open(o) as f:
                r = json.load(f)
            assert os.path.realpath(r["package"]).startswith(os.path.realpath(pkg)), (r["package"], pkg)
            outputs.setdefault(form, r["outputs"])
            assert r["outputs"] == outputs[form], "%s: outputs differ between runs" % form
            runs[form].append({k: r[k] for k in ("wall_s", "split", "n_variants", "n_out")})
            print(form, rep, "%.3f s" % r["wall_s"], r["split"], flush=True)
    pw = [r["wall_s"] for r in runs["parent"]]
    nw = [r["wall_s"] for r in runs["new"]]
    res = {"workload": {"variants": N_VARIANTS, "complex_indels": 0.7, "mnv_snv": 0.3, "genome_bp": GENOME_LEN, "seed": SEED,
                        "soft_masked": True, "warm_up_variants_per_child": 50},
           "outputs_identical": outputs["parent"] == outputs["new"], "n_decomposed_variants": runs["new"][0]["n_out"],
           "parent_loop": {"what": "[v.decompose_complex_variant() for v in vs], parent commit's package", "wall_s": pw,
                           "spread_s": max(pw) - min(pw)},
           "new_call": {"what": "decompose_complex_variants(vs)", "wall_s": nw, "spread_s": max(nw) - min(nw),
                        "split": [r["split"] for r in runs["new"]]},
           "speedup_median": float(np.median(pw) / np.median(nw)),
           "faster_by_more_than_parent_spread": bool(min(pw) - max(nw) > max(pw) - min(pw))}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "new_call"}, indent=1))
    if not res["outputs_identical"]:
        sys.exit("outputs differ between the parent loop and the new call")


def add_kernel_stats(d, out):
    """kernel times of a rocprofv3 --kernel-trace --stats run of one new-call child: totals from the stats file, and per batch (the
    warm-up call, then the workload's) from the trace -- a batch is the alignment pipeline's dispatches up to and including its
    event pass (k_events_count + k_events_emit)"""
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(stats) == 1 and len(trace) == 1, (stats, trace)
    ev_ns = al_ns = 0
    rows = []
    with open(stats[0]) as f:
        for r in csv.DictReader(f):
            ns = int(float(r["TotalDurationNs"]))
            rows.append([r["Name"], int(r["Calls"]), ns])
            if "k_events_" in r["Name"]:
                ev_ns += ns
            else:
                al_ns += ns
    with open(trace[0]) as f:
        disp = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    batches, cur = [], {"pipeline_ns": 0, "event_ns": 0, "pipeline_dispatches": 0}
    for t0, t1, name in disp:
        if "k_events_" in name:
            cur["event_ns"] += t1 - t0
            if name.startswith("k_events_emit"):
                batches.append(cur)
                cur = {"pipeline_ns": 0, "event_ns": 0, "pipeline_dispatches": 0}
        else:
            cur["pipeline_ns"] += t1 - t0
            cur["pipeline_dispatches"] += 1
    for b in batches:
        b["event_fraction"] = b["event_ns"] / b["pipeline_ns"] if b["pipeline_ns"] else None
    with open(out) as f:
        res = json.load(f)
    res["kernel_times"] = {"source": "rocprofv3 --kernel-trace --stats, one new-call child (50 warm-up variants, then the workload)",
                           "alignment_pipeline_ms": al_ns / 1e6, "event_pass_ms": ev_ns / 1e6,
                           "event_pass_fraction_of_pipeline": ev_ns / al_ns if al_ns else None,
                           "per_batch": dict(zip(["warm_up", "workload"], batches)),
                           "event_kernels": [r for r in rows if "k_events_" in r[0]]}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_times"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["parent", "new"])
    ap.add_argument("--drive", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--add-kernel-stats")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.out)
    elif a.drive:
        drive(a.parent, a.out)
    elif a.add_kernel_stats:
        add_kernel_stats(a.add_kernel_stats, a.out)


if __name__ == "__main__":
    main()
