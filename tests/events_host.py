"""The event pass's per-job walk on the host (TEST INFRASTRUCTURE): indelpost_amd/csrc/ipx_events.h compiled with g++ through
tests/events_host.cpp -- the very function the device kernels run -- plus EventPortAligner, the CPU stand-in for the shared GPU
aligner: tests.port_backend.PortAligner's alignments with find_events from the host build of the walk.  Never imported by the
package."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from indelpost_amd._lib import EVENT_DTYPE
from indelpost_amd.batch import _letters

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "events_host.cpp")
HEADER = os.path.join(os.path.dirname(HERE), "indelpost_amd", "csrc", "ipx_events.h")

_lib = None


def load():
    """compile (once per process, into a temporary directory) and load the host build of the walk"""
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ipx_events_host_"), "libipx_events_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", SRC, "-o", out])
        L = C.CDLL(out)
        L.ipx_host_walk_events.restype = C.c_int64
        L.ipx_host_walk_events.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_int64]
        _lib = L
    return _lib


class OutsideError(RuntimeError):
    pass


def walk(ops, ref_begin, read_begin, read, ref, read_len=None, ref_len=None):
    """events (EVENT_DTYPE) of one job: ops = BAM-encoded CIGAR ops; read / ref = letters (str / bytes / uint8), or both None for
    indels only (then read_len / ref_len bound the walk)"""
    L = load()
    ops = np.ascontiguousarray(ops, np.uint32)
    rb = None if read is None else _letters(read)
    fb = None if ref is None else _letters(ref)
    rl = len(rb) if rb is not None else int(read_len)
    fl = len(fb) if fb is not None else int(ref_len)
    # (one spare byte each, so that empty letters still have a valid address)
    rbuf = None if rb is None else np.concatenate([rb, np.zeros(1, np.uint8)])
    fbuf = None if fb is None else np.concatenate([fb, np.zeros(1, np.uint8)])
    pr = None if rbuf is None else rbuf.ctypes.data
    pf = None if fbuf is None else fbuf.ctypes.data
    po = ops.ctypes.data if len(ops) else None
    n = L.ipx_host_walk_events(po, len(ops), int(ref_begin), int(read_begin), pr, rl, pf, fl, None, 0)
    if n < 0:
        raise OutsideError("the walk leaves its read or its window")
    out = np.zeros(max(n, 1), EVENT_DTYPE)
    m = L.ipx_host_walk_events(po, len(ops), int(ref_begin), int(read_begin), pr, rl, pf, fl, out.ctypes.data, len(out))
    assert m == n
    return out[:n]


def cigar_ops(cigarstring):
    """'5M1I3D' -> BAM-encoded ops (M=0 I=1 D=2, the other letters by MIDNSHP=X)"""
    from indelpost_amd.cigar import cigar_tokens
    return np.array([(n << 4) | "MIDNSHP=X".index(op) for n, op in cigar_tokens(cigarstring)], np.uint32)


class EventPortAligner:
    """tests.port_backend.PortAligner (imported, not edited) with find_events from the host build of the walk: the shared aligner's
    interface (set_scoring / align / find_events) on the CPU."""

    def __init__(self, oracle_mod, device=0):
        from tests.port_backend import PortAligner
        self._port = PortAligner(oracle_mod, device)
        self._last = None
        self.n_calls = 0
        self.n_event_calls = 0

    def set_scoring(self, *a, **k):
        self._port.set_scoring(*a, **k)

    def set_routing(self, flags):
        pass

    @property
    def n_jobs(self):
        return self._port.n_jobs

    def align(self, jobs):
        self.n_calls += 1
        res = self._port.align(jobs)
        self._last = (jobs, res)
        return res

    def find_events(self, read_text=None, ref_text=None):
        if (read_text is None) != (ref_text is None):
            raise ValueError("find_events: the read and window letters go together (both or neither)")
        self.n_event_calls += 1
        jobs, res = self._last
        rt = None if read_text is None else _letters(read_text)
        ft = None if ref_text is None else _letters(ref_text)
        n = jobs.n_jobs
        off, cnt, parts, base = np.zeros(n, np.int64), np.zeros(n, np.int32), [], 0
        for j in range(n):
            r = res.records[j]
            if int(r["cigar_len"]) == 0:
                continue
            r0, r1 = int(jobs.read_off[j]), int(jobs.read_off[j + 1])
            w = int(jobs.ref_id[j])
            f0, f1 = int(jobs.ref_off[w]), int(jobs.ref_off[w + 1])
            ev = walk(res.cigar_ops(j), int(r["ref_begin1"]), int(r["read_begin1"]), None if rt is None else rt[r0:r1],
                      None if ft is None else ft[f0:f1], r1 - r0, f1 - f0)
            off[j], cnt[j] = base, len(ev)
            base += len(ev)
            parts.append(ev)
        return off, cnt, (np.concatenate(parts) if parts else np.zeros(0, EVENT_DTYPE))


class StagedEventPort(EventPortAligner):
    """EventPortAligner with the staged interface of GpuAligner (upload / run / sync / download / find_events on the resident slice):
    the part class a MultiStreamAligner cuts its stream slices for (aligner_cls), so that its gathering of events -- slices,
    grouping by read length, the caller's job order -- runs on the CPU."""

    def __init__(self, device=0, match_score=2, mismatch_penalty=2, matrix=None, oracle_mod=None):
        super().__init__(oracle_mod, device)
        self.set_scoring(match_score, mismatch_penalty, matrix)
        self._jobs = None

    def upload(self, jobs):
        self._jobs, self._n_jobs = jobs, jobs.n_jobs

    def run(self):
        self.align(self._jobs)

    def sync(self):
        pass

    def download(self, cigar_ops_per_job=16):
        return self._last[1]
