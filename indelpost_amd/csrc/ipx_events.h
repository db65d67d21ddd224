// ipx_events.h -- the event pass: every job's CIGAR walked as findall_indels walks it (localn.pyx:542-621), on the device
// where the records, the CIGAR pool and the batch already are.  Per job it emits one event per I / D token,
// (kind, ref_idx, read_idx, len) with the window / read indices findall_indels has at that token, and -- when the letters of
// the reads and windows are given -- one 'X' event (len 1) per aligned base whose letters differ.
//
// The ops are read through make_insertion_first (utilities.pyx:384-401) and its merge_consecutive_gaps quirk
// (utilities.pyx:360-381; restated in cigar.py): in every run of adjacent gaps that holds both I and D and whose first token
// is D, the tokens are reversed; where a run of two or more gaps reaches the end of the op list, its last token is not part
// of the run.  Every op that is not I or D advances read and window alike, as the reference's else-branch does (op codes
// above 8 read as M, ssw.h:182-184).
//
// Letters, not codes: two bases differ when their BYTES differ, as the reference's string comparison does (localn.pyx:598).
// The int8 codes of the batch fold case, U and the IUPAC letters, so they cannot decide it.
//
// Past the end of a read or window the walk goes on as the reference's slicing does: ssw.c's banded traceback can hand back a
// CIGAR one base longer than the read or window it aligned (a path that leaves the rectangle by its first row ends in one more
// M, ssw.c:734-751), and findall_indels then compares a base with an empty slice -- an 'X' event whose letter on one side is
// nothing -- and slices indel sequences short.  Letters are only read inside the strings.  A walk that starts at a negative
// index, or whose indices would not fit in 32 bits, has no counterpart there: IPX_EV_OUTSIDE, an internal error of the runtime.
//
// ipx_walk_events is plain C++ (host and device): the kernels below run it one lane per job, and the CPU tests compile the same
// function with g++ (tests/events_host.cpp).
#ifndef IPX_EVENTS_H
#define IPX_EVENTS_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define IPX_EV_HD __host__ __device__
#define IPX_EV_UNROLL _Pragma("unroll")
#else
#define IPX_EV_HD
#define IPX_EV_UNROLL
#endif

struct IpxEvent {            // = ipx_event of include/indelpost_hip.h (16 B)
    int32_t ref_idx;
    int32_t read_idx;
    int32_t len;
    uint8_t kind;            // 'I', 'D' or 'X'
    uint8_t pad[3];
};

enum { IPX_EV_OK = 0, IPX_EV_OUTSIDE = 1 };

// 1: insertion, 2: deletion, 0: every other op (BAM codes, len << 4 | op)
IPX_EV_HD inline int ipx_ev_gap(uint32_t op)
{
    const uint32_t c = op & 0xfu;
    return c == 1u ? 1 : (c == 2u ? 2 : 0);
}

// Walks one job.  ops / n_ops: its BAM ops; ri / qi: reference_start / read_start; read, ref: the job's letters (read_len /
// ref_len bytes; both NULL: indels only).  sink(kind, ref_idx, read_idx, len) is called per
// event in findall_indels' order: the indels in CIGAR order, a run's mismatches in base order.
template <class Sink>
IPX_EV_HD inline int ipx_walk_events(const uint32_t *ops, int32_t n_ops, int64_t ri, int64_t qi, const uint8_t *read,
                                     int64_t read_len, const uint8_t *ref, int64_t ref_len, Sink &sink)
{
    if (ri < 0 || qi < 0) return IPX_EV_OUTSIDE;
    const bool letters = read != nullptr && ref != nullptr;
    const int64_t idx_max = 0x7fffffff;
    int32_t k = 0;
    while (k < n_ops) {
        const uint32_t op = ops[k];
        if (!ipx_ev_gap(op)) {
            const int64_t len = (int64_t)(op >> 4);
            if (ri + len > idx_max || qi + len > idx_max) return IPX_EV_OUTSIDE;
            if (letters) {
                const uint8_t *a = ref + ri, *b = read + qi;
                // the bases both strings hold: byte for byte, eight independent loads per side in flight before the compares
                int64_t both = len;
                if (ri + both > ref_len) both = ref_len > ri ? ref_len - ri : 0;
                if (qi + both > read_len) both = read_len > qi ? read_len - qi : 0;
                int64_t i = 0;
                for (; i + 8 <= both; i += 8) {
                    uint8_t x[8], y[8];
IPX_EV_UNROLL
                    for (int u = 0; u < 8; ++u) { x[u] = a[i + u]; y[u] = b[i + u]; }
IPX_EV_UNROLL
                    for (int u = 0; u < 8; ++u)
                        if (x[u] != y[u]) sink((uint8_t)'X', ri + i + u, qi + i + u, 1);
                }
                for (; i < both; ++i)
                    if (a[i] != b[i]) sink((uint8_t)'X', ri + i, qi + i, 1);
                // past the end of one string its slice is empty: a base against nothing differs, nothing against nothing does not
                for (; i < len; ++i)
                    if ((ri + i < ref_len) != (qi + i < read_len)) sink((uint8_t)'X', ri + i, qi + i, 1);
            }
            ri += len;
            qi += len;
            ++k;
            continue;
        }
        int32_t e = k;                                  // the run of adjacent gaps [k, e)
        while (e < n_ops && ipx_ev_gap(ops[e])) ++e;
        const int32_t cut = (e == n_ops && e - k >= 2) ? e - 1 : e;    // merge_consecutive_gaps stops one token short at the end
        for (int part = 0; part < 2; ++part) {
            const int32_t s = part == 0 ? k : cut, t = part == 0 ? cut : e;
            if (s >= t) continue;
            bool has_i = false, has_d = false;
            for (int32_t p = s; p < t; ++p) {
                if (ipx_ev_gap(ops[p]) == 1) has_i = true;
                else has_d = true;
            }
            const bool rev = has_i && has_d && ipx_ev_gap(ops[s]) == 2;
            for (int32_t p = 0; p < t - s; ++p) {
                const uint32_t g = ops[rev ? t - 1 - p : s + p];
                const int64_t len = (int64_t)(g >> 4);
                if (ri + len > idx_max || qi + len > idx_max) return IPX_EV_OUTSIDE;
                if (ipx_ev_gap(g) == 1) {
                    sink((uint8_t)'I', ri, qi, len);
                    qi += len;
                } else {
                    sink((uint8_t)'D', ri, qi, len);
                    ri += len;
                }
            }
        }
        k = e;
    }
    return IPX_EV_OK;
}

struct IpxEvCount {
    int64_t n = 0;
    IPX_EV_HD void operator()(uint8_t, int64_t, int64_t, int64_t) { ++n; }
};

struct IpxEvWrite {
    IpxEvent *out;
    int64_t n;
    IPX_EV_HD void operator()(uint8_t kind, int64_t ri, int64_t qi, int64_t len)
    {
        IpxEvent e;
        e.ref_idx = (int32_t)ri;
        e.read_idx = (int32_t)qi;
        e.len = (int32_t)len;
        e.kind = kind;
        e.pad[0] = e.pad[1] = e.pad[2] = 0;
        out[n++] = e;
    }
};

#if defined(__HIPCC__) || defined(__HIP__)
// One lane per job, grid-stride.  The job's read is read_txt[read_off[j] .. read_off[j+1]), its window ref_txt[ref_off[w] ..
// ref_off[w+1]) with w = ref_id[j] (the offsets of the last ipx_upload); letters == 0: both text pointers are ignored.
struct IpxEvJob {
    const uint32_t *ops;
    int32_t n_ops;
    int64_t ri, qi, read_len, ref_len;
    const uint8_t *read, *ref;
};

__device__ inline IpxEvJob ipx_ev_job(int64_t j, const IpxResult *res, const uint32_t *cigar_pool, const int64_t *read_off,
                                      const int64_t *ref_off, const int32_t *ref_id, const uint8_t *read_txt, const uint8_t *ref_txt,
                                      int letters)
{
    const IpxResult r = res[j];
    IpxEvJob q;
    q.ops = cigar_pool + r.cigar_off;
    q.n_ops = (int32_t)r.cigar_len;
    q.ri = r.ref_begin1;
    q.qi = r.read_begin1;
    const int64_t r0 = read_off[j], w = ref_id[j], f0 = ref_off[w];
    q.read_len = read_off[j + 1] - r0;
    q.ref_len = ref_off[w + 1] - f0;
    q.read = letters ? read_txt + r0 : nullptr;
    q.ref = letters ? ref_txt + f0 : nullptr;
    return q;
}

// pass 1: count every job's events, reserve its range of the pool (vector atomic on the cursor); a walk that fails (IPX_EV_OUTSIDE)
// sets *status and leaves the lowest such job in *first_bad (the runtime's error message names it)
__global__ void __launch_bounds__(256) k_events_count(const IpxResult *res, const uint32_t *cigar_pool, const int64_t *read_off,
                                                      const int64_t *ref_off, const int32_t *ref_id, const uint8_t *read_txt,
                                                      const uint8_t *ref_txt, int letters, int64_t n_jobs, int64_t *ev_off,
                                                      int32_t *ev_cnt, unsigned long long *cursor, uint32_t *status,
                                                      unsigned long long *first_bad)
{
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_jobs; j += (int64_t)gridDim.x * blockDim.x) {
        IpxEvCount cnt;
        if (res[j].cigar_len) {
            const IpxEvJob q = ipx_ev_job(j, res, cigar_pool, read_off, ref_off, ref_id, read_txt, ref_txt, letters);
            if (ipx_walk_events(q.ops, q.n_ops, q.ri, q.qi, q.read, q.read_len, q.ref, q.ref_len, cnt) != IPX_EV_OK) {
                atomicOr(status, 1u);
                atomicMin(first_bad, (unsigned long long)j);
                cnt.n = 0;
            }
        }
        ev_cnt[j] = (int32_t)cnt.n;
        ev_off[j] = cnt.n ? (int64_t)atomicAdd(cursor, (unsigned long long)cnt.n) : 0;
    }
}

// pass 2: the events themselves, into the ranges pass 1 reserved
__global__ void __launch_bounds__(256) k_events_emit(const IpxResult *res, const uint32_t *cigar_pool, const int64_t *read_off,
                                                     const int64_t *ref_off, const int32_t *ref_id, const uint8_t *read_txt,
                                                     const uint8_t *ref_txt, int letters, int64_t n_jobs, const int64_t *ev_off,
                                                     const int32_t *ev_cnt, IpxEvent *events)
{
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_jobs; j += (int64_t)gridDim.x * blockDim.x) {
        if (!ev_cnt[j]) continue;
        const IpxEvJob q = ipx_ev_job(j, res, cigar_pool, read_off, ref_off, ref_id, read_txt, ref_txt, letters);
        IpxEvWrite w{events + ev_off[j], 0};
        (void)ipx_walk_events(q.ops, q.n_ops, q.ri, q.qi, q.read, q.read_len, q.ref, q.ref_len, w);
    }
}
#endif

#endif
