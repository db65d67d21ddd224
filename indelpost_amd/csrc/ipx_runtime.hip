// ipx_runtime.hip -- host side of libindelpost_hip.so: HIP memory/stream plumbing and the C ABI of
// include/indelpost_hip.h.  HIP runtime only (no PyTorch, no vendor libraries).  Every entry
// point fails loudly when there is no GPU; nothing here computes an alignment on the CPU.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/indelpost_hip.h"
#define IPX_EXTERN_KERNELS 1      // the k_dp_pass families are instantiated in csrc/ipx_dp_*.hip
#include "ipx_pipeline.h"
#include "ipx_events.h"
static_assert(sizeof(IpxEvent) == 16 && sizeof(ipx_event) == 16, "event record is 16 bytes");

static_assert(sizeof(IpxResult) == 32 && sizeof(ipx_result) == 32, "result record is 32 bytes");

static thread_local char g_err[512] = "";
static void set_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return IPX_ERR_NO_DEVICE;                                                       \
        }                                                                                   \
    } while (0)

// grow-only device buffer
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return 0;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { set_err("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); p = nullptr; return IPX_ERR_NO_DEVICE; }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};

struct ipx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int num_cu = 256;
    // parameters
    int8_t mat[25];
    int bias = 0, flag = 1, filters = 0, filterd = 0, score_size = 2;
    int routing = 0;                   // IPX_ROUTE_* (speed only)
    bool static_valid = false;         // the job lists of the static passes match the resident batch and the parameters
    bool async_io = false;             // ipx_set_async_io: the caller keeps its input buffers valid and unchanged until the next
                                       //   ipx_sync and its output buffers until ipx_wait, so no call waits for a copy
    std::vector<int64_t> h_refp;       // host copies that outlive ipx_upload (their H2D copies are asynchronous)
    std::vector<int32_t> h_rlen;
    uint32_t h_used = 0;               // cigar ops of the last run (read back in ipx_sync)
    // resident batch
    int64_t n_jobs = 0;
    int32_t n_refs = 0;
    IpxDims dims;
    bool have_mask = false;
    DevBuf reads, read_off, refs_raw, ref_off, refs_packed, refp_off, ref_len, ref_id, gap_open, gap_ext, mask_len;
    DevBuf res, cigar_pool, small;     // small: cursor, status, plan tables, list counters
    DevBuf perm, tb_list, tb_esc, tb_bw, tb1, maxcol, tbf, long_state, rev;     // perm: three job lists of n_jobs (two static passes + one shared by the dynamic ones)
    uint32_t cigar_cap = 0;
    int64_t read_bytes = 0, ref_bytes = 0;   // letters of the resident batch (ipx_find_events copies that many)
    bool have_results = false;               // the last run of the resident batch completed (ipx_sync returned IPX_OK)
    DevBuf evt_small, evt_off, evt_cnt, evt_pool, read_txt, ref_txt;   // event pass: cursor + status, per-job ranges, events, letters
    IpxWorkspace ws;
    IpxBatch batch;
    // measurement
    bool profiling = false;
    int profiling_level = 1;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<int, int>> ev_used;   // (kernel class, index of start event; stop = +1)
    size_t ev_next = 0;
    float k_ms[IPX_NUM_KEYS];
    int k_launches[IPX_NUM_KEYS];
    int64_t k_units[IPX_NUM_KEYS];              // alignments the launches of a DP timing key processed (planner tile counts x tile size)
    int32_t k_dp_src[IPX_NUM_KEYS];             // DP timing key -> (pass * 256 + class) * 32 + alignments per tile, or -1
    uint32_t k_dp_mask[IPX_NUM_KEYS];           // ... and the classes the launch serves: class + (bits set)
    int runs_since_sync = 0;                    // ipx_run calls the next ipx_sync accounts for (same batch: same tile counts each)
    hipEvent_t run_start = nullptr, run_stop = nullptr;
    float last_run_ms = 0.f;
    int64_t dp_grid_cap = 1;                    // DP blocks per launch (each owns a column-maxima scratch region)
    uint32_t prev_tiles[IPX_NUM_PASSES * (IPX_NUM_CLASSES + 1)] = {0};   // planner tile counts of the previous run, per pass and class
    uint32_t *stats_dev = nullptr;              // ... and where the planner leaves them
    uint8_t *cls_map_dev = nullptr;             // IpxBatch::cls_map (filled from IpxDims::cls_map when the static plans are built)
    bool prev_valid = false;
    std::vector<uint32_t> sync_back;            // ipx_sync's read-back buffer
    bool speculated = false;                    // the last ipx_run left out passes predicted empty: a job found in one makes ipx_sync repeat the run
    int reruns = 0;                             // ... how often that has happened (ipx_debug_reruns)
    std::map<const void *, int> lds_attr;       // kernels whose dynamic-LDS limit was raised
};

// ---- launcher handed to ipx_run_pipeline --------------------------------------------------------
struct HipBackend {
    ipx_ctx *c;
    hipError_t err = hipSuccess;
    int dp_grid() const
    {
        // (every tile of the largest pass a block of its own, twice over for 16-job tiles; the latency tier's tiles hold 2 or 4 jobs --
        //  r04: with n / 8 its 500 tiles of a 1 000-job call got 256 blocks and every block walked two tiles, 124 us instead of 62)
        const int64_t per = c->dims.lat ? 2 * (64 / c->dims.lat) : 8;
        const int64_t g = c->n_jobs / per + IPX_NUM_CLASSES + 1;
        return (int)(g < c->dp_grid_cap ? g : c->dp_grid_cap);
    }
    // Which passes a job takes is decided on the device, so the host does not know how many tiles a DP launch will
    // find; many find none.  A block that finds nothing still has to be dispatched, and on a GPU busy with other
    // streams' kernels it waits for register space first.  So launches are sized from the tile counts the planner
    // saw in the PREVIOUS run of this context (read back in ipx_sync).  Any grid is correct (blocks stride over the
    // tiles); a wrong guess only costs speed.  (r02: a floor of 1/16 of the full grid made every launch that finds
    // nothing -- most classes of most passes -- queue a thousand blocks behind the other streams' kernels.)
    int sized(int64_t tiles) const
    {
        const int64_t full = dp_grid();
        if (!c->prev_valid) return (int)full;
        const int64_t g = tiles + tiles / 4 + 8;
        return (int)(g < full ? g : full);
    }
    int dp_grid(int pass, int cls) const { return sized(c->prev_tiles[pass * (IPX_NUM_CLASSES + 1) + cls]); }
    int sweep_grid(int pass, uint64_t covered_fast, uint64_t covered_slow) const
    {
        int64_t t = 0;
        for (int k = 0; k < IPX_NUM_CLASSES; ++k) {
            const int seg = k >= IPX_SLOW_BASE ? k - IPX_SLOW_BASE : k;
            const uint64_t cov = k >= IPX_SLOW_BASE ? covered_slow : covered_fast;
            if (!(seg < 64 && ((cov >> seg) & 1ull))) t += c->prev_tiles[pass * (IPX_NUM_CLASSES + 1) + k];
        }
        const int64_t g = sized(t), cap = (int64_t)c->num_cu * 8;
        return (int)(c->prev_valid ? g : (g < cap ? g : cap));
    }
    // planner kernels: one wave per block, IPX_PLAN_ROUNDS jobs per lane and iteration
    int plan_grid(int64_t n) const
    {
        int64_t g = (n + 64 * IPX_PLAN_ROUNDS - 1) / (64 * IPX_PLAN_ROUNDS);
        if (g < 1) g = 1;
        const int64_t cap = (int64_t)c->num_cu * 16;
        return (int)(g < cap ? g : cap);
    }
    int flat_grid(int64_t n) const
    {
        int64_t g = (n + 255) / 256;
        if (g < 1) g = 1;
        const int64_t cap = (int64_t)c->num_cu * 8;
        return (int)(g < cap ? g : cap);
    }
    void note_dp(int key, int pass, int cls, int na) { c->k_dp_src[key] = (pass * 256 + cls) * 32 + na; c->k_dp_mask[key] = 1u; }
    // a launch that serves the classes base + (bits of mask)
    void note_dp_set(int key, int pass, int base, uint32_t mask, int na) { c->k_dp_src[key] = (pass * 256 + base) * 32 + na; c->k_dp_mask[key] = mask; }
    int dp_grid_set(int pass, int base, uint32_t mask) const
    {
        int64_t t = 0;
        for (int k = 0; k < 32; ++k) if ((mask >> k) & 1u) t += c->prev_tiles[pass * (IPX_NUM_CLASSES + 1) + base + k];
        return sized(t);
    }
    void note_f16(int, int) {}
    // (latency tier) the previous run of this context planned no tile for the pass: ipx_run_pipeline may leave it out (k_tb_list guards)
    bool pass_predicted_empty(int pass) const { return c->prev_valid && c->prev_tiles[pass * (IPX_NUM_CLASSES + 1) + IPX_NUM_CLASSES] == 0; }
    void copy_u32(uint32_t *dst, const uint32_t *src, int n)
    {
        hipError_t e = hipMemcpyAsync(dst, src, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess && err == hipSuccess) err = e;
    }
    void zero_u32(uint32_t *p, int n)
    {
        hipError_t e = hipMemsetAsync(p, 0, sizeof(uint32_t) * (size_t)n, c->stream);
        if (e != hipSuccess && err == hipSuccess) err = e;
    }
    template <class K, class... A>
    void launch(int kclass, K kern, int grid, int block, int lds, A... args)
    {
        if (lds > 48 * 1024) {
            const void *key = (const void *)kern;
            auto it = c->lds_attr.find(key);
            if (it == c->lds_attr.end() || it->second < lds) {
                hipError_t e = hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
                if (e != hipSuccess && err == hipSuccess) err = e;
                c->lds_attr[key] = lds;
            }
        }
        size_t ei = 0;
        // profiling level 2 = only the striped DP kernels get events (they are the step; events around all ~75
        // launches of a run cost about 1.5 % of a 4-stream step)
        const int kc = kclass / 256;
        const bool timed = c->profiling && (c->profiling_level < 2 || ipx_k_is_dp(kc));
        if (timed) {
            if (c->ev_next + 2 > c->ev_pool.size()) {
                for (int k = 0; k < 64; ++k) { hipEvent_t e; (void)hipEventCreate(&e); c->ev_pool.push_back(e); }
            }
            ei = c->ev_next;
            c->ev_next += 2;
            (void)hipEventRecord(c->ev_pool[ei], c->stream);
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)block), (size_t)lds, c->stream, args...);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess && err == hipSuccess) err = e;
        if (timed) {
            (void)hipEventRecord(c->ev_pool[ei + 1], c->stream);
            c->ev_used.push_back(std::make_pair(kclass, (int)ei));
        }
    }
};

static const char *k_names[IPX_K_NUM] = {"init", "plan", "dp_byte_low", "dp_byte_check", "dp_byte_high", "dp_byte_exact", "dp_word_first",
                                         "dp_word_fwd", "dp_byte_rev", "dp_word_rev", "tb_list", "traceback", "pack_refs", "prove_overflow",
                                         "dp_byte_plain", "dp_byte_low2", "dp_byte_rev_plain", "prove_plain"};

extern "C" {

const char *ipx_last_error(void) { return g_err; }

int ipx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

ipx_ctx *ipx_create(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { set_err("no HIP device available (%s): libindelpost_hip has no CPU fallback", e != hipSuccess ? hipGetErrorString(e) : "device count 0"); return nullptr; }
    if (device < 0 || device >= n) { set_err("device %d out of range (0..%d)", device, n - 1); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { set_err("hipSetDevice(%d) failed", device); return nullptr; }
    ipx_ctx *c = new ipx_ctx();
    c->device = device;
    memset(&c->dims, 0, sizeof c->dims);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { set_err("hipStreamCreate failed"); delete c; return nullptr; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cu = prop.multiProcessorCount;
    (void)hipEventCreate(&c->run_start);
    (void)hipEventCreate(&c->run_stop);
    memset(c->k_ms, 0, sizeof c->k_ms);
    memset(c->k_launches, 0, sizeof c->k_launches);
    memset(c->k_units, 0, sizeof c->k_units);
    memset(c->k_dp_src, 0xFF, sizeof c->k_dp_src);
    memset(c->k_dp_mask, 0, sizeof c->k_dp_mask);
    // default scoring: SSW() class defaults, match 2 / mismatch 2 (sswpy.pyx:112)
    static const int8_t dflt[25] = {2, -2, -2, -2, 0, -2, 2, -2, -2, 0, -2, -2, 2, -2, 0, -2, -2, -2, 2, 0, 0, 0, 0, 0, 0};
    memcpy(c->mat, dflt, 25);
    c->bias = 2;
    memset(&c->ws, 0, sizeof c->ws);
    memset(&c->batch, 0, sizeof c->batch);
    return c;
}

void ipx_destroy(ipx_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (DevBuf *b : {&c->reads, &c->read_off, &c->refs_raw, &c->ref_off, &c->refs_packed, &c->refp_off, &c->ref_len,
                      &c->ref_id, &c->gap_open, &c->gap_ext, &c->mask_len, &c->res, &c->cigar_pool, &c->small, &c->perm,
                      &c->tb_list, &c->tb_esc, &c->tb_bw, &c->tb1, &c->maxcol, &c->tbf, &c->long_state, &c->rev,
                      &c->evt_small, &c->evt_off, &c->evt_cnt, &c->evt_pool, &c->read_txt, &c->ref_txt})
        b->release();
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    (void)hipEventDestroy(c->run_start);
    (void)hipEventDestroy(c->run_stop);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

int ipx_set_params(ipx_ctx *c, const int8_t *mat, int flag, int filters, int filterd, int score_size)
{
    if (!c || !mat || score_size < 0 || score_size > 2) { set_err("ipx_set_params: bad argument"); return IPX_ERR_ARG; }
    memcpy(c->mat, mat, 25);
    int bias = 0;
    for (int k = 0; k < 25; ++k) if (mat[k] < bias) bias = mat[k];          // ssw.c:795-797
    c->bias = -bias;
    c->flag = flag & 255; c->filters = filters & 0xFFFF; c->filterd = filterd; c->score_size = score_size;
    c->static_valid = false;
    c->prev_valid = false;             // (launch sizes and pass predictions learned under other parameters say nothing)
    return IPX_OK;
}

int ipx_set_routing(ipx_ctx *c, int flags)
{
    if (!c) { set_err("ipx_set_routing: null context"); return IPX_ERR_ARG; }
    c->routing = flags;
    c->static_valid = false;
    c->prev_valid = false;
    return IPX_OK;
}

int ipx_upload(ipx_ctx *c, const int8_t *reads, const int64_t *read_off, const int8_t *refs,
               const int64_t *ref_off, const int32_t *ref_id, const uint8_t *gap_open,
               const uint8_t *gap_ext, const int32_t *mask_len, int64_t n_jobs, int32_t n_refs)
{
    if (!c || n_jobs < 0 || n_refs < 0 || !read_off || !ref_off || (n_jobs > 0 && (!ref_id || !gap_open || !gap_ext))) {
        set_err("ipx_upload: bad argument");
        return IPX_ERR_ARG;
    }
    if (n_jobs >= (1ll << 31)) { set_err("ipx_upload: more than 2^31 jobs in one batch"); return IPX_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const int64_t read_bytes = read_off[n_jobs], ref_bytes = ref_off[n_refs];
    // host-side geometry: packed (4-byte aligned, padded) window offsets and the batch maxima
    if (c->async_io) HIPCHK(hipStreamSynchronize(c->stream));   // (the previous upload's copies read h_refp / h_rlen)
    // Everything is validated into locals first: an upload rejected by VALIDATION leaves the resident batch (and its plans) as they were.
    // Past that point buffers are reallocated and overwritten: an upload that fails there (allocation, copy) leaves the context with NO
    // resident batch (n_jobs = 0: ipx_run then does nothing) rather than new dimensions over partly stale buffers.
    std::vector<int64_t> refp((size_t)n_refs + 1, 0);
    std::vector<int32_t> rlen((size_t)n_refs + 1, 0);
    std::vector<IpxDims> dloc(1);
    IpxDims &d = dloc[0];
    memset(&d, 0, sizeof d);
    int64_t tot = 0;
    for (int32_t r = 0; r < n_refs; ++r) {
        const int64_t len = ref_off[r + 1] - ref_off[r];
        if (len < 0 || len > IPX_MAX_REFLEN) { set_err("window %d has length %lld (limit %d)", r, (long long)len, IPX_MAX_REFLEN); return IPX_ERR_REF_TOO_LONG; }
        refp[r] = tot; rlen[r] = (int32_t)len;
        tot += ((len + 3) & ~3ll) + IPX_REF_PAD;
        if (len > d.max_ref_len) d.max_ref_len = (int)len;
    }
    for (int64_t i = 0; i < n_jobs; ++i) {
        const int64_t len = read_off[i + 1] - read_off[i];
        if (len < 0 || len > IPX_LONG_MAX_READ) { set_err("read %lld has length %lld (limit %d)", (long long)i, (long long)len, IPX_LONG_MAX_READ); return IPX_ERR_READ_TOO_LONG; }
        ipx_dims_add_read(d, (int)len, gap_open[i] <= gap_ext[i]);
        if (ref_id[i] < 0 || ref_id[i] >= n_refs) { set_err("job %lld: ref_id %d out of range", (long long)i, ref_id[i]); return IPX_ERR_ARG; }
    }
    c->h_refp.swap(refp);
    c->h_rlen.swap(rlen);
    c->dims = d;
    c->static_valid = false;
    // launch sizes learned from the previous run only carry over to a batch of similar size
    if (c->prev_valid && (n_jobs > 2 * c->n_jobs || 2 * n_jobs < c->n_jobs)) c->prev_valid = false;
    c->have_results = false;
    c->n_jobs = 0; c->n_refs = 0; c->batch.n_jobs = 0;           // (committed at the end, when every allocation and copy has been issued)
    c->have_mask = mask_len != nullptr;

    if (c->reads.ensure((size_t)read_bytes + 64) || c->read_off.ensure(8 * ((size_t)n_jobs + 1)) ||
        c->refs_raw.ensure((size_t)ref_bytes + 64) || c->ref_off.ensure(8 * ((size_t)n_refs + 1)) ||
        c->refs_packed.ensure((size_t)tot + 64) || c->refp_off.ensure(8 * ((size_t)n_refs + 1)) ||
        c->ref_len.ensure(4 * ((size_t)n_refs + 1)) || c->ref_id.ensure(4 * (size_t)n_jobs + 4) ||
        c->gap_open.ensure((size_t)n_jobs + 4) || c->gap_ext.ensure((size_t)n_jobs + 4) ||
        (mask_len && c->mask_len.ensure(4 * (size_t)n_jobs + 4)) || c->res.ensure(32 * (size_t)n_jobs + 32) ||
        c->perm.ensure(12 * (size_t)n_jobs + 16) || c->tb_list.ensure(4 * (size_t)IPX_TB_NLISTS * (size_t)n_jobs + 32) ||
        c->tb_esc.ensure(4 * (size_t)n_jobs + 4) || c->tb_bw.ensure(2 * (size_t)n_jobs + 4) ||
        c->small.ensure(4 * ((size_t)IPX_PLAN_TABLE_WORDS + (size_t)IPX_NUM_PASSES * 3 * (IPX_NUM_CLASSES + 1) + IPX_NUM_CLASSES + 64 + (IPX_NUM_PASSES * IPX_NUM_CLASSES + 3) / 4)))
        return IPX_ERR_NO_DEVICE;
    if (c->cigar_cap < (uint32_t)(n_jobs * 8 + 1024)) c->cigar_cap = (uint32_t)(n_jobs * 8 + 1024);
    if (c->cigar_pool.ensure(4 * (size_t)c->cigar_cap)) return IPX_ERR_NO_DEVICE;

    hipStream_t s = c->stream;
    if (read_bytes) HIPCHK(hipMemcpyAsync(c->reads.p, reads, (size_t)read_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->read_off.p, read_off, 8 * ((size_t)n_jobs + 1), hipMemcpyHostToDevice, s));
    if (ref_bytes) HIPCHK(hipMemcpyAsync(c->refs_raw.p, refs, (size_t)ref_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->ref_off.p, ref_off, 8 * ((size_t)n_refs + 1), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->refp_off.p, c->h_refp.data(), 8 * ((size_t)n_refs + 1), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->ref_len.p, c->h_rlen.data(), 4 * ((size_t)n_refs + 1), hipMemcpyHostToDevice, s));
    if (n_jobs) {
        HIPCHK(hipMemcpyAsync(c->ref_id.p, ref_id, 4 * (size_t)n_jobs, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->gap_open.p, gap_open, (size_t)n_jobs, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->gap_ext.p, gap_ext, (size_t)n_jobs, hipMemcpyHostToDevice, s));
        if (mask_len) HIPCHK(hipMemcpyAsync(c->mask_len.p, mask_len, 4 * (size_t)n_jobs, hipMemcpyHostToDevice, s));
    }
    // without the caller's promise (ipx_set_async_io) the copies above may still be reading its buffers: finish them
    if (!c->async_io) HIPCHK(hipStreamSynchronize(s));
    // re-pack the windows on the device (4-byte aligned starts, padded, codes sanitised)
    HipBackend be{c};
    const bool prof = c->profiling;
    c->profiling = false;
    if (n_refs > 0)
        be.launch(IPX_KEY(IPX_K_PACK, 0), k_pack_refs, be.flat_grid((int64_t)n_refs * 64), 256, 0, (const int8_t *)c->refs_raw.p,
                  (const int64_t *)c->ref_off.p, (const int64_t *)c->refp_off.p, (int8_t *)c->refs_packed.p, n_refs);
    c->profiling = prof;
    if (be.err != hipSuccess) { set_err("k_pack_refs launch failed: %s", hipGetErrorString(be.err)); return IPX_ERR_NO_DEVICE; }

    // traceback scratch: direction words of the fast kernels, direction bytes + CIGAR runs of the general kernel
    const IpxTbSizing s1 = ipx_tb1_sizing(d);
    int wf = (int)((n_jobs + 63) / 64);
    if (wf < 1) wf = 1;
    if (wf > c->num_cu * 16) wf = c->num_cu * 16;
    if (wf < 7 * ((int)((n_jobs + 63) / 64) + 1) && n_jobs <= 65536)        // room for the all-widths launch of small batches
        wf = 7 * ((int)((n_jobs + 63) / 64) + 1);
    c->ws.tbf_waves = wf;
    {
        const int want = d.max_read_len > 0 ? d.max_read_len : 1;
        const int rowcap = want < IPX_TBF_ROWCAP ? want : IPX_TBF_ROWCAP;
        if (c->tbf.ensure(ipx_tbf_scratch_bytes_per_block(rowcap) * (size_t)wf + 64)) return IPX_ERR_NO_DEVICE;
        c->ws.tbf_scratch = c->tbf.as<unsigned char>();
    }
    int w1 = c->num_cu * 16;                                  // one job per block in k_tb_coop (latency-bound: many blocks)
    const size_t lim1 = 1024ull << 20;
    while (w1 > 1 && ipx_tbc_bytes_per_block(s1) * (size_t)w1 > lim1) w1 /= 2;
    if (w1 < 64) {
        // reads of kilobases against windows of tens of kilobases: a block's region (direction bytes for the widest band the rectangle allows)
        // is tens of megabytes and a gigabyte holds a handful -- 2 kb against 20 kb: 8 jobs at a time, 111 ms of traceback for 256 reads whose
        // DP passes take 28 (r04, k_dp_wide).  The card has 288 GB: up to 64 regions, within 16 GB and a sixteenth of what is free
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            size_t cap = free_b / 16;
            if (cap > (16ull << 30)) cap = 16ull << 30;
            int w = 64;
            while (w > w1 && ipx_tbc_bytes_per_block(s1) * (size_t)w > cap) w /= 2;
            if (w > w1) w1 = w;
        }
    }
    c->ws.tb1_waves = w1;
    if (c->tb1.ensure(ipx_tbc_bytes_per_block(s1) * (size_t)w1)) return IPX_ERR_NO_DEVICE;
    memset(&c->ws.tb1, 0, sizeof c->ws.tb1);
    c->ws.tb1.arrcap = s1.arrcap; c->ws.tb1.dircap = (int32_t)(((size_t)s1.dircap + 15) & ~(size_t)15); c->ws.tb1.cigcap = s1.cigcap;
    c->ws.tb1.dir = c->tb1.as<uint8_t>();
    c->ws.tb1.cig = (uint32_t *)(c->tb1.as<char>() + (size_t)c->ws.tb1.dircap * (size_t)w1);
    c->ws.tb1.arrcap_lds = s1.arrcap_lds;
    c->ws.tb1.band = s1.arrcap > s1.arrcap_lds ? (int32_t *)((char *)c->ws.tb1.cig + (((4ull * (size_t)s1.cigcap * (size_t)w1) + 15) & ~15ull)) : nullptr;

    // column-maxima scratch of the forward passes: one region per DP block
    {
        const size_t per_block = 16 * (size_t)(d.max_ref_len + 8) * 4;
        int64_t cap = (int64_t)c->num_cu * IPX_DP_WAVES_PER_CU;
        // never below the resident count for ordinary windows; very long windows (tens of kilobases) keep to twice the budget instead
        const int64_t fit = (int64_t)(IPX_DP_SCRATCH_BUDGET / per_block), floor_ = (int64_t)c->num_cu * 24, hard = (int64_t)(2 * IPX_DP_SCRATCH_BUDGET / per_block);
        if (cap > fit) cap = fit > floor_ ? fit : (floor_ < hard ? floor_ : (hard > 64 ? hard : 64));
        c->dp_grid_cap = cap;
        if (c->maxcol.ensure((size_t)cap * per_block)) return IPX_ERR_NO_DEVICE;
    }

    // striped columns of reads beyond the register-resident kernels (k_dp_long): one region per block, only when such reads exist
    c->ws.long_state = nullptr; c->ws.long_stride = 0; c->ws.long_blocks = 0;
    if (d.max_read_len > 8 * (IPX_MAX_SEG - 1)) {          // class 64 ("64 segments or more") can occur: from 505 bp in the 16-bit passes
        const size_t stride = ipx_long_state_bytes(d.max_read_len);
        int blocks = 256;
        if ((int64_t)blocks > c->dp_grid_cap) blocks = (int)c->dp_grid_cap;
        if (c->long_state.ensure(stride * (size_t)blocks)) return IPX_ERR_NO_DEVICE;
        c->ws.long_state = c->long_state.as<unsigned char>(); c->ws.long_stride = (int64_t)stride; c->ws.long_blocks = blocks;
    }

    // small tables: count + cursor of every pass, class and tile offsets of every pass, planner statistics
    uint32_t *sm = c->small.as<uint32_t>();
    c->ws.plan_tables = sm; sm += IPX_PLAN_TABLE_WORDS;
    uint32_t *offs = sm; sm += (size_t)IPX_NUM_PASSES * 2 * (IPX_NUM_CLASSES + 1);
    uint32_t *cursor = sm; sm += 4;                           // cursor (4 words), status (4 words) and the planner statistics are neighbours:
    uint32_t *status = sm; sm += 4;                           //   ipx_sync reads all three back with ONE copy
    c->stats_dev = sm; sm += (size_t)IPX_NUM_PASSES * (IPX_NUM_CLASSES + 1);
    c->ws.exact_starters = sm; sm += IPX_NUM_CLASSES;
    for (int ps = 0; ps < IPX_NUM_PASSES; ++ps) {
        IpxPlan &p = c->ws.plan[ps];
        p.count = ipx_plan_count_of(c->ws.plan_tables, ps);
        p.cursor = p.count + IPX_NUM_CLASSES;
        p.cls_off = offs + (size_t)ps * 2 * (IPX_NUM_CLASSES + 1);
        p.tile_off = p.cls_off + IPX_NUM_CLASSES + 1;
        p.perm = c->perm.as<uint32_t>() + (size_t)(ps < IPX_FIRST_DYNAMIC_PASS ? ps : IPX_FIRST_DYNAMIC_PASS) * (size_t)n_jobs;
        p.stats = c->stats_dev + (size_t)ps * (IPX_NUM_CLASSES + 1);
    }
    c->ws.tb_list = c->tb_list.as<uint32_t>();
    c->ws.tb_esc = c->tb_esc.as<uint32_t>();
    c->ws.tb_list_n = sm; sm += IPX_TB_NCOUNTERS;
    c->ws.tb_esc_n = c->ws.tb_list_n + IPX_TB_CLS_COOP;
    c->cls_map_dev = (uint8_t *)sm; sm += (IPX_NUM_PASSES * IPX_NUM_CLASSES + 3) / 4;
    HIPCHK(hipMemsetAsync(c->small.p, 0, 4 * (size_t)(sm - c->small.as<uint32_t>()), s));

    IpxBatch &b = c->batch;
    memset(&b, 0, sizeof b);
    b.n_jobs = n_jobs; b.n_refs = n_refs;
    b.reads = c->reads.as<int8_t>(); b.read_off = c->read_off.as<int64_t>();
    b.refs_packed = c->refs_packed.as<int8_t>(); b.refp_off = c->refp_off.as<int64_t>();
    b.ref_len = c->ref_len.as<int32_t>(); b.ref_id = c->ref_id.as<int32_t>();
    b.gap_open = c->gap_open.as<uint8_t>(); b.gap_ext = c->gap_ext.as<uint8_t>();
    b.mask_len = mask_len ? c->mask_len.as<int32_t>() : nullptr;
    b.res = c->res.as<IpxResult>();
    b.cigar_pool = c->cigar_pool.as<uint32_t>(); b.cigar_cap = c->cigar_cap;
    b.cigar_cursor = cursor; b.status = status;
    b.plan_counts = c->ws.plan_tables;
    b.maxcol_scratch = c->maxcol.as<uint32_t>();
    b.tb_bw = c->tb_bw.as<uint16_t>();
    c->ws.tbd_waves = c->num_cu * 8;                         // k_tb_diag: 21 KB of LDS per one-wave block, seven resident per CU
    {   // banded reverse pass: two job lists, counters per class, the second list's class / tile offsets
        if (c->rev.ensure(4 * ipx_rev_words(n_jobs))) return IPX_ERR_NO_DEVICE;
        uint32_t *rv = c->rev.as<uint32_t>();
        c->ws.rev_listA = rv; c->ws.rev_listB = rv + n_jobs; c->ws.rev_cnt = rv + 2 * (size_t)n_jobs;
        c->ws.rev_cls_off = c->ws.rev_cnt + 2 * IPX_NUM_CLASSES; c->ws.rev_tile_off = c->ws.rev_cls_off + IPX_NUM_CLASSES + 2;
    }
    if (!c->async_io) HIPCHK(hipStreamSynchronize(s));
    c->n_jobs = n_jobs; c->n_refs = n_refs;
    c->read_bytes = read_bytes; c->ref_bytes = ref_bytes;
    return IPX_OK;
}

static int ipx_run_impl(ipx_ctx *c, bool allow_speculation)
{
    if (!c) { set_err("ipx_run: null context"); return IPX_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    c->have_results = false;
    IpxBatch &b = c->batch;
    memcpy(b.mat, c->mat, 25);
    b.word_first_len = (c->routing & IPX_ROUTE_NO_WORD_FIRST) ? 0 : ipx_word_first_len(c->mat, c->bias);
    b.use_bracket = ipx_perm_profile_ok(c->mat, c->routing) && !(c->routing & IPX_ROUTE_NO_BRACKET);
    b.bracket_min_len = ipx_bracket_min_len(c->mat);
    b.f16_max_len = ipx_f16_max_len(c->mat);
    b.byte_safe_len = ipx_byte_safe_len(c->mat, c->bias);
    { int mx = 0; for (int k = 0; k < 25; ++k) if (c->mat[k] > mx) mx = c->mat[k]; b.max_match = mx; }
    b.exact_direct = ipx_perm_profile_ok(c->mat, c->routing) && !(c->routing & IPX_ROUTE_NO_EXACT_DIRECT);   // (the stepped selector-profile kernels: cheap where no cut can happen)
    b.tb_diag = !(c->routing & IPX_ROUTE_TB_NO_DIAG);
    b.lat_prio = !(c->routing & IPX_ROUTE_NO_SETPRIO);
    b.bias = c->bias; b.flag = (uint8_t)c->flag; b.score_size = (uint8_t)c->score_size;
    b.filters = (uint16_t)c->filters; b.filterd = c->filterd;
    b.cigar_pool = c->cigar_pool.as<uint32_t>(); b.cigar_cap = c->cigar_cap;
    HipBackend be{c};
    const bool first_run = !c->static_valid && c->n_jobs > 0;
    if (first_run || c->n_jobs == 0) be.zero_u32(b.status, 1);   // (later runs: k_init clears it with the other per-run tables)
    if (!c->static_valid && c->n_jobs > 0) {
        // first run of this batch under these parameters: the job lists of the passes every job starts in
        ipx_plan_classes(c->dims, b, c->routing);
        b.plain_first = c->dims.plain_first;
        b.plain_max_len = c->dims.plain_max_len;
        b.cls_map = c->cls_map_dev;
        HIPCHK(hipMemcpyAsync(c->cls_map_dev, &c->dims.cls_map[0][0], sizeof c->dims.cls_map, hipMemcpyHostToDevice, c->stream));
        ipx_dims_finish(c->dims, b.word_first_len, c->score_size,
                        b.plain_first ? 0 : ipx_exact_start_len(b.byte_safe_len, b.bracket_min_len, b.use_bracket));
        const bool prof = c->profiling;
        c->profiling = false;
        ipx_build_static_plans(be, b, c->ws, c->dims, c->routing);
        c->profiling = prof;
        c->static_valid = true;
    }
    HIPCHK(hipEventRecord(c->run_start, c->stream));
    // speculation on which passes are empty (latency tier): from the previous run of this context, also across batches of similar size
    c->speculated = allow_speculation && c->prev_valid && c->dims.lat != 0 && (7 & c->flag) != 0 && !(c->routing & IPX_ROUTE_NO_SPECULATE);
    if (c->n_jobs > 0) ipx_run_pipeline(be, b, c->ws, c->dims, c->routing, !first_run, c->speculated);
    ++c->runs_since_sync;
    HIPCHK(hipEventRecord(c->run_stop, c->stream));
    if (be.err != hipSuccess) { set_err("kernel launch failed: %s", hipGetErrorString(be.err)); return IPX_ERR_NO_DEVICE; }
    return IPX_OK;
}

int ipx_run(ipx_ctx *c) { return ipx_run_impl(c, true); }

int ipx_sync(ipx_ctx *c)
{
    if (!c) { set_err("ipx_sync: null context"); return IPX_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)hipEventElapsedTime(&c->last_run_ms, c->run_start, c->run_stop);
    if (c->profiling) {
        for (auto &u : c->ev_used) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->ev_pool[(size_t)u.second], c->ev_pool[(size_t)u.second + 1]) == hipSuccess) {
                c->k_ms[u.first] += ms;
                c->k_launches[u.first] += 1;
            }
        }
        c->ev_used.clear();
        c->ev_next = 0;
    }
    if (c->n_jobs == 0) { c->runs_since_sync = 0; return IPX_OK; }
    uint32_t st = 0;
    // cursor, status and the planner's tile counts in one read-back (neighbours in the small-table buffer)
    std::vector<uint32_t> &back = c->sync_back;
    back.resize(8 + sizeof c->prev_tiles / 4);
    const size_t back_bytes = c->stats_dev ? 4 * back.size() : 32;
    HIPCHK(hipMemcpy(back.data(), c->batch.cigar_cursor, back_bytes, hipMemcpyDeviceToHost));
    if ((back[4] & IPX_STATUS_RERUN) && c->speculated) {
        // a job sat in a pass that was predicted empty and left out (ipx_run_pipeline, speculation): the whole run again, every pass launched
        ++c->reruns;
        const int rc = ipx_run_impl(c, false);
        if (rc != IPX_OK) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
        (void)hipEventElapsedTime(&c->last_run_ms, c->run_start, c->run_stop);
        HIPCHK(hipMemcpy(back.data(), c->batch.cigar_cursor, back_bytes, hipMemcpyDeviceToHost));
        --c->runs_since_sync;
    }
    c->h_used = back[0];
    st = back[4];
    if (c->stats_dev) {
        memcpy(c->prev_tiles, back.data() + 8, sizeof c->prev_tiles);
        c->prev_valid = true;
        if (c->profiling)
            for (int k = 0; k < IPX_NUM_KEYS; ++k)
                if (c->k_dp_src[k] >= 0) {
                    const int na = c->k_dp_src[k] & 31, pc = c->k_dp_src[k] >> 5;
                    for (int q = 0; q < 32; ++q)
                        if ((c->k_dp_mask[k] >> q) & 1u)
                            c->k_units[k] += (int64_t)c->prev_tiles[(pc >> 8) * (IPX_NUM_CLASSES + 1) + (pc & 255) + q] * na * c->runs_since_sync;
                }
    }
    c->runs_since_sync = 0;
    if (st & IPX_STATUS_READ_TOO_LONG) { set_err("a read needs more than %d striped segments", IPX_MAX_SEG); return IPX_ERR_READ_TOO_LONG; }
    if (st & IPX_STATUS_REF_TOO_LONG) { set_err("a window is longer than %d", IPX_MAX_REFLEN); return IPX_ERR_REF_TOO_LONG; }
    if (st & IPX_STATUS_CIGAR_POOL) { set_err("device cigar pool exhausted (%u ops)", c->cigar_cap); return IPX_ERR_CIGAR_POOL; }
    if (st & IPX_STATUS_TB_SCRATCH) { set_err("traceback scratch exhausted"); return IPX_ERR_INTERNAL; }
    if (st & IPX_STATUS_INTERNAL) { set_err("internal: a kernel variant met a job it was not built for"); return IPX_ERR_INTERNAL; }
    if (st & IPX_STATUS_RERUN) { set_err("internal: a job was left in a pass that did not run"); return IPX_ERR_INTERNAL; }
    c->have_results = true;
    return IPX_OK;
}

int ipx_download(ipx_ctx *c, ipx_result *out, uint32_t *cigar_pool, int64_t cigar_cap, int64_t *n_cigar_ops)
{
    if (!c || (c->n_jobs > 0 && !out)) { set_err("ipx_download: bad argument"); return IPX_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    uint32_t used = 0;
    if (c->n_jobs > 0) {
        HIPCHK(hipMemcpy(out, c->res.p, 32 * (size_t)c->n_jobs, hipMemcpyDeviceToHost));
        if (c->runs_since_sync == 0) used = c->h_used;        // (read back by ipx_sync)
        else HIPCHK(hipMemcpy(&used, c->batch.cigar_cursor, 4, hipMemcpyDeviceToHost));
    }
    if (n_cigar_ops) *n_cigar_ops = used;
    if (used) {
        if (!cigar_pool || (int64_t)used > cigar_cap) { set_err("cigar pool of %lld ops is too small, %u needed", (long long)cigar_cap, used); return IPX_ERR_CIGAR_POOL; }
        HIPCHK(hipMemcpy(cigar_pool, c->cigar_pool.p, 4 * (size_t)used, hipMemcpyDeviceToHost));
    }
    return IPX_OK;
}

int ipx_set_async_io(ipx_ctx *c, int on)
{
    if (!c) { set_err("ipx_set_async_io: null context"); return IPX_ERR_ARG; }
    c->async_io = on != 0;
    return IPX_OK;
}

int ipx_pin_host(void *p, int64_t bytes)
{
    if (!p || bytes <= 0) { set_err("ipx_pin_host: bad argument"); return IPX_ERR_ARG; }
    hipError_t e = hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); set_err("hipHostRegister(%lld bytes) failed: %s", (long long)bytes, hipGetErrorString(e)); return IPX_ERR_NO_DEVICE; }
    return IPX_OK;
}

int ipx_unpin_host(void *p)
{
    if (!p) return IPX_ERR_ARG;
    if (hipHostUnregister(p) == hipSuccess) return IPX_OK;
    (void)hipGetLastError();                     // (HIP keeps the failure as its sticky "last error": the next launch check would report it)
    set_err("hipHostUnregister failed: the buffer was not page-locked by ipx_pin_host");
    return IPX_ERR_NO_DEVICE;
}

// After ipx_sync: start copying the records and the CIGAR ops of the last run into the caller's buffers on the context's
// stream and return; ipx_wait completes it.  (With pinned buffers the copy runs beside the other contexts' kernels.)
int ipx_download_async(ipx_ctx *c, ipx_result *out, uint32_t *cigar_pool, int64_t cigar_cap, int64_t *n_cigar_ops)
{
    if (!c || (c->n_jobs > 0 && !out)) { set_err("ipx_download_async: bad argument"); return IPX_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const uint32_t used = c->n_jobs > 0 ? c->h_used : 0;
    if (n_cigar_ops) *n_cigar_ops = used;
    if (used && (!cigar_pool || (int64_t)used > cigar_cap)) { set_err("cigar pool of %lld ops is too small, %u needed", (long long)cigar_cap, used); return IPX_ERR_CIGAR_POOL; }
    if (c->n_jobs > 0) HIPCHK(hipMemcpyAsync(out, c->res.p, 32 * (size_t)c->n_jobs, hipMemcpyDeviceToHost, c->stream));
    if (used) HIPCHK(hipMemcpyAsync(cigar_pool, c->cigar_pool.p, 4 * (size_t)used, hipMemcpyDeviceToHost, c->stream));
    return IPX_OK;
}

int ipx_wait(ipx_ctx *c)
{
    if (!c) { set_err("ipx_wait: null context"); return IPX_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return IPX_OK;
}

// The event pass over the last run (include/indelpost_hip.h): two lane-per-job launches on the context's stream -- k_events_count
// sizes every job's range of the pool and reserves it, k_events_emit walks again and writes -- then one read-back.  Nothing is
// written to the caller's buffers unless all of it fits.
int ipx_find_events(ipx_ctx *c, const uint8_t *read_text, const uint8_t *ref_text, int64_t *event_off, int32_t *event_count,
                    ipx_event *events, int64_t cap, int64_t *n_events)
{
    if (!c || !n_events || (read_text == nullptr) != (ref_text == nullptr) || cap < 0) {
        set_err("ipx_find_events: bad argument (the read and window letters go together: both or neither)");
        return IPX_ERR_ARG;
    }
    *n_events = 0;
    if (c->n_jobs > 0 && (!c->have_results || c->runs_since_sync != 0)) { set_err("ipx_find_events: no completed run (ipx_run + ipx_sync first)"); return IPX_ERR_ARG; }
    if (c->n_jobs == 0) return IPX_OK;
    if (!event_off || !event_count) { set_err("ipx_find_events: bad argument"); return IPX_ERR_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const int64_t n = c->n_jobs;
    const int letters = read_text != nullptr;
    hipStream_t s = c->stream;
    if (c->evt_small.ensure(64) || c->evt_off.ensure(8 * (size_t)n) || c->evt_cnt.ensure(4 * (size_t)n)) return IPX_ERR_NO_DEVICE;
    if (letters) {
        if (c->read_txt.ensure((size_t)c->read_bytes + 64) || c->ref_txt.ensure((size_t)c->ref_bytes + 64)) return IPX_ERR_NO_DEVICE;
        if (c->read_bytes) HIPCHK(hipMemcpyAsync(c->read_txt.p, read_text, (size_t)c->read_bytes, hipMemcpyHostToDevice, s));
        if (c->ref_bytes) HIPCHK(hipMemcpyAsync(c->ref_txt.p, ref_text, (size_t)c->ref_bytes, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemsetAsync(c->evt_small.p, 0, 16, s));                 // cursor, status
    HIPCHK(hipMemsetAsync(c->evt_small.as<char>() + 16, 0xFF, 8, s));  // lowest job whose walk failed: none
    const int block = 256;
    int64_t g = (n + block - 1) / block;
    if (g > (int64_t)c->num_cu * 16) g = (int64_t)c->num_cu * 16;
    const IpxBatch &b = c->batch;
    unsigned long long *cursor = c->evt_small.as<unsigned long long>();
    uint32_t *status = (uint32_t *)(cursor + 1);
    unsigned long long *first_bad = cursor + 2;
    hipLaunchKernelGGL(k_events_count, dim3((unsigned)g), dim3(block), 0, s, (const IpxResult *)b.res, (const uint32_t *)b.cigar_pool,
                       (const int64_t *)b.read_off, c->ref_off.as<const int64_t>(), (const int32_t *)b.ref_id, c->read_txt.as<const uint8_t>(),
                       c->ref_txt.as<const uint8_t>(), letters, n, c->evt_off.as<int64_t>(), c->evt_cnt.as<int32_t>(), cursor, status, first_bad);
    HIPCHK(hipGetLastError());
    uint64_t back[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(back, c->evt_small.p, 24, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if ((uint32_t)back[1]) { set_err("internal: the CIGAR walk of job %lld starts at a negative index or leaves 32-bit indices", (long long)back[2]); return IPX_ERR_INTERNAL; }
    const int64_t total = (int64_t)back[0];
    *n_events = total;
    if (total > cap || (total > 0 && !events)) {
        set_err("event pool of %lld events is too small, %lld needed", (long long)cap, (long long)total);
        return IPX_ERR_EVENT_POOL;
    }
    if (total > 0) {
        if (c->evt_pool.ensure(16 * (size_t)total)) return IPX_ERR_NO_DEVICE;
        hipLaunchKernelGGL(k_events_emit, dim3((unsigned)g), dim3(block), 0, s, (const IpxResult *)b.res, (const uint32_t *)b.cigar_pool,
                           (const int64_t *)b.read_off, c->ref_off.as<const int64_t>(), (const int32_t *)b.ref_id, c->read_txt.as<const uint8_t>(),
                           c->ref_txt.as<const uint8_t>(), letters, n, c->evt_off.as<const int64_t>(), c->evt_cnt.as<const int32_t>(),
                           c->evt_pool.as<IpxEvent>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(events, c->evt_pool.p, 16 * (size_t)total, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(event_off, c->evt_off.p, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(event_count, c->evt_cnt.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return IPX_OK;
}

int ipx_align_batch(ipx_ctx *c, const int8_t *reads, const int64_t *read_off, const int8_t *refs,
                    const int64_t *ref_off, const int32_t *ref_id, const uint8_t *gap_open,
                    const uint8_t *gap_ext, const int32_t *mask_len, int64_t n_jobs, int32_t n_refs,
                    ipx_result *out, uint32_t *cigar_pool, int64_t cigar_cap, int64_t *n_cigar_ops)
{
    int rc = ipx_upload(c, reads, read_off, refs, ref_off, ref_id, gap_open, gap_ext, mask_len, n_jobs, n_refs);
    if (rc) return rc;
    for (int attempt = 0; attempt < 6; ++attempt) {
        if ((rc = ipx_run(c))) return rc;
        rc = ipx_sync(c);
        if (rc != IPX_ERR_CIGAR_POOL) break;
        // device pool too small for this batch: grow and re-run (results are recomputed from scratch)
        uint64_t want = (uint64_t)c->cigar_cap * 4ull;
        if (want > 0xFFFFFF00ull) return rc;
        c->cigar_cap = (uint32_t)want;
        if (c->cigar_pool.ensure(4 * (size_t)c->cigar_cap)) return IPX_ERR_NO_DEVICE;
    }
    if (rc) return rc;
    return ipx_download(c, out, cigar_pool, cigar_cap, n_cigar_ops);
}

int ipx_set_profiling(ipx_ctx *c, int on)
{
    if (!c) return IPX_ERR_ARG;
    c->profiling = on != 0;
    c->profiling_level = on >= 2 ? 2 : 1;
    memset(c->k_ms, 0, sizeof c->k_ms);
    memset(c->k_launches, 0, sizeof c->k_launches);
    memset(c->k_units, 0, sizeof c->k_units);
    return IPX_OK;
}
int ipx_num_kernel_classes(void) { return IPX_NUM_KEYS; }
const char *ipx_kernel_class_name(int k)
{
    // key = kernel class * 128 + sub; DP kernels are named after their segLen instantiation
    static thread_local char buf[64];
    if (k < 0 || k >= IPX_NUM_KEYS) return "";
    const int kc = k / 256, sub = k % 256;
    if (ipx_k_is_dp(kc)) {
        if (sub == IPX_SUB_GENERIC) snprintf(buf, sizeof buf, "%s_long", k_names[kc]);
        else if (sub == IPX_SUB_LONG) snprintf(buf, sizeof buf, "%s_kb_loops", k_names[kc]);      // k_dp_long: reads of 64 segments or more, the transcribed loops
        else if (sub == IPX_SUB_WIDE) snprintf(buf, sizeof buf, "%s_kb_wavefront", k_names[kc]);  // k_dp_wide: ... one wavefront per read
        else if (sub == IPX_SUB_BAND) snprintf(buf, sizeof buf, "%s_band", k_names[kc]);          // k_dp_band_rev: the reverse pass as a band (every class of the pass)
        else if (sub >= IPX_SUB_TIER) snprintf(buf, sizeof buf, "%s_tier%d", k_names[kc], sub - IPX_SUB_TIER);
        else if (sub >= IPX_SLOW_BASE) snprintf(buf, sizeof buf, "%s_slowgap_s%d", k_names[kc], sub - IPX_SLOW_BASE);
        else snprintf(buf, sizeof buf, "%s_s%d", k_names[kc], sub);
    } else if (kc == IPX_K_TRACEBACK) { if (sub == 9) snprintf(buf, sizeof buf, "%s_fast_all", k_names[kc]); else if (sub == 10) snprintf(buf, sizeof buf, "%s_fast_bw4to7", k_names[kc]); else if (sub >= 16 && sub <= 18) snprintf(buf, sizeof buf, "%s_diag%d", k_names[kc], 16 << (sub - 16)); else if (sub == 1) snprintf(buf, sizeof buf, "%s_coop", k_names[kc]); else if (sub >= 2) snprintf(buf, sizeof buf, "%s_fast_bw%d", k_names[kc], sub - 1); else snprintf(buf, sizeof buf, "%s_tier%d", k_names[kc], sub); }
    else snprintf(buf, sizeof buf, "%s", k_names[kc]);
    return buf;
}
int ipx_kernel_times(ipx_ctx *c, float *ms, int *launches)
{
    if (!c) return IPX_ERR_ARG;
    for (int k = 0; k < IPX_NUM_KEYS; ++k) { if (ms) ms[k] = c->k_ms[k]; if (launches) launches[k] = c->k_launches[k]; }
    return IPX_OK;
}
int ipx_kernel_units(ipx_ctx *c, int64_t *units)
{
    if (!c || !units) return IPX_ERR_ARG;
    for (int k = 0; k < IPX_NUM_KEYS; ++k) units[k] = c->k_units[k];
    return IPX_OK;
}
float ipx_last_run_ms(ipx_ctx *c) { return c ? c->last_run_ms : 0.f; }

// diagnostic: traceback routing of the last run -- out[0..6] jobs per first band width 1..7, out[7] jobs
// handed to the general (one wave per job) kernel, out[8] unused
int ipx_debug_reruns(ipx_ctx *c) { return c ? c->reruns : -1; }

int ipx_debug_tb_counts(ipx_ctx *c, uint32_t *out)
{
    if (!c || !out || !c->ws.tb_list_n) return IPX_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(out, c->ws.tb_list_n, 11 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    out[11] = 0;
    return IPX_OK;
}

// ---- many loci as one batch (r04): the host-side concatenation of per-locus job tables ---------------------------------------------
// desc: n_tables x 10 int64 -- addresses of a table's reads, read_off, refs, ref_off, ref_id, gap_open, gap_ext, mask_len (0: none), then
// its n_jobs and n_refs (indelpost_amd.batch.JobTable.desc).  ipx_concat_sizes: totals[4] = read bytes, window bytes, jobs, windows, and
// whether every table has a mask_len (return value 1) -- the caller allocates; ipx_concat_tables fills: jobs in table order, windows
// renumbered, offsets rebased.  Plain memcpy per table: 12 500 loci of 96 jobs take ~2 ms where numpy's list handling took 39.
int ipx_concat_sizes(const int64_t *desc, int64_t n_tables, int64_t *totals)
{
    int64_t rb = 0, fb = 0, nj = 0, nr = 0;
    int all_mask = n_tables > 0;
    for (int64_t t = 0; t < n_tables; ++t) {
        const int64_t *d = desc + 10 * t;
        const int64_t *ro = (const int64_t *)d[1], *fo = (const int64_t *)d[3];
        rb += ro[d[8]] - ro[0]; fb += fo[d[9]] - fo[0]; nj += d[8]; nr += d[9];
        if (!d[7]) all_mask = 0;
    }
    totals[0] = rb; totals[1] = fb; totals[2] = nj; totals[3] = nr;
    return all_mask;
}
int ipx_concat_tables(const int64_t *desc, int64_t n_tables, int8_t *reads, int64_t *read_off, int8_t *refs, int64_t *ref_off, int32_t *ref_id,
                      uint8_t *gap_open, uint8_t *gap_ext, int32_t *mask_len)
{
    // pass 1 (serial): where every table's jobs, windows and letters start in the outputs
    std::vector<int64_t> at(4 * ((size_t)n_tables + 1));
    int64_t rb = 0, fb = 0, nj = 0, nr = 0;
    for (int64_t t = 0; t < n_tables; ++t) {
        const int64_t *d = desc + 10 * t;
        const int64_t n = d[8], m = d[9];
        const int64_t *ro = (const int64_t *)d[1], *fo = (const int64_t *)d[3];
        if (n < 0 || m < 0 || ro[n] < ro[0] || fo[m] < fo[0]) { set_err("ipx_concat_tables: table %lld has negative sizes", (long long)t); return IPX_ERR_ARG; }
        at[4 * t] = rb; at[4 * t + 1] = fb; at[4 * t + 2] = nj; at[4 * t + 3] = nr;
        rb += ro[n] - ro[0]; fb += fo[m] - fo[0]; nj += n; nr += m;
        if (nr >= (1ll << 31)) { set_err("ipx_concat_tables: more than 2^31 windows"); return IPX_ERR_ARG; }
    }
    read_off[0] = 0; ref_off[0] = 0;
    // pass 2: the copies, a contiguous range of tables per thread (a quarter of a gigabyte per million jobs: one core's memcpy was most
    // of a many-loci call)
    std::mutex bad_mu;
    int64_t bad_t = -1, bad_k = -1; int bad_v = 0;
    auto work = [&](int64_t t0, int64_t t1) {
        for (int64_t t = t0; t < t1; ++t) {
            const int64_t *d = desc + 10 * t;
            const int64_t n = d[8], m = d[9];
            const int64_t *ro = (const int64_t *)d[1], *fo = (const int64_t *)d[3];
            const int64_t r0 = ro[0], f0 = fo[0], orb = at[4 * t], ofb = at[4 * t + 1], onj = at[4 * t + 2], onr = at[4 * t + 3];
            memcpy(reads + orb, (const int8_t *)d[0] + r0, (size_t)(ro[n] - r0));
            memcpy(refs + ofb, (const int8_t *)d[2] + f0, (size_t)(fo[m] - f0));
            for (int64_t k = 1; k <= n; ++k) read_off[onj + k] = ro[k] - r0 + orb;
            for (int64_t k = 1; k <= m; ++k) ref_off[onr + k] = fo[k] - f0 + ofb;
            const int32_t *rid = (const int32_t *)d[4];
            for (int64_t k = 0; k < n; ++k) {
                if (rid[k] < 0 || rid[k] >= m) { std::lock_guard<std::mutex> g(bad_mu); if (bad_t < 0) { bad_t = t; bad_k = k; bad_v = rid[k]; } break; }
                ref_id[onj + k] = rid[k] + (int32_t)onr;
            }
            memcpy(gap_open + onj, (const uint8_t *)d[5], (size_t)n);
            memcpy(gap_ext + onj, (const uint8_t *)d[6], (size_t)n);
            if (mask_len && d[7]) memcpy(mask_len + onj, (const int32_t *)d[7], 4 * (size_t)n);
        }
    };
    int nth = (int)std::thread::hardware_concurrency();
    if (nth > 8) nth = 8;
    if (nth < 1 || rb + fb < (8ll << 20)) nth = 1;               // (small: a thread costs more than it copies)
    if (nth == 1) work(0, n_tables);
    else {
        std::vector<std::thread> th;
        int64_t t0 = 0;
        for (int q = 0; q < nth; ++q) {                            // equal BYTES per thread, not equal table counts
            const int64_t want = (rb + fb) * (q + 1) / nth;
            int64_t t1 = t0;
            while (t1 < n_tables && (q == nth - 1 || at[4 * t1] + at[4 * t1 + 1] < want)) ++t1;
            th.emplace_back(work, t0, t1);
            t0 = t1;
        }
        for (auto &x : th) x.join();
    }
    if (bad_t >= 0) { set_err("ipx_concat_tables: table %lld, job %lld: ref_id %d out of range", (long long)bad_t, (long long)bad_k, bad_v); return IPX_ERR_ARG; }
    return IPX_OK;
}

// A job table's jobs GROUPED BY READ LENGTH (stable: the given order inside a length), host side.  order[k] = the job that comes k-th; the read
// letters, their offsets and the per-job arrays are written in that order (the windows stay as they are).  A batch of mixed lengths that is
// uploaded once and run many times is cut into stream slices AFTER this (indelpost_amd.batch.MultiStreamAligner.upload): a slice then holds one or
// two length classes, its launches are four times as large and half as many, and the classes are large enough for the banded reverse pass
// (config 4: 58 -> 65 M aln/s).  Counting sort on the lengths, then one memcpy per job on up to eight threads.
int ipx_group_by_length(const int8_t *reads, const int64_t *read_off, const int32_t *ref_id, const uint8_t *gap_open, const uint8_t *gap_ext,
                        const int32_t *mask_len, int64_t n_jobs, uint32_t *order, int8_t *reads_out, int64_t *read_off_out, int32_t *ref_id_out,
                        uint8_t *gap_open_out, uint8_t *gap_ext_out, int32_t *mask_len_out)
{
    if (n_jobs < 0 || n_jobs >= (1ll << 32) || !read_off || !order || !read_off_out) { set_err("ipx_group_by_length: bad argument"); return IPX_ERR_ARG; }
    int64_t maxlen = 0;
    for (int64_t k = 0; k < n_jobs; ++k) {
        const int64_t len = read_off[k + 1] - read_off[k];
        if (len < 0) { set_err("ipx_group_by_length: job %lld has a negative length", (long long)k); return IPX_ERR_ARG; }
        if (len > maxlen) maxlen = len;
    }
    if (maxlen > (1 << 24)) { set_err("ipx_group_by_length: a read of %lld letters", (long long)maxlen); return IPX_ERR_ARG; }
    std::vector<int64_t> first((size_t)maxlen + 2, 0);
    for (int64_t k = 0; k < n_jobs; ++k) ++first[(size_t)(read_off[k + 1] - read_off[k]) + 1];
    for (int64_t l = 0; l <= maxlen; ++l) first[(size_t)l + 1] += first[(size_t)l];
    for (int64_t k = 0; k < n_jobs; ++k) order[first[(size_t)(read_off[k + 1] - read_off[k])]++] = (uint32_t)k;
    read_off_out[0] = 0;
    for (int64_t k = 0; k < n_jobs; ++k) read_off_out[k + 1] = read_off_out[k] + (read_off[order[k] + 1] - read_off[order[k]]);
    auto work = [&](int64_t k0, int64_t k1) {
        for (int64_t k = k0; k < k1; ++k) {
            const uint32_t j = order[k];
            memcpy(reads_out + read_off_out[k], reads + read_off[j], (size_t)(read_off[j + 1] - read_off[j]));
            ref_id_out[k] = ref_id[j]; gap_open_out[k] = gap_open[j]; gap_ext_out[k] = gap_ext[j];
            if (mask_len && mask_len_out) mask_len_out[k] = mask_len[j];
        }
    };
    int nth = (int)std::thread::hardware_concurrency();
    if (nth > 8) nth = 8;
    if (nth < 1 || n_jobs < 100000) nth = 1;
    if (nth == 1) work(0, n_jobs);
    else {
        std::vector<std::thread> th;
        for (int q = 0; q < nth; ++q) th.emplace_back(work, n_jobs * q / nth, n_jobs * (q + 1) / nth);
        for (auto &x : th) x.join();
    }
    return IPX_OK;
}

// ---- synthetic workload generator, host side ----------------------------------------
static inline uint32_t xs_next(uint64_t &s)
{
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return (uint32_t)(s >> 11);
}
uint64_t ipx_synth_window(uint64_t state, int8_t *ref, int32_t wl)
{
    for (int32_t i = 0; i < wl; ++i) ref[i] = (int8_t)(xs_next(state) & 3);
    return state;
}
int64_t ipx_format_cigars(const ipx_result *rec, const uint32_t *cigar_pool, int64_t n, char *out, int64_t cap, int64_t *off)
{
    static const char ops[] = "MIDNSHP=X";
    if (!rec || !off || n < 0) return 0;
    int64_t need = 0;                                     // pass 1: exact size
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t *c = cigar_pool + rec[i].cigar_off;
        for (int k = 0; k < rec[i].cigar_len; ++k) {
            uint32_t len = c[k] >> 4;
            int d = 1;
            while (len >= 10) { len /= 10; ++d; }
            need += d + 1;
        }
    }
    if (need > cap || (!out && need > 0)) return -need;
    int64_t w = 0;
    for (int64_t i = 0; i < n; ++i) {
        off[i] = w;
        const uint32_t *c = cigar_pool + rec[i].cigar_off;
        for (int k = 0; k < rec[i].cigar_len; ++k) {
            char tmp[12];
            uint32_t len = c[k] >> 4;
            int d = 0;
            do { tmp[d++] = (char)('0' + len % 10); len /= 10; } while (len);
            while (d) out[w++] = tmp[--d];
            const uint32_t op = c[k] & 15u;
            out[w++] = op > 8 ? 'M' : ops[op];
        }
    }
    off[n] = w;
    return w;
}

// FNV-1a (32 bit) of every job's BAM-encoded CIGAR ops, 2166136261 (the offset basis) for a job without one: what the test
// suite's CPU checker reports per job (oracle/cpu_baseline.c), so whole batches can be compared op for op without a Python loop
void ipx_cigar_hashes(const ipx_result *rec, const uint32_t *cigar_pool, int64_t n, uint32_t *out)
{
    for (int64_t i = 0; i < n; ++i) {
        uint32_t h = 2166136261u;
        const uint32_t *c = cigar_pool + rec[i].cigar_off;
        for (int k = 0; k < rec[i].cigar_len; ++k) h = (h ^ c[k]) * 16777619u;
        out[i] = h;
    }
}

// XXH64 (Yann Collet's published algorithm, seed 0) of the batch's results in job order: per job ten little-endian int64 -- score1,
// score2, ref_begin1, ref_end1, read_begin1, read_end1, ref_end2, flag, cigar_len and the FNV-1a hash of its CIGAR ops (ipx_cigar_hashes).
// This is the digest bench.py compares with the reference's (tests/golden/bench_digests.json); computed here so that the bench path needs
// no third-party hashing package (tests/test_host_logic.py checks it against the `xxhash` package where that is installed).
static inline uint64_t xxh_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
static inline uint64_t xxh_round(uint64_t acc, uint64_t in) { return xxh_rotl(acc + in * 0xC2B2AE3D27D4EB4FULL, 31) * 0x9E3779B185EBCA87ULL; }
static inline uint64_t xxh_merge(uint64_t h, uint64_t v) { return (h ^ xxh_round(0, v)) * 0x9E3779B185EBCA87ULL + 0x85EBCA77C2B2AE63ULL; }
uint64_t ipx_record_digest(const ipx_result *rec, const uint32_t *cigar_hash, int64_t n)
{
    const uint64_t P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL, P4 = 0x85EBCA77C2B2AE63ULL, P5 = 0x27D4EB2F165667C5ULL;
    const uint64_t total = (uint64_t)n * 80u;
    uint64_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0 - P1;
    uint64_t buf[4];                                             // words waiting for a full 32-byte stripe
    int nb = 0;
    uint64_t h;
    auto word = [&](int64_t i, int k) -> uint64_t {
        const ipx_result &r = rec[i];
        int64_t v;
        switch (k) {
        case 0: v = r.score1; break;
        case 1: v = r.score2; break;
        case 2: v = r.ref_begin1; break;
        case 3: v = r.ref_end1; break;
        case 4: v = r.read_begin1; break;
        case 5: v = r.read_end1; break;
        case 6: v = r.ref_end2; break;
        case 7: v = r.flag; break;
        case 8: v = r.cigar_len; break;
        default: v = (int64_t)cigar_hash[i]; break;
        }
        return (uint64_t)v;
    };
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 10; ++k) {
            buf[nb++] = word(i, k);
            if (nb == 4) { v1 = xxh_round(v1, buf[0]); v2 = xxh_round(v2, buf[1]); v3 = xxh_round(v3, buf[2]); v4 = xxh_round(v4, buf[3]); nb = 0; }
        }
    if (total >= 32) {
        h = xxh_rotl(v1, 1) + xxh_rotl(v2, 7) + xxh_rotl(v3, 12) + xxh_rotl(v4, 18);
        h = xxh_merge(h, v1); h = xxh_merge(h, v2); h = xxh_merge(h, v3); h = xxh_merge(h, v4);
    } else h = P5;                                               // (seed 0)
    h += total;
    for (int k = 0; k < nb; ++k) { h ^= xxh_round(0, buf[k]); h = xxh_rotl(h, 27) * P1 + P4; }   // (the input is whole 8-byte words: no 4- or 1-byte tail)
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}

uint64_t ipx_synth_reads(uint64_t state, const int8_t *ref, int32_t wl, int8_t *reads, int64_t n, int32_t rl)
{
    for (int64_t k = 0; k < n; ++k) {
        int8_t *r = reads + k * rl;
        int32_t st = (int32_t)(xs_next(state) % (uint32_t)(wl - rl + 1)), p = 0, q = st;
        while (p < rl) {
            const uint32_t u = xs_next(state) % 1000u;
            if (q >= wl) { r[p++] = (int8_t)(xs_next(state) & 3); continue; }
            if (u < 20) { r[p++] = (int8_t)(xs_next(state) & 3); ++q; }         // 2 % substitution
            else if (u < 25) { ++q; }                                            // 0.5 % deletion
            else if (u < 30) { r[p++] = (int8_t)(xs_next(state) & 3); }          // 0.5 % insertion
            else { r[p++] = ref[q++]; }
        }
    }
    return state;
}

// Multi-window form of the same generator: `n_windows` windows whose length is
// drawn from [wl_lo, wl_hi], and for each window `per` reads of every length in rls[] (clamped to the window).
// Buffers are caller-owned and sized for the worst case (n_windows*wl_hi codes, n_windows*per*sum(rls) codes,
// n_windows*per*n_rls jobs); returns the number of jobs written.  state is updated in place.
int64_t ipx_synth_mixed(uint64_t *state, int32_t n_windows, int32_t wl_lo, int32_t wl_hi, const int32_t *rls, int32_t n_rls,
                        int32_t per, int8_t *refs, int64_t *ref_off, int8_t *reads, int64_t *read_off, int32_t *ref_id)
{
    if (!state || n_windows < 0 || wl_lo < 1 || wl_hi < wl_lo || n_rls < 0 || per < 0) return -1;
    uint64_t st = *state;
    int64_t job = 0, rpos = 0, fpos = 0;
    ref_off[0] = 0; read_off[0] = 0;
    for (int32_t w = 0; w < n_windows; ++w) {
        const int32_t wl = wl_lo + (int32_t)(xs_next(st) % (uint32_t)(wl_hi - wl_lo + 1));
        st = ipx_synth_window(st, refs + fpos, wl);
        for (int32_t k = 0; k < n_rls; ++k) {
            const int32_t rl = rls[k] < wl ? rls[k] : wl;
            st = ipx_synth_reads(st, refs + fpos, wl, reads + rpos, per, rl);
            for (int32_t q = 0; q < per; ++q) { rpos += rl; read_off[++job] = rpos; ref_id[job - 1] = w; }
        }
        fpos += wl;
        ref_off[w + 1] = fpos;
    }
    *state = st;
    return job;
}

// CIGAR letter -> BAM opcode (ssw.h:34; used by the header's to_cigar_int): index = ASCII code, 0 for everything that is
// not one of MIDNSHP=X ('=' is 61, 'D' 68, 'H' 72, 'I' 73, 'M' 77, 'N' 78, 'P' 80, 'S' 83, 'X' 88)
extern "C" const uint8_t encoded_ops[128] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 0, 0,
    0, 0, 0, 0, 2, 0, 0, 0, 5, 1, 0, 0, 0, 0, 3, 0, 6, 0, 0, 4, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
};

// ---- the reference's four-call interface, executed on GPU 0 ---------------------------------------
struct _profile {                                  // ssw.c:115-123 (fields this path needs)
    const int8_t *read;
    const int8_t *mat;
    int32_t readLen;
    int32_t n;
    int8_t score_size;
};

static ipx_ctx *g_default_ctx = nullptr;
static std::mutex g_default_mu;

s_profile *ssw_init(const int8_t *read, const int32_t readLen, const int8_t *mat, const int32_t n, const int8_t score_size)
{
    s_profile *p = (s_profile *)calloc(1, sizeof(s_profile));
    p->read = read; p->mat = mat; p->readLen = readLen; p->n = n; p->score_size = score_size;   // borrowed (ssw.c:803-804)
    return p;
}
void init_destroy(s_profile *p) { free(p); }

s_align *ssw_align(const s_profile *prof, const int8_t *ref, int32_t refLen, const uint8_t weight_gapO,
                   const uint8_t weight_gapE, const uint8_t flag, const uint16_t filters, const int32_t filterd,
                   const int32_t maskLen)
{
    if (!prof) { fprintf(stderr, "Please call the function ssw_init before ssw_align.\n"); return nullptr; }
    if (prof->n != 5) { fprintf(stderr, "libindelpost_hip: only the 5-letter DNA matrix of sswpy is supported (n=%d).\n", prof->n); return nullptr; }
    std::lock_guard<std::mutex> lock(g_default_mu);
    if (!g_default_ctx) {
        g_default_ctx = ipx_create(0);
        if (!g_default_ctx) { fprintf(stderr, "libindelpost_hip: %s\n", g_err); return nullptr; }
    }
    ipx_ctx *c = g_default_ctx;
    if (ipx_set_params(c, prof->mat, flag, filters, filterd, prof->score_size)) return nullptr;
    int64_t read_off[2] = {0, prof->readLen}, ref_off[2] = {0, refLen};
    int32_t rid = 0, mask = maskLen;
    uint8_t go = weight_gapO, ge = weight_gapE;
    ipx_result r;
    std::vector<uint32_t> pool((size_t)prof->readLen + (size_t)refLen + 16);
    int64_t nops = 0;
    int rc = ipx_align_batch(c, prof->read, read_off, ref, ref_off, &rid, &go, &ge, &mask, 1, 1, &r, pool.data(),
                             (int64_t)pool.size(), &nops);
    if (rc) { fprintf(stderr, "libindelpost_hip: %s\n", g_err); return nullptr; }
    if (r.mode == IPX_MODE_FAIL) {
        fprintf(stderr, "Please set 2 to the score_size parameter of the function ssw_init, otherwise the alignment results will be incorrect.\n");
        return nullptr;                                                                  // ssw.c:848-851
    }
    s_align *a = (s_align *)calloc(1, sizeof(s_align));
    a->score1 = r.score1; a->score2 = r.score2; a->ref_begin1 = r.ref_begin1; a->ref_end1 = r.ref_end1;
    a->read_begin1 = r.read_begin1; a->read_end1 = r.read_end1; a->ref_end2 = r.ref_end2; a->flag = r.flag;
    if (r.cigar_len) {
        a->cigar = (uint32_t *)malloc(sizeof(uint32_t) * r.cigar_len);
        memcpy(a->cigar, pool.data() + r.cigar_off, sizeof(uint32_t) * r.cigar_len);
        a->cigarLen = r.cigar_len;
    }
    return a;
}
void align_destroy(s_align *a) { if (a) { free(a->cigar); free(a); } }

} // extern "C"
