// Host build of the event pass's per-job walk (TEST INFRASTRUCTURE): indelpost_amd/csrc/ipx_events.h compiled with g++, the
// same ipx_walk_events the device kernels run.  Loaded with ctypes by tests/events_host.py.
#include "../indelpost_amd/csrc/ipx_events.h"

extern "C" {

// Events of one job into out[0 .. cap).  Returns the number of events (nothing is written when it exceeds cap), or -1 when the
// walk would leave its read or its window.  read / ref: the letters, or both NULL for indels only.
int64_t ipx_host_walk_events(const uint32_t *ops, int32_t n_ops, int64_t ri, int64_t qi, const uint8_t *read, int64_t read_len,
                             const uint8_t *ref, int64_t ref_len, IpxEvent *out, int64_t cap)
{
    IpxEvCount c;
    if (ipx_walk_events(ops, n_ops, ri, qi, read, read_len, ref, ref_len, c) != IPX_EV_OK) return -1;
    if (c.n > cap) return c.n;
    IpxEvWrite w{out, 0};
    (void)ipx_walk_events(ops, n_ops, ri, qi, read, read_len, ref, ref_len, w);
    return w.n;
}
}
