// rx_host.h -- what the host-side translation units of libselenite_rx.so share: error reporting, device-buffer helpers, and the
// interfaces between rx_api.hip (instance, accessors, entry points), rx_dispatch.hip (the dispatcher), rx_hostpipe.hip (host-pointer
// calls), rx_timing.hip and the stages' own files.  Host code only; not part of the C-ABI.
#pragma once
#include <initializer_list>
#include <vector>

#include "rx_internal.h"
#include "rx_route.h"

// (hidden: these are interfaces between the library's own translation units, none of them an exported name)
#pragma GCC visibility push(hidden)
namespace srx {

// ---- errors: every translation unit reports them the same way ----
// the calling thread's last error without an instance (selenite_rx_error_string(NULL)) (rx_api.hip)
std::string &last_error();

inline int fail(selenite_rx_instance *S, int code, const std::string &msg)
{
    last_error() = msg;
    if (S) {
        if (S->status == SELENITE_RX_SUCCESS) S->status = code;
        S->err = msg;
    }
    return code;
}
#define HIPCHK(S, call)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return srx::fail((S), SELENITE_RX_DEVICE_ERROR,                                 \
                             std::string(#call) + ": " + hipGetErrorString(e_));            \
    } while (0)

// a refused configuration (the set_* calls): the calling thread's last error says why; the instance's status and error string stay as
// they are, so it goes on as it was
inline int refuse(const char *who, const char *why, int code = SELENITE_RX_ARGUMENT_ERROR)
{
    last_error() = std::string(who) + ": " + why;
    return code;
}

// ---- device buffers ----
template <typename T>
inline hipError_t dev_upload(T **d, const T *h, size_t n)
{
    *d = nullptr;
    if (n == 0) return hipSuccess;
    hipError_t e = hipMalloc((void **)d, n * sizeof(T));
    if (e != hipSuccess) return e;
    return hipMemcpy(*d, h, n * sizeof(T), hipMemcpyHostToDevice);
}
// allocation only: every state buffer is initialised by reset_state() on the instance's own stream
// (a null-stream hipMemset here could land AFTER reset_state's writes: the streams do not order)
template <typename T>
inline hipError_t dev_alloc(T **d, size_t n)
{
    *d = nullptr;
    if (n == 0) return hipSuccess;
    return hipMalloc((void **)d, n * sizeof(T));
}
// free these and null them
template <typename... T>
inline void dev_free(T *&...p)
{
    ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...);
}
// a buffer of the instance that grows to the largest call and is never shrunk
inline int ensure(selenite_rx_instance *S, void **buf, size_t *cap, size_t need)
{
    if (*cap >= need) return SELENITE_RX_SUCCESS;
    if (*buf) { HIPCHK(S, hipStreamSynchronize(S->stream)); HIPCHK(S, hipFree(*buf)); *buf = nullptr; *cap = 0; }
    HIPCHK(S, hipMalloc(buf, need));
    *cap = need;
    return SELENITE_RX_SUCCESS;
}
// the instance's device, and its stream drained: in front of every read or write of state from the host
inline int drain(selenite_rx_instance *S)
{
    HIPCHK(S, hipSetDevice(S->device));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    return SELENITE_RX_SUCCESS;
}
// State rows copied out of the device (to_host) or into it, behind one drain.  A row whose host pointer is NULL is skipped: the caller of
// a *_state call did not ask for it, or it does not exist, or it is not copied in this direction.
struct Row { void *dev; const void *host; size_t bytes; };
inline int copy_rows(selenite_rx_instance *S, bool to_host, std::initializer_list<Row> rows)
{
    if (int rc = drain(S)) return rc;
    for (const Row &w : rows) {
        if (!w.host) continue;
        if (to_host) HIPCHK(S, hipMemcpy(const_cast<void *>(w.host), w.dev, w.bytes, hipMemcpyDeviceToHost));
        else HIPCHK(S, hipMemcpy(w.dev, w.host, w.bytes, hipMemcpyHostToDevice));
    }
    return SELENITE_RX_SUCCESS;
}
// A per-channel row filled with one value (n = 1) or with one row of n values per channel, on the instance's stream: everything enqueued
// before it has run on return (the host vector lives until then).
template <typename T>
inline int fill_rows(selenite_rx_instance *S, T *dev, size_t channels, const T *value, size_t n = 1)
{
    std::vector<T> h(channels * n);
    for (size_t i = 0; i < h.size(); ++i) h[i] = value[i % n];
    HIPCHK(S, hipMemcpyAsync(dev, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, S->stream));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    return SELENITE_RX_SUCCESS;
}

// ---- the dispatcher (rx_dispatch.hip; Phase and the route of a launch: rx_route.h) ----
// Where a call starts in the two streams the host tracks: the common NCO phase (valid while every channel shares step and phase) and the
// spectrum tap's position.  Read once per call and handed down: every channel chunk of a host-pointer call starts from the same one.
struct CallStart { uint32_t phase; uint64_t spec_pos; };
inline CallStart call_start(const selenite_rx_instance *S) { return CallStart{ S->phase_host, S->spec.pos }; }
inline ChanRange all_channels(const selenite_rx_instance *S) { return ChanRange{ 0u, S->cfg.channels }; }
// this instance's calls run on the SSB fused kernels (rx_fused.hip), as select() (rx_select.h) decides call by call
inline bool on_ssb_fused(const selenite_rx_instance *S) { return !S->force_generic && S->plan.sel.kind != 0; }

bool block_size_ok(selenite_rx_instance *S, uint32_t block_size, const char *who);
RxParams make_params(selenite_rx_instance *S, ChanRange r, uint32_t block_size);
// enqueues one call over the channels of `r`; moves neither stream position
int run_chain(selenite_rx_instance *S, ChanRange r, CallStart at, const void *src, bool src_q15, void *dst, bool dst_q15,
              uint32_t block_size, Phase phase, float *ext_env);
// the one place the instance's phase_host, spec.pos and tones.pos advance: once per call, after its last launch is enqueued
void advance_streams(selenite_rx_instance *S, uint32_t block_size, Phase phase);
// a device-pointer call over the whole instance: run_chain, then advance_streams
int run_call(selenite_rx_instance *S, const void *src, bool src_q15, void *dst, bool dst_q15, uint32_t block_size, Phase phase, float *ext_env);

// the kernels' flag word (non-finite audio: ARM_MATH_NANINF), read after the stream has drained; latches the status (rx_api.hip)
int check_device_flags(selenite_rx_instance *S);

}  // namespace srx
#pragma GCC visibility pop
