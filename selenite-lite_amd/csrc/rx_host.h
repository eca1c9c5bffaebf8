// rx_host.h -- what the host-side translation units of libselenite_rx.so share: error reporting, device-buffer helpers, and the
// interfaces between rx_api.hip (instance, accessors, entry points), rx_dispatch.hip (the dispatcher), rx_hostpipe.hip (host-pointer
// calls), rx_timing.hip and the stages' own files.  Host code only; not part of the C-ABI.
#pragma once
#include "rx_internal.h"

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

// ---- the dispatcher (rx_dispatch.hip) ----
enum Phase { kAll, kPhase1, kPhase2 };

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
