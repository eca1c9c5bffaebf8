// rx_host.h -- what the host-side translation units of libselenite_rx.so share: error reporting, device-buffer helpers, and the
// interfaces between rx_api.hip (instance, accessors, entry points), rx_dispatch.hip (the dispatcher), rx_hostpipe.hip (host-pointer
// calls), rx_timing.hip and the stages' own files.  Host code only; not part of the C-ABI.
#pragma once
#include <cmath>
#include <cstddef>
#include <initializer_list>
#include <vector>

#include "hip_event_pair.h"
#include "rx_internal.h"
#include "rx_route.h"

struct selenite_tx_instance;

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
inline int fail(std::nullptr_t, int code, const std::string &msg) { return fail(static_cast<selenite_rx_instance *>(nullptr), code, msg); }
// the TX instance's (tx_host.h): the first error latches code and text, the thread's last error is left alone
inline int fail(selenite_tx_instance *S, int code, const std::string &msg);
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

// How selenite_rx_init and selenite_tx_init read a FIR pair of nh taps, which the fused kernels of both directions rely on.
struct TapClass { bool delay_is_impulse = false, hilb_odd_only = false; int delay_index = 0; };
inline TapClass classify_taps(const float *delay, const float *hilb, uint32_t nh)
{
    TapClass t;
    auto plus_zero = [](float v) { return v == 0.0f && !std::signbit(v); };
    // delay FIR that is exactly a unit impulse: arm_fir_f32 then returns x + 0.0f
    int ones = 0;
    bool rest_zero = true;
    for (uint32_t k = 0; k < nh; ++k) {
        if (delay[k] == 1.0f) { ++ones; t.delay_index = (int)k; }
        else if (!plus_zero(delay[k])) rest_zero = false;
    }
    t.delay_is_impulse = ones == 1 && rest_zero;
    // type-III Hilbert: taps at even distance from the centre are exactly +0.0f
    t.hilb_odd_only = nh % 2 == 1;
    for (uint32_t k = (nh / 2) & 1u; k < nh && t.hilb_odd_only; k += 2) t.hilb_odd_only = plus_zero(hilb[k]);
    return t;
}

// ---- device buffers (I: selenite_rx_instance or selenite_tx_instance; HIPCHK finds the instance's fail by overload) ----
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
template <typename I>
inline int ensure(I *S, void **buf, size_t *cap, size_t need)
{
    if (*cap >= need) return SELENITE_RX_SUCCESS;
    if (*buf) { HIPCHK(S, hipStreamSynchronize(S->stream)); HIPCHK(S, hipFree(*buf)); *buf = nullptr; *cap = 0; }
    HIPCHK(S, hipMalloc(buf, need));
    *cap = need;
    return SELENITE_RX_SUCCESS;
}
// the instance's device, and its stream drained: in front of every read or write of state from the host
template <typename I>
inline int drain(I *S)
{
    HIPCHK(S, hipSetDevice(S->device));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    return SELENITE_RX_SUCCESS;
}
// State rows copied out of the device (to_host) or into it, behind one drain.  A row whose host pointer is NULL is skipped: the caller of
// a *_state call did not ask for it, or it does not exist, or it is not copied in this direction; so is a row of no bytes.
struct Row { void *dev; const void *host; size_t bytes; };
template <typename I>
inline int copy_rows(I *S, bool to_host, std::initializer_list<Row> rows)
{
    if (int rc = drain(S)) return rc;
    for (const Row &w : rows) {
        if (!w.host || !w.bytes) continue;
        if (to_host) HIPCHK(S, hipMemcpy(const_cast<void *>(w.host), w.dev, w.bytes, hipMemcpyDeviceToHost));
        else HIPCHK(S, hipMemcpy(w.dev, w.host, w.bytes, hipMemcpyHostToDevice));
    }
    return SELENITE_RX_SUCCESS;
}
// A per-channel row filled with one value (n = 1) or with one row of n values per channel, on the instance's stream: everything enqueued
// before it has run on return (the host vector lives until then).
template <typename I, typename T>
inline int fill_rows(I *S, T *dev, size_t channels, const T *value, size_t n = 1)
{
    std::vector<T> h(channels * n);
    for (size_t i = 0; i < h.size(); ++i) h[i] = value[i % n];
    HIPCHK(S, hipMemcpyAsync(dev, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, S->stream));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    return SELENITE_RX_SUCCESS;
}
// `iters` calls of enqueue() (0, or the error code to return) on the instance's stream between two events, behind one untimed call
// where `warm` says so (it grows what the calls grow); *ms_per_call: their mean
template <typename I, typename F>
inline int timed_loop(I *S, uint32_t iters, float *ms_per_call, F &&enqueue, bool warm = false)
{
    EventPair ev;
    HIPCHK(S, hipEventCreate(&ev.e0));
    HIPCHK(S, hipEventCreate(&ev.e1));
    if (warm)
        if (int rc = enqueue()) return rc;
    HIPCHK(S, hipEventRecord(ev.e0, S->stream));
    for (uint32_t i = 0; i < iters; ++i)
        if (int rc = enqueue()) return rc;
    HIPCHK(S, hipEventRecord(ev.e1, S->stream));
    HIPCHK(S, hipEventSynchronize(ev.e1));
    float ms = 0.0f;
    HIPCHK(S, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *ms_per_call = ms / (float)iters;
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
