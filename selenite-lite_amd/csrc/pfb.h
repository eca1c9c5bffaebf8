// pfb.h -- what the polyphase filter banks share: the channeliser (chan.hip, include/selenite_chan.h) and the combiner (comb.hip,
// include/selenite_comb.h) are one weighted-overlap-add bank run in the two directions.  Device side: the tile constants and the per-rail
// arm_dot_prod_f32 over a lane's shift register.  Host side: the object behind both opaque types and everything about it that does not depend
// on the direction -- validation of the configuration's common fields, creation, release, stream, reset and the state copy.  The transform
// both kernels run is rx_fft8.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/selenite_rx.h"
#include "rx_fft8.h"

namespace srx {

// One single-wave workgroup works a run of kPfbRun = 64 consecutive frames (the channeliser's outputs, the combiner's inputs) of its band(s),
// in tiles of kPfbT = 16: the longer the run, the less the overlap at its start weighs.  A tile is K channel rows x 16 frames in LDS, moved
// to or from memory row-wise: 16 frames x 8 bytes = one 128-byte piece of a channel row, four rows per wave instruction.  The row stride of
// kPfbRow = 17 float2 lets the lanes that touch one frame of 64 rows hit 32 bank pairs once each.
constexpr int kPfbT = 16;
constexpr int kPfbRun = 64;
constexpr int kPfbRow = 17;

// arm_dot_prod_f32 (BasicMathFunctions/arm_dot_prod_f32.c) per rail over a lane's shift register h, oldest first, against the taps
// gs[r + t STRIDE] in LDS: acc = +0.0f, the product rounded, then the sum, t ascending (the unit is built with -ffp-contract=off)
template <int STRIDE, int N>
__device__ __forceinline__ float2 pfb_dot(const float *gs, uint32_t r, const float2 (&h)[N])
{
    float ai = 0.0f, aq = 0.0f;
#pragma unroll
    for (int t = 0; t < N; ++t) {
        const float c = gs[r + (uint32_t)(t * STRIDE)];
        const float pi = c * h[t].x, pq = c * h[t].y;
        ai = ai + pi;
        aq = aq + pq;
    }
    return make_float2(ai, aq);
}

// ---- host side ----
struct PfbObject {
    uint32_t bands = 0, K = 0, ovs = 0, P = 0, n_bins = 0;
    bool all_bins = true;
    int device = 0;
    float *d_taps = nullptr, *d_tw = nullptr;
    uint32_t *d_bins = nullptr;
    float *d_hist[2] = { nullptr, nullptr };     // two buffers of hist_bytes, swapped per call; d_hist[cur] is the state
    size_t hist_bytes = 0;                       // fixed at init
    int cur = 0;
    uint64_t position = 0;
    hipStream_t stream = nullptr, own_stream = nullptr;
    int status = 0;
    std::string err;
    uint32_t D() const { return K / ovs; }
};

inline int fail(PfbObject *O, int code, const std::string &msg)
{
    if (O && O->status == 0) { O->status = code; O->err = msg; }
    return code;
}

#define PFB_CHK(O, call)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return srx::fail((O), SELENITE_RX_DEVICE_ERROR, std::string(#call ": ") + hipGetErrorString(e_)); \
    } while (0)

// The fields the two configurations share, in the order both inits have always checked them (struct_size is the caller's).  own_ok is the
// caller's verdict on the scalar fields only its object has: it ranks with the other scalar fields, behind fft_len and in front of
// everything a pointer leads to.  Touches no device.
template <typename Cfg>
int pfb_validate(const Cfg *cfg, uint32_t max_bands, bool own_ok)
{
    if (cfg->fft_len != 64 && cfg->fft_len != 512) return SELENITE_RX_LENGTH_ERROR;     // the pure radix-8 lengths of arm_cfft_f32
    const uint32_t K = cfg->fft_len, P = cfg->taps_per_branch;
    if (cfg->bands == 0 || (cfg->oversample != 1 && cfg->oversample != 2) || (P != 4 && P != 8 && P != 12 && P != 16) || cfg->n_bins == 0 ||
        !own_ok || cfg->reserved != 0 || !cfg->coeffs)
        return SELENITE_RX_ARGUMENT_ERROR;
    if (cfg->bands > max_bands) return SELENITE_RX_ARGUMENT_ERROR;                      // (the bands are the grid's x: 64 threads each, under 2^32)
    if ((uint64_t)cfg->bands * cfg->n_bins > 0xFFFFFFFFull) return SELENITE_RX_ARGUMENT_ERROR;
    if (!cfg->bins && cfg->n_bins != K) return SELENITE_RX_ARGUMENT_ERROR;
    for (uint32_t i = 0; i < K * P; ++i)
        if (!std::isfinite(cfg->coeffs[i])) return SELENITE_RX_ARGUMENT_ERROR;
    if (cfg->bins)
        for (uint32_t i = 0; i < cfg->n_bins; ++i)
            if (cfg->bins[i] >= K) return SELENITE_RX_ARGUMENT_ERROR;
    return SELENITE_RX_SUCCESS;
}

inline int pfb_reset(PfbObject *O)
{
    PFB_CHK(O, hipSetDevice(O->device));
    PFB_CHK(O, hipMemsetAsync(O->d_hist[O->cur], 0, O->hist_bytes, O->stream));
    PFB_CHK(O, hipStreamSynchronize(O->stream));
    O->position = 0;
    return SELENITE_RX_SUCCESS;
}

// fills a fresh object from a validated configuration: its own stream, the twiddles, taps and bins on the device, both histories, reset.
// On a failure the caller releases the object (pfb_free takes it half-built).
template <typename Cfg>
int pfb_create(PfbObject *O, const Cfg *cfg, size_t hist_bytes)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return SELENITE_RX_DEVICE_ERROR;      // no CPU fallback
    const uint32_t K = cfg->fft_len, P = cfg->taps_per_branch;
    O->bands = cfg->bands; O->K = K; O->ovs = cfg->oversample; O->P = P; O->n_bins = cfg->n_bins; O->all_bins = !cfg->bins;
    O->hist_bytes = hist_bytes;
    if (hipGetDevice(&O->device) != hipSuccess) return SELENITE_RX_DEVICE_ERROR;
    if (hipStreamCreateWithFlags(&O->own_stream, hipStreamNonBlocking) != hipSuccess) return SELENITE_RX_DEVICE_ERROR;
    O->stream = O->own_stream;
    std::vector<float> tw(2 * (size_t)K);
    spec_twiddles(tw.data(), K);
    const size_t taps_bytes = (size_t)K * P * sizeof(float), tw_bytes = tw.size() * sizeof(float), bins_bytes = (size_t)cfg->n_bins * sizeof(uint32_t);
    if (hipMalloc((void **)&O->d_taps, taps_bytes) != hipSuccess || hipMalloc((void **)&O->d_tw, tw_bytes) != hipSuccess ||
        hipMalloc((void **)&O->d_hist[0], hist_bytes) != hipSuccess || hipMalloc((void **)&O->d_hist[1], hist_bytes) != hipSuccess ||
        (cfg->bins && hipMalloc((void **)&O->d_bins, bins_bytes) != hipSuccess))
        return SELENITE_RX_DEVICE_ERROR;
    if (hipMemcpy(O->d_taps, cfg->coeffs, taps_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(O->d_tw, tw.data(), tw_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        (cfg->bins && hipMemcpy(O->d_bins, cfg->bins, bins_bytes, hipMemcpyHostToDevice) != hipSuccess))
        return SELENITE_RX_DEVICE_ERROR;
    return pfb_reset(O) ? SELENITE_RX_DEVICE_ERROR : SELENITE_RX_SUCCESS;
}

// (a template only for the delete: the object types have no virtual destructor)
template <typename Obj>
void pfb_free(Obj *O)
{
    if (!O) return;
    if (O->stream) (void)hipStreamSynchronize(O->stream);
    void *ptrs[] = { O->d_taps, O->d_tw, O->d_bins, O->d_hist[0], O->d_hist[1] };
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (O->own_stream) (void)hipStreamDestroy(O->own_stream);
    delete O;
}

inline int pfb_set_stream(PfbObject *O, void *hip_stream)
{
    if (!O) return SELENITE_RX_ARGUMENT_ERROR;
    PFB_CHK(O, hipStreamSynchronize(O->stream));
    O->stream = hip_stream ? (hipStream_t)hip_stream : O->own_stream;
    return SELENITE_RX_SUCCESS;
}

inline int pfb_sync(PfbObject *O)
{
    if (!O) return SELENITE_RX_ARGUMENT_ERROR;
    PFB_CHK(O, hipStreamSynchronize(O->stream));
    return O->status;
}

// get_state (to_host) and set_state: the history in use and the position; a NULL member of the view is skipped.  who names the set_state
// entry point in its one message
template <typename View>
int pfb_state_copy(PfbObject *O, const View *v, bool to_host, const char *who)
{
    if (!O || !v) return SELENITE_RX_ARGUMENT_ERROR;
    if (!to_host && v->position && *v->position % O->D() != 0)
        return fail(O, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": position is not a multiple of fft_len / oversample");
    PFB_CHK(O, hipSetDevice(O->device));
    PFB_CHK(O, hipStreamSynchronize(O->stream));
    if (v->history && to_host) PFB_CHK(O, hipMemcpy(v->history, O->d_hist[O->cur], O->hist_bytes, hipMemcpyDeviceToHost));
    if (v->history && !to_host) PFB_CHK(O, hipMemcpy(O->d_hist[O->cur], v->history, O->hist_bytes, hipMemcpyHostToDevice));
    if (v->position) {
        if (to_host) *v->position = O->position;
        else O->position = *v->position;
    }
    return SELENITE_RX_SUCCESS;
}

}  // namespace srx
