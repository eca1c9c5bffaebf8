// tx_host.h -- what the host-side translation units of the TX direction share: the instance, error reporting (the generic helpers are
// rx_host.h's, templates over the instance), the two call shapes every entry point has (host-pointer staging; timing is rx_host.h's
// timed_loop), and the interfaces between tx_api.hip (instance, chain, run) and the stages' own files (tx_fm.hip, tx_cw.hip, tx_in.hip, tx_keyer.hip).
// Host code only; not part of the C-ABI.
#pragma once
#include <initializer_list>
#include <string>
#include <vector>

#include "rx_host.h"
#include "tx_internal.h"
#include "tx_select.h"

// Every stage owns its `set` flag, its kernel parameter block `p` (device pointers included), its device rows and grow-only buffers.
struct selenite_tx_instance {
    selenite_tx_config cfg;
    int device = 0;
    float *d_ic = nullptr, *d_hc = nullptr, *d_dc = nullptr, *d_sintab = nullptr;
    uint32_t *d_step = nullptr, *d_phase = nullptr;
    float *d_fir_state = nullptr, *d_int_state = nullptr, *d_gain = nullptr;
    void *d_io_in = nullptr, *d_io_out = nullptr;         // staging of the host-pointer entries
    size_t io_in_bytes = 0, io_out_bytes = 0;
    std::vector<uint32_t> h_step;
    // matrix-kernel planning (tx_select.h, tx_fused.hip) and the shared LO of a call
    srx::TxSelPlan sel;
    bool phase_uniform = true;
    uint32_t delay_index = 0, phase_host = 0;
    float2 *d_lo = nullptr;
    bool lo_valid = false; uint32_t lo_phase = 0, lo_step = 0, lo_n = 0;   // what d_lo holds
    size_t lo_bytes = 0;
    void *d_ttab16 = nullptr;     // k_tx_split16: Toeplitz fragments of the interpolator phases
    int tpost = 0;                // tap scale exponent of that table
    struct Fm {                   // SELENITE_MODE_FM (selenite_tx_set_fm, tx_fm.hip); the rows live as long as the instance once allocated
        bool set = false;
        srx::TxFmParams p{};
        uint32_t *d_tone_step = nullptr, *d_tone_phase = nullptr;
    } fm;
    struct Cw {                   // keyed CW (selenite_tx_set_cw, tx_cw.hip); p.offset holds + offset_step, the mode's sign is applied per call
        bool set = false;
        srx::TxCwParams p{};
        float *d_shape = nullptr;
        uint32_t *d_side_step = nullptr, *d_side_phase = nullptr, *d_tx_on = nullptr, *d_hold = nullptr;
        uint8_t *d_key_state = nullptr;
        void *d_io_side = nullptr;
        size_t io_side_bytes = 0;
    } cw;
    struct In {                   // the audio input stage (selenite_tx_set_in, tx_in.hip)
        bool set = false;
        srx::TxInParams p{};
        float level_init = 0.0f;
        float *d_coeffs = nullptr, *d_dec = nullptr, *d_level = nullptr;
        uint32_t *d_open = nullptr, *d_hold = nullptr;
        uint64_t *d_opens = nullptr, *d_open_blocks = nullptr;
        void *d_audio = nullptr;  // the stage's output of the last frame call: what run() then reads
        size_t audio_bytes = 0;
    } in;
    struct Keyer {                // the keyer stage (selenite_tx_set_keyer, tx_keyer.hip); d_state holds the eleven state rows, [word][channels]
        bool set = false;
        srx::TxKeyerParams p{};
        uint32_t *d_unit = nullptr, *d_state = nullptr;
        uint8_t *d_codes = nullptr, *d_text = nullptr;
        void *d_key = nullptr;    // the stage's output of the last paddle call: what the keyed launch then reads
        size_t key_bytes = 0;
    } keyer;
    hipStream_t stream = nullptr, own_stream = nullptr;
    int status = 0;
    std::string err;
};

#pragma GCC visibility push(hidden)
namespace srx {

inline int fail(selenite_tx_instance *S, int code, const std::string &msg)
{
    if (S && S->status == 0) { S->status = code; S->err = msg; }
    return code;
}

// One host buffer of a host-pointer call and the instance's grow-only device buffer that stages it.  A NULL host pointer: not in this call.
enum : int { kToDevice = 1, kToHost = 2 };
struct Staged { const void *host; size_t bytes; int dir; void **dev; size_t *cap; };
// grow the buffers, copy in, enqueue() (0, or the error code to return), copy out, drain
template <typename F>
inline int staged_call(selenite_tx_instance *S, std::initializer_list<Staged> bufs, F &&enqueue)
{
    if (hipSetDevice(S->device) != hipSuccess) return fail(S, SELENITE_RX_DEVICE_ERROR, "hipSetDevice");
    for (const Staged &b : bufs)
        if (b.host && ensure(S, b.dev, b.cap, b.bytes)) return S->status;
    for (const Staged &b : bufs)
        if (b.host && (b.dir & kToDevice) && hipMemcpyAsync(*b.dev, b.host, b.bytes, hipMemcpyHostToDevice, S->stream) != hipSuccess)
            return fail(S, SELENITE_RX_DEVICE_ERROR, "H2D copy failed");
    if (int rc = enqueue()) return rc;
    for (const Staged &b : bufs)
        if (b.host && (b.dir & kToHost) && hipMemcpyAsync(const_cast<void *>(b.host), *b.dev, b.bytes, hipMemcpyDeviceToHost, S->stream) != hipSuccess)
            return fail(S, SELENITE_RX_DEVICE_ERROR, "D2H copy failed");
    if (hipStreamSynchronize(S->stream) != hipSuccess) return fail(S, SELENITE_RX_DEVICE_ERROR, "D2H copy failed");
    return SELENITE_RX_SUCCESS;
}
inline size_t sample_bytes(bool q15) { return q15 ? sizeof(int16_t) : sizeof(float); }

// ---- tx_api.hip ----
bool block_size_ok(selenite_tx_instance *S, uint32_t block_size, const char *who);
TxParams make_params(const selenite_tx_instance *S, uint32_t block_size);
// the decision (tx_select.h) for a call of this length on the instance as it stands
TxDecision decide(const selenite_tx_instance *S, const TxParams &p, bool key);
// one audio call on device pointers: decides, refuses or moves the host's state, launches
int run(selenite_tx_instance *S, const void *src, void *dst, bool q15, uint32_t block_size);

// ---- the stages: free my buffers, reset my state on the instance's stream (enqueued or drained); their entry points are C-ABI ----
void tx_fm_free(selenite_tx_instance *S);
int tx_fm_reset(selenite_tx_instance *S);
void tx_cw_free(selenite_tx_instance *S);
int tx_cw_reset(selenite_tx_instance *S);
void tx_in_free(selenite_tx_instance *S);
int tx_in_reset(selenite_tx_instance *S);
void tx_keyer_free(selenite_tx_instance *S);
int tx_keyer_reset(selenite_tx_instance *S);
// tx_cw.hip, for the keyer: a key call's refusals (0: none) and its launch on device pointers
int tx_key_call_ok(selenite_tx_instance *S, const void *key, const void *dst, uint32_t block_size, const char *who);
int tx_run_key(selenite_tx_instance *S, const uint8_t *key, void *dst, void *side, bool q15, uint32_t block_size);

}  // namespace srx
#pragma GCC visibility pop
