// rx_internal.h -- instance layout and kernel-launch interfaces shared by the translation units
// of libselenite_rx.so.  Not part of the C-ABI (include/selenite_rx.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/selenite_rx.h"
#include "rx_device.h"
#include "rx_diag.h"
#include "rx_select.h"

struct selenite_rx_instance;

namespace srx {

// A contiguous range of the instance's channels: what one launch serves.  The whole instance is { 0, cfg.channels }; a chunk of a
// host-pointer call (rx_hostpipe.hip) is a part of it.  count is never 0.  Every per-channel array moves with `first`.
struct ChanRange { uint32_t first, count; };

// Everything a kernel needs, passed by value (kernarg segment -> SGPRs).
struct RxParams {
    uint32_t channels;
    uint32_t block;        // DSP block (input samples)
    uint32_t decim;        // M
    uint32_t nd;           // decimator taps (0 = bypass)
    uint32_t nh;           // Hilbert / delay taps (0 = none)
    uint32_t nbiq;         // biquad stages
    uint32_t mode;         // SELENITE_MODE_*
    uint32_t nco;          // 0 = off, 1 = per-channel LO computed in the kernel, 2 = shared LO table `lo` (Decision::nco_rx)
    uint32_t agc;          // AGC enabled
    uint32_t block_size;   // input samples per channel in this call
    uint32_t nout;         // block_size / decim
    uint32_t in_stride;    // complex samples between consecutive channels in the source buffer (>= block_size)
    uint32_t out_stride;   // audio samples between consecutive channels in the destination buffer (>= nout)
    uint32_t pass_out;     // generic front kernel: decimated outputs per pass
    uint32_t q15_round;    // int16 output: 1 = the ARM_MATH_ROUNDING variant of arm_float_to_q15 (arm_float_to_q15.c:90-101), 0 = truncation (the firmware's build)
    uint32_t out_cached;   // 1: the audio this launch writes is read back by a later kernel of the same call (global gain, phase 1):
                           // default store policy; 0: written once -- non-temporal stores
    const float *dec_c, *hilb_c, *delay_c, *biq_c, *sintab;
    const float2 *lo;      // nco == 2: LO[n] = (cos, -sin) for the samples of this call (all channels share it)
    uint32_t lo_period;    // nco == 2: 256 when LO[n + 256] == LO[n] for every n (NCO step a multiple of 2^24), else 0;
                           // nco == 1: 256 when EVERY channel's step is a multiple of 2^24 (each channel's own LO has that period)
    const uint32_t *step;
    uint32_t *phase;
    float *dec_state;      // [C][2][nd-1]
    float *fir_state;      // [C][2][nh-1]
    float *biq_state;      // [C][nbiq][4]
    float *gain;           // [C]
    float *env_part;       // global gain, phase 1 (k_ssb_split16, 16-lane DSP blocks, whole passes): max |audio| of every DSP block,
                           // [channels][block_size / block]; NULL = not wanted
    uint32_t *flags;       // device flag / counter words (kFlag* below): [0] bit 0 = a kernel produced non-finite audio (ARM_MATH_NANINF)
    // ---- parity guard of the split-precision kernels ----
    // A DSP block is GUARDED when max |audio| (before the AGC) < guard_ratio * the largest |component| of the samples its
    // pass's matrix product saw: the region where the split product and CMSIS, two f32-class results with independent
    // rounding noise of ~1e-7 of the INPUT, may differ by more than 1e-5 of the (small) block maximum.
    float guard_ratio;
    uint32_t *guard_ch;    // [channels] sticky count of guarded DSP blocks per channel, or NULL
    uint32_t *guard_calls; // [channels] sticky count of process calls in which the channel had a guarded block, or NULL
    uint32_t *guard_hand;  // [channels] sticky count of "handover" blocks (SELENITE_ARITH_AUTO, k_ssb_split16): guarded blocks inside the
                           // Hilbert-pair history of a call whose predecessor left the channel's state in split16 precision, or NULL
    // SELENITE_ARITH_AUTO: a channel with a guarded block in this call keeps its pre-call streaming state (the split16
    // kernel does not write it back) and raises rerun_flag[channel] (every channel's flag is rewritten every call: plain
    // stores, no atomics -- 48 k atomics on one counter cost 0.7 ms per launch when most channels were guarded); a second
    // launch of the bit-exact kernel (chan_flags = those flags) recomputes the call for the flagged channels -- audio and
    // state -- in the CMSIS arithmetic
    uint32_t *rerun_flag;        // [channels] or NULL (plain SPLIT16: count only).  Word of a channel (SELENITE_ARITH_AUTO):
                                 //   bit 0      recompute this channel's current call in exact arithmetic (kFlagRerun)
                                 //   bits 1-2   provenance of the channel's streaming state (kProv*): what the call before left
                                 //   bit 3      which of the two hist_ext buffers holds the samples in front of that state
                                 //   bit 4      that row holds raw int16 samples (kExtQ15)
                                 //   bit 5      hysteresis (kFlagHold): the exact kernel serves this channel DIRECTLY -- the matrix kernel skips
                                 //              it -- until two calls in a row show no block near the guard ratio (bit 6: one has) (round 4)
                                 //   bits 8-31  the largest |component| the LAST pass of the call before held in its images (the upper 24 bits
                                 //              of the float's bit pattern, rounded up): the first blocks of this call still see Hilbert-pair
                                 //              history computed from those samples, so their guard threshold covers them too (kLvlMask)
    // k_ssb_split16, SELENITE_ARITH_AUTO: the mixed samples in front of the decimator state, hist_ext[buf][channel][ext_len] (I, Q),
    // positions [E - (nd - 1) - ext_len, E - (nd - 1)) of the stream that ends at E -- what it takes to recompute the Hilbert-pair
    // history (the last HH4 decimated samples) in exact arithmetic when the NEXT call has to be rerun (k_hist_exact)
    float2 *hist_ext;            // or NULL
    uint32_t ext_len;            // decim * HH4
    size_t ext_buf_stride;       // elements between the two buffers
    uint32_t *chan_flags;  // exact kernels as the rerun pass of SELENITE_ARITH_AUTO: the channel words (= rerun_flag of the matrix kernel's launch)
    // ... and the channels to recompute as a DENSE list (round 4): k_hist_exact, in front of the rerun pass, appends every channel whose
    // rerun bit is up (one atomic per 16-channel window that has any) -- workgroup b of the rerun pass then takes entries b, b + grid, ...:
    // an even share whatever the pattern of flagged channels (walking the words in windows gave the slowest workgroup ~32 channels when
    // 80 % were flagged: as long as recomputing everything).  Two counters alternate between calls: a call's prepare kernel zeroes
    // the one the NEXT call will count in.
    uint32_t *chan_list;         // [channels]
    uint32_t *chan_count;        // entries in chan_list (device)
    uint32_t *chan_count_next;   // zeroed by this call's prepare kernel
    uint32_t *rerun_par_host;    // HOST word (the instance's): which of the two counters the next prepare kernel counts in -- read and
                                 // flipped where that kernel is launched (rx_fused.hip: launch_shape), so a call that never launches it
                                 // (a short call on the bit-exact kernel) leaves the pair in step
    uint32_t auto_inline;        // SELENITE_ARITH_AUTO: 1 = ONE launch where the matrix kernel can recompute the channel it flagged itself (k_hilb_split16:
                                 // FusedArgs::inl); 0 = always k_hist_exact + the rerun pass behind it.  The bits of the result do not depend on it.
    uint32_t *form_host;         // HOST word (the instance's): the form the last SELENITE_ARITH_AUTO launch took, 1 or 3 (launch_shape writes it; a diagnostic)
    uint32_t *rerun_seen;        // page-locked HOST word the device can write (the instance's): how many channels the rerun pass of the
                                 // last call found on its list -- written by that pass, read by the host WITHOUT synchronising when it sizes
                                 // the next rerun pass (a stale value only picks the other grid: results do not depend on it)
    AgcParams agcp;
};

// words of RxParams::flags
enum { kFlagNanInf = 0, kFlagWords = 4 };
// RxParams::rerun_flag words
enum : uint32_t { kFlagRerun = 1u, kProvShift = 1u, kProvMask = 3u, kProvExact = 0u, kProvSplitExt = 1u, kProvSplit = 2u, kExtBufShift = 3u,
                  kExtQ15 = 16u,       // bit 4: the hist_ext row holds the RAW int16 samples of an int16-slot call (half the bytes; k_hist_exact mixes them again)
                  kFlagHold = 32u,     // bit 5: held on the exact kernel (hysteresis of SELENITE_ARITH_AUTO)
                  kFlagClean1 = 64u,   // bit 6: ... and its last call there had no block near the guard ratio (the second such call in a row hands it back)
                  kLvlMask = 0xFFFFFF00u };

__host__ __device__ inline bool mode_is_cw(uint32_t m) { return m == SELENITE_MODE_CW || m == SELENITE_MODE_CWR; }
__host__ __device__ inline bool mode_is_upper(uint32_t m)
{
    return m == SELENITE_MODE_USB || m == SELENITE_MODE_DIG || m == SELENITE_MODE_CW;
}

// ---- generic path (rx_generic.hip): any configuration, three simple kernels ----
// front: NCO -> decimator -> demodulator, un-scaled audio (f32) to `audio`
hipError_t launch_front_generic(const RxParams &p, int arith, const void *src, bool src_q15,
                                float *audio, hipStream_t st);
size_t front_generic_lds_bytes(const RxParams &p);
// arm_q15_to_float over a whole buffer (SupportFunctions/arm_q15_to_float.c:87): n int16 values -> n floats, any n and any alignment
hipError_t launch_q15_to_f32(const int16_t *src, float *dst, size_t n, hipStream_t st);
// SELENITE_ARITH_AUTO, in front of the rerun pass: the Hilbert-pair history of every flagged channel whose state the call before left
// on the matrix kernel (with its hist_ext) is recomputed in exact arithmetic from hist_ext + the decimator state (rx_generic.hip)
// (all: a call that runs the exact kernel on every channel -- FM, a shape without a matrix kernel for this call length -- repairs every such channel)
hipError_t launch_hist_exact(const RxParams &p, bool all, hipStream_t st);
// CW biquad cascade, in place on f32 audio
hipError_t launch_biquad_generic(const RxParams &p, int arith, float *audio, hipStream_t st);
// per-channel AGC (or plain copy/convert when p.agc == 0): audio -> dst
hipError_t launch_agc_generic(const RxParams &p, int arith, const float *audio, void *dst,
                              bool dst_q15, hipStream_t st);
// global-gain AGC pieces: env[b] = max over channels of max|audio| in DSP block b
uint32_t env_global_rows(const RxParams &p);
hipError_t launch_env_global(const RxParams &p, const float *audio, float *part, float *env, hipStream_t st);
// env[b] = max over `rows` rows of part[row][b]; part holds env_fold_scratch_floats(rows, nblk) floats (scratch behind the rows)
size_t env_fold_scratch_floats(uint32_t rows, uint32_t nblk);
hipError_t launch_env_fold(float *part, float *env, uint32_t rows, uint32_t nblk, hipStream_t st);
hipError_t launch_agc_apply_global(const RxParams &p, int arith, const float *audio, const float *env,
                                   void *dst, bool dst_q15, hipStream_t st);

// ---- NLMS noise reduction / automatic notch (rx_nlms.hip): in place on un-scaled f32 audio, between the demodulator and the AGC ----
struct NrParams {
    uint32_t channels;     // channels of this launch (a ChanRange: the arrays below are offset to it)
    uint32_t nout;         // audio samples per channel in this call
    uint32_t stride;       // audio samples between consecutive channels (RxParams::out_stride)
    uint32_t delay;        // D
    uint32_t notch;        // 1: output e = x - y (SELENITE_RX_NR_NOTCH), 0: y (SELENITE_RX_NR_DENOISE)
    float mu;
    float *coeffs;         // [C][N]
    float *window;         // [C][N-1] oldest first
    float *delay_line;     // [C][D] oldest first
    float *energy;         // [C]
    float *x0;             // [C]
    uint32_t *flags;       // RxParams::flags (kFlagNanInf)
};
hipError_t launch_nlms(const NrParams &q, uint32_t num_taps, float *audio, hipStream_t st);
// the stage's part of the instance (selenite_rx_set_nr): kind SELENITE_RX_NR_OFF = no stage, no buffers
struct __attribute__((visibility("hidden"))) NrStage {
    uint32_t kind = SELENITE_RX_NR_OFF, taps = 0, delay = 0;
    float mu = 0.0f;
    std::vector<float> h_init;         // [taps] the weights set_nr / reset start from
    float *d_coeffs = nullptr, *d_window = nullptr, *d_delay = nullptr, *d_energy = nullptr, *d_x0 = nullptr;
    void release();                                         // frees the buffers: no stage
    int init_state(selenite_rx_instance *S);                // the state arm_lms_norm_init_f32 leaves
    NrParams params(ChanRange r, const RxParams &p) const;  // the stage's view of a launch: the channels and the audio geometry of `p`
};

// ---- audio output stage (rx_out.hip): arm_fir_interpolate_f32 -> [arm_float_to_q15] -> mono / stereo frames, behind the AGC ----
struct OutParams {
    uint32_t channels;     // channels of this launch (a ChanRange: `state` is offset to it)
    uint32_t nout;         // audio samples per channel in this call (input of the stage)
    uint32_t stride;       // audio samples between consecutive channels of `audio`
    uint32_t phase_len;    // P = ni_taps / interp; 0: no FIR (interp == 1), the samples pass as they are
    uint32_t q15_round;    // int16 output: RxParams::q15_round
    uint32_t vec;          // 1: dst and every row of it are 16-byte aligned -- whole 16-byte stores per lane; 0: element stores
    const float *coeffs;   // [interp * P] pCoeffs order
    float *state;          // [C][P - 1] oldest first
    uint32_t *flags;       // RxParams::flags (kFlagNanInf)
};
// bytes of one interpolated sample in dst
inline uint32_t out_sample_bytes(bool stereo, bool q15) { return (q15 ? 2u : 4u) * (stereo ? 2u : 1u); }
hipError_t launch_out(const OutParams &q, uint32_t interp, bool stereo, bool dst_q15, const float *audio, void *dst, hipStream_t st);
// the stage's part of the instance (selenite_rx_set_out): on = false: no stage, no buffers
struct __attribute__((visibility("hidden"))) OutStage {
    bool on = false;
    uint32_t interp = 1, taps = 0, frames = SELENITE_RX_OUT_MONO;
    float *d_coeffs = nullptr, *d_state = nullptr;          // [taps] | [channels][taps / interp - 1]
    float *d_audio = nullptr; size_t audio_bytes = 0;       // f32 audio of the chain in front of the stage, [channels of the launch][blockSize / decim]
    void release();                                         // frees the buffers: no stage
    int init_state(selenite_rx_instance *S);                // the state arm_fir_interpolate_init_f32 leaves
    OutParams params(const selenite_rx_instance *S, ChanRange r, const void *dst, bool dst_q15, uint32_t block_size) const;
    // d_audio, grown to the launch: where the chain writes in front of the stage
    int audio_buffer(selenite_rx_instance *S, ChanRange r, uint32_t block_size, float **audio);
    // the stage kernel, once over the whole call: `audio` (audio_buffer) -> the caller's dst
    int run(selenite_rx_instance *S, ChanRange r, const float *audio, void *dst, bool dst_q15, uint32_t block_size) const;
};

// ---- spectrum tap (rx_spectrum.hip): window -> arm_cfft_f32 -> arm_cmplx_mag_squared_f32 -> averaged, display-ordered row, on the raw input ----
struct SpecParams {
    uint32_t channels;     // channels of this launch (a ChanRange: rows and pending are offset to it)
    uint32_t block_size;   // input samples per channel in this call
    uint32_t in_stride;    // complex samples between consecutive channels of the source
    uint32_t off;          // samples of the call's first frame that arrived with earlier calls (stream position % fft_len)
    uint32_t first;        // frames from the call's first frame to the first one that is transformed (frame index % stride == 0), < stride
    uint32_t stride;
    uint32_t average;      // 1: row += alpha * (p - row); 0: row = p
    float alpha;
    const float *tw;       // [fft_len][2] (cos, sin) (rx_spectrum.hip: spec_twiddles)
    const float *window;   // [fft_len] or NULL
    float *rows;           // [C][fft_len] display order
    float *pending;        // [C][fft_len][2] the samples so far of the frame the stream stands in
};
hipError_t launch_spectrum(const SpecParams &q, uint32_t fft_len, const void *src, bool src_q15, hipStream_t st);
// the stage's part of the instance (selenite_rx_set_spectrum): len = 0: no stage, no buffers
struct __attribute__((visibility("hidden"))) SpecStage {
    uint32_t len = 0, stride = 1, average = 0;
    float alpha = 1.0f;
    uint64_t pos = 0;                  // input samples per channel since set_spectrum / reset: advanced once per call (rx_dispatch.hip: advance_streams)
    float *d_tw = nullptr, *d_window = nullptr;             // [len][2] | [len] or NULL
    float *d_rows = nullptr, *d_pending = nullptr;          // [channels][len] | [channels][len][2]
    void release();                                         // frees the buffers: no stage
    int init_state(selenite_rx_instance *S);                // the state set_spectrum leaves
    // false: a call of block_size samples that starts at stream position `at` touches no transformed frame -- nothing to launch
    bool params(ChanRange r, uint64_t at, uint32_t block_size, SpecParams &q) const;
    // one launch on the instance's stream, on the caller's own input (f32, or int16 read directly)
    int run(selenite_rx_instance *S, ChanRange r, uint64_t at, const void *src, bool src_q15, uint32_t block_size) const;
};
// (host: spec_twiddles, twiddleCoef_n regenerated as the reference's table holds it, lives in rx_fft8.h)

// ---- impulse noise blanker (rx_nb.hip): frame power -> arm_mean_f32 -> level, hits over threshold * level blanked, on the raw input ----
struct NbParams {
    uint32_t channels;     // channels of this launch (a ChanRange: level and the counters are offset to it)
    uint32_t block_size;   // input samples per channel in this call = complex samples between consecutive channels of source and copy
    uint32_t guard;        // samples blanked on either side of a hit
    uint32_t max_hits;     // more hits than this in a frame: a burst, nothing blanked
    float threshold, alpha, clamp;
    float *level;          // [C]
    uint64_t *blanked;     // [C] samples blanked so far
    uint64_t *bursts;      // [C] frames with more than max_hits hits so far
};
hipError_t launch_nb(const NbParams &q, uint32_t frame, const void *src, bool src_q15, void *dst, hipStream_t st);
// the stage's part of the instance (selenite_rx_set_nb): frame = 0: no stage, no buffers
struct __attribute__((visibility("hidden"))) NbStage {
    uint32_t frame = 0, guard = 0, max_hits = 0;
    float threshold = 0.0f, alpha = 0.0f, clamp = 0.0f;
    float *d_level = nullptr;                               // [channels]
    uint64_t *d_blanked = nullptr, *d_bursts = nullptr;     // [channels] each
    void *d_buf = nullptr; size_t buf_bytes = 0;            // the blanked copy of a call's input, [channels of the launch][blockSize][2], f32 or int16
    void release();                                         // frees the buffers: no stage
    int init_state(selenite_rx_instance *S);                // the state set_nb leaves
    // one launch on the instance's stream: `src` (f32, or int16 as it is) -> d_buf, grown to the launch; *blanked_src = d_buf
    int run(selenite_rx_instance *S, ChanRange r, const void *src, bool src_q15, uint32_t block_size, const void **blanked_src);
};

// ---- I/Q correction (rx_iqc.hip): DC offset, gain and phase imbalance of the raw input, estimated per frame and removed ----
struct IqcParams {
    uint32_t channels;     // channels of this launch (a ChanRange: the five state rows are offset to it)
    uint32_t block_size;   // input samples per channel in this call = complex samples between consecutive channels of source and copy
    float alpha, dc_alpha; // 0: that estimate is off
    float p_max, g_min, g_max, min_power;
    float *dc_i, *dc_q;    // [C] each
    float *p, *g;          // [C] each
    uint64_t *held;        // [C] frames whose imbalance estimate was not valid so far
};
hipError_t launch_iqc(const IqcParams &q, uint32_t frame, const void *src, bool src_q15, float *dst, hipStream_t st);
// the stage's part of the instance (selenite_rx_set_iqc): frame = 0: no stage, no buffers
struct __attribute__((visibility("hidden"))) IqcStage {
    uint32_t frame = 0;
    float alpha = 0.0f, dc_alpha = 0.0f, p_max = 0.0f, g_min = 0.0f, g_max = 0.0f, min_power = 0.0f;
    float p_init = 0.0f, g_init = 0.0f, dc_i_init = 0.0f, dc_q_init = 0.0f;
    float *d_dc_i = nullptr, *d_dc_q = nullptr, *d_p = nullptr, *d_g = nullptr;      // [channels] each
    uint64_t *d_held = nullptr;                             // [channels]
    float *d_buf = nullptr; size_t buf_bytes = 0;           // the corrected copy of a call's input, [channels of the launch][blockSize][2] f32
    void release();                                         // frees the buffers: no stage
    int init_state(selenite_rx_instance *S);                // the state set_iqc leaves
    // one launch on the instance's stream: `src` (f32, or int16 as it is) -> d_buf (always f32), grown to the launch; *corrected_src = d_buf
    int run(selenite_rx_instance *S, ChanRange r, const void *src, bool src_q15, uint32_t block_size, const void **corrected_src);
};

// ---- signal-level meter and squelch (rx_meter.hip): arm_power_f32 per DSP block of the un-scaled audio -> level -> open / close, in front
// of the AGC; the gate zeroes the closed blocks behind it ----
struct MeterParams {
    uint32_t channels;     // channels of this launch (a ChanRange: the five state rows and `bits` are offset to it)
    uint32_t n;            // audio samples of a DSP block: block / decim
    uint32_t nblk;         // DSP blocks per channel in this launch
    uint32_t stride;       // audio samples between consecutive channels (RxParams::out_stride)
    uint32_t sense;        // SELENITE_RX_SQ_*
    uint32_t hang;
    float attack, decay, open_level, close_level;
    float *level;          // [C]
    uint32_t *open;        // [C] 0 / 1
    uint32_t *hold;        // [C]
    uint64_t *opens;       // [C] closed -> open transitions so far
    uint64_t *open_blocks; // [C] blocks that ended open so far
    uint8_t *bits;         // [C][nblk] the gate of every block of this launch: `open` behind its update (k_meter writes, k_gate reads)
};
hipError_t launch_meter(const MeterParams &q, const float *audio, hipStream_t st);
// zeros over the blocks of dst (f32 or int16, rows `stride` apart) whose byte in q.bits is 0
hipError_t launch_gate(const MeterParams &q, void *dst, bool dst_q15, hipStream_t st);
// the stage's part of the instance (selenite_rx_set_meter): on = false: no stage, no buffers
struct __attribute__((visibility("hidden"))) MeterStage {
    bool on = false;
    uint32_t sense = 0, gate = 0, hang = 0;
    float attack = 0.0f, decay = 0.0f, open_level = 0.0f, close_level = 0.0f, level_init = 0.0f;
    float *d_level = nullptr;                               // [channels]
    uint32_t *d_open = nullptr, *d_hold = nullptr;          // [channels] each
    uint64_t *d_opens = nullptr, *d_open_blocks = nullptr;  // [channels] each
    // the gate bytes of the last launch, [cfg.channels][blocks of the launch], indexed by absolute channel; grown by the first call that needs
    // it; lives from selenite_rx_global_phase1_device to _phase2_device
    uint8_t *d_bits = nullptr; size_t bits_bytes = 0;
    void release();                                         // frees the buffers: no stage
    int init_state(selenite_rx_instance *S);                // the state set_meter leaves
    MeterParams params(ChanRange r, const RxParams &p) const;   // the stage's view of a launch: the channels and the audio geometry of `p`
};

// ---- audio biquad filter (rx_afilt.hip): arm_biquad_cascade_df1_f32 in place on the un-scaled audio, behind the demodulator and the CW
// filter, in front of NLMS, the meter and the AGC ----
struct AfiltParams {
    uint32_t channels;     // channels of this launch (a ChanRange: `state` and per-channel `coeffs` are offset to it)
    uint32_t nout;         // audio samples per channel in this call
    uint32_t stride;       // audio samples between consecutive channels (RxParams::out_stride)
    uint32_t n_stages;     // 1 .. 8
    uint32_t per_channel;  // 0: coeffs [n_stages][5]; 1: coeffs [C][n_stages][5]
    const float *coeffs;
    float *state;          // [C][n_stages][4] { x1, x2, y1, y2 }
};
hipError_t launch_afilt(const AfiltParams &q, float *audio, hipStream_t st);
// the stage's part of the instance (selenite_rx_set_afilt): on = false: no stage, no buffers
struct __attribute__((visibility("hidden"))) AfiltStage {
    bool on = false;
    uint32_t n_stages = 0, per_channel = 0;
    float *d_coeffs = nullptr;                              // [n_stages][5] | [channels][n_stages][5]
    float *d_state = nullptr;                               // [channels][n_stages][4]
    void release();                                         // frees the buffers: no stage
    int init_state(selenite_rx_instance *S);                // the state set_afilt leaves: +0.0f
    AfiltParams params(ChanRange r, const RxParams &p) const;   // the stage's view of a launch: the channels and the audio geometry of `p`
};

// ---- tone-detector bank (rx_tones.hip): K Goertzel recurrences and the frame energy per channel, a tap on the un-scaled audio behind the
// demodulator and the CW filter, in front of the audio filter, NLMS, the meter and the AGC ----
struct TonesParams {
    uint32_t channels;     // channels of this launch (a ChanRange: the state rows are offset to it)
    uint32_t nout;         // audio samples per channel in this launch: whole DSP blocks
    uint32_t stride;       // audio samples between consecutive channels (RxParams::out_stride)
    uint32_t n;            // audio samples per DSP block (block / decim)
    uint32_t n_tones;      // K: 1 .. 64
    uint32_t frame_blocks; // DSP blocks per frame
    uint32_t fb0;          // DSP blocks of the running frame that lie in front of this launch: 0 .. frame_blocks - 1
    uint32_t confirm, release;
    float ratio, min_power;
    const float *coeffs;   // [K][3] { 2 cos w, cos w, sin w }
    float *s;              // [C][K][2] { s1, s2 }
    float *energy;         // [C] the running frame's E
    float *power;          // [C][K] of the last whole frame
    float *frame_energy;   // [C] of the last whole frame
    uint32_t *last_best, *tone, *cand, *run;
    uint64_t *changes;
};
hipError_t launch_tones(const TonesParams &q, const float *audio, hipStream_t st);
// the stage's part of the instance (selenite_rx_set_tones): on = false: no stage, no buffers
struct __attribute__((visibility("hidden"))) TonesStage {
    bool on = false;
    uint32_t n_tones = 0, frame_blocks = 0, confirm = 0, rel = 0;
    float ratio = 0.0f, min_power = 0.0f;
    uint64_t pos = 0;                  // DSP blocks per channel since set_tones / reset: advanced once per call (rx_dispatch.hip: advance_streams)
    float *d_coeffs = nullptr, *d_s = nullptr, *d_energy = nullptr, *d_power = nullptr, *d_frame_energy = nullptr;
    uint32_t *d_last_best = nullptr, *d_tone = nullptr, *d_cand = nullptr, *d_run = nullptr;
    uint64_t *d_changes = nullptr;
    void release();                                         // frees the buffers: no stage
    int init_state(selenite_rx_instance *S);                // the state set_tones leaves
    TonesParams params(ChanRange r, const RxParams &p, uint32_t blocks_before) const;
};

// ---- Morse decoder (rx_cwdec.hip): arm_power_f32 per DSP block of the un-scaled audio -> peak / floor followers -> debounced key ->
// element timing -> text, a tap at the tone bank's place ----
struct CwdecParams {
    uint32_t channels;     // channels of this launch (a ChanRange: the state rows and `text` are offset to it)
    uint32_t n;            // audio samples of a DSP block: block / decim
    uint32_t nblk;         // DSP blocks per channel in this launch
    uint32_t stride;       // audio samples between consecutive channels (RxParams::out_stride)
    float peak_attack, peak_decay, floor_attack, floor_decay, on_frac, off_frac, snr, min_power;
    uint32_t debounce, adapt, track, unit_min, unit_max;
    uint32_t ring;         // a power of two
    const uint8_t *table;  // [256]
    float *peak, *floor;   // [C] each
    uint32_t *primed, *key, *flip, *run, *unit, *code, *word;      // [C] each
    uint64_t *count;       // [C]
    uint8_t *text;         // [C][ring]
};
hipError_t launch_cwdec(const CwdecParams &q, const float *audio, hipStream_t st);
// the stage's part of the instance (selenite_rx_set_cwdec): on = false: no stage, no buffers
struct __attribute__((visibility("hidden"))) CwdecStage {
    bool on = false;
    float peak_attack = 0.0f, peak_decay = 0.0f, floor_attack = 0.0f, floor_decay = 0.0f, on_frac = 0.0f, off_frac = 0.0f, snr = 0.0f, min_power = 0.0f;
    uint32_t debounce = 0, adapt = 0, track = 0, unit_min = 0, unit_init = 0, unit_max = 0, ring = 0;
    uint8_t *d_table = nullptr;                             // [256]
    float *d_peak = nullptr, *d_floor = nullptr;            // [channels] each
    uint32_t *d_primed = nullptr, *d_key = nullptr, *d_flip = nullptr, *d_run = nullptr, *d_unit = nullptr, *d_code = nullptr, *d_word = nullptr;
    uint64_t *d_count = nullptr;                            // [channels]
    uint8_t *d_text = nullptr;                              // [channels][ring]
    void release();                                         // frees the buffers: no stage
    int init_state(selenite_rx_instance *S);                // the state set_cwdec leaves
    CwdecParams params(ChanRange r, const RxParams &p) const;   // the stage's view of a launch: the channels and the audio geometry of `p`
};

// ---- FSK teleprinter decoder (rx_fskdec.hip): two one-section arm_biquad_cascade_df1_f32 tone filters and arm_power_f32 per tick of the
// un-scaled audio -> three followers -> level with hysteresis -> start / data / stop bit clock -> ITA2 text, a tap at the tone bank's place ----
struct FskdecParams {
    uint32_t channels;     // channels of this launch (a ChanRange: the state rows and `text` are offset to it)
    uint32_t n;            // audio samples of a DSP block: block / decim
    uint32_t nblk;         // DSP blocks per channel in this launch
    uint32_t stride;       // audio samples between consecutive channels (RxParams::out_stride)
    uint32_t tick;         // T: divides n
    uint32_t reverse, usos;
    uint32_t ring;         // a power of two
    float mark[5], space[5];   // {b0, b1, b2, a1, a2}
    float alpha, hyst, frac, min_power;
    const uint8_t *table;  // [64]
    float *filt;           // [C][2][4]
    float *em, *es, *ew;   // [C] each
    uint32_t *lvl, *k, *t_q8, *shift, *figs, *ferr, *bit;      // [C] each
    uint64_t *count;       // [C]
    uint8_t *text;         // [C][ring]
};
hipError_t launch_fskdec(const FskdecParams &q, const float *audio, hipStream_t st);
// the stage's part of the instance (selenite_rx_set_fskdec): on = false: no stage, no buffers
struct __attribute__((visibility("hidden"))) FskdecStage {
    bool on = false;
    uint32_t tick = 0, bit_q8 = 0, reverse = 0, usos = 0, ring = 0;
    float mark[5] = {}, space[5] = {};
    float alpha = 0.0f, hyst = 0.0f, frac = 0.0f, min_power = 0.0f;
    uint8_t *d_table = nullptr;                             // [64]
    float *d_filt = nullptr;                                // [channels][2][4]
    float *d_em = nullptr, *d_es = nullptr, *d_ew = nullptr;    // [channels] each
    uint32_t *d_lvl = nullptr, *d_k = nullptr, *d_t_q8 = nullptr, *d_shift = nullptr, *d_figs = nullptr, *d_ferr = nullptr, *d_bit = nullptr;
    uint64_t *d_count = nullptr;                            // [channels]
    uint8_t *d_text = nullptr;                              // [channels][ring]
    void release();                                         // frees the buffers: no stage
    int init_state(selenite_rx_instance *S);                // the state set_fskdec leaves
    FskdecParams params(ChanRange r, const RxParams &p) const;  // the stage's view of a launch: the channels and the audio geometry of `p`
};

// ---- fused fast paths (rx_fused.hip); return false when the configuration is not covered ----
struct FusedPlan {
    SelPlan sel;                  // what select() reads: the shape (kind 0 = none), dense or not, which operands exist (rx_select.h)
    const char *name = "generic";
    std::string name_buf;         // storage behind `name` for the composed kernel names
    float *d_cq = nullptr;        // zero-padded decimator taps in the fused kernel's indexing
    float *d_btab = nullptr;      // banded-Toeplitz B operand of the MFMA decimator
    void *d_btab16 = nullptr;     // same operand split into f16 hi / lo parts (SELENITE_ARITH_SPLIT16)
    float split_post = 1.0f;      // 2^-(sample scale + tap scale) applied to the split-precision result (k_hilb_split16)
    int split_sc = 0;             // tap scale exponent of the split-precision decimator (k_ssb_split16)
    float *d_ptab = nullptr;      // the DENSE flavour of k_ssb_fused: its tap tables [2][DenseTab::LEN]
    uint32_t dense_t0 = 0;        // ... first FIR step with a tap that is not padding
    bool dense_delay_impulse = false;   // ... the delay FIR is a unit impulse (only the Hilbert FIR runs dense)
    bool tables_built = false;
};
hipError_t plan_fused(const selenite_rx_config &cfg, bool delay_is_impulse, bool hilb_odd_only, FusedPlan &plan);
void free_fused(FusedPlan &plan);
// launches what `d` names (rx_select.h: select) -- the kernel, and the launches SELENITE_ARITH_AUTO puts in front of and behind it
hipError_t launch_fused(const FusedPlan &plan, const RxParams &p, const Decision &d, const void *src,
                        bool src_q15, void *dst, bool dst_q15, int delay_index, hipStream_t st);

// fused CW kernel (rx_cw.hip): NCO -> real part -> 4-stage biquad cascade -> AGC
bool cw_fused_ok(const selenite_rx_config &cfg, uint32_t block_size);
bool cw_strides_ok(uint64_t in_stride, uint64_t out_stride);
// no-DSP kernel with the fetch pattern, launch shape and residency of k_cw_fused (rx_cw.hip; bench.py `pattern_roof`)
hipError_t launch_cw_roof(const RxParams &p, const void *src, bool q15, void *dst, float4 *state, uint32_t work, hipStream_t st);
hipError_t launch_cw_fused(const RxParams &p, const void *src, bool src_q15, void *dst, bool dst_q15, hipStream_t st);

// shared local-oscillator table for one call (rx_fused.hip)
hipError_t launch_lo_table(float2 *lo, const float *sintab, uint32_t phase0, uint32_t step, uint32_t nsamp,
                           hipStream_t st);

// ---- synthetic input (rx_synth.hip) ----
hipError_t launch_synth(float *dIQ, const float *sintab, uint32_t first_channel, uint32_t nch,
                        uint64_t first_sample, uint32_t nsamp, uint64_t seed, hipStream_t st);
void synth_host(float *iq, const float *sintab, uint32_t first_channel, uint32_t nch,
                uint64_t first_sample, uint32_t nsamp, uint64_t seed);

// no-arithmetic streaming kernel with the traffic of one process call (rx_synth.hip; bench.py `streaming_roof`)
hipError_t launch_stream_roof(const void *in, void *out, float *state, uint32_t channels, uint32_t in_bytes, uint32_t out_bytes,
                              uint32_t state_words, hipStream_t st);

// host copy of sinTable_f32 regenerated from its documented generator (rx_api.hip)
const float *host_sin_table();

}  // namespace srx

struct selenite_rx_instance {
    selenite_rx_config cfg;            // pointers inside refer to the host copies below
    std::vector<float> h_dec, h_hilb, h_delay, h_biq;
    std::vector<uint32_t> h_step;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    float *d_dec_c = nullptr, *d_hilb_c = nullptr, *d_delay_c = nullptr, *d_biq_c = nullptr, *d_sintab = nullptr;
    uint32_t *d_step = nullptr, *d_phase = nullptr;
    float *d_dec_state = nullptr, *d_fir_state = nullptr, *d_biq_state = nullptr, *d_gain = nullptr;
    uint32_t *d_flags = nullptr;       // kFlagWords words
    uint32_t *d_guard_ch = nullptr;    // [3][channels] guarded DSP blocks per channel | process calls with a guarded block | handover blocks (sticky)
    uint32_t *d_rerun_flag = nullptr;  // [channels] SELENITE_ARITH_AUTO: rerun bit + state provenance (RxParams::rerun_flag)
    uint32_t *d_rerun_list = nullptr;  // [channels + 2] dense list of the channels to recompute, behind its two alternating counters (RxParams::chan_list)
    uint32_t rerun_par = 0;            // which counter the next call counts in
    uint32_t *h_rerun_seen = nullptr;  // page-locked, device-writable: entries of the last rerun pass's list (RxParams::rerun_seen)
    int auto_launches = 1;             // selenite_rx_set_auto_launches: 1 = one launch where the matrix kernel recomputes a channel itself, 3 = never
    uint32_t auto_form_last = 0;       // 1 / 3: the form of the last SELENITE_ARITH_AUTO launch on a matrix kernel (selenite_rx_auto_launches_last)
    float2 *d_hist_ext = nullptr;      // [2][channels][ext_len] SELENITE_ARITH_AUTO with k_ssb_split16: RxParams::hist_ext
    uint32_t ext_len = 0;
    bool handover_repair = true;       // selenite_rx_set_handover_repair
    float guard_ratio = 0.25f;         // -12 dB
    bool steps_grid256 = false;        // every NCO step is a multiple of 2^24: every channel's LO repeats every 256 samples
    float *d_scratch = nullptr;  size_t scratch_bytes = 0;   // intermediate f32 audio
    float *d_conv_in = nullptr;  size_t conv_in_bytes = 0;   // f32 copy of int16 input (int16 slots with a global gain on the fused kernels)
    float *d_env = nullptr;      size_t env_cap = 0;
    float *d_env_part = nullptr; size_t env_part_cap = 0;   // per-wavefront envelope maxima
    void *d_io_in = nullptr;     size_t io_in_bytes = 0;     // staging for the host-pointer entry points (global-gain calls)
    void *d_io_out = nullptr;    size_t io_out_bytes = 0;
    // chunked, double-buffered pipeline of the host-pointer entry points (rx_hostpipe.hip: process_host)
    struct HostPipe {
        hipStream_t h2d = nullptr, d2h = nullptr;
        hipEvent_t ev_in[2] = { nullptr, nullptr }, ev_done[2] = { nullptr, nullptr }, ev_out[2] = { nullptr, nullptr };
        void *d_in[2] = { nullptr, nullptr }, *d_out[2] = { nullptr, nullptr };     // device chunk buffers
        void *h_in[2] = { nullptr, nullptr }, *h_out[2] = { nullptr, nullptr };     // pinned staging (pageable callers only)
        size_t d_in_bytes = 0, d_out_bytes = 0, h_in_bytes = 0, h_out_bytes = 0;
    } pipe;
    float2 *d_lo = nullptr;      size_t lo_bytes = 0;        // shared LO table of the current call
    bool lo_valid = false; uint32_t lo_phase = 0, lo_step = 0, lo_n = 0;   // what d_lo holds: LO[n], n < lo_n, from (lo_phase, lo_step)
    bool steps_uniform = false;        // every channel has the same NCO step
    bool phase_uniform = true;         // ... and the same phase (true after init/reset)
    uint32_t phase_host = 0;           // that common phase, tracked on the host: advanced once per call (rx_dispatch.hip: advance_streams)
    bool delay_is_impulse = false; int delay_index = 0; bool hilb_odd_only = false;
    srx::FusedPlan plan;
    int no_shared_lo = 0;              // SELENITE_RX_NO_SHARED_LO=1: always compute the LO per channel
    int no_periodic_lo = 0;            // SELENITE_RX_NO_PERIODIC_LO=1: never keep a periodic shared LO in registers
    int force_generic = 0;             // SELENITE_RX_FORCE_GENERIC=1 (tests cross-check both paths)
    srx::TonesStage tones;             // tone-detector bank, a tap behind the demodulator / CW filter, in front of the audio filter (rx_tones.hip)
    srx::CwdecStage cwdec;             // Morse decoder, a tap at the tone bank's place (rx_cwdec.hip)
    srx::FskdecStage fskdec;           // FSK teleprinter decoder, a tap at the tone bank's place (rx_fskdec.hip)
    srx::AfiltStage afilt;             // audio biquad filter, behind the demodulator / CW filter, in front of NLMS (rx_afilt.hip)
    srx::NrStage nr;                   // NLMS noise reduction / automatic notch, in front of the AGC (rx_nlms.hip)
    srx::MeterStage meter;             // signal-level meter and squelch, between NLMS and the AGC; its gate behind the AGC (rx_meter.hip)
    srx::OutStage out;                 // audio output stage, behind the chain (rx_out.hip)
    srx::SpecStage spec;               // spectrum tap, in front of the chain (rx_spectrum.hip)
    srx::IqcStage iqc;                 // I/Q correction, between the spectrum tap and the noise blanker (rx_iqc.hip)
    srx::NbStage nb;                   // impulse noise blanker, between the spectrum tap and the chain (rx_nb.hip)
    int status = SELENITE_RX_SUCCESS;
    std::string err;
};
