// rx_afilt.hip -- audio biquad filter (step 4a of DESIGN.md section 2, section 5.12): a manual notch, FM de-emphasis, tone control, an audio
// high-pass or low-pass on the UN-SCALED audio -- behind the demodulator and behind the CW filter, in front of NLMS, the level meter and the
// AGC.  Per channel, the call's nout = blockSize / decim samples continue one stream:
//     arm_biquad_cascade_df1_f32(S, x, x, nout)     FilteringFunctions/arm_biquad_cascade_df1_f32.c:165-407, in place, stage-outer
//       per stage s = 0 .. n_stages-1, coefficients {b0, b1, b2, a1, a2} (CMSIS sign: the a's are ADDED), state {x1, x2, y1, y2}:
//       acc = b0 * x[n];  acc = acc + b1 * x1;  acc = acc + b2 * x2;  acc = acc + a1 * y1;  acc = acc + a2 * y2
//       x2 = x1; x1 = x[n]; y2 = y1; y1 = acc; x[n] = acc
// Every product is rounded, then every sum, in that order (biquad_step<0> of rx_device.h); the unit is compiled with -ffp-contract=off and
// IEEE denormals: bit-exact given its input in every arith mode, whatever the cut of the stream into calls.  The stage never touches the
// NaN / Inf flag word.
//
// k_afilt<NS>: the recurrence has no time parallelism at the reference's rounding, so the parallelism is channels x stages -- the systolic
// array of rx_cw.hip.  Single-wave workgroups; NS = 1, 2, 4 or 8 stage lanes per channel (n_stages 3 runs NS = 4, 5 .. 7 run NS = 8):
//      lane = 16 * row + CPR * stage + channel-in-row      CPR = 16 / NS channels per 16-lane DPP row: 64 / 32 / 16 / 8 channels per wave
// At step k stage s works on sample k - s; one DPP row_shr:CPR hands a stage's output to the next stage's lane.  A lane keeps its five
// coefficients and its four state words in registers for the whole call (per-channel coefficients cost nothing in the loop); the state is
// one 16-byte load and one 16-byte store per lane and call.  The tile's output is taken from the lanes of stage n_stages - 1; the lanes of
// stages n_stages .. NS - 1 compute on whatever reaches them, load no state, store nothing and are never read (no identity padding:
// {1, 0, 0, 0, 0} turns -0.0f into +0.0f and 0 * Inf into NaN).
// The rows stream through LDS in tiles of kAfTile = 64 samples of every channel of the wave: one wave load per row piece (64 consecutive
// floats of one channel: 256 bytes, coalesced; rows are `stride` floats apart and need no alignment), LDS rows 65 words apart (the lanes of
// a step read 65 words apart: conflict-free).  A tile takes tn + NS - 1 steps: NS - 1 masked fill and NS - 1 masked drain steps (a step of
// a stage that has no sample of this tile leaves its state alone), tn - (NS - 1) plain ones.  The last stage writes y[n] over x[n] in the
// tile (x[n] was consumed n_stages - 1 steps before), whole-wave stores write the rows back in place.  The loads of tile t + 1 are in
// flight under the steps of tile t; behind the steps the tile's output is taken out of LDS into registers and the next tile put in BEFORE
// the stores go out, so the wait for loaded data is never a wait for store acknowledgements.
#include "rx_host.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace srx {

constexpr int kAfTile = 64;                      // samples of a channel row per tile: one wave load
constexpr int kAfRow = kAfTile + 1;              // words between the rows in LDS

__device__ __forceinline__ void af_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the input of a lane's stage at one step: the sample `xs` in the stage-0 lanes, elsewhere the output `y` of the lane CPR below (the stage
// before it, same channel) -- lanes of a row are stage-major, so with 2 and 4 stages the stage-0 lanes are whole DPP banks of the row
template <int NS>
__device__ __forceinline__ float af_stage_input(float xs, float y, bool first)
{
    if constexpr (NS == 1) {
        return xs;
    } else {
        constexpr int CPR = 16 / NS;
        if constexpr (CPR >= 4) {
            // ONE DPP move: row_shr:CPR into the banks of stages 1 .. NS-1; the masked-out banks keep `old` = xs
            constexpr int bank_mask = 0xf & ~((1 << (CPR / 4)) - 1);
            return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(xs), __float_as_int(y), 0x110 + CPR, 0xf, bank_mask, false));
        } else {
            // 8 stages: the stage-0 lanes are half a bank -- shift (they read 0: bound_ctrl), then select
            const float prev = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(y), 0x110 + CPR, 0xf, 0xf, true));
            return first ? xs : prev;
        }
    }
}

template <int NS>
__global__ __launch_bounds__(64) void k_afilt(AfiltParams q, float *audio)
{
    constexpr int CH = 64 / NS, CPR = 16 / NS, D = NS - 1;
    // (slack behind the last row: the fill and drain steps of the stage-0 lanes read up to D words past a row's tile, never used)
    __shared__ float tile[CH * kAfRow + 8];

    const int lane = threadIdx.x;
    const int s = (lane & 15) / CPR, ch = (lane >> 4) * CPR + (lane & (CPR - 1));
    const uint32_t ns = q.n_stages, nout = q.nout;
    const uint32_t c0 = blockIdx.x * CH, c = c0 + ch;
    const uint32_t nrow = min((uint32_t)CH, q.channels - c0);                 // channel rows of this wave
    const bool live = c < q.channels && (uint32_t)s < ns;                     // this lane is a stage of a channel
    const bool is_out = (uint32_t)s == ns - 1;                                // ... the one whose output is the cascade's
    const int dn = (int)ns - 1;

    // per-lane stage constants and state
    float b0 = 0.0f;
    typedef float af_v2 __attribute__((ext_vector_type(2)));
    af_v2 c1 = { 0.0f, 0.0f }, c2 = { 0.0f, 0.0f };
    af_v2 PA = { 0.0f, 0.0f }, PB = { 0.0f, 0.0f };                            // (x1, y1), (x2, y2)
    float *const st_row = q.state + ((size_t)c * ns + (uint32_t)s) * 4;
    if (live) {
        const float *k5 = q.coeffs + ((q.per_channel ? (size_t)c * ns : (size_t)0) + (uint32_t)s) * 5;
        b0 = k5[0];
        c1 = af_v2{ k5[1], k5[3] };
        c2 = af_v2{ k5[2], k5[4] };
        const float4 st = *reinterpret_cast<const float4 *>(st_row);         // { x1, x2, y1, y2 } (arm_biquad_cascade_df1_f32.c:73-82)
        PA = af_v2{ st.x, st.z };
        PB = af_v2{ st.y, st.w };
    }

    // one DF1 step of this lane's stage; xs = stage-0 input of the step.  The delay lines are the register pairs A = (x1, y1) and
    // B = (x2, y2): on return B holds the new (x1, y1) and A the new (x2, y2) -- the shift is a change of names (rx_cw.hip)
    auto step = [&](float xs, af_v2 &A, af_v2 &B) -> float {
        const float xin = af_stage_input<NS>(xs, A.y, s == 0);
        const af_v2 t1 = A * c1, t2 = B * c2;
        const float p0 = b0 * xin;
        float y = p0 + t1.x;
        y = y + t2.x;
        y = y + t1.y;
        y = y + t2.y;
        B = af_v2{ xin, y };
        return y;
    };
    float *const xrow = tile + ch * kAfRow;
    // a step whose state update is suppressed where stage s has no sample of this tile at step k (fill / drain); PA stays (x1, y1)
    auto step_masked = [&](int k, int tn) {
        const af_v2 oa = PA, ob = PB;
        const float y = step(xrow[k], PA, PB);
        const bool valid = k - s >= 0 && k - s < tn;
        const af_v2 n1 = PB;
        PA.x = valid ? n1.x : oa.x; PA.y = valid ? n1.y : oa.y;
        PB.x = valid ? oa.x : ob.x; PB.y = valid ? oa.y : ob.y;
        if (is_out && (uint32_t)(k - dn) < (uint32_t)tn) xrow[k - dn] = y;
    };

    // the wave's piece of tile t: row r = 64 consecutive floats of channel c0 + r
    float pre[CH];
    auto load_tile = [&](uint32_t t) {
        const uint32_t i = t * kAfTile + (uint32_t)lane;
#pragma unroll
        for (int r = 0; r < CH; ++r)
            pre[r] = ((uint32_t)r < nrow && i < nout) ? audio[(size_t)(c0 + r) * q.stride + i] : 0.0f;
    };
    const uint32_t ntile = (nout + kAfTile - 1) / kAfTile;
    load_tile(0);
#pragma unroll
    for (int r = 0; r < CH; ++r) tile[r * kAfRow + lane] = pre[r];
    if (ntile > 1) load_tile(1);
    af_lds_sync();

    for (uint32_t t = 0; t < ntile; ++t) {
        const int tn = (int)min((uint32_t)kAfTile, nout - t * kAfTile);      // samples of this tile
        int k = 0;
#pragma unroll
        for (; k < D; ++k) step_masked(k, tn);                               // fill
        if (k < tn) {                                                        // every stage has a sample: tn - D plain steps, two at a time
            float xa = xrow[k], xb = xrow[k + 1];                            // (read one pair ahead of the steps: the words behind k are still input)
            for (; k + 1 < tn; k += 2) {
                const float xa_n = xrow[k + 2], xb_n = xrow[k + 3];
                const float ya = step(xa, PA, PB);
                if (is_out) xrow[k - dn] = ya;
                const float yb = step(xb, PB, PA);
                if (is_out) xrow[k + 1 - dn] = yb;
                xa = xa_n; xb = xb_n;
            }
            if (k < tn) {
                const float ya = step(xa, PA, PB);
                if (is_out) xrow[k - dn] = ya;
                const af_v2 sw = PA; PA = PB; PB = sw;
                ++k;
            }
        }
        if constexpr (D > 0) {
#pragma unroll 1
            for (; k < tn + D; ++k) step_masked(k, tn);                      // drain (and, with tn < D, the rest of the fill)
        }
        af_lds_sync();
        // the tile's output out of LDS, the next tile in, then the stores
        float out[CH];
#pragma unroll
        for (int r = 0; r < CH; ++r) out[r] = tile[r * kAfRow + lane];
        if (t + 1 < ntile) {
#pragma unroll
            for (int r = 0; r < CH; ++r) tile[r * kAfRow + lane] = pre[r];
        }
        af_lds_sync();
        const uint32_t i = t * kAfTile + (uint32_t)lane;
#pragma unroll
        for (int r = 0; r < CH; ++r)
            if ((uint32_t)r < nrow && i < nout) audio[(size_t)(c0 + r) * q.stride + i] = out[r];
        if (t + 2 < ntile) load_tile(t + 2);
    }
    if (live) *reinterpret_cast<float4 *>(st_row) = make_float4(PA.x, PB.x, PA.y, PB.y);
}

hipError_t launch_afilt(const AfiltParams &q, float *audio, hipStream_t st)
{
    if (q.channels == 0) return hipSuccess;
    if (q.nout == 0 || q.nout > q.stride || q.n_stages == 0 || q.n_stages > SELENITE_RX_AFILT_MAX_STAGES) return hipErrorInvalidValue;
#define SRX_AFILT_LAUNCH(NS) hipLaunchKernelGGL(k_afilt<NS>, dim3((q.channels + 64 / NS - 1) / (64 / NS)), dim3(kWave), 0, st, q, audio)
    if (q.n_stages == 1) SRX_AFILT_LAUNCH(1);
    else if (q.n_stages == 2) SRX_AFILT_LAUNCH(2);
    else if (q.n_stages <= 4) SRX_AFILT_LAUNCH(4);
    else SRX_AFILT_LAUNCH(8);
#undef SRX_AFILT_LAUNCH
    return hipGetLastError();
}

// ---- host side of the stage ----
void AfiltStage::release()
{
    dev_free(d_coeffs, d_state);
    on = false;
    n_stages = per_channel = 0;
}

// the stage's state as set_afilt leaves it: +0.0f
int AfiltStage::init_state(selenite_rx_instance *S)
{
    if (!on) return SELENITE_RX_SUCCESS;
    HIPCHK(S, hipMemsetAsync(d_state, 0, (size_t)S->cfg.channels * n_stages * 4 * sizeof(float), S->stream));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    return SELENITE_RX_SUCCESS;
}

// the stage's view of a launch: the channels and the audio geometry of `p`; the state and the per-channel coefficient rows move with the range
AfiltParams AfiltStage::params(ChanRange r, const RxParams &p) const
{
    const size_t c0 = r.first;
    AfiltParams q{};
    q.channels = p.channels; q.nout = p.nout; q.stride = p.out_stride;
    q.n_stages = n_stages; q.per_channel = per_channel;
    q.coeffs = per_channel ? d_coeffs + c0 * n_stages * 5 : d_coeffs;
    q.state = d_state + c0 * n_stages * 4;
    return q;
}

static bool all_finite(const float *v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_rx_set_afilt(selenite_rx_instance *S, const selenite_rx_afilt_config *f)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_afilt: S is NULL");
    // everything is validated before anything changes: a refused call leaves the instance as it was
    size_t ncoef = 0;
    if (f) {
        const char *bad = nullptr;
        if (f->struct_size != sizeof(selenite_rx_afilt_config)) bad = "struct_size is not sizeof(selenite_rx_afilt_config)";
        else if (f->n_stages < 1u || f->n_stages > SELENITE_RX_AFILT_MAX_STAGES) bad = "n_stages is not 1 .. 8";
        else if (f->per_channel > 1u) bad = "per_channel is not 0 or 1";
        else if (f->reserved != 0u) bad = "reserved is not 0";
        else if (!f->coeffs) bad = "coeffs is NULL";
        else {
            ncoef = (f->per_channel ? (size_t)S->cfg.channels : (size_t)1) * f->n_stages * 5;
            if (!all_finite(f->coeffs, ncoef)) bad = "a coefficient is not finite";
        }
        if (bad) return refuse("selenite_rx_set_afilt", bad);
    }
    if (int rc = drain(S)) return rc;                       // calls in flight still read the old stage
    AfiltStage &st = S->afilt;
    st.release();
    if (!f) return SELENITE_RX_SUCCESS;
    hipError_t e = dev_alloc(&st.d_coeffs, ncoef);
    if (e == hipSuccess) e = dev_alloc(&st.d_state, (size_t)S->cfg.channels * f->n_stages * 4);
    if (e == hipSuccess) e = hipMemcpy(st.d_coeffs, f->coeffs, ncoef * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        st.release();
        return fail(S, SELENITE_RX_DEVICE_ERROR, std::string("selenite_rx_set_afilt: ") + hipGetErrorString(e));
    }
    st.on = true;
    st.n_stages = f->n_stages; st.per_channel = f->per_channel;
    return st.init_state(S);
}

extern "C" int selenite_rx_set_afilt_coeffs(selenite_rx_instance *S, uint32_t first_channel, uint32_t n_channels, const float *coeffs)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_afilt_coeffs: S is NULL");
    AfiltStage &st = S->afilt;
    const uint32_t rows = st.per_channel ? S->cfg.channels : 1u;
    const char *bad = nullptr;
    if (!st.on) bad = "the audio filter is off";
    else if (n_channels == 0 || first_channel >= rows || n_channels > rows - first_channel)
        bad = st.per_channel ? "the channel range is not inside the instance" : "one coefficient set for all channels: the only range is (0, 1)";
    else if (!coeffs) bad = "coeffs is NULL";
    else if (!all_finite(coeffs, (size_t)n_channels * st.n_stages * 5)) bad = "a coefficient is not finite";
    if (bad) return refuse("selenite_rx_set_afilt_coeffs", bad);
    HIPCHK(S, hipSetDevice(S->device));
    // on the instance's stream: behind the calls issued so far, in front of the ones to come; drained, so the caller's array is free on return
    const size_t row = (size_t)st.n_stages * 5;
    HIPCHK(S, hipMemcpyAsync(st.d_coeffs + first_channel * row, coeffs, n_channels * row * sizeof(float), hipMemcpyHostToDevice, S->stream));
    HIPCHK(S, hipStreamSynchronize(S->stream));
    return SELENITE_RX_SUCCESS;
}

static int afilt_state_copy(selenite_rx_instance *S, const selenite_rx_afilt_state_view *v, bool to_host)
{
    if (!S || !v || !S->afilt.on) return SELENITE_RX_ARGUMENT_ERROR;
    const AfiltStage &st = S->afilt;
    const size_t C = S->cfg.channels;
    const size_t sbytes = C * st.n_stages * 4 * sizeof(float), cbytes = (st.per_channel ? C : 1) * st.n_stages * 5 * sizeof(float);
    // (the coefficients are read only: selenite_rx_set_afilt_coeffs sets them)
    return copy_rows(S, to_host, { { st.d_state, v->state, sbytes }, { st.d_coeffs, to_host ? v->coeffs : nullptr, cbytes } });
}
extern "C" int selenite_rx_get_afilt_state(selenite_rx_instance *S, const selenite_rx_afilt_state_view *v) { return afilt_state_copy(S, v, true); }
extern "C" int selenite_rx_set_afilt_state(selenite_rx_instance *S, const selenite_rx_afilt_state_view *v) { return afilt_state_copy(S, v, false); }
