// rx_nlms.hip -- NLMS noise reduction / automatic notch (step 4b of DESIGN.md section 2): arm_lms_norm_f32 of CMSIS-DSP 1.5.3
// (FilteringFunctions/arm_lms_norm_f32.c:196-348, the ARM_MATH_DSP branch) per channel, on u[n] = x[n - D] against the reference x[n],
// in place on the un-scaled f32 audio between the demodulator and the AGC.
//
// The recurrence is sequential in time (sample n + 1 needs the weights sample n left), so the only parallelism is across channels:
// ONE LANE PER CHANNEL, weights and window in VGPRs (num_taps is a template parameter: 2N registers), 64 channels per workgroup.
// Every operation is the reference's, in its order -- products then sums in tap order from 0.0f, energy -= x0*x0 then += in*in,
// w = (e*mu) / (energy + eps) correctly rounded, pb[k] += w*px[k] -- and the unit is compiled with -ffp-contract=off: bit-exact
// against the reference in every arith mode (no cross-lane reduction, which would change the summation order).
//
// Data movement: the audio of the workgroup's 64 channels streams through an LDS ring of 128 samples per channel in tiles of 32 samples.
// While tile t computes, the ring holds the 64 samples before it (u[n] = x[n - D], D <= 64, is read from there: the delay line costs no
// copy inside a call), tile t itself, and the slots tile t + 1 arrives in.  Tile t + 1 is fetched in four batches of eight wave loads
// (each 32 consecutive samples of two channels), one batch per eight samples of tile t: only eight registers of it are live across the
// recurrence, and eight samples of compute stand between a batch's loads and its ring writes.  Once u[n] is read its slot is dead and takes
// the stage output of sample n; the outputs of tile t - 1 leave during tile t, batch by batch, the way the input came.  The eight samples
// of a batch are unrolled, so the window's shift is a renaming of registers, not N - 1 moves per sample.
#include "rx_host.h"

#include <cmath>
#include <cstring>

namespace srx {

constexpr uint32_t kNrTile = 32;     // audio samples per tile
constexpr uint32_t kNrBatch = 8;     // samples computed per batch of the next tile's loads (kNrTile / kNrBatch batches per tile)
constexpr uint32_t kNrRing = 128;    // ring of one channel: 64 samples of history, this tile, the next tile
constexpr uint32_t kNrRow = kNrRing + 1;   // odd row stride: lane l reading slot i of its own row hits bank (l + i) mod 64
constexpr uint32_t kNrHist = 64;     // sample m of a call lives in slot (m + kNrHist) & (kNrRing - 1) of its channel's row

__device__ __forceinline__ uint32_t nr_slot(uint32_t m) { return (m + kNrHist) & (kNrRing - 1); }

// one step of arm_lms_norm_f32 (:199-302) for one channel: in = u[n], x = x[n]; returns the stage output (e for the notch, else y)
template <int N>
__device__ __forceinline__ float nlms_step(float (&w)[N], float (&win)[N - 1], float &energy, float &x0, float in, float x, float mu, uint32_t notch)
{
    // :211-214
    const float ex = x0 * x0;
    energy = energy - ex;
    const float ei = in * in;
    energy = energy + ei;
    // :216-245 -- px[k] = window (oldest first), then the new sample; sum from 0.0f in tap order
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {
        const float p = win[k] * w[k];
        sum = sum + p;
    }
    {
        const float p = in * w[N - 1];
        sum = sum + p;
    }
    // :248-258
    const float e = x - sum;
    const float num = e * mu;
    const float den = energy + 0.000000119209289f;
    const float wf = __fdiv_rn(num, den);
    // :264-297 -- pb[k] += w * px[k]
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {
        const float p = wf * win[k];
        w[k] = w[k] + p;
    }
    {
        const float p = wf * in;
        w[N - 1] = w[N - 1] + p;
    }
    // :299-302 -- x0 = the oldest sample of this window; the window moves on by one
    x0 = win[0];
#pragma unroll
    for (int k = 0; k < N - 2; ++k) win[k] = win[k + 1];
    win[N - 2] = in;
    return notch ? e : sum;
}

template <int N>
__global__ __launch_bounds__(64) void k_nlms(NrParams q, float *__restrict__ audio)
{
    __shared__ float ring[kWave * kNrRow];
    const uint32_t lane = threadIdx.x;
    const uint32_t c0 = blockIdx.x * (uint32_t)kWave;
    const uint32_t c = c0 + lane;
    const bool live = c < q.channels;
    const uint32_t nrows = q.channels - c0 < (uint32_t)kWave ? q.channels - c0 : (uint32_t)kWave;
    const uint32_t D = q.delay;
    float *row = ring + lane * kNrRow;
    // the batch layout of the coalesced loads and stores: lane -> (sample s of the tile, row 2 k + half of the batch)
    const uint32_t s = lane & (kNrTile - 1), half = lane / kNrTile;

    float w[N], win[N - 1];
    float energy = 0.0f, x0 = 0.0f;
    if (live) {
#pragma unroll
        for (int k = 0; k < N; ++k) w[k] = q.coeffs[(size_t)c * N + k];
#pragma unroll
        for (int k = 0; k < N - 1; ++k) win[k] = q.window[(size_t)c * (N - 1) + k];
        energy = q.energy[c];
        x0 = q.x0[c];
        for (uint32_t j = 0; j < D; ++j) row[kNrHist - D + j] = q.delay_line[(size_t)c * D + j];
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) w[k] = 0.0f;
#pragma unroll
        for (int k = 0; k < N - 1; ++k) win[k] = 0.0f;
    }

    // batch b of a tile starting at n0: rows 16 b + 2 k + half, k < 8, sample n0 + s.  Addresses: the workgroup's first row (uniform) plus a
    // 32-bit element offset (launch_nlms checks 64 rows of the call fit) -- 64-bit row addresses of every batch, hoisted out of the tile
    // loop, cost the registers the weights need
    float *const wg_audio = audio + (size_t)c0 * q.stride;
    auto load_batch = [&](uint32_t n0, uint32_t b, float (&v)[kNrBatch]) {
        const uint32_t n = n0 + s;
#pragma unroll
        for (uint32_t k = 0; k < kNrBatch; ++k) {
            const uint32_t r = 16u * b + 2u * k + half;
            v[k] = (n < q.nout && r < nrows) ? wg_audio[r * q.stride + n] : 0.0f;
        }
    };
    auto put_batch = [&](uint32_t n0, uint32_t b, const float (&v)[kNrBatch]) {
#pragma unroll
        for (uint32_t k = 0; k < kNrBatch; ++k) ring[(16u * b + 2u * k + half) * kNrRow + nr_slot(n0 + s)] = v[k];
    };
    // the outputs of the tile at n0, rows of batch b: sample n's output sits in u[n]'s slot
    auto store_batch = [&](uint32_t n0, uint32_t b) {
        const uint32_t n = n0 + s;
#pragma unroll
        for (uint32_t k = 0; k < kNrBatch; ++k) {
            const uint32_t r = 16u * b + 2u * k + half;
            if (n < q.nout && r < nrows) wg_audio[r * q.stride + n] = ring[r * kNrRow + nr_slot(n - D)];
        }
    };

    const uint32_t ntile = (q.nout + kNrTile - 1) / kNrTile;
    bool nonfinite = false;
    for (uint32_t b = 0; b < kNrTile / kNrBatch; ++b) {      // tile 0, straight into the ring
        float v[kNrBatch];
        load_batch(0, b, v);
        put_batch(0, b, v);
    }
    for (uint32_t t = 0; t < ntile; ++t) {
        const uint32_t n0 = t * kNrTile;
        const bool next = t + 1 < ntile;
        for (uint32_t b = 0; b < kNrTile / kNrBatch; ++b) {
            float v[kNrBatch];
            if (next) load_batch(n0 + kNrTile, b, v);       // requested eight samples of compute ahead of its use
            __syncthreads();                                  // (one wave: orders the ring's LDS traffic across lanes for the compiler)
            if (t > 0) store_batch(n0 - kNrTile, b);          // before put_batch below reuses these rows' slots (D = 64)
            __syncthreads();
            const uint32_t i0 = n0 + b * kNrBatch;
            if (i0 + kNrBatch <= q.nout) {
                // unrolled: the window's shift is a renaming of registers; N = 64 by two samples only (by eight the scheduler's
                // interleaving of the steps needs more than the 512 registers of a lane and spills into the accumulation registers)
                constexpr uint32_t U = N >= 64 ? 2u : kNrBatch;
#pragma unroll 1
                for (uint32_t i1 = 0; i1 < kNrBatch; i1 += U) {
#pragma unroll
                    for (uint32_t i = 0; i < U; ++i) {
                        const uint32_t n = i0 + i1 + i, su = nr_slot(n - D);
                        const float out = nlms_step<N>(w, win, energy, x0, row[su], row[nr_slot(n)], q.mu, q.notch);
                        nonfinite = nonfinite || (live && !__builtin_isfinite(out));
                        row[su] = out;                        // u[n]'s slot is dead from here on
                    }
                }
            } else {
                for (uint32_t n = i0; n < q.nout; ++n) {      // the call's last, partial batch
                    const uint32_t su = nr_slot(n - D);
                    const float out = nlms_step<N>(w, win, energy, x0, row[su], row[nr_slot(n)], q.mu, q.notch);
                    nonfinite = nonfinite || (live && !__builtin_isfinite(out));
                    row[su] = out;
                }
            }
            __syncthreads();
            if (next) put_batch(n0 + kNrTile, b, v);
        }
    }
    __syncthreads();
    for (uint32_t b = 0; b < kNrTile / kNrBatch; ++b) store_batch((ntile - 1) * kNrTile, b);

    if (live) {
#pragma unroll
        for (int k = 0; k < N; ++k) q.coeffs[(size_t)c * N + k] = w[k];
#pragma unroll
        for (int k = 0; k < N - 1; ++k) q.window[(size_t)c * (N - 1) + k] = win[k];
        q.energy[c] = energy;
        q.x0[c] = x0;
        // the last D samples of x (oldest first): none of their slots took an output (those are the samples up to nout - 1 - D)
        for (uint32_t j = 0; j < D; ++j) q.delay_line[(size_t)c * D + j] = row[nr_slot(q.nout - D + j)];
    }
    if (nonfinite) q.flags[kFlagNanInf] = 1u;        // ARM_MATH_NANINF, read by selenite_rx_sync / the host-pointer calls
}

hipError_t launch_nlms(const NrParams &q, uint32_t num_taps, float *audio, hipStream_t st)
{
    if (q.channels == 0 || q.nout == 0) return hipSuccess;
    if (q.delay < 1 || q.delay > kNrHist) return hipErrorInvalidValue;
    if ((uint64_t)kWave * q.stride >= (1ull << 32)) return hipErrorInvalidValue;     // (32-bit offsets inside a workgroup's 64 rows)
    const dim3 grid((q.channels + kWave - 1) / kWave), blk(kWave);
    switch (num_taps) {
    case 8: hipLaunchKernelGGL(k_nlms<8>, grid, blk, 0, st, q, audio); break;
    case 16: hipLaunchKernelGGL(k_nlms<16>, grid, blk, 0, st, q, audio); break;
    case 32: hipLaunchKernelGGL(k_nlms<32>, grid, blk, 0, st, q, audio); break;
    case 64: hipLaunchKernelGGL(k_nlms<64>, grid, blk, 0, st, q, audio); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- host side of the stage ----
void NrStage::release()
{
    dev_free(d_coeffs, d_window, d_delay, d_energy, d_x0);
    kind = SELENITE_RX_NR_OFF;
    taps = delay = 0;
    mu = 0.0f;
    h_init.clear();
}

// the NLMS stage's state as arm_lms_norm_init_f32 leaves it (arm_lms_norm_init_f32.c:69-86): weights = the initial ones, the rest 0
int NrStage::init_state(selenite_rx_instance *S)
{
    if (kind == SELENITE_RX_NR_OFF) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels, N = taps, D = delay;
    HIPCHK(S, hipMemsetAsync(d_window, 0, C * (N - 1) * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(d_delay, 0, C * D * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(d_energy, 0, C * sizeof(float), S->stream));
    HIPCHK(S, hipMemsetAsync(d_x0, 0, C * sizeof(float), S->stream));
    return fill_rows(S, d_coeffs, C, h_init.data(), N);     // (drains the stream)
}

NrParams NrStage::params(ChanRange r, const RxParams &p) const
{
    const size_t c0 = r.first;
    NrParams q{};
    q.channels = p.channels; q.nout = p.nout; q.stride = p.out_stride;
    q.delay = delay; q.notch = kind == SELENITE_RX_NR_NOTCH ? 1u : 0u; q.mu = mu;
    q.coeffs = d_coeffs + c0 * taps; q.window = d_window + c0 * (taps - 1); q.delay_line = d_delay + c0 * delay;
    q.energy = d_energy + c0; q.x0 = d_x0 + c0;
    q.flags = p.flags;
    return q;
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_rx_set_nr(selenite_rx_instance *S, const selenite_rx_nr_config *nr)
{
    if (!S) return fail(nullptr, SELENITE_RX_ARGUMENT_ERROR, "selenite_rx_set_nr: S is NULL");
    // everything is validated before anything changes: a refused call leaves the instance as it was
    if (nr && nr->struct_size != sizeof(selenite_rx_nr_config)) return refuse("selenite_rx_set_nr", "struct_size is not sizeof(selenite_rx_nr_config)");
    if (nr && nr->kind != SELENITE_RX_NR_OFF) {
        const uint32_t N = nr->num_taps;
        const char *bad = nullptr;
        if (nr->kind != SELENITE_RX_NR_DENOISE && nr->kind != SELENITE_RX_NR_NOTCH) bad = "kind is not a SELENITE_RX_NR_* value";
        else if (N != 8 && N != 16 && N != 32 && N != 64) bad = "num_taps is not 8, 16, 32 or 64";
        else if (nr->delay < 1 || nr->delay > 64) bad = "delay is not 1 .. 64";
        else if (!(nr->mu > 0.0f && nr->mu < 2.0f)) bad = "mu is not finite in (0, 2)";
        else if (nr->coeffs_init)
            for (uint32_t k = 0; k < N && !bad; ++k)
                if (!std::isfinite(nr->coeffs_init[k])) bad = "coeffs_init holds a non-finite weight";
        if (bad) return refuse("selenite_rx_set_nr", bad);
    }
    if (int rc = drain(S)) return rc;                       // calls in flight still read the old stage
    NrStage &st = S->nr;
    st.release();
    if (!nr || nr->kind == SELENITE_RX_NR_OFF) return SELENITE_RX_SUCCESS;
    const size_t C = S->cfg.channels, N = nr->num_taps, D = nr->delay;
    st.h_init.assign(N, 0.0f);
    if (nr->coeffs_init) std::memcpy(st.h_init.data(), nr->coeffs_init, N * sizeof(float));
    hipError_t e = dev_alloc(&st.d_coeffs, C * N);
    if (e == hipSuccess) e = dev_alloc(&st.d_window, C * (N - 1));
    if (e == hipSuccess) e = dev_alloc(&st.d_delay, C * D);
    if (e == hipSuccess) e = dev_alloc(&st.d_energy, C);
    if (e == hipSuccess) e = dev_alloc(&st.d_x0, C);
    if (e != hipSuccess) {
        st.release();
        return fail(S, SELENITE_RX_DEVICE_ERROR, std::string("selenite_rx_set_nr: hipMalloc: ") + hipGetErrorString(e));
    }
    st.kind = nr->kind; st.taps = (uint32_t)N; st.delay = (uint32_t)D; st.mu = nr->mu;
    return st.init_state(S);
}

// the five arrays of selenite_rx_nr_state_view copied out of the device (to_host) or into it
static int nr_state_copy(selenite_rx_instance *S, const selenite_rx_nr_state_view *v, bool to_host)
{
    if (!S || !v || S->nr.kind == SELENITE_RX_NR_OFF) return SELENITE_RX_ARGUMENT_ERROR;
    const NrStage &st = S->nr;
    const size_t b = S->cfg.channels * sizeof(float);       // bytes of one float per channel
    return copy_rows(S, to_host, { { st.d_coeffs, v->coeffs, b * st.taps }, { st.d_window, v->window, b * (st.taps - 1) }, { st.d_delay, v->delay, b * st.delay },
                                   { st.d_energy, v->energy, b }, { st.d_x0, v->x0, b } });
}
extern "C" int selenite_rx_get_nr_state(selenite_rx_instance *S, const selenite_rx_nr_state_view *v) { return nr_state_copy(S, v, true); }
extern "C" int selenite_rx_set_nr_state(selenite_rx_instance *S, const selenite_rx_nr_state_view *v) { return nr_state_copy(S, v, false); }
