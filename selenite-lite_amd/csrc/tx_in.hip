// tx_in.hip -- the audio input stage of the batched TX chain (include/selenite_tx_in.h: selenite_tx_set_in; DESIGN.md section 2 "TX input",
// section 5.18).  Slot-rate frames (f32 or int16, mono or interleaved left / right) -> pick / mix -> mic gain -> arm_fir_decimate_f32 by M
// -> VOX per DSP block -> gate -> the chain's audio (f32 or int16) in a buffer of the instance, on which run() of tx_api.hip then works.
//
// k_out's mirror image (rx_out.hip): no recurrence, a streaming kernel, one single-wave workgroup per channel row.  The row streams through
// LDS in tiles of whole DSP blocks (about 1024 input samples) behind nt - 1 samples of history -- the first tile's history is the channel's
// state, the last nt - 1 samples of history + tile are the next tile's history and, behind the last tile, the new state: a call shorter
// than the history shifts the state, it does not overwrite it.
//   load    16 bytes per lane (2 f32 stereo frames, 4 int16 stereo frames, 4 f32 or 8 int16 mono samples), coalesced, kept RAW in
//           registers: the next tile's loads are issued before the current tile's compute and are decoded (arm_q15_to_float, pick / mix,
//           gain) on the way into LDS, so LDS holds the mono g only.  Rows or source pointers that are not 16-byte aligned take element
//           loads with a bound per sample.
//   LDS     polyphase order: position i of history + tile sits at [i % M][i / M].  Lanes own consecutive outputs, output n reads position
//           n M + k at tap k: row k % M, column n + k / M -- a wave's reads at one tap are consecutive words.
//   taps    wave-uniform, read from global memory through the scalar cache (s_load_dwordx8 per eight taps of the unrolled loop); four
//           outputs per lane (n, n + 64, n + 128, n + 192) share every tap: two v_pk_mul_f32 and two v_pk_add_f32 per tap, the product
//           rounded, then the sum rounded, one accumulator per output from +0.0f, taps in pCoeffs order (arm_fir_decimate_f32.c).
//           The unit is compiled with -ffp-contract=off: nothing is fused.
//   VOX     a (in front of the gate) goes to LDS with an odd stride between DSP blocks; lane j sums block j's squares in order, one
//           accumulator, product rounded (arm_power_f32) -- k_meter's way: the sum is sequential, the parallelism is across the blocks of
//           the tile -- then every lane runs the tile's blocks through the law in order (the mean square of block j is a bpermute from
//           lane j): the update is wave-uniform.
//   store   the gate, arm_float_to_q15 for the int16 chain, 16 bytes per lane where the row length allows, else element stores with a bound.
// The decimator tail and the VOX words are written back once per channel.  Element offsets are 64-bit throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cfloat>
#include <cmath>

#include "../../include/selenite_tx.h"
#include "rx_device.h"
#include "tx_host.h"

namespace srx {

namespace {

constexpr uint32_t kInTileIn = 1024;             // input samples (of the mono g) a tile aims at, and the samples of one register chunk

typedef float in_v2f __attribute__((ext_vector_type(2)));

__host__ __device__ inline uint32_t in_hist(uint32_t nt) { return nt ? nt - 1u : 0u; }
__host__ __device__ inline uint32_t in_tile(uint32_t block, uint32_t M)
{
    const uint32_t want = kInTileIn / M;         // outputs
    return block >= want ? block : block * (want / block);
}
// LDS of k_tx_in, in words: X [M][rs] (history + tile, polyphase) | A [blocks of the tile][bs1] (a, odd stride) | bits [blocks of the tile]
struct InLds { uint32_t rs, bs1, nblk, A, bits; uint64_t total; };
__host__ __device__ inline InLds in_layout(uint32_t nt, uint32_t M, uint32_t block, uint32_t tile)
{
    InLds L;
    const uint64_t rs = (uint64_t)tile + (in_hist(nt) + M - 1u) / M;           // the sum in 64 bits: block is the caller's
    L.rs = (uint32_t)rs;
    L.bs1 = block | 1u;
    L.nblk = tile / block;
    const uint64_t x = ((uint64_t)M * rs + 3u) & ~3ull;
    const uint64_t a = ((uint64_t)L.nblk * L.bs1 + 3u) & ~3ull;
    L.A = (uint32_t)x;
    L.bits = (uint32_t)(x + a);
    L.total = x + a + L.nblk;
    return L;
}

template <typename TIn> struct InFmt;
template <> struct InFmt<float> { static constexpr uint32_t kWords = 4; };      // frame words of a 16-byte load
template <> struct InFmt<int16_t> { static constexpr uint32_t kWords = 8; };

__device__ __forceinline__ float in_word(const uint4 &r, uint32_t i)              // dword i of the raw load (i is a constant after unrolling)
{
    return __builtin_bit_cast(float, i == 0 ? r.x : i == 1 ? r.y : i == 2 ? r.z : r.w);
}
__device__ __forceinline__ uint32_t in_dword(const uint4 &r, uint32_t i) { return i == 0 ? r.x : i == 1 ? r.y : i == 2 ? r.z : r.w; }

// sample i of a lane's raw 16 bytes -> s (pick / mix); the mic gain is the caller's
template <int PICK, typename TIn>
__device__ __forceinline__ float in_decode(const uint4 &r, uint32_t i)
{
    if constexpr (sizeof(TIn) == 4) {
        if constexpr (PICK == SELENITE_TX_IN_MONO) return in_word(r, i);
        else if constexpr (PICK == SELENITE_TX_IN_LEFT) return in_word(r, 2 * i);
        else if constexpr (PICK == SELENITE_TX_IN_RIGHT) return in_word(r, 2 * i + 1);
        else { const float t = in_word(r, 2 * i) + in_word(r, 2 * i + 1); return t * 0.5f; }
    } else {
        if constexpr (PICK == SELENITE_TX_IN_MONO) {
            const uint32_t w = in_dword(r, i >> 1);
            return q15_to_float((int16_t)((i & 1u) ? (w >> 16) : (w & 0xFFFFu)));
        } else {
            const uint32_t w = in_dword(r, i);                                    // pbuf[k] = left: the low half
            const float l = q15_to_float((int16_t)(w & 0xFFFFu)), rr = q15_to_float((int16_t)(w >> 16));
            if constexpr (PICK == SELENITE_TX_IN_LEFT) return l;
            else if constexpr (PICK == SELENITE_TX_IN_RIGHT) return rr;
            else { const float t = l + rr; return t * 0.5f; }
        }
    }
}

__device__ __forceinline__ void in_store16(float *p, const float (&v)[4], uint32_t)
{
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void in_store16(int16_t *p, const float (&v)[8], uint32_t round)
{
    uint32_t w0, w1, w2, w3;
    float4_to_q15(v[0], v[1], v[2], v[3], round, w0, w1);
    float4_to_q15(v[4], v[5], v[6], v[7], round, w2, w3);
    *reinterpret_cast<uint4 *>(p) = make_uint4(w0, w1, w2, w3);
}

template <int M, int PICK, typename TIn, typename TOut>
__global__ __launch_bounds__(64) void k_tx_in(TxInParams q, const float *__restrict__ cf, const TIn *__restrict__ frames,
                                              TOut *__restrict__ audio, uint32_t wide_in, uint32_t wide_out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr uint32_t FW = PICK == SELENITE_TX_IN_MONO ? 1u : 2u;               // words of a frame
    constexpr uint32_t E = InFmt<TIn>::kWords, SPL = E / FW;                     // words and samples of a lane's 16 bytes
    constexpr uint32_t NLD = kInTileIn / (kWave * SPL);                          // 16-byte loads of a lane per chunk of 1024 samples
    constexpr uint32_t OW = 16u / sizeof(TOut);                                  // outputs of a lane's 16-byte store

    const uint32_t lane = threadIdx.x, c = blockIdx.x;
    const uint32_t nt = q.nt, h1 = in_hist(nt), block = q.block;
    const uint32_t tile = in_tile(block, M);
    const InLds Y = in_layout(nt, M, block, tile);
    float *X = lds, *A = lds + Y.A;
    uint32_t *bits = reinterpret_cast<uint32_t *>(lds + Y.bits);
    const uint32_t rs = Y.rs, bs1 = Y.bs1;
    const TIn *row = frames + (size_t)c * q.block_size * M * FW;                 // the channel's frames
    TOut *orow = audio + (size_t)c * q.block_size;
    const float gain = q.gain;

    // one chunk of a tile, raw: samples [s, s + SPL) of the tile for load l of the lane, s = ch * 1024 + (l * 64 + lane) * SPL
    auto load_chunk = [&](uint4 (&raw)[NLD], uint32_t t0, uint32_t tg, uint32_t ch) {
        const TIn *base = row + (size_t)t0 * M * FW;                             // t0: the tile's first output
#pragma unroll
        for (uint32_t l = 0; l < NLD; ++l) {
            const uint32_t s = ch * kInTileIn + (l * kWave + lane) * SPL;
            raw[l] = make_uint4(0u, 0u, 0u, 0u);
            if (wide_in) {                                                       // tg is a multiple of SPL: all of the 16 bytes or none
                if (s < tg) raw[l] = *reinterpret_cast<const uint4 *>(base + (size_t)s * FW);
            } else {
                uint32_t w[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
                for (uint32_t i = 0; i < SPL; ++i) {
                    if (s + i < tg) {                                            // the bound of every sample
                        const TIn *f = base + (size_t)(s + i) * FW;
#pragma unroll
                        for (uint32_t k = 0; k < FW; ++k) {
                            const uint32_t e = i * FW + k;                       // word of the 16 bytes
                            if constexpr (sizeof(TIn) == 4) w[e] = __builtin_bit_cast(uint32_t, f[k]);
                            else w[e >> 1] |= (uint32_t)(uint16_t)f[k] << (16u * (e & 1u));
                        }
                    }
                }
                raw[l] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    };
    // decoded, picked and scaled on the way into LDS: position h1 + s of history + tile, polyphase
    auto stage_chunk = [&](const uint4 (&raw)[NLD], uint32_t tg, uint32_t ch) {
#pragma unroll
        for (uint32_t l = 0; l < NLD; ++l) {
            const uint32_t s = ch * kInTileIn + (l * kWave + lane) * SPL;
#pragma unroll
            for (uint32_t i = 0; i < SPL; ++i) {
                if (s + i < tg) {
                    const float sv = in_decode<PICK, TIn>(raw[l], i);
                    const uint32_t pos = h1 + s + i;
                    X[(pos % M) * rs + pos / M] = sv * gain;                    // arm_scale_f32
                }
            }
        }
    };

    for (uint32_t i = lane; i < h1; i += kWave) X[(i % M) * rs + i / M] = q.dec_state[(size_t)c * h1 + i];
    float level = 0.0f;
    uint32_t open = 0u, hold = 0u, opens = 0u, open_blocks = 0u;
    if (q.vox) { level = q.level[c]; open = q.open[c]; hold = q.hold[c]; }
    const float fn = (float)block;

    uint4 raw[NLD];
    {
        const uint32_t tl0 = q.block_size < tile ? q.block_size : tile;
        load_chunk(raw, 0u, tl0 * M, 0u);
    }
    for (uint32_t t0 = 0; t0 < q.block_size; t0 += tile) {
        const uint32_t tl = q.block_size - t0 < tile ? q.block_size - t0 : tile;     // outputs of this tile: whole DSP blocks
        const uint32_t tg = tl * M, nch = (tg + kInTileIn - 1u) / kInTileIn;
        stage_chunk(raw, tg, 0u);
        for (uint32_t ch = 1; ch < nch; ++ch) {                                  // (a DSP block of more than 1024 input samples)
            load_chunk(raw, t0, tg, ch);
            stage_chunk(raw, tg, ch);
        }
        if (t0 + tile < q.block_size) {                                          // the next tile's first chunk: in flight under this tile's compute
            const uint32_t tn = q.block_size - (t0 + tile) < tile ? q.block_size - (t0 + tile) : tile;
            load_chunk(raw, t0 + tile, tn * M, 0u);
        }
        __syncthreads();                                                         // (one wave: orders the LDS traffic across lanes)

        // the decimator: outputs n, n + 64, n + 128, n + 192 of a group share the taps
        for (uint32_t o0 = 0; o0 < tl; o0 += 4 * kWave) {
            uint32_t n[4], nn[4];
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) {
                n[r] = o0 + r * kWave + lane;
                nn[r] = n[r] < tl ? n[r] : 0u;                                   // lanes past the tile read in bounds, store nothing
            }
            in_v2f a01 = { 0.0f, 0.0f }, a23 = { 0.0f, 0.0f };
            if (nt) {
#pragma unroll 8
                for (uint32_t k = 0; k < nt; ++k) {
                    const float cc = cf[k];
                    const float *xr = X + (k % M) * rs + k / M;
                    const in_v2f p01 = in_v2f{ xr[nn[0]], xr[nn[1]] } * in_v2f{ cc, cc };
                    const in_v2f p23 = in_v2f{ xr[nn[2]], xr[nn[3]] } * in_v2f{ cc, cc };
                    a01 = a01 + p01;
                    a23 = a23 + p23;
                }
            } else {                                                             // M == 1 && nd_taps == 0: a = g
                a01 = in_v2f{ X[nn[0]], X[nn[1]] };
                a23 = in_v2f{ X[nn[2]], X[nn[3]] };
            }
            const float av[4] = { a01.x, a01.y, a23.x, a23.y };
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r)
                if (n[r] < tl) A[(n[r] / block) * bs1 + n[r] % block] = av[r];
        }
        __syncthreads();

        // VOX: arm_power_f32 of every block of the tile, then the law, block by block
        const uint32_t nblk = tl / block;
        if (q.vox) {
            for (uint32_t b0 = 0; b0 < nblk; b0 += kWave) {
                const uint32_t j = b0 + lane, nb = nblk - b0 < kWave ? nblk - b0 : kWave;
                float sum = 0.0f;
                if (j < nblk) {
                    const float *ar = A + j * bs1;
#pragma unroll 8
                    for (uint32_t i = 0; i < block; ++i) {
                        const float v = ar[i];
                        const float p = v * v;
                        sum = sum + p;
                    }
                }
                const float ms = __fdiv_rn(sum, fn);
                uint32_t mine = 0u;
                for (uint32_t jj = 0; jj < nb; ++jj) {
                    const float m = __shfl(ms, (int)jj);
                    if (m <= FLT_MAX) {                                          // (false for NaN: a NaN / Inf block leaves the level)
                        const float r = m > level ? q.attack : q.decay;
                        const float d = m - level;
                        const float s = r * d;
                        level = level + s;
                    }
                    const bool want_open = level > q.open_level, want_close = level < q.close_level;
                    if (!open) {
                        if (want_open) { open = 1u; hold = q.hang; opens += 1u; }
                    } else if (want_close) {
                        if (hold == 0u) open = 0u; else hold -= 1u;
                    } else {
                        hold = q.hang;
                    }
                    open_blocks += open;
                    if (lane == jj) mine = open;
                }
                if (j < nblk) bits[j] = mine;
            }
            __syncthreads();
        }
        const bool gated = q.vox && q.gate;

        // the gate, the chain's audio type, the store
        TOut *ot = orow + t0;
        if (wide_out) {                                                          // tl is a multiple of OW here
            for (uint32_t g0 = lane * OW; g0 < tl; g0 += kWave * OW) {
                float v[OW];
#pragma unroll
                for (uint32_t i = 0; i < OW; ++i) {
                    const uint32_t o = g0 + i, b = o / block;
                    const float a = A[b * bs1 + o % block];
                    v[i] = (gated && bits[b] == 0u) ? 0.0f : a;
                }
                in_store16(ot + g0, v, q.q15_round);
            }
        } else {
            for (uint32_t o = lane; o < tl; o += kWave) {                        // the bound of every output
                const uint32_t b = o / block;
                const float a = A[b * bs1 + o % block];
                store_audio(ot, o, (gated && bits[b] == 0u) ? 0.0f : a, q.q15_round);
            }
        }

        // the last h1 positions of history + tile become the history: position p moves to p - tl M, the same row, tl columns down
        __syncthreads();
        if (h1) {
            const uint32_t hc = (h1 + M - 1u) / M, ne = M * hc;                  // columns of the history, elements to move
            for (uint32_t e0 = 0; e0 < ne; e0 += kWave) {                        // ascending 64-wide slices: a slice reads ahead of every write
                const uint32_t e = e0 + lane, r = e / hc, col = e % hc;
                const bool live = e < ne && col * M + r < h1;
                const float t = live ? X[r * rs + col + tl] : 0.0f;
                __syncthreads();
                if (live) X[r * rs + col] = t;
                __syncthreads();
            }
        }
    }
    for (uint32_t i = lane; i < h1; i += kWave) q.dec_state[(size_t)c * h1 + i] = X[(i % M) * rs + i / M];
    if (q.vox && lane == 0) {
        q.level[c] = level; q.open[c] = open; q.hold[c] = hold;
        q.opens[c] += opens; q.open_blocks[c] += open_blocks;
    }
}

template <int M, int PICK, typename TIn, typename TOut>
hipError_t launch_in(const TxInParams &q, const void *frames, void *audio, hipStream_t st)
{
    constexpr uint32_t FW = PICK == SELENITE_TX_IN_MONO ? 1u : 2u;
    const size_t lds = tx_in_lds_bytes(q);
    auto k = k_tx_in<M, PICK, TIn, TOut>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    // 16 bytes per lane: the source, every row and every tile start on a 16-byte boundary (the last tile may be shorter: it ends the row)
    const uint64_t tile = in_tile(q.block, M);
    const uint64_t row_in = (uint64_t)q.block_size * M * FW * sizeof(TIn), tile_in = tile * M * FW * sizeof(TIn);
    const uint64_t row_out = (uint64_t)q.block_size * sizeof(TOut), tile_out = tile * sizeof(TOut);
    const uint32_t wide_in = reinterpret_cast<uintptr_t>(frames) % 16 == 0 && row_in % 16 == 0 && tile_in % 16 == 0 ? 1u : 0u;
    const uint32_t wide_out = reinterpret_cast<uintptr_t>(audio) % 16 == 0 && row_out % 16 == 0 && tile_out % 16 == 0 ? 1u : 0u;
    hipLaunchKernelGGL(k, dim3(q.channels), dim3(64), lds, st, q, q.coeffs, static_cast<const TIn *>(frames), static_cast<TOut *>(audio), wide_in, wide_out);
    return hipGetLastError();
}

template <int M, typename TIn, typename TOut>
hipError_t launch_in_pick(const TxInParams &q, const void *frames, void *audio, hipStream_t st)
{
    switch (q.pick) {
    case SELENITE_TX_IN_MONO: return launch_in<M, SELENITE_TX_IN_MONO, TIn, TOut>(q, frames, audio, st);
    case SELENITE_TX_IN_LEFT: return launch_in<M, SELENITE_TX_IN_LEFT, TIn, TOut>(q, frames, audio, st);
    case SELENITE_TX_IN_RIGHT: return launch_in<M, SELENITE_TX_IN_RIGHT, TIn, TOut>(q, frames, audio, st);
    case SELENITE_TX_IN_MIX: return launch_in<M, SELENITE_TX_IN_MIX, TIn, TOut>(q, frames, audio, st);
    }
    return hipErrorInvalidValue;
}

template <typename TIn, typename TOut>
hipError_t launch_in_m(const TxInParams &q, const void *frames, void *audio, hipStream_t st)
{
    switch (q.M) {
    case 1: return launch_in_pick<1, TIn, TOut>(q, frames, audio, st);
    case 2: return launch_in_pick<2, TIn, TOut>(q, frames, audio, st);
    case 4: return launch_in_pick<4, TIn, TOut>(q, frames, audio, st);
    case 8: return launch_in_pick<8, TIn, TOut>(q, frames, audio, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace

uint32_t tx_in_tile(const TxInParams &q) { return in_tile(q.block, q.M); }

size_t tx_in_lds_bytes(const TxInParams &q)
{
    const uint64_t words = in_layout(q.nt, q.M, q.block, in_tile(q.block, q.M)).total;
    return words > (1ull << 40) ? (size_t)1 << 42 : (size_t)(sizeof(float) * words);
}

// the three type pairs of the entries: f32 -> f32, int16 -> int16, int16 -> f32
hipError_t launch_tx_in(const TxInParams &q, const void *frames, bool in_q15, void *audio, bool out_q15, hipStream_t st)
{
    if (q.channels == 0 || q.block == 0 || q.block_size == 0 || q.block_size % q.block != 0) return hipErrorInvalidValue;
    if (tx_in_lds_bytes(q) > 64 * 1024) return hipErrorInvalidValue;
    if (!in_q15 && !out_q15) return launch_in_m<float, float>(q, frames, audio, st);
    if (in_q15 && out_q15) return launch_in_m<int16_t, int16_t>(q, frames, audio, st);
    if (in_q15) return launch_in_m<int16_t, float>(q, frames, audio, st);
    return hipErrorInvalidValue;
}

// ---- the host side (tx_host.h): selenite_tx_set_in, the stage's state accessors, the frame entries ----

void tx_in_free(selenite_tx_instance *S)
{
    selenite_tx_instance::In &I = S->in;
    dev_free(I.d_coeffs, I.d_dec, I.d_level, I.d_open, I.d_hold, I.d_opens, I.d_open_blocks, I.d_audio);
}

// the stage's state as the first selenite_tx_set_in leaves it: the decimator tail +0.0f and, with `vox`, level_init, closed, counters 0
static int in_clear_state(selenite_tx_instance *S, bool vox)
{
    const selenite_tx_instance::In &I = S->in;
    const size_t C = S->cfg.channels, h1 = I.p.nt ? I.p.nt - 1 : 0;
    if (h1) HIPCHK(S, hipMemsetAsync(I.d_dec, 0, C * h1 * sizeof(float), S->stream));
    if (!vox) return drain(S);
    for (uint32_t *row : { I.d_open, I.d_hold }) HIPCHK(S, hipMemsetAsync(row, 0, C * sizeof(uint32_t), S->stream));
    for (uint64_t *row : { I.d_opens, I.d_open_blocks }) HIPCHK(S, hipMemsetAsync(row, 0, C * sizeof(uint64_t), S->stream));
    return fill_rows(S, I.d_level, C, &I.level_init);      // (drains the stream)
}

int tx_in_reset(selenite_tx_instance *S) { return S->in.set ? in_clear_state(S, true) : 0; }

static TxInParams in_params(const selenite_tx_instance *S, uint32_t bs)
{
    TxInParams q = S->in.p;
    q.channels = S->cfg.channels; q.block = S->cfg.block; q.block_size = bs; q.q15_round = S->cfg.q15_rounding ? 1u : 0u;
    return q;
}

// frame calls: every refusal comes before anything is written, what run() would refuse behind the stage included
static int frames_call_ok(selenite_tx_instance *S, const void *frames, const void *dst, uint32_t bs, const char *who)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    if (!S->in.set) return fail(S, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": the input stage is not configured (selenite_tx_set_in)");
    if (!frames || !dst) return fail(S, SELENITE_RX_ARGUMENT_ERROR, std::string(who) + ": NULL buffer");
    if (!block_size_ok(S, bs, who)) return SELENITE_RX_LENGTH_ERROR;
    if (tx_in_lds_bytes(in_params(S, bs)) > kTxLdsLimit || decide(S, make_params(S, bs), false).refused)
        return fail(S, SELENITE_RX_LENGTH_ERROR, std::string(who) + ": the layout exceeds the LDS budget of a TX kernel");
    return 0;
}

static int run_in_stage(selenite_tx_instance *S, const void *frames, bool in_q15, bool out_q15, uint32_t bs)
{
    HIPCHK(S, hipSetDevice(S->device));
    if (ensure(S, &S->in.d_audio, &S->in.audio_bytes, (size_t)S->cfg.channels * bs * sample_bytes(out_q15))) return S->status;
    HIPCHK(S, launch_tx_in(in_params(S, bs), frames, in_q15, S->in.d_audio, out_q15, S->stream));
    return 0;
}

static int run_frames(selenite_tx_instance *S, const void *frames, bool in_q15, void *dst, bool out_q15, uint32_t bs)
{
    if (int r = run_in_stage(S, frames, in_q15, out_q15, bs)) return r;
    return run(S, S->in.d_audio, dst, out_q15, bs);              // the existing chain on the stage's audio, unchanged
}

static int process_frames_device(selenite_tx_instance *S, const void *frames, bool in_q15, void *dst, bool out_q15, uint32_t bs, const char *who)
{
    if (int r = frames_call_ok(S, frames, dst, bs, who)) return r;
    return run_frames(S, frames, in_q15, dst, out_q15, bs);
}

static int process_frames_host(selenite_tx_instance *S, const void *frames, void *dst, uint32_t bs, bool q15, const char *who)
{
    if (int r = frames_call_ok(S, frames, dst, bs, who)) return r;
    const size_t fw = S->in.p.pick == SELENITE_TX_IN_MONO ? 1 : 2, na = (size_t)S->cfg.channels * bs * sample_bytes(q15);
    return staged_call(S, { { frames, na * S->in.p.M * fw, kToDevice, &S->d_io_in, &S->io_in_bytes },
                            { dst, na * S->cfg.interp * 2, kToHost, &S->d_io_out, &S->io_out_bytes } },
                       [&] { return run_frames(S, S->d_io_in, q15, S->d_io_out, q15, bs); });
}

static int in_state_copy(selenite_tx_instance *S, const selenite_tx_in_state_view *v, bool to_host)
{
    if (!S || !v || !S->in.set) return SELENITE_RX_ARGUMENT_ERROR;
    const selenite_tx_instance::In &I = S->in;
    const size_t C = S->cfg.channels, h1 = I.p.nt ? I.p.nt - 1 : 0;
    return copy_rows(S, to_host, { { I.d_dec, v->dec_state, C * h1 * sizeof(float) }, { I.d_level, v->level, C * sizeof(float) },
                                   { I.d_open, v->open, C * sizeof(uint32_t) }, { I.d_hold, v->hold, C * sizeof(uint32_t) },
                                   { I.d_opens, v->opens, C * sizeof(uint64_t) }, { I.d_open_blocks, v->open_blocks, C * sizeof(uint64_t) } });
}

}  // namespace srx

using namespace srx;

extern "C" int selenite_tx_set_in(selenite_tx_instance *S, const selenite_tx_in_config *f)
{
    if (!S) return SELENITE_RX_ARGUMENT_ERROR;
    static_assert(sizeof(selenite_tx_in_config) == 72 && offsetof(selenite_tx_in_config, coeffs) == 16 && offsetof(selenite_tx_in_config, meter) == 32 &&
                  sizeof(selenite_tx_in_state_view) == 48, "selenite_tx_in_config layout (LP64)");
    selenite_tx_instance::In &I = S->in;
    if (!f) {                                               // the stage off again, in any mode: the audio and key entries never needed it
        I.set = false;
        return SELENITE_RX_SUCCESS;
    }
    if (f->struct_size != sizeof(selenite_tx_in_config) || f->reserved != 0 || !(f->M == 1 || f->M == 2 || f->M == 4 || f->M == 8) ||
        f->nd_taps > 256 || (f->nd_taps == 0 && f->M != 1) || (f->nd_taps && !f->coeffs) || f->pick > SELENITE_TX_IN_MIX ||
        !std::isfinite(f->gain) || f->vox > 1u)
        return SELENITE_RX_ARGUMENT_ERROR;                  // the previous setting stays
    for (uint32_t k = 0; k < f->nd_taps; ++k)
        if (!std::isfinite(f->coeffs[k])) return SELENITE_RX_ARGUMENT_ERROR;
    const selenite_rx_meter_config &m = f->meter;
    if (f->vox) {                                           // selenite_rx_set_meter's own rules, sense ABOVE
        if (m.struct_size != sizeof(selenite_rx_meter_config) || m.sense != SELENITE_RX_SQ_ABOVE || m.gate > 1u || m.hang > 65535u ||
            !(m.attack > 0.0f && m.attack <= 1.0f) || !(m.decay > 0.0f && m.decay <= 1.0f) ||
            !(std::isfinite(m.open_level) && m.open_level >= 0.0f) || !(std::isfinite(m.close_level) && m.close_level >= 0.0f) ||
            !(m.close_level <= m.open_level) || !(std::isfinite(m.level_init) && m.level_init >= 0.0f))
            return SELENITE_RX_ARGUMENT_ERROR;
    }
    const size_t C = S->cfg.channels, h1 = f->nd_taps ? f->nd_taps - 1 : 0;
    const bool first = !I.set, new_len = first || f->nd_taps != I.p.nt;
    if (int rc = drain(S)) return rc;
    if (!I.d_level) HIPCHK(S, dev_alloc(&I.d_level, C));
    for (uint32_t **row : { &I.d_open, &I.d_hold })
        if (!*row) HIPCHK(S, dev_alloc(row, C));
    for (uint64_t **row : { &I.d_opens, &I.d_open_blocks })
        if (!*row) HIPCHK(S, dev_alloc(row, C));
    if (new_len) {                                          // what depends on nd_taps is allocated before anything of the previous setting is given up
        float *coeffs = nullptr, *dec = nullptr;
        HIPCHK(S, dev_alloc(&coeffs, (size_t)f->nd_taps));
        if (dev_alloc(&dec, C * h1) != hipSuccess) {
            (void)hipFree(coeffs);
            return fail(S, SELENITE_RX_DEVICE_ERROR, "hipMalloc(dec_state)");
        }
        dev_free(I.d_coeffs, I.d_dec);
        I.d_coeffs = coeffs; I.d_dec = dec;
    }
    if (f->nd_taps) HIPCHK(S, hipMemcpy(I.d_coeffs, f->coeffs, f->nd_taps * sizeof(float), hipMemcpyHostToDevice));
    TxInParams q{};
    q.M = f->M; q.nt = f->nd_taps; q.pick = f->pick; q.gain = f->gain; q.vox = f->vox;
    if (f->vox) {
        q.gate = m.gate; q.hang = m.hang; q.attack = m.attack; q.decay = m.decay; q.open_level = m.open_level; q.close_level = m.close_level;
        I.level_init = m.level_init;
    }
    q.coeffs = I.d_coeffs; q.dec_state = I.d_dec; q.level = I.d_level; q.open = I.d_open; q.hold = I.d_hold;
    q.opens = I.d_opens; q.open_blocks = I.d_open_blocks;
    I.p = q;
    if (new_len) {                                          // a retune keeps the decimator tail (same nd_taps) and the VOX state
        if (first && !f->vox) I.level_init = 0.0f;
        if (in_clear_state(S, first)) return S->status;
    }
    I.set = true;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_tx_get_in_state(selenite_tx_instance *S, const selenite_tx_in_state_view *v) { return in_state_copy(S, v, true); }
extern "C" int selenite_tx_set_in_state(selenite_tx_instance *S, const selenite_tx_in_state_view *v) { return in_state_copy(S, v, false); }

extern "C" int selenite_tx_process_frames_f32_device(selenite_tx_instance *S, const float *frames, float *dst, uint32_t bs) { return process_frames_device(S, frames, false, dst, false, bs, "selenite_tx_process_frames_f32_device"); }
extern "C" int selenite_tx_process_frames_q15_device(selenite_tx_instance *S, const int16_t *frames, int16_t *dst, uint32_t bs) { return process_frames_device(S, frames, true, dst, true, bs, "selenite_tx_process_frames_q15_device"); }
extern "C" int selenite_tx_process_frames_q15_f32_device(selenite_tx_instance *S, const int16_t *frames, float *dst, uint32_t bs) { return process_frames_device(S, frames, true, dst, false, bs, "selenite_tx_process_frames_q15_f32_device"); }
extern "C" int selenite_tx_process_frames_f32(selenite_tx_instance *S, const float *frames, float *dst, uint32_t bs) { return process_frames_host(S, frames, dst, bs, false, "selenite_tx_process_frames_f32"); }
extern "C" int selenite_tx_process_frames_q15(selenite_tx_instance *S, const int16_t *frames, int16_t *dst, uint32_t bs) { return process_frames_host(S, frames, dst, bs, true, "selenite_tx_process_frames_q15"); }

extern "C" const uint32_t *selenite_tx_in_vox_device(selenite_tx_instance *S) { return (S && S->in.set) ? S->in.d_open : nullptr; }
extern "C" const void *selenite_tx_in_audio_device(selenite_tx_instance *S) { return (S && S->in.set) ? S->in.d_audio : nullptr; }

extern "C" int selenite_tx_time_in_stage_device(selenite_tx_instance *S, const void *frames, uint32_t kind, uint32_t bs, uint32_t iters,
                                                float *ms_per_launch)
{
    if (!S || !ms_per_launch || iters == 0 || kind > SELENITE_TX_IN_Q15_F32) return SELENITE_RX_ARGUMENT_ERROR;
    if (int r = frames_call_ok(S, frames, ms_per_launch, bs, "selenite_tx_time_in_stage_device")) return r;
    const bool in_q15 = kind != SELENITE_TX_IN_F32, out_q15 = kind == SELENITE_TX_IN_Q15;
    // (the untimed first launch grows the audio buffer outside the timed span)
    return timed_loop(S, iters, ms_per_launch, [&] { return run_in_stage(S, frames, in_q15, out_q15, bs); }, true);
}
