// tx_in.hip -- the audio input stage of the batched TX chain (include/selenite_tx_in.h: selenite_tx_set_in; DESIGN.md section 2 "TX input",
// section 5.18).  Slot-rate frames (f32 or int16, mono or interleaved left / right) -> pick / mix -> mic gain -> arm_fir_decimate_f32 by M
// -> VOX per DSP block -> gate -> the chain's audio (f32 or int16) in a buffer of the instance, on which run() of tx.hip then works.
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

#include "../../include/selenite_tx.h"
#include "rx_device.h"
#include "tx_internal.h"

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

}  // namespace srx
