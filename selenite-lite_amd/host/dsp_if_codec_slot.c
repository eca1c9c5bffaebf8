/*
 * dsp_if_codec_slot.c -- the firmware's per-block callback slot as the codec sees it: `frames` int16 I/Q frames in, `frames` int16
 * left / right frames out, through the C-ABI only (include/selenite_rx.h).
 *
 * HAL_I2SEx_TxRx{Half,}CpltCallback (Core/Src/dsp_if.c:50-67) takes I2S_BUFF_HALF_SIZE words from the codec (DSP_In_Buff_Write,
 * dsp_if.c:250-301) and hands the same number of words back (DSP_Out_Buff_Read, dsp_if.c:204-219: pbuf[k] = i, pbuf[k + 1] = q).
 * dsp_if_slot.c stops at the decimated mono audio; here the audio output stage (selenite_rx_set_out) brings it back to the slot rate
 * (arm_fir_interpolate_f32 by DSP_DECIM) and writes each sample as a left / right pair, so the slot is symmetric as the firmware's is.
 *
 * Build (GPU box):  gcc -O2 -I../../include dsp_if_codec_slot.c -L.. -lselenite_rx -Wl,-rpath,'$ORIGIN/..' -lm -o dsp_if_codec_slot
 * This file is an integration example and a smoke test of the pure-C linkage; it contains no DSP.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "selenite_rx.h"

#define DSP_CHANNELS   64u      /* independent receivers handled per callback */
#define DSP_BLOCK      96u      /* one I2S half-buffer: 96 I/Q frames per millisecond at 96 kHz (Core/Inc/dsp_if.h:69-73) */
#define DSP_DECIM      4u
#define DSP_ND_TAPS    256u
#define DSP_NH_TAPS    63u
#define DSP_NI_TAPS    32u      /* interpolator: phase length 8 */

static selenite_rx_instance *rx;

/* mirrors void DSP_Init(void) (dsp_if.c:377-383) */
int DSP_Init(void)
{
    static float dec[DSP_ND_TAPS], hilb[DSP_NH_TAPS], dly[DSP_NH_TAPS], itp[DSP_NI_TAPS];
    selenite_rx_config cfg;
    selenite_rx_out_config out;
    int rc;
    memset(&cfg, 0, sizeof cfg);
    memset(&out, 0, sizeof out);
    if (selenite_rx_design_lowpass(dec, DSP_ND_TAPS, 0.4 / DSP_DECIM)) return -1;
    if (selenite_rx_design_hilbert(hilb, dly, DSP_NH_TAPS)) return -1;
    if (selenite_rx_design_interp(itp, DSP_NI_TAPS, DSP_DECIM, 0.4 / DSP_DECIM)) return -1;
    cfg.struct_size = sizeof cfg;
    cfg.abi_version = SELENITE_RX_ABI_VERSION;
    cfg.channels = DSP_CHANNELS; cfg.block = DSP_BLOCK; cfg.decim = DSP_DECIM;
    cfg.nd_taps = DSP_ND_TAPS; cfg.nh_taps = DSP_NH_TAPS;
    cfg.arith = SELENITE_ARITH_CMSIS;
    cfg.mode = SELENITE_MODE_LSB;            /* RXTX_Init() boots in LSB (rxtx_if.c:686-699) */
    cfg.nco_enable = 1; cfg.nco_step_all = 0x01000000u;
    cfg.agc_enable = 1;
    cfg.dec_coeffs = dec; cfg.hilb_coeffs = hilb; cfg.delay_coeffs = dly;
    cfg.agc_target = 0.5f; cfg.agc_attack = 0.5f; cfg.agc_decay = 0.05f;
    cfg.agc_gain_min = 1e-3f; cfg.agc_gain_max = 1e4f; cfg.agc_env_floor = 1e-6f; cfg.agc_gain_init = 1.0f;
    rc = selenite_rx_init(&rx, &cfg);
    if (rc != SELENITE_RX_SUCCESS) return rc;
    out.struct_size = sizeof out;
    out.interp = DSP_DECIM; out.ni_taps = DSP_NI_TAPS; out.frames = SELENITE_RX_OUT_STEREO; out.coeffs = itp;
    return selenite_rx_set_out(rx, &out);
}

/* mirrors void DSP_Set_Mode(uint8_t mode) (dsp_if.c:367-370) */
void DSP_Set_Mode(uint8_t mode) { (void)selenite_rx_set_mode(rx, mode); }

/* the slot, symmetric as the firmware's:
 * pbuf_in : int16 [DSP_CHANNELS][frames][2]   I, Q interleaved (dsp_if.c:286-289)
 * pbuf_out: int16 [DSP_CHANNELS][frames][2]   left, right      (dsp_if.c:213-214) */
void DSP_Process_Block(const int16_t *pbuf_in, int16_t *pbuf_out, uint16_t frames)
{
    selenite_rx_process_q15(rx, pbuf_in, pbuf_out, frames);
}

int main(void)
{
    const uint32_t frames = DSP_BLOCK;                       /* one slot per call, as the firmware's callback gets it */
    int rc = DSP_Init();
    if (rc != SELENITE_RX_SUCCESS) {
        fprintf(stderr, "DSP_Init failed: %d (%s)\n", rc, selenite_rx_error_string(NULL));
        return rc == SELENITE_RX_DEVICE_ERROR ? 77 : 1;      /* 77: no GPU here */
    }
    if (selenite_rx_out_values(rx, frames) != 2 * frames) {
        fprintf(stderr, "the slot is not symmetric: %u values out for %u frames in\n", selenite_rx_out_values(rx, frames), frames);
        return 1;
    }
    const size_t words = (size_t)DSP_CHANNELS * frames * 2;  /* the same number of words each way */
    float *f = malloc(sizeof(float) * words);
    int16_t *in = malloc(sizeof(int16_t) * words);
    int16_t *out = malloc(sizeof(int16_t) * words);
    for (int call = 0; call < 24; ++call) {                  /* 24 ms of signal */
        selenite_rx_synth_iq_host(f, 0, DSP_CHANNELS, (uint64_t)call * frames, frames, 0x5E1E917Eull);
        for (size_t i = 0; i < words; ++i) in[i] = (int16_t)(f[i] * 32768.0f);
        if (call == 16) DSP_Set_Mode(SELENITE_MODE_USB);
        DSP_Process_Block(in, out, (uint16_t)frames);
        if (selenite_rx_status(rx) != SELENITE_RX_SUCCESS) {
            fprintf(stderr, "process failed: %s\n", selenite_rx_error_string(rx));
            return 1;
        }
        long peak = 0;
        for (size_t i = 0; i < words; i += 2) {
            if (out[i] != out[i + 1]) { fprintf(stderr, "left != right at word %zu\n", i); return 1; }
            if (labs(out[i]) > peak) peak = labs(out[i]);
        }
        if (call % 8 == 7) printf("call %d: kernel %s, %u L/R frames per channel, audio peak %ld / 32768\n", call, selenite_rx_kernel_name(rx), frames, peak);
    }
    selenite_rx_free(rx);
    free(f); free(in); free(out);
    return 0;
}
