/*
 * dsp_if_mic_slot.c -- the firmware's per-block callback slot in TX as the codec sees it: `frames` int16 left / right microphone frames
 * in, `frames` int16 I/Q frames out, through the C-ABI only (include/selenite_tx.h).  The TX twin of dsp_if_codec_slot.c.
 *
 * In TX HAL_I2SEx_TxRx{Half,}CpltCallback (Core/Src/dsp_if.c:50-67) takes I2S_BUFF_HALF_SIZE words from the codec's microphone path
 * (DSP_In_Buff_Write, dsp_if.c:250-301: pbuf[k] = left, pbuf[k + 1] = right) and hands the same number of words back as I/Q.  The audio
 * input stage (selenite_tx_set_in) picks the left word, applies the mic gain, brings the audio down to the chain's rate
 * (arm_fir_decimate_f32 by DSP_DECIM) and keeps a voice-operated flag per channel; the chain interpolates by the same factor, so the
 * slot is symmetric as the firmware's is.
 *
 * Build (GPU box):  gcc -O2 -I../../include dsp_if_mic_slot.c -L.. -lselenite_rx -Wl,-rpath,'$ORIGIN/..' -lm -o dsp_if_mic_slot
 * This file is an integration example and a smoke test of the pure-C linkage; it contains no DSP.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "selenite_tx.h"

#define DSP_CHANNELS   64u      /* independent transmitters handled per callback */
#define DSP_BLOCK      96u      /* one I2S half-buffer: 96 L/R frames per millisecond at 96 kHz (Core/Inc/dsp_if.h:69-73) */
#define DSP_DECIM      4u
#define DSP_ND_TAPS    64u
#define DSP_NH_TAPS    63u
#define DSP_NI_TAPS    32u      /* interpolator: phase length 8 */

static selenite_tx_instance *tx;

/* mirrors void DSP_Init(void) (dsp_if.c:377-383) */
int DSP_Init(void)
{
    static float dec[DSP_ND_TAPS], hilb[DSP_NH_TAPS], dly[DSP_NH_TAPS], itp[DSP_NI_TAPS];
    selenite_tx_config cfg;
    selenite_tx_in_config in;
    int rc;
    memset(&cfg, 0, sizeof cfg);
    memset(&in, 0, sizeof in);
    if (selenite_rx_design_lowpass(dec, DSP_ND_TAPS, 0.4 / DSP_DECIM)) return -1;
    if (selenite_rx_design_hilbert(hilb, dly, DSP_NH_TAPS)) return -1;
    if (selenite_rx_design_interp(itp, DSP_NI_TAPS, DSP_DECIM, 0.4 / DSP_DECIM)) return -1;
    cfg.struct_size = sizeof cfg;
    cfg.abi_version = SELENITE_RX_ABI_VERSION;
    cfg.channels = DSP_CHANNELS; cfg.block = DSP_BLOCK / DSP_DECIM; cfg.interp = DSP_DECIM;
    cfg.ni_taps = DSP_NI_TAPS; cfg.nh_taps = DSP_NH_TAPS;
    cfg.arith = SELENITE_ARITH_CMSIS;
    cfg.mode = SELENITE_MODE_LSB;            /* RXTX_Init() boots in LSB (rxtx_if.c:686-699) */
    cfg.nco_enable = 1; cfg.nco_step_all = 0x01000000u;
    cfg.alc_enable = 1;
    cfg.interp_coeffs = itp; cfg.hilb_coeffs = hilb; cfg.delay_coeffs = dly;
    cfg.alc_target = 0.5f; cfg.alc_attack = 0.5f; cfg.alc_decay = 0.05f;
    cfg.alc_gain_min = 1e-3f; cfg.alc_gain_max = 1e2f; cfg.alc_env_floor = 1e-6f; cfg.alc_gain_init = 1.0f;
    rc = selenite_tx_init(&tx, &cfg);
    if (rc != SELENITE_RX_SUCCESS) return rc;
    in.struct_size = sizeof in;
    in.M = DSP_DECIM; in.nd_taps = DSP_ND_TAPS; in.pick = SELENITE_TX_IN_LEFT; in.coeffs = dec; in.gain = 1.0f;
    in.vox = 1;
    in.meter.struct_size = sizeof in.meter;
    in.meter.sense = SELENITE_RX_SQ_ABOVE; in.meter.gate = 0; in.meter.hang = 2;
    in.meter.attack = 0.5f; in.meter.decay = 1.0f; in.meter.open_level = 1e-3f; in.meter.close_level = 5e-4f; in.meter.level_init = 0.0f;
    return selenite_tx_set_in(tx, &in);
}

/* mirrors void DSP_Set_Mode(uint8_t mode) (dsp_if.c:367-370) */
void DSP_Set_Mode(uint8_t mode) { (void)selenite_tx_set_mode(tx, mode); }

/* the slot in TX, symmetric as the firmware's:
 * pbuf_in : int16 [DSP_CHANNELS][frames][2]   left, right      (dsp_if.c:286-289)
 * pbuf_out: int16 [DSP_CHANNELS][frames][2]   I, Q interleaved */
int DSP_Process_Block(const int16_t *pbuf_in, int16_t *pbuf_out, uint16_t frames)
{
    return selenite_tx_process_frames_q15(tx, pbuf_in, pbuf_out, frames / DSP_DECIM);
}

int main(void)
{
    const uint32_t frames = DSP_BLOCK;                       /* one slot per call, as the firmware's callback gets it */
    int rc = DSP_Init();
    if (rc != SELENITE_RX_SUCCESS) {
        fprintf(stderr, "DSP_Init failed: %d\n", rc);
        return rc == SELENITE_RX_DEVICE_ERROR ? 77 : 1;      /* 77: no GPU here */
    }
    const size_t words = (size_t)DSP_CHANNELS * frames * 2;  /* the same number of words each way */
    float *f = malloc(sizeof(float) * words);
    int16_t *in = malloc(sizeof(int16_t) * words);
    int16_t *out = malloc(sizeof(int16_t) * words);
    selenite_tx_in_state_view v;
    uint32_t open[DSP_CHANNELS];
    memset(&v, 0, sizeof v);
    v.open = open;
    for (int call = 0; call < 24; ++call) {                  /* 24 ms of signal; the microphone is silent in calls 8 .. 15 */
        selenite_rx_synth_iq_host(f, 0, DSP_CHANNELS, (uint64_t)call * frames, frames, 0x5E1E917Eull);
        for (size_t i = 0; i < words; ++i) in[i] = (call / 8 == 1) ? 0 : (int16_t)(f[i] * 32768.0f);
        if (call == 16) DSP_Set_Mode(SELENITE_MODE_USB);
        rc = DSP_Process_Block(in, out, (uint16_t)frames);
        if (rc != SELENITE_RX_SUCCESS || selenite_tx_status(tx) != SELENITE_RX_SUCCESS) {
            fprintf(stderr, "process failed: %d (%s)\n", rc, selenite_tx_error_string(tx));
            return 1;
        }
        if (selenite_tx_get_in_state(tx, &v) != SELENITE_RX_SUCCESS) { fprintf(stderr, "get_in_state failed\n"); return 1; }
        long peak = 0;
        unsigned nopen = 0;
        for (size_t i = 0; i < words; ++i)
            if (labs(out[i]) > peak) peak = labs(out[i]);
        for (unsigned c = 0; c < DSP_CHANNELS; ++c) nopen += open[c];
        if (call % 8 == 7) {
            printf("call %d: kernel %s, %u I/Q frames per channel, I/Q peak %ld / 32768, VOX open on %u of %u channels\n", call,
                   selenite_tx_kernel_name(tx), frames, peak, nopen, DSP_CHANNELS);
            if ((call == 15) != (nopen == 0)) { fprintf(stderr, "the VOX flag does not follow the microphone\n"); return 1; }
            if (peak == 0 && call != 15) { fprintf(stderr, "no I/Q out\n"); return 1; }
        }
    }
    selenite_tx_free(tx);
    free(f); free(in); free(out);
    return 0;
}
