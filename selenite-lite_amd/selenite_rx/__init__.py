"""ctypes face of libselenite_rx.so (include/selenite_rx.h).

Thin plumbing for tests and bench.py: every call goes straight through the C-ABI into the HIP
library.  There is no Python or CPU implementation of the chain here -- if the shared library is
missing or no HIP device is usable, construction fails loudly.

This module holds the C-ABI as ctypes sees it (constants, structs, the symbols every header declares, SIGNATURES), lib() and the host
helpers that need no instance.  The objects live in rx, tx, ring and bank (Channelizer, Combiner), the state round trip they share in
_state; they take what they need with `from . import ...` and are re-exported at the bottom.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(PKG_ROOT, "libselenite_rx.so")
if os.environ.get("SELENITE_RX_LIB"):            # A/B experiments: another build of the same library
    LIB_PATH = os.environ["SELENITE_RX_LIB"]

MODE_LSB, MODE_USB, MODE_CW, MODE_CWR, MODE_AM, MODE_FM, MODE_DIG, MODE_PKT = 0, 1, 2, 3, 4, 8, 0x0A, 0x0C
ARITH_CMSIS, ARITH_FMA, ARITH_SPLIT16, ARITH_AUTO = 0, 1, 2, 3
ABI_VERSION, CONFIG_SIZE_V1, TX_CONFIG_SIZE_V1 = 2, 112, 96      # include/selenite_rx.h, selenite_tx.h
OPT_FORCE_GENERIC, OPT_NO_SHARED_LO, OPT_NO_PERIODIC_LO, OPT_RERUN_GRID, OPT_TX_FORCE_GENERIC, OPT_CW_GRID = 0, 1, 2, 3, 4, 5      # selenite_rx_set_plan_option
SUCCESS, ARGUMENT_ERROR, LENGTH_ERROR, NANINF, DEVICE_ERROR = 0, -1, -2, -4, -7
NR_OFF, NR_DENOISE, NR_NOTCH = 0, 1, 2                         # selenite_rx_set_nr: the NLMS stage's kind
OUT_MONO, OUT_STEREO = 0, 1                                    # selenite_rx_set_out: the output stage's frame format
WINDOW_HANN, WINDOW_BLACKMAN_HARRIS = 0, 1                     # selenite_rx_design_window
SQ_ABOVE, SQ_BELOW = 0, 1                                      # selenite_rx_set_meter: the squelch's sense
IN_MONO, IN_LEFT, IN_RIGHT, IN_MIX = 0, 1, 2, 3                # selenite_tx_set_in: which words of a frame make the audio
IN_F32, IN_Q15, IN_Q15_F32 = 0, 1, 2                           # the frame entries: f32 -> f32 I/Q, int16 -> int16 I/Q, int16 -> f32 I/Q
KEYER_STRAIGHT, KEYER_IAMBIC_A, KEYER_IAMBIC_B = 0, 1, 2       # selenite_tx_set_keyer: the mode
PADDLE_DIT, PADDLE_DAH, PADDLE_KEY = 1, 2, 4                   # the paddle byte's bits

f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
i16p = C.POINTER(C.c_int16)
u64p = C.POINTER(C.c_uint64)
u8p = C.POINTER(C.c_uint8)
u16p = C.POINTER(C.c_uint16)


class Config(C.Structure):
    """struct selenite_rx_config."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("channels", C.c_uint32), ("block", C.c_uint32),
        ("decim", C.c_uint32), ("nd_taps", C.c_uint32), ("nh_taps", C.c_uint32),
        ("n_biquad", C.c_uint32), ("arith", C.c_uint32),
        ("mode", C.c_uint8), ("nco_enable", C.c_uint8), ("agc_enable", C.c_uint8), ("agc_global", C.c_uint8),
        ("nco_step_all", C.c_uint32),
        ("dec_coeffs", f32p), ("hilb_coeffs", f32p), ("delay_coeffs", f32p), ("biquad_coeffs", f32p),
        ("nco_step", u32p),
        ("agc_target", C.c_float), ("agc_attack", C.c_float), ("agc_decay", C.c_float),
        ("agc_gain_min", C.c_float), ("agc_gain_max", C.c_float), ("agc_env_floor", C.c_float),
        ("agc_gain_init", C.c_float),
        ("q15_rounding", C.c_uint32), ("abi_version", C.c_uint32), ("reserved", C.c_uint32),     # ABI version 2 (version 1 ends with agc_gain_init)
    ]


class StateView(C.Structure):
    """struct selenite_rx_state_view."""
    _fields_ = [("dec_state", f32p), ("fir_state", f32p), ("biq_state", f32p),
                ("agc_gain", f32p), ("nco_phase", u32p)]


class NrConfig(C.Structure):
    """struct selenite_rx_nr_config."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("num_taps", C.c_uint32), ("delay", C.c_uint32),
                ("mu", C.c_float), ("coeffs_init", f32p)]


class NrStateView(C.Structure):
    """struct selenite_rx_nr_state_view."""
    _fields_ = [("coeffs", f32p), ("window", f32p), ("delay", f32p), ("energy", f32p), ("x0", f32p)]


class OutConfig(C.Structure):
    """struct selenite_rx_out_config."""
    _fields_ = [("struct_size", C.c_uint32), ("interp", C.c_uint32), ("ni_taps", C.c_uint32), ("frames", C.c_uint32),
                ("coeffs", f32p)]


class SpecConfig(C.Structure):
    """struct selenite_rx_spec_config."""
    _fields_ = [("struct_size", C.c_uint32), ("fft_len", C.c_uint32), ("stride", C.c_uint32), ("average", C.c_uint32),
                ("alpha", C.c_float), ("window", f32p)]


class SpecStateView(C.Structure):
    """struct selenite_rx_spec_state_view."""
    _fields_ = [("rows", f32p), ("pending", f32p), ("position", u64p)]


class NbConfig(C.Structure):
    """struct selenite_rx_nb_config."""
    _fields_ = [("struct_size", C.c_uint32), ("frame", C.c_uint32), ("guard", C.c_uint32), ("max_hits", C.c_uint32),
                ("threshold", C.c_float), ("alpha", C.c_float), ("clamp", C.c_float)]


class NbStateView(C.Structure):
    """struct selenite_rx_nb_state_view."""
    _fields_ = [("level", f32p), ("blanked", u64p), ("bursts", u64p)]


class IqcConfig(C.Structure):
    """struct selenite_rx_iqc_config."""
    _fields_ = [("struct_size", C.c_uint32), ("frame", C.c_uint32), ("alpha", C.c_float), ("dc_alpha", C.c_float), ("p_max", C.c_float),
                ("g_max", C.c_float), ("min_power", C.c_float), ("p_init", C.c_float), ("g_init", C.c_float), ("dc_i_init", C.c_float),
                ("dc_q_init", C.c_float)]


class IqcStateView(C.Structure):
    """struct selenite_rx_iqc_state_view."""
    _fields_ = [("dc_i", f32p), ("dc_q", f32p), ("p", f32p), ("g", f32p), ("held", u64p)]


class MeterConfig(C.Structure):
    """struct selenite_rx_meter_config."""
    _fields_ = [("struct_size", C.c_uint32), ("sense", C.c_uint32), ("gate", C.c_uint32), ("hang", C.c_uint32), ("attack", C.c_float),
                ("decay", C.c_float), ("open_level", C.c_float), ("close_level", C.c_float), ("level_init", C.c_float)]


class MeterStateView(C.Structure):
    """struct selenite_rx_meter_state_view."""
    _fields_ = [("level", f32p), ("open", u32p), ("hold", u32p), ("opens", u64p), ("open_blocks", u64p)]


class AfiltConfig(C.Structure):
    """struct selenite_rx_afilt_config."""
    _fields_ = [("struct_size", C.c_uint32), ("n_stages", C.c_uint32), ("per_channel", C.c_uint32), ("reserved", C.c_uint32), ("coeffs", f32p)]


class AfiltStateView(C.Structure):
    """struct selenite_rx_afilt_state_view."""
    _fields_ = [("state", f32p), ("coeffs", f32p)]


BIQUAD_NOTCH, BIQUAD_PEAKING, BIQUAD_LOWPASS, BIQUAD_HIGHPASS = 0, 1, 2, 3      # selenite_rx_design_biquad: kind


class TonesConfig(C.Structure):
    """struct selenite_rx_tones_config."""
    _fields_ = [("struct_size", C.c_uint32), ("n_tones", C.c_uint32), ("frame_blocks", C.c_uint32), ("confirm", C.c_uint32),
                ("release", C.c_uint32), ("reserved", C.c_uint32), ("ratio", C.c_float), ("min_power", C.c_float), ("coeffs", f32p)]


class TonesStateView(C.Structure):
    """struct selenite_rx_tones_state_view."""
    _fields_ = [("s", f32p), ("energy", f32p), ("power", f32p), ("frame_energy", f32p), ("last_best", u32p), ("tone", u32p), ("cand", u32p),
                ("run", u32p), ("changes", u64p), ("position", u64p)]


TONES_MAX, TONE_NONE = 64, 0xFFFFFFFF


class CwdecConfig(C.Structure):
    """struct selenite_rx_cwdec_config."""
    _fields_ = [("struct_size", C.c_uint32), ("peak_attack", C.c_float), ("peak_decay", C.c_float), ("floor_attack", C.c_float),
                ("floor_decay", C.c_float), ("on_frac", C.c_float), ("off_frac", C.c_float), ("snr", C.c_float), ("min_power", C.c_float),
                ("debounce", C.c_uint32), ("adapt", C.c_uint32), ("track", C.c_uint32), ("unit_min", C.c_uint32), ("unit_init", C.c_uint32),
                ("unit_max", C.c_uint32), ("ring", C.c_uint32), ("table", u8p)]


class CwdecStateView(C.Structure):
    """struct selenite_rx_cwdec_state_view."""
    _fields_ = [("peak", f32p), ("floor", f32p), ("primed", u32p), ("key", u32p), ("flip", u32p), ("run", u32p), ("unit", u32p),
                ("code", u32p), ("word", u32p), ("count", u64p), ("text", u8p)]


# the documented defaults of Rx.set_cwdec (10 - 40 WPM at DSP blocks of about 5 ms)
CWDEC_DEFAULTS = dict(peak_attack=0.5, peak_decay=0.002, floor_attack=0.25, floor_decay=0.002, on_frac=0.4, off_frac=0.25, snr=4.0,
                      min_power=1e-8, debounce=2, adapt=1, track=2, unit_min=2 * 256, unit_init=10 * 256, unit_max=64 * 256, ring=256)

class FskdecConfig(C.Structure):
    """struct selenite_rx_fskdec_config."""
    _fields_ = [("struct_size", C.c_uint32), ("tick", C.c_uint32), ("bit_q8", C.c_uint32), ("reverse", C.c_uint32), ("usos", C.c_uint32),
                ("ring", C.c_uint32), ("mark", C.c_float * 5), ("space", C.c_float * 5), ("alpha", C.c_float), ("hyst", C.c_float),
                ("frac", C.c_float), ("min_power", C.c_float), ("table", u8p)]


class FskdecStateView(C.Structure):
    """struct selenite_rx_fskdec_state_view."""
    _fields_ = [("filt", f32p), ("em", f32p), ("es", f32p), ("ew", f32p), ("lvl", u32p), ("k", u32p), ("t_q8", u32p), ("shift", u32p),
                ("figs", u32p), ("ferr", u32p), ("bit", u32p), ("count", u64p), ("text", u8p)]


# the documented defaults of Rx.set_fskdec (45.45 baud at 12 kHz of audio and ticks of 16 samples: 16.5 ticks per bit)
FSKDEC_DEFAULTS = dict(tick=16, bit_q8=4224, reverse=0, usos=1, ring=256, alpha=0.25, hyst=0.1, frac=0.35, min_power=1e-6)

# every symbol include/selenite_rx.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "selenite_rx_init", "selenite_rx_free", "selenite_rx_set_mode", "selenite_rx_status",
    "selenite_rx_error_string", "selenite_rx_process_f32", "selenite_rx_process_f32_device",
    "selenite_rx_process_q15", "selenite_rx_process_q15_device",
    "selenite_rx_global_phase1_device", "selenite_rx_global_phase2_device",
    "selenite_rx_set_stream", "selenite_rx_sync", "selenite_rx_get_state", "selenite_rx_set_state",
    "selenite_rx_reset", "selenite_rx_device_alloc", "selenite_rx_device_free",
    "selenite_rx_memcpy_h2d", "selenite_rx_memcpy_d2h", "selenite_rx_device_count",
    "selenite_rx_set_device", "selenite_rx_synth_iq_host", "selenite_rx_synth_iq_device",
    "selenite_rx_time_process_device", "selenite_rx_time_process_q15_device", "selenite_rx_kernel_name", "selenite_rx_nco_path", "selenite_rx_algorithmic_bytes",
    "selenite_rx_design_lowpass", "selenite_rx_design_hilbert", "selenite_rx_design_bandpass",
    "selenite_rx_abi_version",
    "selenite_rx_global_process_f32_device",
    "selenite_rx_host_alloc", "selenite_rx_host_free", "selenite_rx_host_register", "selenite_rx_host_unregister",
    "selenite_rx_time_process_each_device", "selenite_rx_time_streaming_roof_device", "selenite_rx_time_pattern_roof_device", "selenite_rx_device_pci_bus_id", "selenite_rx_set_plan_option", "selenite_rx_get_plan_option",
    "selenite_rx_set_guard_ratio", "selenite_rx_guard_stats", "selenite_rx_guard_channels", "selenite_rx_auto_words", "selenite_rx_guard_handover", "selenite_rx_set_handover_repair", "selenite_rx_set_auto_launches", "selenite_rx_auto_launches_last", "selenite_rx_guard_clear",
    "selenite_rx_set_nr", "selenite_rx_get_nr_state", "selenite_rx_set_nr_state",
    "selenite_rx_set_out", "selenite_rx_out_values", "selenite_rx_get_out_state", "selenite_rx_set_out_state", "selenite_rx_design_interp",
    "selenite_rx_set_spectrum", "selenite_rx_get_spectrum", "selenite_rx_spectrum_device", "selenite_rx_get_spectrum_state",
    "selenite_rx_set_spectrum_state", "selenite_rx_spectrum_twiddles", "selenite_rx_design_window",
    "selenite_rx_set_nb", "selenite_rx_get_nb_state", "selenite_rx_set_nb_state",
    "selenite_rx_set_iqc", "selenite_rx_get_iqc_state", "selenite_rx_set_iqc_state",
    "selenite_rx_set_meter", "selenite_rx_get_meter_state", "selenite_rx_set_meter_state", "selenite_rx_meter_level_device",
    "selenite_rx_meter_open_device",
    "selenite_rx_set_afilt", "selenite_rx_set_afilt_coeffs", "selenite_rx_get_afilt_state", "selenite_rx_set_afilt_state",
    "selenite_rx_design_biquad", "selenite_rx_design_deemphasis",
    "selenite_rx_set_tones", "selenite_rx_get_tones_state", "selenite_rx_set_tones_state", "selenite_rx_get_tones",
    "selenite_rx_tones_tone_device", "selenite_rx_tones_power_device", "selenite_rx_design_tones", "selenite_rx_ctcss_hz",
    "selenite_rx_set_cwdec", "selenite_rx_get_cwdec_state", "selenite_rx_set_cwdec_state", "selenite_rx_get_cwdec",
    "selenite_rx_cwdec_text_device", "selenite_rx_cwdec_count_device", "selenite_rx_cwdec_unit_device", "selenite_rx_design_morse",
    "selenite_rx_set_fskdec", "selenite_rx_get_fskdec_state", "selenite_rx_set_fskdec_state", "selenite_rx_get_fskdec",
    "selenite_rx_fskdec_text_device", "selenite_rx_fskdec_count_device", "selenite_rx_fskdec_lvl_device", "selenite_rx_design_fsk",
    "selenite_rx_design_ita2",
]

class TxConfig(C.Structure):
    """struct selenite_tx_config (include/selenite_tx.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("channels", C.c_uint32), ("block", C.c_uint32),
        ("interp", C.c_uint32), ("ni_taps", C.c_uint32), ("nh_taps", C.c_uint32),
        ("arith", C.c_uint8), ("mode", C.c_uint8), ("nco_enable", C.c_uint8), ("alc_enable", C.c_uint8),
        ("nco_step_all", C.c_uint32),
        ("interp_coeffs", f32p), ("hilb_coeffs", f32p), ("delay_coeffs", f32p), ("nco_step", u32p),
        ("alc_target", C.c_float), ("alc_attack", C.c_float), ("alc_decay", C.c_float),
        ("alc_gain_min", C.c_float), ("alc_gain_max", C.c_float), ("alc_env_floor", C.c_float),
        ("alc_gain_init", C.c_float),
        ("q15_rounding", C.c_uint32), ("abi_version", C.c_uint32), ("reserved", C.c_uint32),     # ABI version 2
    ]


class TxStateView(C.Structure):
    """struct selenite_tx_state_view."""
    _fields_ = [("fir_state", f32p), ("interp_state", f32p), ("alc_gain", f32p), ("nco_phase", u32p)]


class TxFmConfig(C.Structure):
    """struct selenite_tx_fm_config."""
    _fields_ = [("struct_size", C.c_uint32), ("deviation", C.c_float), ("amplitude", C.c_float), ("tone_enable", C.c_uint32),
                ("tone_level", C.c_float), ("tone_step_all", C.c_uint32), ("tone_step", u32p), ("reserved", C.c_uint32)]


class TxFmStateView(C.Structure):
    """struct selenite_tx_fm_state_view."""
    _fields_ = [("tone_phase", u32p)]


# every symbol include/selenite_tx.h declares
TX_ABI_SYMBOLS = [
    "selenite_tx_init", "selenite_tx_free", "selenite_tx_set_mode", "selenite_tx_status", "selenite_tx_error_string",
    "selenite_tx_kernel_name",
    "selenite_tx_process_f32", "selenite_tx_process_q15", "selenite_tx_process_f32_device",
    "selenite_tx_process_q15_device", "selenite_tx_set_stream", "selenite_tx_sync", "selenite_tx_get_state",
    "selenite_tx_set_state", "selenite_tx_reset", "selenite_tx_time_process_device",
]

# every symbol include/selenite_tx_fm.h declares (the FM transmit mode; selenite_tx.h includes it)
TXFM_ABI_SYMBOLS = ["selenite_tx_set_fm", "selenite_tx_get_fm_state", "selenite_tx_set_fm_state", "selenite_tx_tone_step"]

class TxCwConfig(C.Structure):
    """struct selenite_tx_cw_config (include/selenite_tx_cw.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("ns_taps", C.c_uint32), ("shape_coeffs", f32p), ("amplitude", C.c_float),
                ("offset_step", C.c_uint32), ("side_level", C.c_float), ("side_step_all", C.c_uint32), ("side_step", u32p),
                ("side_mix", C.c_uint32), ("hang_blocks", C.c_uint32), ("reserved", C.c_uint32)]


class TxCwStateView(C.Structure):
    """struct selenite_tx_cw_state_view."""
    _fields_ = [("key_state", u8p), ("side_phase", u32p), ("tx_on", u32p), ("hold", u32p)]


# every symbol include/selenite_tx_cw.h declares (the keyed CW path; selenite_tx.h includes it)
TXCW_ABI_SYMBOLS = [
    "selenite_tx_set_cw", "selenite_tx_get_cw_state", "selenite_tx_set_cw_state",
    "selenite_tx_process_key_f32_device", "selenite_tx_process_key_q15_device", "selenite_tx_process_key_f32", "selenite_tx_process_key_q15",
    "selenite_tx_cw_txon_device", "selenite_tx_time_process_key_device", "selenite_tx_design_keyshape",
]

class TxInConfig(C.Structure):
    """struct selenite_tx_in_config (include/selenite_tx_in.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("M", C.c_uint32), ("nd_taps", C.c_uint32), ("pick", C.c_uint32), ("coeffs", f32p),
                ("gain", C.c_float), ("vox", C.c_uint32), ("meter", MeterConfig), ("reserved", C.c_uint32)]


class TxInStateView(C.Structure):
    """struct selenite_tx_in_state_view."""
    _fields_ = [("dec_state", f32p), ("level", f32p), ("open", u32p), ("hold", u32p), ("opens", u64p), ("open_blocks", u64p)]


# every symbol include/selenite_tx_in.h declares (the audio input stage; selenite_tx.h includes it)
TXIN_ABI_SYMBOLS = [
    "selenite_tx_set_in", "selenite_tx_get_in_state", "selenite_tx_set_in_state",
    "selenite_tx_process_frames_f32_device", "selenite_tx_process_frames_q15_device", "selenite_tx_process_frames_q15_f32_device",
    "selenite_tx_process_frames_f32", "selenite_tx_process_frames_q15",
    "selenite_tx_in_vox_device", "selenite_tx_in_audio_device", "selenite_tx_time_in_stage_device",
]

class TxKeyerConfig(C.Structure):
    """struct selenite_tx_keyer_config (include/selenite_tx_keyer.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_uint32), ("unit_all", C.c_uint32), ("unit", u32p), ("ring", C.c_uint32),
                ("codes", u8p), ("reserved", C.c_uint32)]


KEYER_STATE_WORDS = ("phase", "left", "last", "dit_mem", "dah_mem", "squeeze", "code", "tgap", "tail", "head", "skipped")


class TxKeyerStateView(C.Structure):
    """struct selenite_tx_keyer_state_view."""
    _fields_ = [(k, u32p) for k in KEYER_STATE_WORDS] + [("text", u8p)]


# every symbol include/selenite_tx_keyer.h declares (the keyer stage; selenite_tx.h includes it)
TXKEYER_ABI_SYMBOLS = [
    "selenite_tx_set_keyer", "selenite_tx_keyer_send", "selenite_tx_keyer_pending",
    "selenite_tx_process_paddles_f32_device", "selenite_tx_process_paddles_q15_device", "selenite_tx_process_paddles_f32",
    "selenite_tx_process_paddles_q15", "selenite_tx_keyer_run_device", "selenite_tx_keyer_key_device",
    "selenite_tx_get_keyer_state", "selenite_tx_set_keyer_state", "selenite_tx_time_keyer_stage_device",
    "selenite_tx_design_morse_codes", "selenite_tx_keyer_unit",
]

# every symbol include/selenite_ring.h declares
RING_ABI_SYMBOLS = [
    "selenite_ring_init", "selenite_ring_free", "selenite_ring_status", "selenite_ring_error_string",
    "selenite_ring_set_stream", "selenite_ring_sync",
    "selenite_ring_in_write_device", "selenite_ring_in_read_device",
    "selenite_ring_out_write_device", "selenite_ring_out_read_device", "selenite_ring_mute",
    "selenite_ring_in_write", "selenite_ring_in_read", "selenite_ring_out_write", "selenite_ring_out_read",
    "selenite_ring_get_state", "selenite_ring_set_state", "selenite_ring_time_device",
]


class ChanConfig(C.Structure):
    """struct selenite_chan_config (include/selenite_chan.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("bands", C.c_uint32), ("fft_len", C.c_uint32), ("oversample", C.c_uint32),
                ("taps_per_branch", C.c_uint32), ("n_bins", C.c_uint32), ("reserved", C.c_uint32),
                ("coeffs", f32p), ("bins", u32p)]


class ChanStateView(C.Structure):
    """struct selenite_chan_state_view."""
    _fields_ = [("history", f32p), ("position", u64p)]


# every symbol include/selenite_chan.h declares
CHAN_ABI_SYMBOLS = [
    "selenite_chan_init", "selenite_chan_free", "selenite_chan_status", "selenite_chan_error_string",
    "selenite_chan_set_stream", "selenite_chan_sync", "selenite_chan_reset", "selenite_chan_get_state", "selenite_chan_set_state",
    "selenite_chan_out_channels", "selenite_chan_out_len",
    "selenite_chan_process_f32_device", "selenite_chan_process_q15_device", "selenite_chan_design_prototype",
]

class CombConfig(C.Structure):
    """struct selenite_comb_config (include/selenite_comb.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("bands", C.c_uint32), ("fft_len", C.c_uint32), ("oversample", C.c_uint32),
                ("taps_per_branch", C.c_uint32), ("n_bins", C.c_uint32), ("q15_rounding", C.c_uint32), ("reserved", C.c_uint32),
                ("coeffs", f32p), ("bins", u32p)]


class CombStateView(C.Structure):
    """struct selenite_comb_state_view."""
    _fields_ = [("history", f32p), ("position", u64p)]


# every symbol include/selenite_comb.h declares
COMB_ABI_SYMBOLS = [
    "selenite_comb_init", "selenite_comb_free", "selenite_comb_status", "selenite_comb_error_string",
    "selenite_comb_set_stream", "selenite_comb_sync", "selenite_comb_reset", "selenite_comb_get_state", "selenite_comb_set_state",
    "selenite_comb_in_channels", "selenite_comb_out_len",
    "selenite_comb_process_f32_device", "selenite_comb_process_q15_device", "selenite_comb_design_prototype",
]


class RingStateView(C.Structure):
    """struct selenite_ring_state_view."""
    _fields_ = [("i", i16p), ("q", i16p), ("buff_enable", u8p), ("rd_ptr", u16p), ("wr_ptr", u16p)]


_lib = None


def build(force=False):
    """Compile libselenite_rx.so in-tree with hipcc for gfx950 (selenite-lite_amd/Makefile)."""
    if force:
        subprocess.run(["make", "-s", "-C", PKG_ROOT, "clean"], check=True)
    subprocess.run(["make", "-s", "-j4", "-C", PKG_ROOT], check=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# SIGNATURES: symbol -> (restype, argtypes), for every symbol of the lists above.  lib() binds each one the opened library exports and
# skips the others, so an older build named by SELENITE_RX_LIB still loads for an A/B run.  A row of sig() gives the symbols (without
# the prefix) that share one prototype; the restype is int unless the row says otherwise.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _signatures():
    table = {}

    def sig(prefix, names, argtypes, restype=C.c_int):
        for n in names.split():
            table[prefix + n] = (restype, argtypes)

    vp, u8, u16, u32, u64, f64, size_t = C.c_void_p, C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64, C.c_double, C.c_size_t
    P = C.POINTER

    sig("selenite_rx_", "init", [P(vp), P(Config)])
    sig("selenite_rx_", "free status sync reset device_free host_unregister guard_clear auto_launches_last", [vp])
    sig("selenite_rx_", "error_string kernel_name nco_path", [vp], C.c_char_p)
    sig("selenite_rx_", "set_mode", [vp, u8])
    sig("selenite_rx_", "process_f32", [vp, f32p, f32p, u32])
    sig("selenite_rx_", "process_q15", [vp, i16p, i16p, u32])
    sig("selenite_rx_", "process_f32_device process_q15_device global_phase2_device", [vp, vp, vp, u32])
    sig("selenite_rx_", "global_phase1_device", [vp, vp, vp, vp, u32])
    sig("selenite_rx_", "global_process_f32_device", [vp, vp, vp, u32, vp])
    sig("selenite_rx_", "set_stream", [vp, vp])
    sig("selenite_rx_", "get_state set_state", [vp, P(StateView)])
    sig("selenite_rx_", "device_alloc host_alloc", [size_t], vp)
    sig("selenite_rx_", "host_free", [vp], None)
    sig("selenite_rx_", "host_register", [vp, size_t])
    sig("selenite_rx_", "memcpy_h2d memcpy_d2h", [vp, vp, size_t])
    sig("selenite_rx_", "device_count abi_version", [])
    sig("selenite_rx_", "set_device", [C.c_int])
    sig("selenite_rx_", "device_pci_bus_id", [C.c_int, C.c_char_p, size_t])
    sig("selenite_rx_", "synth_iq_host", [f32p, u32, u32, u64, u32, u64])
    sig("selenite_rx_", "synth_iq_device", [vp, vp, u32, u32, u64, u32, u64])
    sig("selenite_rx_", "time_process_device time_process_q15_device", [vp, vp, vp, u32, u32, f32p])
    sig("selenite_rx_", "time_process_each_device time_streaming_roof_device", [vp, vp, vp, u32, u32, f32p, C.c_int])
    sig("selenite_rx_", "time_pattern_roof_device", [vp, vp, vp, u32, u32, f32p, C.c_int, u32])
    sig("selenite_rx_", "algorithmic_bytes", [P(Config), u32, u64p], u64)
    sig("selenite_rx_", "set_plan_option", [C.c_int, u32])
    sig("selenite_rx_", "get_plan_option", [C.c_int], u32)
    sig("selenite_rx_", "set_guard_ratio", [vp, C.c_float])
    sig("selenite_rx_", "guard_stats", [vp, u64p, u64p, u64p])
    sig("selenite_rx_", "guard_channels auto_words", [vp, u32p])
    sig("selenite_rx_", "guard_handover", [vp, u64p])
    sig("selenite_rx_", "set_handover_repair set_auto_launches", [vp, C.c_int])
    sig("selenite_rx_", "design_lowpass", [f32p, u32, f64])
    sig("selenite_rx_", "design_hilbert", [f32p, f32p, u32])
    sig("selenite_rx_", "design_bandpass", [f32p, u32, f64, f64])
    # the stages: set_X takes the config, get_X_state / set_X_state the view
    for _x, _cfg, _view in (("nr", NrConfig, NrStateView), ("spectrum", SpecConfig, SpecStateView), ("nb", NbConfig, NbStateView),
                            ("iqc", IqcConfig, IqcStateView), ("meter", MeterConfig, MeterStateView), ("afilt", AfiltConfig, AfiltStateView),
                            ("tones", TonesConfig, TonesStateView), ("cwdec", CwdecConfig, CwdecStateView),
                            ("fskdec", FskdecConfig, FskdecStateView)):
        sig("selenite_rx_", "set_%s" % _x, [vp, P(_cfg)])
        sig("selenite_rx_", "get_%s_state set_%s_state" % (_x, _x), [vp, P(_view)])
    sig("selenite_rx_", "set_out", [vp, P(OutConfig)])
    sig("selenite_rx_", "out_values", [vp, u32], u32)
    sig("selenite_rx_", "get_out_state set_out_state", [vp, f32p])
    sig("selenite_rx_", "design_interp", [f32p, u32, u32, f64])
    sig("selenite_rx_", "get_spectrum", [vp, f32p, u64p])
    sig("selenite_rx_", "spectrum_device meter_level_device meter_open_device tones_tone_device tones_power_device "
         "cwdec_text_device cwdec_count_device cwdec_unit_device fskdec_text_device fskdec_count_device fskdec_lvl_device", [vp], vp)
    sig("selenite_rx_", "spectrum_twiddles", [f32p, u32])
    sig("selenite_rx_", "design_window", [f32p, u32, C.c_int])
    sig("selenite_rx_", "set_afilt_coeffs", [vp, u32, u32, f32p])
    sig("selenite_rx_", "design_biquad", [f32p, C.c_int, f64, f64, f64])
    sig("selenite_rx_", "design_deemphasis", [f32p, f64])
    sig("selenite_rx_", "get_tones", [vp, u32p, f32p, u64p])
    sig("selenite_rx_", "design_tones", [f32p, P(f64), u32])
    sig("selenite_rx_", "ctcss_hz", [P(f64)], u32)
    sig("selenite_rx_", "get_cwdec", [vp, u8p, u64p, u32p, u32p])
    sig("selenite_rx_", "design_morse", [u8p, u8])
    sig("selenite_rx_", "get_fskdec", [vp, u8p, u64p, u32p, u32p])
    sig("selenite_rx_", "design_fsk", [f64, f64, f64, f32p, f32p])
    sig("selenite_rx_", "design_ita2", [u8p])

    sig("selenite_tx_", "init", [P(vp), P(TxConfig)])
    sig("selenite_tx_", "free status sync reset", [vp])
    sig("selenite_tx_", "error_string kernel_name", [vp], C.c_char_p)
    sig("selenite_tx_", "set_mode", [vp, u8])
    sig("selenite_tx_", "process_f32 process_q15 process_f32_device process_q15_device", [vp, vp, vp, u32], None)
    sig("selenite_tx_", "set_stream", [vp, vp])
    sig("selenite_tx_", "get_state set_state", [vp, P(TxStateView)])
    sig("selenite_tx_", "time_process_device", [vp, vp, vp, u32, u32, f32p])
    for _x, _cfg, _view in (("fm", TxFmConfig, TxFmStateView), ("cw", TxCwConfig, TxCwStateView), ("in", TxInConfig, TxInStateView),
                            ("keyer", TxKeyerConfig, TxKeyerStateView)):
        sig("selenite_tx_", "set_%s" % _x, [vp, P(_cfg)])
        sig("selenite_tx_", "get_%s_state set_%s_state" % (_x, _x), [vp, P(_view)])
    sig("selenite_tx_", "tone_step keyer_unit", [f64, f64], u32)
    sig("selenite_tx_", "process_key_f32_device process_key_q15_device process_key_f32 process_key_q15 "
         "process_paddles_f32_device process_paddles_q15_device process_paddles_f32 process_paddles_q15", [vp, vp, vp, vp, u32])
    sig("selenite_tx_", "cw_txon_device in_vox_device in_audio_device keyer_key_device", [vp], vp)
    sig("selenite_tx_", "time_process_key_device", [vp, vp, vp, vp, u32, u32, f32p])
    sig("selenite_tx_", "design_keyshape", [u32, f32p])
    sig("selenite_tx_", "process_frames_f32_device process_frames_q15_device process_frames_q15_f32_device process_frames_f32 "
         "process_frames_q15 keyer_run_device", [vp, vp, vp, u32])
    sig("selenite_tx_", "time_in_stage_device", [vp, vp, u32, u32, u32, f32p])
    sig("selenite_tx_", "keyer_send", [vp, u32, u32, vp, u32, u32])
    sig("selenite_tx_", "keyer_pending", [vp, u32p])
    sig("selenite_tx_", "time_keyer_stage_device", [vp, vp, u32, u32, f32p])
    sig("selenite_tx_", "design_morse_codes", [u8p, u8p])

    sig("selenite_ring_", "init", [P(vp), u32, u32])
    sig("selenite_ring_", "free status sync", [vp])
    sig("selenite_ring_", "error_string", [vp], C.c_char_p)
    sig("selenite_ring_", "set_stream", [vp, vp])
    sig("selenite_ring_", "in_write in_write_device out_read out_read_device", [vp, vp, u16], None)      # sizes in words
    sig("selenite_ring_", "in_read in_read_device out_write out_write_device", [vp, vp, u32], None)      # sizes in bytes
    sig("selenite_ring_", "mute", [vp], None)
    sig("selenite_ring_", "get_state set_state", [vp, P(RingStateView)])
    sig("selenite_ring_", "time_device", [vp, vp, vp, u16, u32, f32p])

    for _pre, _cfg, _view, _io in (("selenite_chan_", ChanConfig, ChanStateView, "out_channels"),
                                   ("selenite_comb_", CombConfig, CombStateView, "in_channels")):
        sig(_pre, "init", [P(vp), P(_cfg)])
        sig(_pre, "free", [vp], None)
        sig(_pre, "status sync reset", [vp])
        sig(_pre, "error_string", [vp], C.c_char_p)
        sig(_pre, "set_stream", [vp, vp])
        sig(_pre, "get_state set_state", [vp, P(_view)])
        sig(_pre, _io, [vp], u32)
        sig(_pre, "out_len", [vp, u32], u32)
        sig(_pre, "process_f32_device process_q15_device", [vp, vp, vp, u32], None)
    sig("selenite_chan_", "design_prototype", [f32p, u32, u32, f64])
    sig("selenite_comb_", "design_prototype", [f32p, u32, u32, f64, u32])
    return table


SIGNATURES = _signatures()


def lib():
    """the opened library, every symbol of SIGNATURES it exports bound to its prototype (an older build lacks the newer ones)"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libselenite_rx.so is not built (run __graft_entry__.build() or make -C selenite-lite_amd); "
                "there is no CPU fallback for the RX chain")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(f32p)


def device_pci_bus_id(ordinal):
    buf = C.create_string_buffer(32)
    rc = lib().selenite_rx_device_pci_bus_id(ordinal, buf, 32)
    return buf.value.decode() if rc == 0 else "unknown"


def design_lowpass(num_taps, cutoff):
    h = np.empty(num_taps, np.float32)
    rc = lib().selenite_rx_design_lowpass(_fp(h), num_taps, cutoff)
    if rc:
        raise ValueError("selenite_rx_design_lowpass: %d" % rc)
    return h


def design_biquad(kind, f0, q, gain_db=0.0):
    """one RBJ section for Rx.set_afilt, CMSIS order and sign {b0, b1, b2, -a1, -a2} / a0; f0 in cycles per sample of the audio rate"""
    c = np.empty(5, np.float32)
    rc = lib().selenite_rx_design_biquad(_fp(c), int(kind), float(f0), float(q), float(gain_db))
    if rc:
        raise ValueError("selenite_rx_design_biquad: %d" % rc)
    return c


def design_deemphasis(tau_samples):
    """one-pole FM de-emphasis for Rx.set_afilt: p = exp(-1 / tau_samples), {1 - p, 0, 0, p, 0}"""
    c = np.empty(5, np.float32)
    rc = lib().selenite_rx_design_deemphasis(_fp(c), float(tau_samples))
    if rc:
        raise ValueError("selenite_rx_design_deemphasis: %d" % rc)
    return c


def design_tones(freq):
    """the tone table for Rx.set_tones: [K][3] {2 cos w, cos w, sin w}, w = 2 pi freq; freq in cycles per sample of the audio rate"""
    f = np.ascontiguousarray(freq, np.float64).reshape(-1)
    c = np.empty((f.size, 3), np.float32)
    rc = lib().selenite_rx_design_tones(_fp(c), f.ctypes.data_as(C.POINTER(C.c_double)), f.size)
    if rc:
        raise ValueError("selenite_rx_design_tones: %d" % rc)
    return c


def morse_table(unknown="#"):
    """the Morse decoder's built-in table (selenite_rx_design_morse): uint8 [256], index = the element pattern behind a leading 1 (dit 0,
    dah 1; `.-` is 0b101); every index without a character, 0 (overflow) included, is `unknown`"""
    t = np.zeros(256, np.uint8)
    rc = lib().selenite_rx_design_morse(t.ctypes.data_as(u8p), ord(unknown) if isinstance(unknown, str) else int(unknown))
    if rc:
        raise ValueError("selenite_rx_design_morse: %d" % rc)
    return t


def fsk_bandpass(f_mark, f_space, bandwidth):
    """the FSK decoder's tone filters (selenite_rx_design_fsk): (mark, space), float32 [5] each, {b0, b1, b2, a1, a2} of the
    constant-peak-gain band-pass at f_mark / f_space, `bandwidth` wide; all three in cycles per sample of the audio rate"""
    m, s = np.empty(5, np.float32), np.empty(5, np.float32)
    rc = lib().selenite_rx_design_fsk(float(f_mark), float(f_space), float(bandwidth), _fp(m), _fp(s))
    if rc:
        raise ValueError("selenite_rx_design_fsk: %d" % rc)
    return m, s


def ita2_table():
    """the FSK decoder's built-in table (selenite_rx_design_ita2): uint8 [64], ITA2 letters then the US-TTY figures by the 5-bit code; 0
    where a code prints nothing"""
    t = np.zeros(64, np.uint8)
    rc = lib().selenite_rx_design_ita2(t.ctypes.data_as(u8p))
    if rc:
        raise ValueError("selenite_rx_design_ita2: %d" % rc)
    return t


def ring_text(ring, count):
    """the last min(count, len(ring)) characters of one channel's ring in order, as str (character i lies at ring[i % len(ring)])"""
    ring = np.asarray(ring, np.uint8)
    n = len(ring)
    if count <= n:
        return ring[:count].tobytes().decode("latin-1")
    at = count % n
    return (ring[at:].tobytes() + ring[:at].tobytes()).decode("latin-1")


def morse_key(text, unit_samples, table=None):
    """key bytes (uint8 0 / 1 per sample) of `text` for Tx.process_key and the tests: a dit is unit_samples samples down, a dah three
    times that; one unit up between the elements of a character, three between characters, seven for a blank.  Starts with the first
    element and ends with the last one: the caller adds the silence around it.  Characters are looked up in `table` (morse_table())."""
    t = morse_table() if table is None else np.asarray(table, np.uint8)
    code_of = {}
    for code in range(2, 256):
        code_of.setdefault(int(t[code]), code)
    unit_samples = int(unit_samples)
    if unit_samples < 1:
        raise ValueError("morse_key: unit_samples < 1")
    units, gap = [], 0                           # (down?, units) runs
    for ch in text.upper():
        if ch == " ":
            gap = 7 if units else 0
            continue
        code = code_of.get(ord(ch)) if ord(ch) != int(t[0]) else None
        if code is None:
            raise ValueError("morse_key: no pattern for %r" % ch)
        if gap or units:
            units.append((0, gap or 3))
        gap = 0
        els = [(code >> b) & 1 for b in range(code.bit_length() - 2, -1, -1)]
        for i, dah in enumerate(els):
            if i:
                units.append((0, 1))
            units.append((1, 3 if dah else 1))
    return np.concatenate([np.full(u * unit_samples, d, np.uint8) for d, u in units]) if units else np.zeros(0, np.uint8)


def morse_codes(table=None):
    """the keyer's character -> pattern table (selenite_tx_design_morse_codes): uint8 [256], the inverse of `table` (morse_table());
    lower case as upper case, ' ' -> 1 (the word blank), a byte without a pattern -> 0 (skipped)"""
    codes = np.zeros(256, np.uint8)
    t = None if table is None else np.ascontiguousarray(table, np.uint8)
    if t is not None and t.shape != (256,):
        raise ValueError("morse_codes: table is uint8 [256]")
    rc = lib().selenite_tx_design_morse_codes(codes.ctypes.data_as(u8p), None if t is None else t.ctypes.data_as(u8p))
    if rc:
        raise ValueError("selenite_tx_design_morse_codes: %d" % rc)
    return codes


def keyer_unit(wpm, fs_audio):
    """audio samples per dit at `wpm` words per minute (PARIS timing): round(1.2 * fs_audio / wpm), at least 1"""
    return int(lib().selenite_tx_keyer_unit(wpm, fs_audio))


def ctcss_hz():
    """the 50 standard CTCSS frequencies in Hz, ascending"""
    hz = np.zeros(50, np.float64)
    n = lib().selenite_rx_ctcss_hz(hz.ctypes.data_as(C.POINTER(C.c_double)))
    return hz[:n]


def tone_step(hz, fs_out):
    """phase increment per output sample of a tone (Tx.set_fm tone_step, nco_step): round(hz / fs_out * 2^32)"""
    return int(lib().selenite_tx_tone_step(hz, fs_out))


def keyshape(ns):
    """the keying shape for Tx.set_cw: a Hann window of `ns` taps normalised to sum 1 (selenite_tx_design_keyshape); ns = 1: hard keying"""
    h = np.empty(int(ns), np.float32)
    rc = lib().selenite_tx_design_keyshape(int(ns), _fp(h))
    if rc:
        raise ValueError("selenite_tx_design_keyshape: %d" % rc)
    return h


def design_interp(ni_taps, interp, cutoff):
    """the output stage's interpolation low-pass: design_lowpass(ni_taps, cutoff) * interp, pCoeffs order"""
    h = np.empty(ni_taps, np.float32)
    rc = lib().selenite_rx_design_interp(_fp(h), ni_taps, interp, cutoff)
    if rc:
        raise ValueError("selenite_rx_design_interp: %d" % rc)
    return h


def design_window(n, kind=WINDOW_HANN):
    """a window for the spectrum tap (WINDOW_HANN / WINDOW_BLACKMAN_HARRIS), periodic form"""
    w = np.empty(n, np.float32)
    rc = lib().selenite_rx_design_window(_fp(w), n, kind)
    if rc:
        raise ValueError("selenite_rx_design_window: %d" % rc)
    return w


def spectrum_twiddles(fft_len):
    """[fft_len][2] (cos, sin): the twiddle table the spectrum kernel uses (host only, no device)"""
    tw = np.empty((fft_len, 2), np.float32)
    rc = lib().selenite_rx_spectrum_twiddles(_fp(tw), fft_len)
    if rc:
        raise ValueError("selenite_rx_spectrum_twiddles: %d" % rc)
    return tw


def design_hilbert(num_taps):
    h, d = np.empty(num_taps, np.float32), np.empty(num_taps, np.float32)
    rc = lib().selenite_rx_design_hilbert(_fp(h), _fp(d), num_taps)
    if rc:
        raise ValueError("selenite_rx_design_hilbert: %d" % rc)
    return h, d


def design_bandpass(n_stages, f0, q):
    c = np.empty(5 * n_stages, np.float32)
    rc = lib().selenite_rx_design_bandpass(_fp(c), n_stages, f0, q)
    if rc:
        raise ValueError("selenite_rx_design_bandpass: %d" % rc)
    return c


def synth_iq_host(first_channel, nch, first_sample, nsamp, seed):
    iq = np.empty((nch, nsamp, 2), np.float32)
    lib().selenite_rx_synth_iq_host(_fp(iq), first_channel, nch, first_sample, nsamp, seed)
    return iq


class _PinnedOwner:
    def __init__(self, nbytes):
        self.ptr = lib().selenite_rx_host_alloc(nbytes)
        if not self.ptr:
            raise MemoryError("selenite_rx_host_alloc(%d) failed" % nbytes)

    def __del__(self):
        try:
            lib().selenite_rx_host_free(self.ptr)
        except Exception:
            pass


def pinned_array(shape, dtype):
    """numpy array over page-locked host memory (selenite_rx_host_alloc): the host-pointer process calls DMA
    straight from / into it."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    owner = _PinnedOwner(max(n, 1))
    buf = (C.c_char * max(n, 1)).from_address(owner.ptr)
    buf._owner = owner                       # the array keeps `buf` alive (arr.base), `buf` keeps the allocation
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


class DeviceBuffer:
    """hipMalloc'ed bytes owned through the C-ABI helpers."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().selenite_rx_device_alloc(self.nbytes)
        if not self.ptr:
            raise MemoryError("selenite_rx_device_alloc(%d) failed" % nbytes)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        rc = lib().selenite_rx_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes)
        if rc:
            raise RuntimeError("h2d failed")

    def download(self, shape, dtype):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        rc = lib().selenite_rx_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes)
        if rc:
            raise RuntimeError("d2h failed")
        return out

    def free(self):
        if self.ptr:
            lib().selenite_rx_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("selenite_rx error %d: %s" % (code, msg))
        self.code = code


class plan_option:
    """`with plan_option(OPT_FORCE_GENERIC):` -- a kernel-selection override of the library (selenite_rx_set_plan_option) for the instances created
    inside the block; restored afterwards.  Results do not depend on it: the tests use it to reach every product path."""

    def __init__(self, option, value=1):
        self.option, self.value = option, value

    def __enter__(self):
        self.old = lib().selenite_rx_get_plan_option(self.option)
        if lib().selenite_rx_set_plan_option(self.option, self.value) != SUCCESS:
            raise ValueError("selenite_rx_set_plan_option(%d, %d)" % (self.option, self.value))
        return self

    def __exit__(self, *exc):
        lib().selenite_rx_set_plan_option(self.option, self.old)
        return False


# (the submodules take lib(), RxError and the helpers above from here: `from . import lib`)
from .rx import Rx  # noqa: E402,F401
from .tx import Tx  # noqa: E402,F401
from .ring import Ring  # noqa: E402,F401
from .bank import Channelizer, Combiner, _FilterBank, design_chan_prototype, design_comb_prototype  # noqa: E402,F401
