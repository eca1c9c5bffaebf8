"""ctypes face of libselenite_rx.so (include/selenite_rx.h).

Thin plumbing for tests and bench.py: every call goes straight through the C-ABI into the HIP
library.  There is no Python or CPU implementation of the chain here -- if the shared library is
missing or no HIP device is usable, construction fails loudly.
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

u8p = C.POINTER(C.c_uint8)


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
    _fields_ = [("key_state", C.POINTER(C.c_uint8)), ("side_phase", u32p), ("tx_on", u32p), ("hold", u32p)]


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
                ("codes", C.POINTER(C.c_uint8)), ("reserved", C.c_uint32)]


KEYER_STATE_WORDS = ("phase", "left", "last", "dit_mem", "dah_mem", "squeeze", "code", "tgap", "tail", "head", "skipped")


class TxKeyerStateView(C.Structure):
    """struct selenite_tx_keyer_state_view."""
    _fields_ = [(k, u32p) for k in KEYER_STATE_WORDS] + [("text", C.POINTER(C.c_uint8))]


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

_lib = None


def build(force=False):
    """Compile libselenite_rx.so in-tree with hipcc for gfx950 (selenite-lite_amd/Makefile)."""
    if force:
        subprocess.run(["make", "-s", "-C", PKG_ROOT, "clean"], check=True)
    subprocess.run(["make", "-s", "-j4", "-C", PKG_ROOT], check=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libselenite_rx.so is not built (run __graft_entry__.build() or make -C selenite-lite_amd); "
                "there is no CPU fallback for the RX chain")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.selenite_rx_init.argtypes = [C.POINTER(vp), C.POINTER(Config)]
        L.selenite_rx_free.argtypes = [vp]
        L.selenite_rx_set_mode.argtypes = [vp, C.c_uint8]
        L.selenite_rx_status.argtypes = [vp]
        L.selenite_rx_error_string.argtypes = [vp]
        L.selenite_rx_error_string.restype = C.c_char_p
        L.selenite_rx_process_f32.argtypes = [vp, f32p, f32p, C.c_uint32]
        L.selenite_rx_process_f32_device.argtypes = [vp, vp, vp, C.c_uint32]
        L.selenite_rx_process_q15.argtypes = [vp, i16p, i16p, C.c_uint32]
        L.selenite_rx_process_q15_device.argtypes = [vp, vp, vp, C.c_uint32]
        L.selenite_rx_global_phase1_device.argtypes = [vp, vp, vp, vp, C.c_uint32]
        L.selenite_rx_global_phase2_device.argtypes = [vp, vp, vp, C.c_uint32]
        L.selenite_rx_set_stream.argtypes = [vp, vp]
        L.selenite_rx_sync.argtypes = [vp]
        L.selenite_rx_get_state.argtypes = [vp, C.POINTER(StateView)]
        L.selenite_rx_set_state.argtypes = [vp, C.POINTER(StateView)]
        L.selenite_rx_reset.argtypes = [vp]
        L.selenite_rx_device_alloc.argtypes = [C.c_size_t]
        L.selenite_rx_device_alloc.restype = vp
        L.selenite_rx_device_free.argtypes = [vp]
        L.selenite_rx_host_alloc.argtypes = [C.c_size_t]
        L.selenite_rx_host_alloc.restype = vp
        L.selenite_rx_host_free.argtypes = [vp]
        L.selenite_rx_host_free.restype = None
        L.selenite_rx_host_register.argtypes = [vp, C.c_size_t]
        L.selenite_rx_host_unregister.argtypes = [vp]
        L.selenite_rx_memcpy_h2d.argtypes = [vp, vp, C.c_size_t]
        L.selenite_rx_memcpy_d2h.argtypes = [vp, vp, C.c_size_t]
        L.selenite_rx_set_device.argtypes = [C.c_int]
        L.selenite_rx_synth_iq_host.argtypes = [f32p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64]
        L.selenite_rx_synth_iq_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64]
        L.selenite_rx_time_process_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, f32p]
        L.selenite_rx_kernel_name.argtypes = [vp]
        L.selenite_rx_kernel_name.restype = C.c_char_p
        L.selenite_rx_nco_path.argtypes = [vp]
        L.selenite_rx_nco_path.restype = C.c_char_p
        L.selenite_rx_algorithmic_bytes.argtypes = [C.POINTER(Config), C.c_uint32, C.POINTER(C.c_uint64)]
        L.selenite_rx_algorithmic_bytes.restype = C.c_uint64
        u64p = C.POINTER(C.c_uint64)
        L.selenite_rx_time_process_each_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, f32p, C.c_int]
        L.selenite_rx_time_streaming_roof_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, f32p, C.c_int]
        if hasattr(L, "selenite_rx_set_plan_option"):      # (round-6 entry points: an older build named by SELENITE_RX_LIB for an A/B run lacks them)
            L.selenite_rx_set_plan_option.argtypes = [C.c_int, C.c_uint32]
            L.selenite_rx_get_plan_option.argtypes = [C.c_int]
            L.selenite_rx_get_plan_option.restype = C.c_uint32
            L.selenite_rx_time_pattern_roof_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, f32p, C.c_int, C.c_uint32]
        L.selenite_rx_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        L.selenite_rx_set_guard_ratio.argtypes = [vp, C.c_float]
        L.selenite_rx_guard_stats.argtypes = [vp, u64p, u64p, u64p]
        L.selenite_rx_guard_channels.argtypes = [vp, u32p]
        L.selenite_rx_auto_words.argtypes = [vp, u32p]
        L.selenite_rx_guard_clear.argtypes = [vp]
        L.selenite_rx_guard_handover.argtypes = [vp, u64p]
        L.selenite_rx_set_handover_repair.argtypes = [vp, C.c_int]
        L.selenite_rx_set_auto_launches.argtypes = [vp, C.c_int]
        L.selenite_rx_auto_launches_last.argtypes = [vp]
        if hasattr(L, "selenite_rx_set_nr"):                # (an older build named by SELENITE_RX_LIB lacks the NLMS stage)
            L.selenite_rx_set_nr.argtypes = [vp, C.POINTER(NrConfig)]
            L.selenite_rx_get_nr_state.argtypes = [vp, C.POINTER(NrStateView)]
            L.selenite_rx_set_nr_state.argtypes = [vp, C.POINTER(NrStateView)]
        if hasattr(L, "selenite_rx_set_out"):               # (an older build named by SELENITE_RX_LIB lacks the output stage)
            L.selenite_rx_set_out.argtypes = [vp, C.POINTER(OutConfig)]
            L.selenite_rx_out_values.argtypes = [vp, C.c_uint32]
            L.selenite_rx_out_values.restype = C.c_uint32
            L.selenite_rx_get_out_state.argtypes = [vp, f32p]
            L.selenite_rx_set_out_state.argtypes = [vp, f32p]
            L.selenite_rx_design_interp.argtypes = [f32p, C.c_uint32, C.c_uint32, C.c_double]
        if hasattr(L, "selenite_rx_set_spectrum"):          # (an older build named by SELENITE_RX_LIB lacks the spectrum tap)
            L.selenite_rx_set_spectrum.argtypes = [vp, C.POINTER(SpecConfig)]
            L.selenite_rx_get_spectrum.argtypes = [vp, f32p, u64p]
            L.selenite_rx_spectrum_device.argtypes = [vp]
            L.selenite_rx_spectrum_device.restype = vp
            L.selenite_rx_get_spectrum_state.argtypes = [vp, C.POINTER(SpecStateView)]
            L.selenite_rx_set_spectrum_state.argtypes = [vp, C.POINTER(SpecStateView)]
            L.selenite_rx_spectrum_twiddles.argtypes = [f32p, C.c_uint32]
            L.selenite_rx_design_window.argtypes = [f32p, C.c_uint32, C.c_int]
        if hasattr(L, "selenite_rx_set_nb"):                # (an older build named by SELENITE_RX_LIB lacks the noise blanker)
            L.selenite_rx_set_nb.argtypes = [vp, C.POINTER(NbConfig)]
            L.selenite_rx_get_nb_state.argtypes = [vp, C.POINTER(NbStateView)]
            L.selenite_rx_set_nb_state.argtypes = [vp, C.POINTER(NbStateView)]
        if hasattr(L, "selenite_rx_set_iqc"):               # (an older build named by SELENITE_RX_LIB lacks the I/Q correction)
            L.selenite_rx_set_iqc.argtypes = [vp, C.POINTER(IqcConfig)]
            L.selenite_rx_get_iqc_state.argtypes = [vp, C.POINTER(IqcStateView)]
            L.selenite_rx_set_iqc_state.argtypes = [vp, C.POINTER(IqcStateView)]
        if hasattr(L, "selenite_rx_set_meter"):             # (an older build named by SELENITE_RX_LIB lacks the level meter)
            L.selenite_rx_set_meter.argtypes = [vp, C.POINTER(MeterConfig)]
            L.selenite_rx_get_meter_state.argtypes = [vp, C.POINTER(MeterStateView)]
            L.selenite_rx_set_meter_state.argtypes = [vp, C.POINTER(MeterStateView)]
            L.selenite_rx_meter_level_device.argtypes = [vp]
            L.selenite_rx_meter_level_device.restype = vp
            L.selenite_rx_meter_open_device.argtypes = [vp]
            L.selenite_rx_meter_open_device.restype = vp
        if hasattr(L, "selenite_rx_set_afilt"):             # (an older build named by SELENITE_RX_LIB lacks the audio filter)
            L.selenite_rx_set_afilt.argtypes = [vp, C.POINTER(AfiltConfig)]
            L.selenite_rx_set_afilt_coeffs.argtypes = [vp, C.c_uint32, C.c_uint32, f32p]
            L.selenite_rx_get_afilt_state.argtypes = [vp, C.POINTER(AfiltStateView)]
            L.selenite_rx_set_afilt_state.argtypes = [vp, C.POINTER(AfiltStateView)]
            L.selenite_rx_design_biquad.argtypes = [f32p, C.c_int, C.c_double, C.c_double, C.c_double]
            L.selenite_rx_design_deemphasis.argtypes = [f32p, C.c_double]
        if hasattr(L, "selenite_rx_set_tones"):             # (an older build named by SELENITE_RX_LIB lacks the tone detector)
            L.selenite_rx_set_tones.argtypes = [vp, C.POINTER(TonesConfig)]
            L.selenite_rx_get_tones_state.argtypes = [vp, C.POINTER(TonesStateView)]
            L.selenite_rx_set_tones_state.argtypes = [vp, C.POINTER(TonesStateView)]
            L.selenite_rx_get_tones.argtypes = [vp, C.POINTER(C.c_uint32), f32p, u64p]
            L.selenite_rx_tones_tone_device.argtypes = [vp]
            L.selenite_rx_tones_tone_device.restype = vp
            L.selenite_rx_tones_power_device.argtypes = [vp]
            L.selenite_rx_tones_power_device.restype = vp
            L.selenite_rx_design_tones.argtypes = [f32p, C.POINTER(C.c_double), C.c_uint32]
            L.selenite_rx_ctcss_hz.argtypes = [C.POINTER(C.c_double)]
            L.selenite_rx_ctcss_hz.restype = C.c_uint32
        if hasattr(L, "selenite_rx_set_cwdec"):             # (an older build named by SELENITE_RX_LIB lacks the Morse decoder)
            L.selenite_rx_set_cwdec.argtypes = [vp, C.POINTER(CwdecConfig)]
            L.selenite_rx_get_cwdec_state.argtypes = [vp, C.POINTER(CwdecStateView)]
            L.selenite_rx_set_cwdec_state.argtypes = [vp, C.POINTER(CwdecStateView)]
            L.selenite_rx_get_cwdec.argtypes = [vp, u8p, u64p, u32p, u32p]
            for n in ("text", "count", "unit"):
                getattr(L, "selenite_rx_cwdec_%s_device" % n).argtypes = [vp]
                getattr(L, "selenite_rx_cwdec_%s_device" % n).restype = vp
            L.selenite_rx_design_morse.argtypes = [u8p, C.c_uint8]
        if hasattr(L, "selenite_tx_set_fm"):                # (an older build named by SELENITE_RX_LIB lacks the FM transmit mode)
            L.selenite_tx_set_fm.argtypes = [vp, C.POINTER(TxFmConfig)]
            L.selenite_tx_get_fm_state.argtypes = [vp, C.POINTER(TxFmStateView)]
            L.selenite_tx_set_fm_state.argtypes = [vp, C.POINTER(TxFmStateView)]
            L.selenite_tx_tone_step.argtypes = [C.c_double, C.c_double]
            L.selenite_tx_tone_step.restype = C.c_uint32
        if hasattr(L, "selenite_tx_set_cw"):                # (an older build named by SELENITE_RX_LIB lacks the keyed CW path)
            L.selenite_tx_set_cw.argtypes = [vp, C.POINTER(TxCwConfig)]
            L.selenite_tx_get_cw_state.argtypes = [vp, C.POINTER(TxCwStateView)]
            L.selenite_tx_set_cw_state.argtypes = [vp, C.POINTER(TxCwStateView)]
            for n in ("f32_device", "q15_device", "f32", "q15"):
                getattr(L, "selenite_tx_process_key_" + n).argtypes = [vp, vp, vp, vp, C.c_uint32]
            L.selenite_tx_cw_txon_device.argtypes = [vp]
            L.selenite_tx_cw_txon_device.restype = vp
            L.selenite_tx_time_process_key_device.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
            L.selenite_tx_design_keyshape.argtypes = [C.c_uint32, f32p]
        if hasattr(L, "selenite_tx_set_in"):                # (an older build named by SELENITE_RX_LIB lacks the audio input stage)
            L.selenite_tx_set_in.argtypes = [vp, C.POINTER(TxInConfig)]
            L.selenite_tx_get_in_state.argtypes = [vp, C.POINTER(TxInStateView)]
            L.selenite_tx_set_in_state.argtypes = [vp, C.POINTER(TxInStateView)]
            for n in ("f32_device", "q15_device", "q15_f32_device", "f32", "q15"):
                getattr(L, "selenite_tx_process_frames_" + n).argtypes = [vp, vp, vp, C.c_uint32]
            L.selenite_tx_in_vox_device.argtypes = [vp]
            L.selenite_tx_in_vox_device.restype = vp
            L.selenite_tx_in_audio_device.argtypes = [vp]
            L.selenite_tx_in_audio_device.restype = vp
            L.selenite_tx_time_in_stage_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        if hasattr(L, "selenite_tx_set_keyer"):             # (an older build named by SELENITE_RX_LIB lacks the keyer stage)
            L.selenite_tx_set_keyer.argtypes = [vp, C.POINTER(TxKeyerConfig)]
            L.selenite_tx_keyer_send.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32]
            L.selenite_tx_keyer_pending.argtypes = [vp, u32p]
            for n in ("f32_device", "q15_device", "f32", "q15"):
                getattr(L, "selenite_tx_process_paddles_" + n).argtypes = [vp, vp, vp, vp, C.c_uint32]
            L.selenite_tx_keyer_run_device.argtypes = [vp, vp, vp, C.c_uint32]
            L.selenite_tx_keyer_key_device.argtypes = [vp]
            L.selenite_tx_keyer_key_device.restype = vp
            L.selenite_tx_get_keyer_state.argtypes = [vp, C.POINTER(TxKeyerStateView)]
            L.selenite_tx_set_keyer_state.argtypes = [vp, C.POINTER(TxKeyerStateView)]
            L.selenite_tx_time_keyer_stage_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
            L.selenite_tx_design_morse_codes.argtypes = [u8p, u8p]
            L.selenite_tx_keyer_unit.argtypes = [C.c_double, C.c_double]
            L.selenite_tx_keyer_unit.restype = C.c_uint32
        L.selenite_rx_design_lowpass.argtypes = [f32p, C.c_uint32, C.c_double]
        L.selenite_rx_design_hilbert.argtypes = [f32p, f32p, C.c_uint32]
        L.selenite_rx_design_bandpass.argtypes = [f32p, C.c_uint32, C.c_double, C.c_double]
        if hasattr(L, "selenite_chan_init"):                # (an older build named by SELENITE_RX_LIB lacks the channeliser)
            L.selenite_chan_init.argtypes = [C.POINTER(vp), C.POINTER(ChanConfig)]
            L.selenite_chan_free.argtypes = [vp]
            L.selenite_chan_free.restype = None
            L.selenite_chan_status.argtypes = [vp]
            L.selenite_chan_error_string.argtypes = [vp]
            L.selenite_chan_error_string.restype = C.c_char_p
            L.selenite_chan_set_stream.argtypes = [vp, vp]
            L.selenite_chan_sync.argtypes = [vp]
            L.selenite_chan_reset.argtypes = [vp]
            L.selenite_chan_get_state.argtypes = [vp, C.POINTER(ChanStateView)]
            L.selenite_chan_set_state.argtypes = [vp, C.POINTER(ChanStateView)]
            L.selenite_chan_out_channels.argtypes = [vp]
            L.selenite_chan_out_channels.restype = C.c_uint32
            L.selenite_chan_out_len.argtypes = [vp, C.c_uint32]
            L.selenite_chan_out_len.restype = C.c_uint32
            L.selenite_chan_process_f32_device.argtypes = [vp, vp, vp, C.c_uint32]
            L.selenite_chan_process_f32_device.restype = None
            L.selenite_chan_process_q15_device.argtypes = [vp, vp, vp, C.c_uint32]
            L.selenite_chan_process_q15_device.restype = None
            L.selenite_chan_design_prototype.argtypes = [f32p, C.c_uint32, C.c_uint32, C.c_double]
        if hasattr(L, "selenite_comb_init"):                # (an older build named by SELENITE_RX_LIB lacks the combiner)
            L.selenite_comb_init.argtypes = [C.POINTER(vp), C.POINTER(CombConfig)]
            L.selenite_comb_free.argtypes = [vp]
            L.selenite_comb_free.restype = None
            L.selenite_comb_status.argtypes = [vp]
            L.selenite_comb_error_string.argtypes = [vp]
            L.selenite_comb_error_string.restype = C.c_char_p
            L.selenite_comb_set_stream.argtypes = [vp, vp]
            L.selenite_comb_sync.argtypes = [vp]
            L.selenite_comb_reset.argtypes = [vp]
            L.selenite_comb_get_state.argtypes = [vp, C.POINTER(CombStateView)]
            L.selenite_comb_set_state.argtypes = [vp, C.POINTER(CombStateView)]
            L.selenite_comb_in_channels.argtypes = [vp]
            L.selenite_comb_in_channels.restype = C.c_uint32
            L.selenite_comb_out_len.argtypes = [vp, C.c_uint32]
            L.selenite_comb_out_len.restype = C.c_uint32
            L.selenite_comb_process_f32_device.argtypes = [vp, vp, vp, C.c_uint32]
            L.selenite_comb_process_f32_device.restype = None
            L.selenite_comb_process_q15_device.argtypes = [vp, vp, vp, C.c_uint32]
            L.selenite_comb_process_q15_device.restype = None
            L.selenite_comb_design_prototype.argtypes = [f32p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32]
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


class Rx:
    """One selenite_rx_instance.  `cfg` is a filled Config whose coefficient arrays the caller keeps
    alive until construction returns (the library copies them)."""

    def __init__(self, cfg):
        self.L = lib()
        self.cfg = cfg
        self.h = C.c_void_p()
        rc = self.L.selenite_rx_init(C.byref(self.h), C.byref(cfg))
        if rc != SUCCESS:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode())

    # -- CMSIS-style calls ------------------------------------------------------------------
    def out_len(self, block_size):
        """values per channel a call of block_size writes: block_size / decim, or what the output stage makes of it (out_values)"""
        if getattr(self, "_out", None) is not None:
            return self.out_values(block_size)
        return block_size // self.cfg.decim

    def process(self, iq, out=None):
        """selenite_rx_process_f32 on host arrays (pageable numpy memory, or page-locked `pinned_array`s)."""
        iq = np.ascontiguousarray(iq, np.float32)
        c, bs = iq.shape[0], iq.shape[1]
        if out is None:
            out = np.empty((c, self.out_len(bs)), np.float32)
        self.L.selenite_rx_process_f32(self.h, _fp(iq), _fp(out), bs)
        self.check()
        return out

    def process_q15(self, iq, out=None):
        iq = np.ascontiguousarray(iq, np.int16)
        c, bs = iq.shape[0], iq.shape[1]
        if out is None:
            out = np.empty((c, self.out_len(bs)), np.int16)
        self.L.selenite_rx_process_q15(self.h, iq.ctypes.data_as(i16p), out.ctypes.data_as(i16p), bs)
        self.check()
        return out

    def process_device(self, d_src, d_dst, block_size):
        self.L.selenite_rx_process_f32_device(self.h, d_src, d_dst, block_size)

    def process_q15_device(self, d_src, d_dst, block_size):
        self.L.selenite_rx_process_q15_device(self.h, d_src, d_dst, block_size)

    def global_phase1(self, d_src, d_dst, d_env, block_size):
        self.L.selenite_rx_global_phase1_device(self.h, d_src, d_dst, d_env, block_size)

    def global_phase2(self, d_dst, d_env, block_size):
        self.L.selenite_rx_global_phase2_device(self.h, d_dst, d_env, block_size)

    def set_mode(self, mode):
        return self.L.selenite_rx_set_mode(self.h, mode)

    def set_stream(self, stream_ptr):
        return self.L.selenite_rx_set_stream(self.h, stream_ptr)

    def sync(self):
        rc = self.L.selenite_rx_sync(self.h)
        if rc:
            raise RxError(rc, self.error())

    def reset(self):
        return self.L.selenite_rx_reset(self.h)

    def status(self):
        return self.L.selenite_rx_status(self.h)

    def error(self):
        return self.L.selenite_rx_error_string(self.h).decode()

    def check(self):
        rc = self.status()
        if rc:
            raise RxError(rc, self.error())

    def kernel_name(self):
        return self.L.selenite_rx_kernel_name(self.h).decode()

    # -- parity guard of the split-precision arithmetic ----------------------------------------
    def set_guard_ratio(self, ratio):
        rc = self.L.selenite_rx_set_guard_ratio(self.h, ratio)
        if rc:
            raise RxError(rc, "selenite_rx_set_guard_ratio")

    def guard_stats(self):
        """dict(blocks, channel_calls, rerun_channel_calls, handover_blocks) since init / the last guard_clear()."""
        b, c, r = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = self.L.selenite_rx_guard_stats(self.h, C.byref(b), C.byref(c), C.byref(r))
        if rc:
            raise RxError(rc, self.error())
        h = C.c_uint64()
        rc = self.L.selenite_rx_guard_handover(self.h, C.byref(h))
        if rc:
            raise RxError(rc, self.error())
        return dict(blocks=int(b.value), channel_calls=int(c.value), rerun_channel_calls=int(r.value), handover_blocks=int(h.value))

    def set_handover_repair(self, on):
        return self.L.selenite_rx_set_handover_repair(self.h, int(bool(on)))

    def set_auto_launches(self, launches):
        """SELENITE_ARITH_AUTO: 1 (default) = the matrix kernel recomputes a channel it guarded itself where it can (k_hilb_split16: one launch
        per call), 3 = always k_hist_exact and the rerun pass behind it.  Same bits either way."""
        return self.L.selenite_rx_set_auto_launches(self.h, int(launches))

    def auto_launches_last(self):
        """1 / 3: the form the last SELENITE_ARITH_AUTO call on a matrix kernel took (0: none yet)."""
        return int(self.L.selenite_rx_auto_launches_last(self.h))

    def guard_channels(self):
        out = np.zeros(self.cfg.channels, np.uint32)
        rc = self.L.selenite_rx_guard_channels(self.h, out.ctypes.data_as(u32p))
        if rc:
            raise RxError(rc, self.error())
        return out

    def auto_words(self):
        """Diagnostic: the per-channel words of SELENITE_ARITH_AUTO (bit 0 rerun, bits 1-2 provenance, bit 5 held by the exact kernel, ...)."""
        out = np.zeros(self.cfg.channels, np.uint32)
        rc = self.L.selenite_rx_auto_words(self.h, out.ctypes.data_as(u32p))
        if rc:
            raise RxError(rc, self.error())
        return out

    def guard_clear(self):
        return self.L.selenite_rx_guard_clear(self.h)

    def nco_path(self):
        return self.L.selenite_rx_nco_path(self.h).decode()

    def time_process(self, d_src, d_dst, block_size, iters):
        ms = C.c_float()
        rc = self.L.selenite_rx_time_process_device(self.h, d_src, d_dst, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.error())
        return ms.value

    def time_process_q15(self, d_src, d_dst, block_size, iters):
        ms = C.c_float()
        self.L.selenite_rx_time_process_q15_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                               C.c_uint32, C.POINTER(C.c_float)]
        rc = self.L.selenite_rx_time_process_q15_device(self.h, d_src, d_dst, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.error())
        return ms.value

    def time_process_each(self, d_src, d_dst, block_size, iters, q15=False):
        """per-call durations (ms) of `iters` back-to-back device calls, one HIP event between calls"""
        ms = np.zeros(iters, np.float32)
        rc = self.L.selenite_rx_time_process_each_device(self.h, d_src, d_dst, block_size, iters, _fp(ms), int(q15))
        if rc:
            raise RxError(rc, self.error())
        return ms

    def time_streaming_roof(self, d_src, d_dst, block_size, iters, q15=False):
        """per-launch durations (ms) of the no-arithmetic kernel that moves the algorithmic bytes of one call (d_dst is overwritten)"""
        ms = np.zeros(iters, np.float32)
        rc = self.L.selenite_rx_time_streaming_roof_device(self.h, d_src, d_dst, block_size, iters, _fp(ms), int(q15))
        if rc:
            raise RxError(rc, self.error())
        return ms

    def time_pattern_roof(self, d_src, d_dst, block_size, iters, q15=False, work=0):
        """per-launch durations (ms) of the no-DSP kernel with the fetch pattern and launch shape of the systolic CW kernel, `work` dependent
        vector instructions per chunk where its biquad steps are (d_dst is overwritten; CW shapes only)"""
        ms = np.zeros(iters, np.float32)
        rc = self.L.selenite_rx_time_pattern_roof_device(self.h, d_src, d_dst, block_size, iters, _fp(ms), int(q15), int(work))
        if rc:
            raise RxError(rc, self.error())
        return ms

    def synth_device(self, d_iq, first_channel, nch, first_sample, nsamp, seed):
        rc = self.L.selenite_rx_synth_iq_device(self.h, d_iq, first_channel, nch, first_sample, nsamp, seed)
        if rc:
            raise RxError(rc, self.error())

    def algorithmic_bytes(self, block_size):
        rd = C.c_uint64()
        tot = self.L.selenite_rx_algorithmic_bytes(C.byref(self.cfg), block_size, C.byref(rd))
        return int(tot), int(rd.value)

    # -- state ------------------------------------------------------------------------------
    def _state_arrays(self):
        g = self.cfg
        c = g.channels
        return dict(
            dec_state=np.zeros((c, 2, max(g.nd_taps - 1, 0)), np.float32),
            fir_state=np.zeros((c, 2, max(g.nh_taps - 1, 0)), np.float32),
            biq_state=np.zeros((c, g.n_biquad, 4), np.float32),
            agc_gain=np.zeros((c,), np.float32),
            nco_phase=np.zeros((c,), np.uint32),
        )

    @staticmethod
    def _view(arrs):
        v = StateView()
        v.dec_state = _fp(arrs["dec_state"]) if arrs["dec_state"].size else None
        v.fir_state = _fp(arrs["fir_state"]) if arrs["fir_state"].size else None
        v.biq_state = _fp(arrs["biq_state"]) if arrs["biq_state"].size else None
        v.agc_gain = _fp(arrs["agc_gain"])
        v.nco_phase = arrs["nco_phase"].ctypes.data_as(u32p)
        return v

    def state(self):
        arrs = self._state_arrays()
        v = self._view(arrs)
        rc = self.L.selenite_rx_get_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, self.error())
        return arrs

    def set_state(self, arrs):
        arrs = {k: np.ascontiguousarray(a) for k, a in arrs.items()}
        v = self._view(arrs)
        rc = self.L.selenite_rx_set_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, self.error())

    # -- NLMS noise reduction / automatic notch (selenite_rx_set_nr) --------------------------
    def set_nr(self, kind, num_taps=32, delay=16, mu=0.05, coeffs_init=None):
        """(Re)initialise the NLMS stage of every channel (NR_DENOISE / NR_NOTCH), or remove it (NR_OFF).  Raises RxError on a bad field;
        the instance is then left as it was."""
        g = NrConfig()
        g.struct_size = C.sizeof(NrConfig)
        g.kind, g.num_taps, g.delay, g.mu = int(kind), int(num_taps), int(delay), float(mu)
        w = None
        if coeffs_init is not None:
            w = np.ascontiguousarray(coeffs_init, np.float32)
            g.coeffs_init = _fp(w)
        # (a refused field leaves the old stage in place, but a failed allocation leaves NO stage: forget it until the call succeeds, and
        # on a refusal ask the library whether the old one is still there)
        old, self._nr = getattr(self, "_nr", None), None
        rc = self.L.selenite_rx_set_nr(self.h, C.byref(g))
        if rc == ARGUMENT_ERROR:
            self._nr = old
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc == ARGUMENT_ERROR else self.error())
        self._nr = (int(num_taps), int(delay)) if kind != NR_OFF else None

    def _nr_arrays(self):
        if getattr(self, "_nr", None) is None:
            raise RxError(ARGUMENT_ERROR, "the NLMS stage is off")
        n, d = self._nr
        c = self.cfg.channels
        return dict(coeffs=np.zeros((c, n), np.float32), window=np.zeros((c, n - 1), np.float32),
                    delay=np.zeros((c, d), np.float32), energy=np.zeros(c, np.float32), x0=np.zeros(c, np.float32))

    def nr_state(self):
        a = self._nr_arrays()
        v = NrStateView(*[_fp(a[k]) for k in ("coeffs", "window", "delay", "energy", "x0")])
        rc = self.L.selenite_rx_get_nr_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_get_nr_state")
        return a

    def set_nr_state(self, d):
        shapes = self._nr_arrays()
        a = {k: np.ascontiguousarray(d[k], np.float32) for k in d}
        for k in a:
            assert a[k].shape == shapes[k].shape, (k, a[k].shape)
        v = NrStateView(*[_fp(a[k]) if k in a else None for k in ("coeffs", "window", "delay", "energy", "x0")])
        rc = self.L.selenite_rx_set_nr_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_set_nr_state")

    # -- audio output stage (selenite_rx_set_out) ---------------------------------------------
    def set_out(self, interp=1, coeffs=None, frames=OUT_MONO):
        """Put the output stage behind the AGC -- arm_fir_interpolate_f32 by `interp` with `coeffs` (pCoeffs order; None with interp 1: no
        FIR, frames only), mono or stereo frames -- or remove it (interp=None).  Clears the stage's state.  Raises RxError on a bad field;
        the instance is then left as it was."""
        old, self._out = getattr(self, "_out", None), None
        if interp is None:
            rc = self.L.selenite_rx_set_out(self.h, None)
        else:
            g = OutConfig()
            g.struct_size = C.sizeof(OutConfig)
            w = np.ascontiguousarray(coeffs if coeffs is not None else [], np.float32)
            g.interp, g.ni_taps, g.frames = int(interp), int(w.size), int(frames)
            g.coeffs = _fp(w) if w.size else None
            rc = self.L.selenite_rx_set_out(self.h, C.byref(g))
        if rc in (ARGUMENT_ERROR, LENGTH_ERROR):
            self._out = old
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc in (ARGUMENT_ERROR, LENGTH_ERROR) else self.error())
        self._out = (int(interp), int(w.size) // int(interp), int(frames)) if interp is not None else None

    def out_values(self, block_size):
        """selenite_rx_out_values: values per channel a process call of block_size writes"""
        if not hasattr(self.L, "selenite_rx_out_values"):      # (an older build named by SELENITE_RX_LIB: no stage)
            return block_size // self.cfg.decim
        return int(self.L.selenite_rx_out_values(self.h, block_size))

    def _out_state_array(self):
        if getattr(self, "_out", None) is None or self._out[1] < 2:
            raise RxError(ARGUMENT_ERROR, "the output stage is off or keeps no state (phase length <= 1)")
        return np.zeros((self.cfg.channels, self._out[1] - 1), np.float32)

    def out_state(self):
        """[channels][P - 1]: the interpolator's history, oldest first"""
        a = self._out_state_array()
        rc = self.L.selenite_rx_get_out_state(self.h, _fp(a))
        if rc:
            raise RxError(rc, "selenite_rx_get_out_state")
        return a

    def set_out_state(self, state):
        a = np.ascontiguousarray(state, np.float32)
        assert a.shape == self._out_state_array().shape, a.shape
        rc = self.L.selenite_rx_set_out_state(self.h, _fp(a))
        if rc:
            raise RxError(rc, "selenite_rx_set_out_state")

    # -- spectrum tap (selenite_rx_set_spectrum) ------------------------------------------------
    def set_spectrum(self, fft_len=512, stride=1, average=0, alpha=1.0, window=None):
        """Put the spectrum tap on the raw input of every channel, or remove it (fft_len=None).  Clears the tap's state.  Raises RxError on a
        bad field; the instance is then left as it was."""
        old, self._spec = getattr(self, "_spec", None), None
        if fft_len is None:
            rc = self.L.selenite_rx_set_spectrum(self.h, None)
        else:
            g = SpecConfig()
            g.struct_size = C.sizeof(SpecConfig)
            g.fft_len, g.stride, g.average, g.alpha = int(fft_len), int(stride), int(average), float(alpha)
            w = None
            if window is not None:
                w = np.ascontiguousarray(window, np.float32)
                assert w.shape == (int(fft_len),), w.shape
                g.window = _fp(w)
            rc = self.L.selenite_rx_set_spectrum(self.h, C.byref(g))
        if rc in (ARGUMENT_ERROR, LENGTH_ERROR):
            self._spec = old
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc in (ARGUMENT_ERROR, LENGTH_ERROR) else self.error())
        self._spec = int(fft_len) if fft_len is not None else None

    def _spec_len(self):
        if getattr(self, "_spec", None) is None:
            raise RxError(ARGUMENT_ERROR, "the spectrum tap is off")
        return self._spec

    def spectrum(self):
        """(rows [channels][fft_len] display order, frames transformed so far); drains the stream"""
        rows = np.zeros((self.cfg.channels, self._spec_len()), np.float32)
        n = C.c_uint64(0)
        rc = self.L.selenite_rx_get_spectrum(self.h, _fp(rows), C.byref(n))
        if rc:
            raise RxError(rc, "selenite_rx_get_spectrum")
        return rows, int(n.value)

    def spectrum_device(self):
        """device address of the row buffer (None while the tap is off)"""
        return self.L.selenite_rx_spectrum_device(self.h)

    def spectrum_state(self):
        n, c = self._spec_len(), self.cfg.channels
        a = dict(rows=np.zeros((c, n), np.float32), pending=np.zeros((c, n, 2), np.float32), position=np.zeros(1, np.uint64))
        v = SpecStateView(_fp(a["rows"]), _fp(a["pending"]), a["position"].ctypes.data_as(u64p))
        rc = self.L.selenite_rx_get_spectrum_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_get_spectrum_state")
        return a

    def set_spectrum_state(self, d):
        n, c = self._spec_len(), self.cfg.channels
        shapes = dict(rows=(c, n), pending=(c, n, 2), position=(1,))
        a = {k: np.ascontiguousarray(d[k], np.uint64 if k == "position" else np.float32) for k in d}
        for k in a:
            assert a[k].shape == shapes[k], (k, a[k].shape)
        v = SpecStateView(_fp(a["rows"]) if "rows" in a else None, _fp(a["pending"]) if "pending" in a else None,
                          a["position"].ctypes.data_as(u64p) if "position" in a else None)
        rc = self.L.selenite_rx_set_spectrum_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_set_spectrum_state")

    # -- impulse noise blanker (selenite_rx_set_nb) ---------------------------------------------
    def set_nb(self, frame=64, guard=2, max_hits=8, threshold=8.0, alpha=0.125, clamp=2.0):
        """Put the noise blanker on the raw input of every channel, in front of the NCO, or remove it (frame=None).  Clears the blanker's
        state.  Raises RxError on a bad field; the instance is then left as it was."""
        old, self._nb = getattr(self, "_nb", None), None
        if frame is None:
            rc = self.L.selenite_rx_set_nb(self.h, None)
        else:
            g = NbConfig()
            g.struct_size = C.sizeof(NbConfig)
            g.frame, g.guard, g.max_hits = int(frame), int(guard), int(max_hits)
            g.threshold, g.alpha, g.clamp = float(threshold), float(alpha), float(clamp)
            rc = self.L.selenite_rx_set_nb(self.h, C.byref(g))
        if rc in (ARGUMENT_ERROR, LENGTH_ERROR):
            self._nb = old
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc in (ARGUMENT_ERROR, LENGTH_ERROR) else self.error())
        self._nb = int(frame) if frame is not None else None

    def nb_state(self):
        """dict(level [channels] f32, blanked [channels] u64, bursts [channels] u64); drains the stream"""
        if getattr(self, "_nb", None) is None:
            raise RxError(ARGUMENT_ERROR, "the noise blanker is off")
        c = self.cfg.channels
        a = dict(level=np.zeros(c, np.float32), blanked=np.zeros(c, np.uint64), bursts=np.zeros(c, np.uint64))
        v = NbStateView(_fp(a["level"]), a["blanked"].ctypes.data_as(u64p), a["bursts"].ctypes.data_as(u64p))
        rc = self.L.selenite_rx_get_nb_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_get_nb_state")
        return a

    def set_nb_state(self, d):
        if getattr(self, "_nb", None) is None:
            raise RxError(ARGUMENT_ERROR, "the noise blanker is off")
        a = {k: np.ascontiguousarray(d[k], np.float32 if k == "level" else np.uint64) for k in d}
        for k in a:
            assert a[k].shape == (self.cfg.channels,), (k, a[k].shape)
        v = NbStateView(_fp(a["level"]) if "level" in a else None, a["blanked"].ctypes.data_as(u64p) if "blanked" in a else None,
                        a["bursts"].ctypes.data_as(u64p) if "bursts" in a else None)
        rc = self.L.selenite_rx_set_nb_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_set_nb_state")

    # -- I/Q correction (selenite_rx_set_iqc) ----------------------------------------------------
    IQC_FLOATS = ("dc_i", "dc_q", "p", "g")

    def set_iqc(self, frame=64, alpha=1.0 / 64, dc_alpha=1.0 / 16, p_max=0.25, g_max=1.5, min_power=1e-12, p_init=0.0, g_init=1.0,
                dc_i_init=0.0, dc_q_init=0.0):
        """Put the I/Q correction (DC offset, gain and phase imbalance) on the raw input of every channel, in front of the noise blanker, or
        remove it (frame=None).  Sets the stage's state to the inits.  Raises RxError on a bad field; the instance is then left as it was."""
        old, self._iqc = getattr(self, "_iqc", None), None
        if frame is None:
            rc = self.L.selenite_rx_set_iqc(self.h, None)
        else:
            g = IqcConfig()
            g.struct_size, g.frame = C.sizeof(IqcConfig), int(frame)
            g.alpha, g.dc_alpha, g.p_max, g.g_max, g.min_power = float(alpha), float(dc_alpha), float(p_max), float(g_max), float(min_power)
            g.p_init, g.g_init, g.dc_i_init, g.dc_q_init = float(p_init), float(g_init), float(dc_i_init), float(dc_q_init)
            rc = self.L.selenite_rx_set_iqc(self.h, C.byref(g))
        if rc in (ARGUMENT_ERROR, LENGTH_ERROR):
            self._iqc = old
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc in (ARGUMENT_ERROR, LENGTH_ERROR) else self.error())
        self._iqc = int(frame) if frame is not None else None

    def iqc_state(self):
        """dict(dc_i, dc_q, p, g [channels] f32, held [channels] u64); drains the stream"""
        if getattr(self, "_iqc", None) is None:
            raise RxError(ARGUMENT_ERROR, "the I/Q correction is off")
        c = self.cfg.channels
        a = {k: np.zeros(c, np.float32) for k in self.IQC_FLOATS}
        a["held"] = np.zeros(c, np.uint64)
        v = IqcStateView(*([_fp(a[k]) for k in self.IQC_FLOATS] + [a["held"].ctypes.data_as(u64p)]))
        rc = self.L.selenite_rx_get_iqc_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_get_iqc_state")
        return a

    def set_iqc_state(self, d):
        if getattr(self, "_iqc", None) is None:
            raise RxError(ARGUMENT_ERROR, "the I/Q correction is off")
        a = {k: np.ascontiguousarray(d[k], np.uint64 if k == "held" else np.float32) for k in d}
        for k in a:
            assert a[k].shape == (self.cfg.channels,), (k, a[k].shape)
        v = IqcStateView(*([_fp(a[k]) if k in a else None for k in self.IQC_FLOATS] + [a["held"].ctypes.data_as(u64p) if "held" in a else None]))
        rc = self.L.selenite_rx_set_iqc_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_set_iqc_state")

    # -- signal-level meter and squelch (selenite_rx_set_meter) -----------------------------------
    METER_TYPES = dict(level=np.float32, open=np.uint32, hold=np.uint32, opens=np.uint64, open_blocks=np.uint64)
    METER_PTRS = dict(level=f32p, open=u32p, hold=u32p, opens=u64p, open_blocks=u64p)

    def set_meter(self, sense=SQ_ABOVE, gate=1, hang=0, attack=0.5, decay=0.125, open_level=1e-6, close_level=5e-7, level_init=0.0):
        """Put the level meter / squelch on the un-scaled audio of every channel, in front of the AGC (gate=1: closed DSP blocks leave as
        zeros, behind the AGC), or remove it (sense=None).  Sets the stage's state to level_init, closed, counters zero.  Raises RxError on
        a bad field; the instance is then left as it was."""
        old, self._meter = getattr(self, "_meter", None), None
        if sense is None:
            rc = self.L.selenite_rx_set_meter(self.h, None)
        else:
            g = MeterConfig()
            g.struct_size, g.sense, g.gate, g.hang = C.sizeof(MeterConfig), int(sense), int(gate), int(hang)
            g.attack, g.decay, g.open_level, g.close_level, g.level_init = float(attack), float(decay), float(open_level), float(close_level), float(level_init)
            rc = self.L.selenite_rx_set_meter(self.h, C.byref(g))
        if rc == ARGUMENT_ERROR:
            self._meter = old
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc == ARGUMENT_ERROR else self.error())
        self._meter = True if sense is not None else None

    def meter_state(self):
        """dict(level f32, open u32, hold u32, opens u64, open_blocks u64, each [channels]); drains the stream"""
        if getattr(self, "_meter", None) is None:
            raise RxError(ARGUMENT_ERROR, "the level meter is off")
        a = {k: np.zeros(self.cfg.channels, t) for k, t in self.METER_TYPES.items()}
        v = MeterStateView(*[a[k].ctypes.data_as(self.METER_PTRS[k]) for k in self.METER_TYPES])
        rc = self.L.selenite_rx_get_meter_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_get_meter_state")
        return a

    def set_meter_state(self, d):
        if getattr(self, "_meter", None) is None:
            raise RxError(ARGUMENT_ERROR, "the level meter is off")
        a = {k: np.ascontiguousarray(d[k], self.METER_TYPES[k]) for k in d}
        for k in a:
            assert a[k].shape == (self.cfg.channels,), (k, a[k].shape)
        v = MeterStateView(*[a[k].ctypes.data_as(self.METER_PTRS[k]) if k in a else None for k in self.METER_TYPES])
        rc = self.L.selenite_rx_set_meter_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_set_meter_state")

    def meter_level_device(self):
        """device address of the level row (None while the stage is off)"""
        return self.L.selenite_rx_meter_level_device(self.h)

    def meter_open_device(self):
        """device address of the open row (None while the stage is off)"""
        return self.L.selenite_rx_meter_open_device(self.h)

    # -- audio biquad filter (selenite_rx_set_afilt) -----------------------------------------------
    def set_afilt(self, coeffs, per_channel=False):
        """Put a biquad cascade (arm_biquad_cascade_df1_f32) on the un-scaled audio of every channel, in front of NLMS, the meter and the
        AGC, or remove it (coeffs=None).  coeffs: [n_stages][5] for all channels, or with per_channel [channels][n_stages][5]; CMSIS order
        and sign.  Clears the stage's state.  Raises RxError on a bad field; the instance is then left as it was."""
        old, self._afilt = getattr(self, "_afilt", None), None
        if coeffs is None:
            rc, new = self.L.selenite_rx_set_afilt(self.h, None), None
        else:
            a = np.ascontiguousarray(coeffs, np.float32)
            want = 3 if per_channel else 2
            if a.ndim == 1 and not per_channel and a.size == 5:
                a = a.reshape(1, 5)
            if a.ndim != want or a.shape[-1] != 5 or (per_channel and a.shape[0] != self.cfg.channels):
                self._afilt = old
                raise RxError(ARGUMENT_ERROR, "set_afilt: coeffs is not [n_stages][5] / [channels][n_stages][5]")
            g = AfiltConfig()
            g.struct_size, g.n_stages, g.per_channel, g.reserved, g.coeffs = C.sizeof(AfiltConfig), a.shape[-2], int(bool(per_channel)), 0, _fp(a)
            rc, new = self.L.selenite_rx_set_afilt(self.h, C.byref(g)), (int(a.shape[-2]), bool(per_channel))
        if rc == ARGUMENT_ERROR:
            self._afilt = old
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc == ARGUMENT_ERROR else self.error())
        self._afilt = new

    def set_afilt_coeffs(self, coeffs, first_channel=0):
        """Replace the coefficient rows of channels first_channel .. (coeffs [n][n_stages][5]; one shared set: [n_stages][5]) and keep the
        state; ordered on the instance's stream."""
        a = np.ascontiguousarray(coeffs, np.float32)
        n = a.shape[0] if a.ndim == 3 else 1
        rc = self.L.selenite_rx_set_afilt_coeffs(self.h, int(first_channel), int(n), _fp(a))
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc == ARGUMENT_ERROR else self.error())

    def _afilt_shapes(self):
        if getattr(self, "_afilt", None) is None:
            raise RxError(ARGUMENT_ERROR, "the audio filter is off")
        ns, per = self._afilt
        return (self.cfg.channels, ns, 4), ((self.cfg.channels, ns, 5) if per else (ns, 5))

    def afilt_state(self):
        """dict(state f32 [channels][n_stages][4] {x1, x2, y1, y2}, coeffs f32 as configured); drains the stream"""
        ss, cs = self._afilt_shapes()
        a = dict(state=np.zeros(ss, np.float32), coeffs=np.zeros(cs, np.float32))
        v = AfiltStateView(_fp(a["state"]), _fp(a["coeffs"]))
        rc = self.L.selenite_rx_get_afilt_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_get_afilt_state")
        return a

    def set_afilt_state(self, state):
        ss, _ = self._afilt_shapes()
        a = np.ascontiguousarray(state["state"] if isinstance(state, dict) else state, np.float32)
        assert a.shape == ss, (a.shape, ss)
        v = AfiltStateView(_fp(a), None)
        rc = self.L.selenite_rx_set_afilt_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_set_afilt_state")

    # -- tone-detector bank (selenite_rx_set_tones) --------------------------------------------------
    TONES_TYPES = dict(s=np.float32, energy=np.float32, power=np.float32, frame_energy=np.float32, last_best=np.uint32, tone=np.uint32,
                       cand=np.uint32, run=np.uint32, changes=np.uint64, position=np.uint64)
    TONES_PTRS = dict(s=f32p, energy=f32p, power=f32p, frame_energy=f32p, last_best=u32p, tone=u32p, cand=u32p, run=u32p, changes=u64p,
                      position=u64p)

    def set_tones(self, coeffs, frame_blocks=1, confirm=1, release=1, ratio=0.0, min_power=0.0):
        """Put the tone-detector bank on the un-scaled audio of every channel (a tap in front of the audio filter, NLMS, the meter and the
        AGC), or remove it (coeffs=None).  coeffs: [K][3] {2 cos w, cos w, sin w} (design_tones).  Puts the stage's state at its start.
        Raises RxError on a bad field; the instance is then left as it was."""
        old, self._tones = getattr(self, "_tones", None), None
        if coeffs is None:
            rc, new = self.L.selenite_rx_set_tones(self.h, None), None
        else:
            a = np.ascontiguousarray(coeffs, np.float32)
            if a.ndim != 2 or a.shape[1] != 3:
                self._tones = old
                raise RxError(ARGUMENT_ERROR, "set_tones: coeffs is not [n_tones][3]")
            g = TonesConfig()
            g.struct_size, g.n_tones, g.frame_blocks, g.confirm, g.release, g.reserved = C.sizeof(TonesConfig), a.shape[0], int(frame_blocks), int(confirm), int(release), 0
            g.ratio, g.min_power, g.coeffs = float(ratio), float(min_power), _fp(a)
            rc, new = self.L.selenite_rx_set_tones(self.h, C.byref(g)), int(a.shape[0])
        if rc == ARGUMENT_ERROR:
            self._tones = old
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc == ARGUMENT_ERROR else self.error())
        self._tones = new

    def _tones_shapes(self):
        if getattr(self, "_tones", None) is None:
            raise RxError(ARGUMENT_ERROR, "the tone detector is off")
        ch, k = self.cfg.channels, self._tones
        return dict(s=(ch, k, 2), energy=(ch,), power=(ch, k), frame_energy=(ch,), last_best=(ch,), tone=(ch,), cand=(ch,), run=(ch,),
                    changes=(ch,), position=(1,))

    def tones_state(self):
        """dict(s f32 [channels][K][2], energy, frame_energy f32 [channels], power f32 [channels][K], last_best, tone, cand, run u32
        [channels], changes u64 [channels], position u64 [1]); drains the stream"""
        a = {k: np.zeros(sh, self.TONES_TYPES[k]) for k, sh in self._tones_shapes().items()}
        v = TonesStateView(*[a[k].ctypes.data_as(self.TONES_PTRS[k]) for k in self.TONES_TYPES])
        rc = self.L.selenite_rx_get_tones_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_get_tones_state")
        return a

    def set_tones_state(self, d):
        sh = self._tones_shapes()
        a = {k: np.ascontiguousarray(d[k], self.TONES_TYPES[k]) for k in d}
        for k in a:
            assert a[k].shape == sh[k], (k, a[k].shape, sh[k])
        v = TonesStateView(*[a[k].ctypes.data_as(self.TONES_PTRS[k]) if k in a else None for k in self.TONES_TYPES])
        rc = self.L.selenite_rx_set_tones_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_set_tones_state")

    def tones(self):
        """(tone u32 [channels], power f32 [channels][K] of the last whole frame, whole frames since set_tones / reset); drains the stream"""
        sh = self._tones_shapes()
        tone, power, frames = np.zeros(sh["tone"], np.uint32), np.zeros(sh["power"], np.float32), C.c_uint64(0)
        rc = self.L.selenite_rx_get_tones(self.h, tone.ctypes.data_as(u32p), _fp(power), C.byref(frames))
        if rc:
            raise RxError(rc, "selenite_rx_get_tones")
        return tone, power, int(frames.value)

    def tones_tone_device(self):
        """device address of the tone row (None while the stage is off)"""
        return self.L.selenite_rx_tones_tone_device(self.h)

    def tones_power_device(self):
        """device address of the power rows (None while the stage is off)"""
        return self.L.selenite_rx_tones_power_device(self.h)

    # -- Morse decoder (selenite_rx_set_cwdec) ----------------------------------------------------------
    CWDEC_TYPES = dict(peak=np.float32, floor=np.float32, primed=np.uint32, key=np.uint32, flip=np.uint32, run=np.uint32, unit=np.uint32,
                       code=np.uint32, word=np.uint32, count=np.uint64, text=np.uint8)
    CWDEC_PTRS = dict(peak=f32p, floor=f32p, primed=u32p, key=u32p, flip=u32p, run=u32p, unit=u32p, code=u32p, word=u32p, count=u64p, text=u8p)

    def set_cwdec(self, on=True, table=None, **par):
        """Put the Morse decoder on the un-scaled audio of every channel (a tap at the tone bank's place: it changes no audio), or remove
        it (set_cwdec(None)).  par: the fields of selenite_rx_cwdec_config; the defaults are CWDEC_DEFAULTS: peak_attack 0.5, peak_decay
        0.002, floor_attack 0.25, floor_decay 0.002, on_frac 0.4, off_frac 0.25, snr 4, min_power 1e-8, debounce 2, adapt 1, track 2,
        unit_min 2 * 256, unit_init 10 * 256, unit_max 64 * 256 (Q8 DSP blocks), ring 256.  table: uint8 [256] (None: morse_table()).
        Puts the stage's state at its start.  Raises RxError on a bad field; the instance is then left as it was."""
        old, self._cwdec = getattr(self, "_cwdec", None), None
        if on is None or on is False:
            rc, new = self.L.selenite_rx_set_cwdec(self.h, None), None
        else:
            unknown = set(par) - set(CWDEC_DEFAULTS)
            if unknown:
                self._cwdec = old
                raise TypeError("set_cwdec: unknown fields %s" % sorted(unknown))
            p = dict(CWDEC_DEFAULTS, **par)
            g = CwdecConfig()
            g.struct_size = C.sizeof(CwdecConfig)
            for k, v in p.items():
                setattr(g, k, float(v) if isinstance(CWDEC_DEFAULTS[k], float) else int(v))
            t = None
            if table is not None:
                t = np.ascontiguousarray(table, np.uint8)
                if t.shape != (256,):
                    self._cwdec = old
                    raise RxError(ARGUMENT_ERROR, "set_cwdec: table is not [256]")
                g.table = t.ctypes.data_as(u8p)
            rc, new = self.L.selenite_rx_set_cwdec(self.h, C.byref(g)), int(p["ring"])
        if rc == ARGUMENT_ERROR:
            self._cwdec = old
        if rc:
            raise RxError(rc, self.L.selenite_rx_error_string(None).decode() if rc == ARGUMENT_ERROR else self.error())
        self._cwdec = new

    def _cwdec_shapes(self):
        if getattr(self, "_cwdec", None) is None:
            raise RxError(ARGUMENT_ERROR, "the Morse decoder is off")
        ch = self.cfg.channels
        return {k: ((ch, self._cwdec) if k == "text" else (ch,)) for k in self.CWDEC_TYPES}

    def cwdec_state(self):
        """dict(peak, floor f32; primed, key, flip, run, unit, code, word u32; count u64, each [channels]; text u8 [channels][ring]); drains
        the stream"""
        a = {k: np.zeros(sh, self.CWDEC_TYPES[k]) for k, sh in self._cwdec_shapes().items()}
        v = CwdecStateView(*[a[k].ctypes.data_as(self.CWDEC_PTRS[k]) for k in self.CWDEC_TYPES])
        rc = self.L.selenite_rx_get_cwdec_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_get_cwdec_state")
        return a

    def set_cwdec_state(self, d):
        sh = self._cwdec_shapes()
        a = {k: np.ascontiguousarray(d[k], self.CWDEC_TYPES[k]) for k in d}
        for k in a:
            assert a[k].shape == sh[k], (k, a[k].shape, sh[k])
        v = CwdecStateView(*[a[k].ctypes.data_as(self.CWDEC_PTRS[k]) if k in a else None for k in self.CWDEC_TYPES])
        rc = self.L.selenite_rx_set_cwdec_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_rx_set_cwdec_state")

    def cwdec(self):
        """(text u8 [channels][ring], count u64, unit u32, key u32 [channels]): selenite_rx_get_cwdec; drains the stream"""
        sh = self._cwdec_shapes()
        text, count = np.zeros(sh["text"], np.uint8), np.zeros(sh["count"], np.uint64)
        unit, key = np.zeros(sh["unit"], np.uint32), np.zeros(sh["key"], np.uint32)
        rc = self.L.selenite_rx_get_cwdec(self.h, text.ctypes.data_as(u8p), count.ctypes.data_as(u64p), unit.ctypes.data_as(u32p),
                                          key.ctypes.data_as(u32p))
        if rc:
            raise RxError(rc, "selenite_rx_get_cwdec")
        return text, count, unit, key

    def cw_text(self, channel=None):
        """the last min(count, ring) characters of a channel in order, as str; channel=None: a list for all channels.  Drains the stream."""
        text, count, _, _ = self.cwdec()
        out = [ring_text(text[c], int(count[c])) for c in (range(self.cfg.channels) if channel is None else [channel])]
        return out if channel is None else out[0]

    def cw_unit(self):
        """the dit length of every channel in DSP blocks (unit / 256), float64 [channels]; drains the stream"""
        return self.cwdec()[2].astype(np.float64) / 256.0

    def cwdec_text_device(self):
        """device address of the rings, u8 [channels][ring] (None while the stage is off)"""
        return self.L.selenite_rx_cwdec_text_device(self.h)

    def cwdec_count_device(self):
        """device address of the count row, u64 [channels] (None while the stage is off)"""
        return self.L.selenite_rx_cwdec_count_device(self.h)

    def cwdec_unit_device(self):
        """device address of the unit row, u32 [channels] (None while the stage is off)"""
        return self.L.selenite_rx_cwdec_unit_device(self.h)

    def close(self):
        if self.h:
            self.L.selenite_rx_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RingStateView(C.Structure):
    """struct selenite_ring_state_view."""
    _fields_ = [("i", C.POINTER(C.c_int16)), ("q", C.POINTER(C.c_int16)), ("buff_enable", C.POINTER(C.c_uint8)),
                ("rd_ptr", C.POINTER(C.c_uint16)), ("wr_ptr", C.POINTER(C.c_uint16))]


class Ring:
    """`channels` reference DSP_Buff_TypeDef rings in HBM (include/selenite_ring.h; dsp_if.c:83-340).
    Method names and size units follow the reference functions they replace."""

    def __init__(self, channels, frames=384):
        self.L = lib()
        L = self.L
        vp = C.c_void_p
        L.selenite_ring_init.argtypes = [C.POINTER(vp), C.c_uint32, C.c_uint32]
        L.selenite_ring_free.argtypes = [vp]
        L.selenite_ring_status.argtypes = [vp]
        L.selenite_ring_error_string.argtypes = [vp]
        L.selenite_ring_error_string.restype = C.c_char_p
        L.selenite_ring_set_stream.argtypes = [vp, vp]
        L.selenite_ring_sync.argtypes = [vp]
        for n, a in (("in_write", C.c_uint16), ("in_read", C.c_uint32), ("out_write", C.c_uint32), ("out_read", C.c_uint16)):
            getattr(L, "selenite_ring_%s" % n).argtypes = [vp, vp, a]
            getattr(L, "selenite_ring_%s" % n).restype = None
            getattr(L, "selenite_ring_%s_device" % n).argtypes = [vp, vp, a]
            getattr(L, "selenite_ring_%s_device" % n).restype = None
        L.selenite_ring_mute.argtypes = [vp]
        L.selenite_ring_mute.restype = None
        L.selenite_ring_get_state.argtypes = [vp, C.POINTER(RingStateView)]
        L.selenite_ring_set_state.argtypes = [vp, C.POINTER(RingStateView)]
        L.selenite_ring_time_device.argtypes = [vp, vp, vp, C.c_uint16, C.c_uint32, C.POINTER(C.c_float)]
        self.channels, self.frames = int(channels), int(frames)
        self.h = vp()
        rc = L.selenite_ring_init(C.byref(self.h), self.channels, self.frames)
        if rc:
            raise RxError(rc, "selenite_ring_init failed (no GPU, or bad channels/frames)")

    def check(self):
        rc = self.L.selenite_ring_status(self.h)
        if rc:
            raise RxError(rc, self.L.selenite_ring_error_string(self.h).decode())

    def _packet(self, arr, words):
        arr = np.ascontiguousarray(arr, np.int16)
        assert arr.shape == (self.channels, words), arr.shape
        return arr

    def in_write(self, pkt):                       # DSP_In_Buff_Write (words)
        pkt = np.ascontiguousarray(pkt, np.int16)
        self.L.selenite_ring_in_write(self.h, self._packet(pkt, pkt.shape[1]).ctypes.data, pkt.shape[1])
        self.check()

    def out_write(self, pkt):                      # DSP_Out_Buff_Write (bytes)
        pkt = np.ascontiguousarray(pkt, np.int16)
        self.L.selenite_ring_out_write(self.h, self._packet(pkt, pkt.shape[1]).ctypes.data, 2 * pkt.shape[1])
        self.check()

    def in_read(self, size_bytes):                 # DSP_In_Buff_Read (bytes)
        out = np.empty((self.channels, size_bytes // 2), np.int16)
        self.L.selenite_ring_in_read(self.h, out.ctypes.data, size_bytes)
        self.check()
        return out

    def out_read(self, size_words):                # DSP_Out_Buff_Read (words)
        out = np.empty((self.channels, size_words), np.int16)
        self.L.selenite_ring_out_read(self.h, out.ctypes.data, size_words)
        self.check()
        return out

    def mute(self):
        self.L.selenite_ring_mute(self.h)
        self.L.selenite_ring_sync(self.h)
        self.check()

    def _arrays(self):
        return {"i": np.zeros((self.channels, self.frames), np.int16),
                "q": np.zeros((self.channels, self.frames), np.int16),
                "buff_enable": np.zeros(self.channels, np.uint8),
                "rd_ptr": np.zeros(self.channels, np.uint16),
                "wr_ptr": np.zeros(self.channels, np.uint16)}

    @staticmethod
    def _view(a):
        return RingStateView(a["i"].ctypes.data_as(C.POINTER(C.c_int16)), a["q"].ctypes.data_as(C.POINTER(C.c_int16)),
                             a["buff_enable"].ctypes.data_as(C.POINTER(C.c_uint8)),
                             a["rd_ptr"].ctypes.data_as(C.POINTER(C.c_uint16)),
                             a["wr_ptr"].ctypes.data_as(C.POINTER(C.c_uint16)))

    def state(self):
        a = self._arrays()
        v = self._view(a)
        rc = self.L.selenite_ring_get_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, self.L.selenite_ring_error_string(self.h).decode())
        return a

    def set_state(self, a):
        a = {k: np.ascontiguousarray(v) for k, v in a.items()}
        v = self._view(a)
        rc = self.L.selenite_ring_set_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, self.L.selenite_ring_error_string(self.h).decode())

    def time_pair(self, d_src, d_dst, size_words, iters):
        ms = C.c_float()
        rc = self.L.selenite_ring_time_device(self.h, d_src, d_dst, size_words, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.L.selenite_ring_error_string(self.h).decode())
        return ms.value

    def close(self):
        if self.h:
            self.L.selenite_ring_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tx:
    """One batched TX chain instance (include/selenite_tx.h); mirror of Rx."""

    def __init__(self, cfg):
        self.L = lib()
        L = self.L
        vp = C.c_void_p
        L.selenite_tx_init.argtypes = [C.POINTER(vp), C.POINTER(TxConfig)]
        L.selenite_tx_free.argtypes = [vp]
        L.selenite_tx_set_mode.argtypes = [vp, C.c_uint8]
        L.selenite_tx_status.argtypes = [vp]
        L.selenite_tx_error_string.argtypes = [vp]
        L.selenite_tx_error_string.restype = C.c_char_p
        for n in ("process_f32", "process_q15", "process_f32_device", "process_q15_device"):
            getattr(L, "selenite_tx_" + n).argtypes = [vp, vp, vp, C.c_uint32]
            getattr(L, "selenite_tx_" + n).restype = None
        L.selenite_tx_set_stream.argtypes = [vp, vp]
        L.selenite_tx_sync.argtypes = [vp]
        L.selenite_tx_get_state.argtypes = [vp, C.POINTER(TxStateView)]
        L.selenite_tx_set_state.argtypes = [vp, C.POINTER(TxStateView)]
        L.selenite_tx_reset.argtypes = [vp]
        L.selenite_tx_time_process_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        self.cfg = cfg
        self.h = vp()
        rc = L.selenite_tx_init(C.byref(self.h), C.byref(cfg))
        if rc:
            raise RxError(rc, "selenite_tx_init failed")

    def check(self):
        rc = self.L.selenite_tx_status(self.h)
        if rc:
            raise RxError(rc, self.L.selenite_tx_error_string(self.h).decode())

    def process(self, audio):
        audio = np.ascontiguousarray(audio, np.float32)
        c, bs = audio.shape
        out = np.empty((c, bs * self.cfg.interp, 2), np.float32)
        self.L.selenite_tx_process_f32(self.h, audio.ctypes.data, out.ctypes.data, bs)
        self.check()
        return out

    def process_q15(self, audio):
        audio = np.ascontiguousarray(audio, np.int16)
        c, bs = audio.shape
        out = np.empty((c, bs * self.cfg.interp, 2), np.int16)
        self.L.selenite_tx_process_q15(self.h, audio.ctypes.data, out.ctypes.data, bs)
        self.check()
        return out

    def process_device(self, d_src, d_dst, block_size):
        self.L.selenite_tx_process_f32_device(self.h, d_src, d_dst, block_size)

    def kernel_name(self):
        self.L.selenite_tx_kernel_name.argtypes = [C.c_void_p]
        self.L.selenite_tx_kernel_name.restype = C.c_char_p
        return self.L.selenite_tx_kernel_name(self.h).decode()

    def set_mode(self, mode):
        return self.L.selenite_tx_set_mode(self.h, mode)

    def sync(self):
        return self.L.selenite_tx_sync(self.h)

    def reset(self):
        return self.L.selenite_tx_reset(self.h)

    def _arrays(self):
        g = self.cfg
        return {"fir_state": np.zeros((g.channels, 2, max(g.nh_taps - 1, 0)), np.float32),
                "interp_state": np.zeros((g.channels, 2, max(g.ni_taps // g.interp - 1, 0) if g.ni_taps else 0), np.float32),
                "alc_gain": np.zeros(g.channels, np.float32), "nco_phase": np.zeros(g.channels, np.uint32)}

    @staticmethod
    def _view(a):
        v = TxStateView()
        v.fir_state = a["fir_state"].ctypes.data_as(f32p) if a["fir_state"].size else None
        v.interp_state = a["interp_state"].ctypes.data_as(f32p) if a["interp_state"].size else None
        v.alc_gain = a["alc_gain"].ctypes.data_as(f32p)
        v.nco_phase = a["nco_phase"].ctypes.data_as(u32p)
        return v

    def state(self):
        a = self._arrays()
        v = self._view(a)
        rc = self.L.selenite_tx_get_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, self.L.selenite_tx_error_string(self.h).decode())
        return a

    def set_state(self, a):
        a = {k: np.ascontiguousarray(x) for k, x in a.items()}
        v = self._view(a)
        rc = self.L.selenite_tx_set_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, self.L.selenite_tx_error_string(self.h).decode())

    def set_fm(self, deviation=0.25, amplitude=1.0, tone_level=0.0, tone_step=None, tone_enable=None):
        """FM transmit mode (selenite_tx_set_fm; then set_mode(MODE_FM)).  tone_step: None (no tone), one phase increment per output
        sample for every channel, or an array [channels]; tone_enable defaults to `tone_step is not None`.  Returns the status code."""
        g = TxFmConfig()
        g.struct_size, g.deviation, g.amplitude, g.tone_level, g.reserved = C.sizeof(TxFmConfig), deviation, amplitude, tone_level, 0
        g.tone_enable = int(tone_step is not None) if tone_enable is None else int(tone_enable)
        steps = None
        if tone_step is not None and np.ndim(tone_step):
            steps = np.ascontiguousarray(tone_step, np.uint32)
            if steps.shape != (self.cfg.channels,):
                raise ValueError("tone_step: one value or [channels]")
            g.tone_step = steps.ctypes.data_as(u32p)
        elif tone_step is not None:
            g.tone_step_all = int(tone_step)
        return self.L.selenite_tx_set_fm(self.h, C.byref(g))

    def clear_fm(self):
        """selenite_tx_set_fm(S, NULL): FM off again (ARGUMENT_ERROR while the mode is FM)"""
        return self.L.selenite_tx_set_fm(self.h, None)

    def fm_state(self):
        a = {"tone_phase": np.zeros(self.cfg.channels, np.uint32)}
        v = TxFmStateView()
        v.tone_phase = a["tone_phase"].ctypes.data_as(u32p)
        rc = self.L.selenite_tx_get_fm_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_tx_get_fm_state: FM is not configured (set_fm)")
        return a

    def set_fm_state(self, a):
        tp = np.ascontiguousarray(a["tone_phase"], np.uint32)
        if tp.shape != (self.cfg.channels,):
            raise ValueError("tone_phase: [channels]")
        v = TxFmStateView()
        v.tone_phase = tp.ctypes.data_as(u32p)
        rc = self.L.selenite_tx_set_fm_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_tx_set_fm_state: FM is not configured (set_fm)")

    def set_cw(self, shape, amplitude=1.0, offset_step=0, side_level=0.0, side_step=0, side_mix=0, hang_blocks=0):
        """the keyed CW path (selenite_tx_set_cw; valid while the mode is MODE_CW or MODE_CWR).  shape: the keying taps (sr.keyshape);
        offset_step: the pitch as a phase increment per OUTPUT sample; side_step: per AUDIO sample, one value or [channels].
        Returns the status code."""
        g = TxCwConfig()
        taps = np.ascontiguousarray(shape, np.float32).reshape(-1)
        g.struct_size, g.ns_taps, g.shape_coeffs = C.sizeof(TxCwConfig), taps.size, taps.ctypes.data_as(f32p)
        g.amplitude, g.offset_step, g.side_level, g.side_mix, g.hang_blocks, g.reserved = amplitude, int(offset_step), side_level, int(side_mix), int(hang_blocks), 0
        steps = None
        if np.ndim(side_step):
            steps = np.ascontiguousarray(side_step, np.uint32)
            if steps.shape != (self.cfg.channels,):
                raise ValueError("side_step: one value or [channels]")
            g.side_step = steps.ctypes.data_as(u32p)
        else:
            g.side_step_all = int(side_step)
        rc = self.L.selenite_tx_set_cw(self.h, C.byref(g))
        if rc == 0:
            self._cw_ns = taps.size
        return rc

    def clear_cw(self):
        """selenite_tx_set_cw(S, NULL): keyed CW off again"""
        return self.L.selenite_tx_set_cw(self.h, None)

    def process_key(self, d_key, d_iq, d_side, block_size, q15=False):
        """key states [channels][block_size] uint8 -> I/Q [channels][block_size * interp][2] and, unless d_side is None, the sidetone
        [channels][block_size]; device pointers (f32, or int16 with q15=True), asynchronous.  Returns the status code."""
        f = self.L.selenite_tx_process_key_q15_device if q15 else self.L.selenite_tx_process_key_f32_device
        return f(self.h, d_key, d_iq, d_side, block_size)

    def process_key_host(self, key, side=None, q15=False):
        """the host entries: key [channels][n] uint8 -> (status, I/Q, sidetone or None); `side` is the buffer the sidetone is written or
        mixed into (a copy is returned)"""
        key = np.ascontiguousarray(key, np.uint8)
        c, bs = key.shape
        dt = np.int16 if q15 else np.float32
        out = np.zeros((c, bs * self.cfg.interp, 2), dt)
        sd = None if side is None else np.array(side, dt, order="C")
        f = self.L.selenite_tx_process_key_q15 if q15 else self.L.selenite_tx_process_key_f32
        rc = f(self.h, key.ctypes.data, out.ctypes.data, None if sd is None else sd.ctypes.data, bs)
        return rc, out, sd

    def _cw_arrays(self):
        c = self.cfg.channels
        return {"key_state": np.zeros((c, getattr(self, "_cw_ns", 1) - 1), np.uint8), "side_phase": np.zeros(c, np.uint32),
                "tx_on": np.zeros(c, np.uint32), "hold": np.zeros(c, np.uint32)}

    @staticmethod
    def _cw_view(a):
        v = TxCwStateView()
        v.key_state = a["key_state"].ctypes.data_as(C.POINTER(C.c_uint8)) if "key_state" in a and a["key_state"].size else None
        for k in ("side_phase", "tx_on", "hold"):
            setattr(v, k, a[k].ctypes.data_as(u32p) if k in a else None)
        return v

    def cw_state(self):
        a = self._cw_arrays()
        v = self._cw_view(a)
        rc = self.L.selenite_tx_get_cw_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_tx_get_cw_state: keyed CW is not configured (set_cw)")
        return a

    def set_cw_state(self, a):
        """members that are missing from `a` are left as they are"""
        want = self._cw_arrays()
        a = {k: np.ascontiguousarray(a[k], want[k].dtype) for k in want if k in a}
        for k, x in a.items():
            if x.shape != want[k].shape:
                raise ValueError("%s: %s expected" % (k, want[k].shape))
        v = self._cw_view(a)
        rc = self.L.selenite_tx_set_cw_state(self.h, C.byref(v))
        if rc:
            raise RxError(rc, "selenite_tx_set_cw_state: keyed CW is not configured (set_cw)")

    def cw_txon(self):
        """device pointer of the break-in flags, uint32 [channels] (None before set_cw)"""
        return self.L.selenite_tx_cw_txon_device(self.h)

    def time_process_key(self, d_key, d_iq, d_side, block_size, iters):
        ms = C.c_float()
        rc = self.L.selenite_tx_time_process_key_device(self.h, d_key, d_iq, d_side, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.L.selenite_tx_error_string(self.h).decode())
        return ms.value

    def set_in(self, M=1, coeffs=None, pick=IN_MONO, gain=1.0, vox=None):
        """the audio input stage (selenite_tx_set_in): slot-rate frames -> pick -> gain -> arm_fir_decimate_f32 by M -> VOX -> the chain.
        coeffs: the decimator's taps in CMSIS order (None or empty: no FIR, M = 1 only); vox: None (off) or a dict of
        selenite_rx_meter_config fields (gate, hang, attack, decay, open_level, close_level, level_init; sense defaults to SQ_ABOVE).
        Returns the status code."""
        g = TxInConfig()
        taps = np.zeros(0, np.float32) if coeffs is None else np.ascontiguousarray(coeffs, np.float32).reshape(-1)
        g.struct_size, g.M, g.nd_taps, g.pick, g.gain, g.reserved = C.sizeof(TxInConfig), int(M), taps.size, int(pick), gain, 0
        g.coeffs = taps.ctypes.data_as(f32p) if taps.size else None
        if vox is not None:
            v = dict(sense=SQ_ABOVE, gate=0, hang=0, attack=0.5, decay=0.125, open_level=1e-6, close_level=5e-7, level_init=0.0)
            v.update(vox)
            g.vox = 1
            g.meter.struct_size = C.sizeof(MeterConfig)
            for k, x in v.items():
                setattr(g.meter, k, x)
        rc = self.L.selenite_tx_set_in(self.h, C.byref(g))
        if rc == 0:
            self._in_nt, self._in_M, self._in_fw = taps.size, int(M), 1 if int(pick) == IN_MONO else 2
        return rc

    def clear_in(self):
        """selenite_tx_set_in(S, NULL): the input stage off again"""
        return self.L.selenite_tx_set_in(self.h, None)

    def process_frames(self, d_frames, d_iq, block_size, kind=IN_F32):
        """frames [channels][block_size * M * (1 or 2)] -> I/Q [channels][block_size * interp][2]; device pointers, asynchronous.
        kind: IN_F32 (f32 frames, f32 I/Q), IN_Q15 (int16, int16) or IN_Q15_F32 (int16 frames, f32 I/Q).  Returns the status code."""
        f = (self.L.selenite_tx_process_frames_f32_device, self.L.selenite_tx_process_frames_q15_device,
             self.L.selenite_tx_process_frames_q15_f32_device)[kind]
        return f(self.h, d_frames, d_iq, block_size)

    def process_frames_host(self, frames, q15=False):
        """the host entries: frames [channels][n * M * (1 or 2)] -> (status, I/Q)"""
        dt = np.int16 if q15 else np.float32
        frames = np.ascontiguousarray(frames, dt)
        c = frames.shape[0]
        bs = frames[0].size // (getattr(self, "_in_M", 1) * getattr(self, "_in_fw", 1))
        out = np.zeros((c, bs * self.cfg.interp, 2), dt)
        f = self.L.selenite_tx_process_frames_q15 if q15 else self.L.selenite_tx_process_frames_f32
        rc = f(self.h, frames.ctypes.data, out.ctypes.data, bs)
        return rc, out

    def _in_arrays(self):
        c = self.cfg.channels
        return {"dec_state": np.zeros((c, max(getattr(self, "_in_nt", 0) - 1, 0)), np.float32), "level": np.zeros(c, np.float32),
                "open": np.zeros(c, np.uint32), "hold": np.zeros(c, np.uint32), "opens": np.zeros(c, np.uint64),
                "open_blocks": np.zeros(c, np.uint64)}

    @staticmethod
    def _in_view(a):
        v = TxInStateView()
        for k, t in (("dec_state", f32p), ("level", f32p), ("open", u32p), ("hold", u32p), ("opens", u64p), ("open_blocks", u64p)):
            setattr(v, k, a[k].ctypes.data_as(t) if k in a and a[k].size else None)
        return v

    def in_state(self):
        a = self._in_arrays()
        rc = self.L.selenite_tx_get_in_state(self.h, C.byref(self._in_view(a)))
        if rc:
            raise RxError(rc, "selenite_tx_get_in_state: the input stage is not configured (set_in)")
        return a

    def set_in_state(self, a):
        """members that are missing from `a` are left as they are"""
        want = self._in_arrays()
        a = {k: np.ascontiguousarray(a[k], want[k].dtype) for k in want if k in a}
        for k, x in a.items():
            if x.shape != want[k].shape:
                raise ValueError("%s: %s expected" % (k, want[k].shape))
        rc = self.L.selenite_tx_set_in_state(self.h, C.byref(self._in_view(a)))
        if rc:
            raise RxError(rc, "selenite_tx_set_in_state: the input stage is not configured (set_in)")

    def in_vox(self):
        """device pointer of the VOX flags, uint32 [channels] (None before set_in)"""
        return self.L.selenite_tx_in_vox_device(self.h)

    def in_audio_device(self):
        """device pointer of the stage's output of the last frame call, [channels][block_size] in the entry's audio type (None before it)"""
        return self.L.selenite_tx_in_audio_device(self.h)

    def time_in_stage(self, d_frames, block_size, iters, kind=IN_F32):
        """mean ms of the stage kernel alone over `iters` launches"""
        ms = C.c_float()
        rc = self.L.selenite_tx_time_in_stage_device(self.h, d_frames, kind, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.L.selenite_tx_error_string(self.h).decode())
        return ms.value

    def set_keyer(self, mode=KEYER_IAMBIC_B, unit=720, ring=256, codes=None, reserved=0):
        """the keyer stage in front of the keyed CW path (selenite_tx_set_keyer; needs set_cw).  unit: audio samples per dit, one value
        or [channels]; ring: text bytes per channel; codes: morse_codes() of another table, None = the built-in one.  Returns the status code."""
        g = TxKeyerConfig()
        g.struct_size, g.mode, g.ring, g.reserved = C.sizeof(TxKeyerConfig), int(mode), int(ring), int(reserved)
        units = table = None
        if np.ndim(unit):
            units = np.ascontiguousarray(unit, np.uint32)
            if units.shape != (self.cfg.channels,):
                raise ValueError("unit: one value or [channels]")
            g.unit = units.ctypes.data_as(u32p)
        else:
            g.unit_all = int(unit)
        if codes is not None:
            table = np.ascontiguousarray(codes, np.uint8)
            if table.shape != (256,):
                raise ValueError("codes: uint8 [256]")
            g.codes = table.ctypes.data_as(C.POINTER(C.c_uint8))
        rc = self.L.selenite_tx_set_keyer(self.h, C.byref(g))
        if rc == 0:
            self._keyer_ring = int(ring)
        return rc

    def clear_keyer(self):
        """selenite_tx_set_keyer(S, NULL): the keyer off again"""
        return self.L.selenite_tx_set_keyer(self.h, None)

    def keyer_send(self, text, first_channel=0, n_channels=None):
        """queue text: one str / bytes for every channel of the range, or a list of n_channels texts of one length.  Returns the status
        code (LENGTH_ERROR: a channel lacks room; nothing was written)."""
        n = self.cfg.channels - first_channel if n_channels is None else int(n_channels)
        enc = lambda x: x.encode("latin-1") if isinstance(x, str) else bytes(x)
        if isinstance(text, (str, bytes, bytearray)):
            buf, per = np.frombuffer(enc(text), np.uint8), 0
            ln = buf.size
        else:
            rows = [enc(x) for x in text]
            if len(rows) != n or any(len(r) != len(rows[0]) for r in rows):
                raise ValueError("keyer_send: n_channels texts of one length")
            buf, per, ln = np.frombuffer(b"".join(rows), np.uint8), 1, len(rows[0])
        return self.L.selenite_tx_keyer_send(self.h, int(first_channel), n, buf.ctypes.data if buf.size else None, ln, per)

    def keyer_pending(self):
        """characters queued and not yet begun, uint32 [channels]"""
        a = np.zeros(self.cfg.channels, np.uint32)
        rc = self.L.selenite_tx_keyer_pending(self.h, a.ctypes.data_as(u32p))
        if rc:
            raise RxError(rc, "selenite_tx_keyer_pending: the keyer is not configured (set_keyer)")
        return a

    def process_paddles(self, d_paddles, d_iq, d_side, block_size, q15=False):
        """paddle bytes [channels][block_size] uint8 (bit 0 dit, bit 1 dah, bit 2 straight key; None: the text memory alone) -> the keyer
        -> the keyed CW path: I/Q and sidetone as process_key writes them; device pointers, asynchronous.  Returns the status code."""
        f = self.L.selenite_tx_process_paddles_q15_device if q15 else self.L.selenite_tx_process_paddles_f32_device
        return f(self.h, d_paddles, d_iq, d_side, block_size)

    def process_paddles_host(self, paddles, block_size=None, side=None, q15=False):
        """the host entries: paddles [channels][n] uint8, or None with block_size -> (status, I/Q, sidetone or None)"""
        if paddles is not None:
            paddles = np.ascontiguousarray(paddles, np.uint8)
            block_size = paddles.shape[1]
        c, bs = self.cfg.channels, int(block_size)
        dt = np.int16 if q15 else np.float32
        out = np.zeros((c, bs * self.cfg.interp, 2), dt)
        sd = None if side is None else np.array(side, dt, order="C")
        f = self.L.selenite_tx_process_paddles_q15 if q15 else self.L.selenite_tx_process_paddles_f32
        rc = f(self.h, None if paddles is None else paddles.ctypes.data, out.ctypes.data, None if sd is None else sd.ctypes.data, bs)
        return rc, out, sd

    def keyer_run(self, d_paddles, d_key, block_size):
        """the stage alone: key bytes [channels][block_size] into d_key; device pointers, asynchronous.  Returns the status code."""
        return self.L.selenite_tx_keyer_run_device(self.h, d_paddles, d_key, block_size)

    def keyer_key_device(self):
        """device pointer of the key bytes of the last paddle call, uint8 [channels][block_size] (None before it)"""
        return self.L.selenite_tx_keyer_key_device(self.h)

    def _keyer_arrays(self):
        c = self.cfg.channels
        a = {k: np.zeros(c, np.uint32) for k in KEYER_STATE_WORDS}
        a["text"] = np.zeros((c, getattr(self, "_keyer_ring", 1)), np.uint8)
        return a

    @staticmethod
    def _keyer_view(a):
        v = TxKeyerStateView()
        for k in KEYER_STATE_WORDS:
            setattr(v, k, a[k].ctypes.data_as(u32p) if k in a else None)
        v.text = a["text"].ctypes.data_as(C.POINTER(C.c_uint8)) if "text" in a else None
        return v

    def keyer_state(self):
        a = self._keyer_arrays()
        rc = self.L.selenite_tx_get_keyer_state(self.h, C.byref(self._keyer_view(a)))
        if rc:
            raise RxError(rc, "selenite_tx_get_keyer_state: the keyer is not configured (set_keyer)")
        return a

    def set_keyer_state(self, a):
        """members that are missing from `a` are left as they are"""
        want = self._keyer_arrays()
        a = {k: np.ascontiguousarray(a[k], want[k].dtype) for k in want if k in a}
        for k, x in a.items():
            if x.shape != want[k].shape:
                raise ValueError("%s: %s expected" % (k, want[k].shape))
        rc = self.L.selenite_tx_set_keyer_state(self.h, C.byref(self._keyer_view(a)))
        if rc:
            raise RxError(rc, "selenite_tx_set_keyer_state: the keyer is not configured (set_keyer)")

    def time_keyer_stage(self, d_paddles, block_size, iters):
        """mean ms of the stage kernel alone over `iters` launches behind one untimed launch; the state moves"""
        ms = C.c_float()
        rc = self.L.selenite_tx_time_keyer_stage_device(self.h, d_paddles, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.L.selenite_tx_error_string(self.h).decode())
        return ms.value

    def time_process(self, d_src, d_dst, block_size, iters):
        ms = C.c_float()
        rc = self.L.selenite_tx_time_process_device(self.h, d_src, d_dst, block_size, iters, C.byref(ms))
        if rc:
            raise RxError(rc, self.L.selenite_tx_error_string(self.h).decode())
        return ms.value

    def close(self):
        if self.h:
            self.L.selenite_tx_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def design_chan_prototype(fft_len, taps_per_branch, width=1.0):
    """the channeliser's prototype g[K P] in CMSIS order: design_lowpass(K P, 0.5 * width / K), width in channel spacings (0 < width <= 2)"""
    g = np.empty(fft_len * taps_per_branch, np.float32)
    rc = lib().selenite_chan_design_prototype(_fp(g), fft_len, taps_per_branch, float(width))
    if rc:
        raise ValueError("selenite_chan_design_prototype: %d" % rc)
    return g


class _FilterBank:
    """What Channelizer and Combiner share: one object of the C prefix `_prefix` (selenite_chan_ / selenite_comb_) whose state is a history
    of shape _hist_shape() and a position.  Device pointers only (DeviceBuffer.ptr)."""
    _prefix = None
    _config = None
    _state_view = None

    def _init(self, bands, fft_len, oversample, taps_per_branch, coeffs, bins, *own_fields):
        self.L = lib()
        coeffs = np.ascontiguousarray(coeffs, np.float32)
        assert coeffs.size == fft_len * taps_per_branch, coeffs.shape
        b = None if bins is None else np.ascontiguousarray(bins, np.uint32)
        self.bands, self.fft_len, self.oversample, self.taps_per_branch = int(bands), int(fft_len), int(oversample), int(taps_per_branch)
        self.n_bins = self.fft_len if b is None else int(b.size)
        cfg = self._config(C.sizeof(self._config), self.bands, self.fft_len, self.oversample, self.taps_per_branch, self.n_bins, *own_fields, 0,
                           _fp(coeffs), None if b is None else b.ctypes.data_as(u32p))
        self.h = C.c_void_p()
        rc = self._c("init")(C.byref(self.h), C.byref(cfg))
        if rc:
            raise RxError(rc, "%sinit failed (no GPU, or a bad configuration)" % self._prefix)

    def _c(self, name):
        return getattr(self.L, self._prefix + name)

    def _raise(self, rc):
        if rc:
            raise RxError(rc, self._c("error_string")(self.h).decode())

    def status(self):
        return self._c("status")(self.h)

    def check(self):
        self._raise(self.status())

    def out_len(self, block_size):
        return self._c("out_len")(self.h, block_size)

    def process_device(self, d_src, d_dst, block_size):
        """f32 in, f32 out, asynchronous; a refused call raises"""
        self._c("process_f32_device")(self.h, d_src, d_dst, block_size)
        self.check()

    def process_q15_device(self, d_src, d_dst, block_size):
        """the int16 side of the object (Channelizer: the input; Combiner: the output)"""
        self._c("process_q15_device")(self.h, d_src, d_dst, block_size)
        self.check()

    def set_stream(self, stream_ptr):
        return self._c("set_stream")(self.h, stream_ptr)

    def sync(self):
        self._raise(self._c("sync")(self.h))

    def reset(self):
        return self._c("reset")(self.h)

    def state(self):
        a = {"history": np.zeros(self._hist_shape(), np.float32), "position": np.zeros(1, np.uint64)}
        v = self._state_view(_fp(a["history"]), a["position"].ctypes.data_as(u64p))
        self._raise(self._c("get_state")(self.h, C.byref(v)))
        return a

    def set_state(self, a):
        hist = np.ascontiguousarray(a["history"], np.float32) if a.get("history") is not None else None
        pos = np.ascontiguousarray(a["position"], np.uint64) if a.get("position") is not None else None
        assert hist is None or hist.shape == self._hist_shape(), hist.shape
        v = self._state_view(None if hist is None else _fp(hist), None if pos is None else pos.ctypes.data_as(u64p))
        self._raise(self._c("set_state")(self.h, C.byref(v)))

    def close(self):
        if self.h:
            self._c("free")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Channelizer(_FilterBank):
    """One selenite_chan object (include/selenite_chan.h): `bands` wideband I/Q streams in, bands * n_bins channels out, in the layout
    Rx.process_device reads: d_src [bands][block_size][2] f32 (process_q15_device: int16, arm_q15_to_float) -> d_dst
    [bands * n_bins][block_size / D][2] f32."""
    _prefix, _config, _state_view = "selenite_chan_", ChanConfig, ChanStateView

    def __init__(self, bands, fft_len, oversample, taps_per_branch, coeffs, bins=None):
        self._init(bands, fft_len, oversample, taps_per_branch, coeffs, bins)
        self.decim = self.fft_len // self.oversample
        self.hist_len = self.fft_len * self.taps_per_branch - self.decim

    def _hist_shape(self):
        return (self.bands, self.hist_len, 2)

    def out_channels(self):
        return self._c("out_channels")(self.h)


def design_comb_prototype(fft_len, taps_per_branch, width=1.0, oversample=1):
    """the combiner's prototype g[K P] in CMSIS order: design_chan_prototype(K, P, width) times K * D, D = K / oversample, so that a constant
    on channel 0 leaves as that constant (the 1 / K is arm_cfft_f32's own)"""
    g = np.empty(fft_len * taps_per_branch, np.float32)
    rc = lib().selenite_comb_design_prototype(_fp(g), fft_len, taps_per_branch, float(width), oversample)
    if rc:
        raise ValueError("selenite_comb_design_prototype: %d" % rc)
    return g


class Combiner(_FilterBank):
    """One selenite_comb object (include/selenite_comb.h): bands * n_bins TX channel rows in, in the layout Tx.process_device writes, `bands`
    wideband I/Q streams out: d_src [bands * n_bins][block_size][2] f32 -> d_dst [bands][block_size * D][2] f32 (process_q15_device: int16,
    arm_float_to_q15, saturating)."""
    _prefix, _config, _state_view = "selenite_comb_", CombConfig, CombStateView

    def __init__(self, bands, fft_len, oversample, taps_per_branch, coeffs, bins=None, q15_rounding=0):
        self._init(bands, fft_len, oversample, taps_per_branch, coeffs, bins, int(q15_rounding))
        self.interp = self.fft_len // self.oversample
        self.hist_len = self.taps_per_branch * self.oversample - 1

    def _hist_shape(self):
        return (self.bands * self.n_bins, self.hist_len, 2)

    def in_channels(self):
        return self._c("in_channels")(self.h)
