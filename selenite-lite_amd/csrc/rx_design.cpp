// rx_design.cpp -- coefficient design helpers of include/selenite_rx.h (host only).
//
// Conveniences for callers: the chain itself only ever sees coefficient arrays.  Everything is
// computed in double and rounded once to float; arrays are written in CMSIS order
// ({b[N-1] .. b[0]}, arm_fir_decimate_f32.c:64-69) and with CMSIS's biquad sign convention
// (feedback added, arm_biquad_cascade_df1_f32.c:52-63).
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/selenite_rx.h"
#include "../../include/selenite_tx.h"

static const double kPi = 3.14159265358979323846;

static double hamming(uint32_t n, uint32_t num_taps)
{
    return 0.54 - 0.46 * std::cos(2.0 * kPi * (double)n / (double)(num_taps - 1));
}

extern "C" int selenite_rx_design_lowpass(float *coeffs, uint32_t num_taps, double cutoff)
{
    if (!coeffs || num_taps < 2 || !(cutoff > 0.0 && cutoff < 0.5)) return SELENITE_RX_ARGUMENT_ERROR;
    std::vector<double> h(num_taps);
    double sum = 0.0;
    for (uint32_t n = 0; n < num_taps; ++n) {
        const double m = (double)n - (double)(num_taps - 1) / 2.0;
        const double x = 2.0 * cutoff * m;
        const double sinc = (x == 0.0) ? 1.0 : std::sin(kPi * x) / (kPi * x);
        h[n] = 2.0 * cutoff * sinc * hamming(n, num_taps);
        sum += h[n];
    }
    for (uint32_t n = 0; n < num_taps; ++n) coeffs[num_taps - 1 - n] = (float)(h[n] / sum);
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_design_interp(float *coeffs, uint32_t ni_taps, uint32_t interp, double cutoff)
{
    if (interp != 1 && interp != 2 && interp != 4 && interp != 8) return SELENITE_RX_ARGUMENT_ERROR;
    if (ni_taps % interp != 0) return SELENITE_RX_LENGTH_ERROR;          // arm_fir_interpolate_init_f32.c:91-96
    const int rc = selenite_rx_design_lowpass(coeffs, ni_taps, cutoff);
    if (rc != SELENITE_RX_SUCCESS) return rc;
    for (uint32_t n = 0; n < ni_taps; ++n) coeffs[n] = coeffs[n] * (float)interp;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_design_hilbert(float *hilb, float *delay, uint32_t num_taps)
{
    if (!hilb || !delay || num_taps < 3 || (num_taps % 2) == 0) return SELENITE_RX_ARGUMENT_ERROR;
    const int c = (int)(num_taps - 1) / 2;
    for (uint32_t n = 0; n < num_taps; ++n) {
        const int m = (int)n - c;
        double v = 0.0;
        if (m & 1) v = 2.0 / (kPi * (double)m) * hamming(n, num_taps);
        hilb[num_taps - 1 - n] = (float)v;
        delay[num_taps - 1 - n] = (m == 0) ? 1.0f : 0.0f;
    }
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_design_bandpass(float *coeffs, uint32_t n_stages, double f0, double q)
{
    if (!coeffs || n_stages == 0 || !(f0 > 0.0 && f0 < 0.5) || !(q > 0.0)) return SELENITE_RX_ARGUMENT_ERROR;
    const double w0 = 2.0 * kPi * f0, alpha = std::sin(w0) / (2.0 * q), a0 = 1.0 + alpha;
    const double b0 = alpha / a0, b1 = 0.0, b2 = -alpha / a0;
    const double a1 = -2.0 * std::cos(w0) / a0, a2 = (1.0 - alpha) / a0;
    for (uint32_t s = 0; s < n_stages; ++s) {
        coeffs[5 * s + 0] = (float)b0;
        coeffs[5 * s + 1] = (float)b1;
        coeffs[5 * s + 2] = (float)b2;
        coeffs[5 * s + 3] = (float)(-a1);
        coeffs[5 * s + 4] = (float)(-a2);
    }
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_design_window(float *w, uint32_t n, int kind)
{
    if (!w || n < 2 || (kind != SELENITE_RX_WINDOW_HANN && kind != SELENITE_RX_WINDOW_BLACKMAN_HARRIS)) return SELENITE_RX_ARGUMENT_ERROR;
    for (uint32_t i = 0; i < n; ++i) {
        const double a = 2.0 * kPi * (double)i / (double)n;      // periodic form: the frame is one period of the transform
        const double v = kind == SELENITE_RX_WINDOW_HANN
                             ? 0.5 - 0.5 * std::cos(a)
                             : 0.35875 - 0.48829 * std::cos(a) + 0.14128 * std::cos(2.0 * a) - 0.01168 * std::cos(3.0 * a);
        w[i] = (float)v;
    }
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_design_biquad(float coeffs[5], int kind, double f0, double q, double gain_db)
{
    if (!coeffs || !(f0 > 0.0 && f0 < 0.5) || !(q > 0.0) || !std::isfinite(q)) return SELENITE_RX_ARGUMENT_ERROR;
    const double w0 = 2.0 * kPi * f0, cw = std::cos(w0), alpha = std::sin(w0) / (2.0 * q);
    double b0, b1, b2, a0, a1, a2;
    switch (kind) {
    case SELENITE_RX_BIQUAD_NOTCH:
        b0 = 1.0; b1 = -2.0 * cw; b2 = 1.0;
        a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha;
        break;
    case SELENITE_RX_BIQUAD_PEAKING: {
        if (!std::isfinite(gain_db)) return SELENITE_RX_ARGUMENT_ERROR;
        const double A = std::pow(10.0, gain_db / 40.0);
        b0 = 1.0 + alpha * A; b1 = -2.0 * cw; b2 = 1.0 - alpha * A;
        a0 = 1.0 + alpha / A; a1 = -2.0 * cw; a2 = 1.0 - alpha / A;
        break;
    }
    case SELENITE_RX_BIQUAD_LOWPASS:
        b0 = (1.0 - cw) / 2.0; b1 = 1.0 - cw; b2 = (1.0 - cw) / 2.0;
        a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha;
        break;
    case SELENITE_RX_BIQUAD_HIGHPASS:
        b0 = (1.0 + cw) / 2.0; b1 = -(1.0 + cw); b2 = (1.0 + cw) / 2.0;
        a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha;
        break;
    default:
        return SELENITE_RX_ARGUMENT_ERROR;
    }
    coeffs[0] = (float)(b0 / a0);
    coeffs[1] = (float)(b1 / a0);
    coeffs[2] = (float)(b2 / a0);
    coeffs[3] = (float)(-a1 / a0);
    coeffs[4] = (float)(-a2 / a0);
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_design_deemphasis(float coeffs[5], double tau_samples)
{
    if (!coeffs || !(tau_samples > 0.0) || !std::isfinite(tau_samples)) return SELENITE_RX_ARGUMENT_ERROR;
    const double p = std::exp(-1.0 / tau_samples);
    coeffs[0] = (float)(1.0 - p);
    coeffs[1] = 0.0f;
    coeffs[2] = 0.0f;
    coeffs[3] = (float)p;
    coeffs[4] = 0.0f;
    return SELENITE_RX_SUCCESS;
}

extern "C" int selenite_rx_design_tones(float *coeffs, const double *freq, uint32_t n_tones)
{
    if (!coeffs || !freq || n_tones == 0) return SELENITE_RX_ARGUMENT_ERROR;
    for (uint32_t k = 0; k < n_tones; ++k)
        if (!(freq[k] > 0.0 && freq[k] < 0.5)) return SELENITE_RX_ARGUMENT_ERROR;
    for (uint32_t k = 0; k < n_tones; ++k) {
        const double w = 2.0 * kPi * freq[k];
        coeffs[3 * k] = (float)(2.0 * std::cos(w));
        coeffs[3 * k + 1] = (float)std::cos(w);
        coeffs[3 * k + 2] = (float)std::sin(w);
    }
    return SELENITE_RX_SUCCESS;
}

extern "C" uint32_t selenite_rx_ctcss_hz(double hz[50])
{
    static const double kCtcss[50] = { 67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8,
                                       118.8, 123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3,
                                       179.9, 183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3,
                                       254.1 };
    if (hz)
        for (int k = 0; k < 50; ++k) hz[k] = kCtcss[k];
    return 50u;
}

// the Morse decoder's table (rx_cwdec.hip): index = the elements behind a leading 1, dit 0, dah 1
extern "C" int selenite_rx_design_morse(uint8_t table[256], uint8_t unknown)
{
    static const struct { char c; const char *pattern; } kMorse[] = {
        { 'A', ".-" },    { 'B', "-..." },  { 'C', "-.-." },  { 'D', "-.." },   { 'E', "." },     { 'F', "..-." },  { 'G', "--." },
        { 'H', "...." },  { 'I', ".." },    { 'J', ".---" },  { 'K', "-.-" },   { 'L', ".-.." },  { 'M', "--" },    { 'N', "-." },
        { 'O', "---" },   { 'P', ".--." },  { 'Q', "--.-" },  { 'R', ".-." },   { 'S', "..." },   { 'T', "-" },     { 'U', "..-" },
        { 'V', "...-" },  { 'W', ".--" },   { 'X', "-..-" },  { 'Y', "-.--" },  { 'Z', "--.." },
        { '0', "-----" }, { '1', ".----" }, { '2', "..---" }, { '3', "...--" }, { '4', "....-" }, { '5', "....." }, { '6', "-...." },
        { '7', "--..." }, { '8', "---.." }, { '9', "----." },
        { '.', ".-.-.-" }, { ',', "--..--" }, { '?', "..--.." }, { '/', "-..-." }, { '=', "-...-" }, { '+', ".-.-." }, { '-', "-....-" },
        { '@', ".--.-." },
    };
    if (!table) return SELENITE_RX_ARGUMENT_ERROR;
    for (int i = 0; i < 256; ++i) table[i] = unknown;
    for (const auto &m : kMorse) {
        uint32_t code = 1u;
        for (const char *p = m.pattern; *p; ++p) code = (code << 1) | (*p == '-' ? 1u : 0u);
        table[code] = (uint8_t)m.c;
    }
    return SELENITE_RX_SUCCESS;
}

// include/selenite_tx.h: the phase increment per output sample of a tone of `hz` at the output rate `fs_out`, for
// selenite_tx_fm_config::tone_step (and nco_step): round(hz / fs_out * 2^32) in double, rounded once, modulo 2^32 (a negative
// frequency is its two's complement); 0 for arguments that are not finite or a rate that is not positive
extern "C" uint32_t selenite_tx_tone_step(double hz, double fs_out)
{
    if (!std::isfinite(hz) || !std::isfinite(fs_out) || !(fs_out > 0.0)) return 0u;
    const double turns = hz / fs_out;
    const double frac = turns - std::floor(turns);          // [0, 1): the step is periodic in whole turns
    return (uint32_t)((uint64_t)std::llround(frac * 4294967296.0) & 0xFFFFFFFFull);
}

// include/selenite_tx_cw.h: the keying shape for selenite_tx_cw_config::shape_coeffs -- the Hann window w[k] = 0.5 - 0.5 cos(2 pi (k + 1) /
// (ns + 1)) (no zero end taps), normalised to sum 1 in double and rounded to f32 once.  Its running sum, the step response of the shaping
// FIR, is a raised-cosine edge of ns samples; ns = 1 is {1.0f}: hard keying.  The window is symmetric, so CMSIS order is its own.
extern "C" int selenite_tx_design_keyshape(uint32_t ns_taps, float *coeffs)
{
    if (ns_taps == 0 || !coeffs) return SELENITE_RX_ARGUMENT_ERROR;
    const double kPi = 3.14159265358979323846;
    std::vector<double> w(ns_taps);
    for (uint32_t k = 0; k < ns_taps / 2 + (ns_taps & 1u); ++k)                     // both halves from one evaluation: symmetric on bits
        w[k] = w[ns_taps - 1 - k] = 0.5 - 0.5 * std::cos(2.0 * kPi * (double)(k + 1) / ((double)ns_taps + 1.0));
    double sum = 0.0;
    for (uint32_t k = 0; k < ns_taps; ++k) sum += w[k];
    for (uint32_t k = 0; k < ns_taps; ++k) coeffs[k] = (float)(w[k] / sum);
    return SELENITE_RX_SUCCESS;
}

// the FSK decoder's tone filters (rx_fskdec.hip): the constant-peak-gain band-pass of design_biquad's family, Q = f0 / bandwidth
extern "C" int selenite_rx_design_fsk(double f_mark, double f_space, double bandwidth, float mark[5], float space[5])
{
    if (!mark || !space) return SELENITE_RX_ARGUMENT_ERROR;
    if (!(std::isfinite(bandwidth) && bandwidth > 0.0)) return SELENITE_RX_ARGUMENT_ERROR;
    const double f[2] = { f_mark, f_space };
    float *out[2] = { mark, space };
    for (double f0 : f)
        if (!(std::isfinite(f0) && f0 > 0.0 && f0 < 0.5)) return SELENITE_RX_ARGUMENT_ERROR;
    for (int i = 0; i < 2; ++i) {
        const double w = 2.0 * kPi * f[i], alpha = std::sin(w) / (2.0 * f[i] / bandwidth), a0 = 1.0 + alpha;
        out[i][0] = (float)(alpha / a0);
        out[i][1] = 0.0f;
        out[i][2] = (float)(-alpha / a0);
        out[i][3] = (float)(2.0 * std::cos(w) / a0);
        out[i][4] = (float)(-(1.0 - alpha) / a0);
    }
    return SELENITE_RX_SUCCESS;
}

// the FSK decoder's table (rx_fskdec.hip): ITA2 letters, then the US-TTY figures, by the 5-bit code (bit 0 sent first)
extern "C" int selenite_rx_design_ita2(uint8_t table[64])
{
    static const char kLetters[33] = "\0E\nA SIU\rDRJNFCKTZLWHYPQOBG\0MXV";
    static const char kFigures[33] = "\0" "3\n- \a87\r$4',!:(5\")2#6019?&\0./;";
    if (!table) return SELENITE_RX_ARGUMENT_ERROR;
    for (int i = 0; i < 32; ++i) {
        table[i] = (uint8_t)kLetters[i];
        table[32 + i] = (uint8_t)kFigures[i];
    }
    return SELENITE_RX_SUCCESS;
}

// include/selenite_tx_keyer.h: character -> element pattern, the inverse of selenite_rx_design_morse's table (NULL: the built-in one).
// The smallest pattern >= 2 of a character wins; the filler table[0] has none; a lower-case letter takes its upper-case letter's; the
// blank is 1 (the keyer's word blank); every other byte is 0 (the keyer skips and counts it).
extern "C" int selenite_tx_design_morse_codes(uint8_t codes[256], const uint8_t table[256])
{
    if (!codes) return SELENITE_RX_ARGUMENT_ERROR;
    uint8_t own[256];
    if (!table) {
        (void)selenite_rx_design_morse(own, (uint8_t)'#');
        table = own;
    }
    for (int i = 0; i < 256; ++i) codes[i] = 0;
    for (int code = 255; code >= 2; --code)
        if (table[code] != table[0]) codes[table[code]] = (uint8_t)code;
    for (int ch = 'a'; ch <= 'z'; ++ch)
        if (codes[ch] == 0) codes[ch] = codes[ch - 'a' + 'A'];
    codes[(uint8_t)' '] = 1;
    return SELENITE_RX_SUCCESS;
}

// include/selenite_tx_keyer.h: the dit length in audio samples at `wpm` words per minute (PARIS: 50 units a word, 1.2 s / wpm a unit)
extern "C" uint32_t selenite_tx_keyer_unit(double wpm, double fs_audio)
{
    if (!std::isfinite(wpm) || !std::isfinite(fs_audio) || !(wpm > 0.0) || !(fs_audio > 0.0)) return 0u;
    const double u = std::round(1.2 * fs_audio / wpm);
    return u < 1.0 ? 1u : (u > 4294967295.0 ? 4294967295u : (uint32_t)u);
}
