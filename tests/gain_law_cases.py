"""The AGC / ALC gain law away from its default parameters: the parameter sets, the level plan, the kernel-form cases and the restatement
with its mutants, shared by tests/test_gain_law_oracle.py (CPU) and tests/test_gpu_gain_law.py (GPU).

The law: e = max(env, floor); d = clamp(target / e, gmin, gmax); g += (d < g ? attack : decay) * (d - g);
audio * g.  The defaults (target 0.5, attack 0.5, decay 0.05, gain in [1e-3, 1e4], floor 1e-6, init 1) are degenerate for it: scaling by a
power of two does not round, so 0.5 * rn(1 / e) == rn(0.5 / e) and g + 0.5 * diff is the same number fused or not; the initial gain is the
literal 1 a kernel could carry; the lower clamp needs a block maximum of 500.  SETS are not.

TEST INFRASTRUCTURE.  Nothing here is imported by the product.
"""
import copy

import numpy as np

import rxcommon as rc

f32 = np.float32
KEYS = ("target", "attack", "decay", "gain_min", "gain_max", "env_floor", "gain_init")
SETS = {
    "odd": dict(target=0.3, attack=0.37, decay=0.011, gain_min=0.7, gain_max=3.1, env_floor=0.05, gain_init=2.3),
    "fast": dict(target=0.9, attack=1.0, decay=1.0, gain_min=1e-2, gain_max=50.0, env_floor=1e-3, gain_init=0.25),
    "slow": dict(target=0.11, attack=0.013, decay=0.0007, gain_min=1e-4, gain_max=1e6, env_floor=0.0, gain_init=7.5),
}
SET_NAMES = tuple(SETS)
RX_DEFAULTS = dict(target=0.5, attack=0.5, decay=0.05, gain_min=1e-3, gain_max=1e4, env_floor=1e-6, gain_init=1.0)
TX_DEFAULTS = dict(RX_DEFAULTS, gain_max=1e2)
CHANNELS = (3, 65, 130)          # one partial wavefront group, an odd count, more than one workgroup row
CALLS = (1024, 256, 2048, 1024, 1024, 512)
QUIET, SILENT = (2, 3), 4        # calls 2 and 3 a further 0.01 down, call 4 all zeros (calls counted from 0)


def to_q15(x):
    return np.clip(np.trunc(np.asarray(x, f32) * f32(32768.0)), -32768, 32767).astype(np.int16)


def q15_to_f32(q):
    return q.astype(f32) / f32(32768.0)


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        u = {2: np.uint16, 4: np.uint32}[got.itemsize]
        bad = np.argwhere(got.view(u) != want.view(u))
        raise AssertionError("%s: %d of %d values differ, first at %s: %r vs %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def no_gain(spec):
    """the same ChainSpec / TxSpec with its AGC / ALC off: what leaves it is the un-scaled audio (TX: takes audio as it comes)"""
    s = copy.copy(spec)
    if hasattr(s, "alc"):
        s.alc = False
    else:
        s.agc = s.agc_global = False
    return s


def levels(channels, q15=False):
    """channel c is scaled by 10^linspace(-5, 2) over the channels (int16 slots: 10^linspace(-4, 0))"""
    lo, hi = (-4.0, 0.0) if q15 else (-5.0, 2.0)
    return (10.0 ** np.linspace(lo, hi, channels)).astype(f32)


SPARSE_ROWS, SPARSE_ENVELOPES = 16, 2400
# Where the default run (the six calls once; SPARSE_ENVELOPES envelopes under SPARSE_ROWS rows) leaves the restatement short of a condition
# -- in every case `slow` against target * (1 / e): a one-ulp change of d moves g + rate * diff across a rounding boundary with probability
# about rate * d / g, and `slow` has rates 0.013 and 0.0007 and a gain in the thousands behind its first silent call -- the run gets more
# envelopes (found by doubling) or, where only its first blocks can show it, another start of the level walk (the first that works).
# tests/test_gain_law_oracle.py asserts every condition on every run.  key: (shape or "tx", rows, int16 slots) -> plan()'s envelopes, first
RUNS = {("cfg2_128", 3, False): dict(envelopes=4200), ("cfg3_64", 3, False): dict(envelopes=4200),
        ("wide", 1, False): dict(first=2), ("tx", 3, True): dict(first=3)}


def run_kw(shape, rows, q15=False):
    return RUNS.get((shape, rows, q15), {})


def plan(channels, block, lens=CALLS, q15=False, audio=False, rows=None, envelopes=None, fm=False, first=0):
    """The calls of the level plan: synthetic I/Q [channels][n][2] (audio: the TX input [channels][n]), f32 or int16 slots.  block: input
    samples per DSP block; rows: envelopes per DSP block -- the channels, or 1 with a global gain (the loudest channel's); envelopes: how
    many the run must have (the six calls run as many times over as that takes; 0: once).

    Under SPARSE_ROWS rows the channels alone give too few levels (three channels sit at 1e-5, 0.03 and 100, where every block of `odd`
    is clamped): every stretch of 256 samples of the stream then has a level of its own on top of its channel's, 10^-(D u_k) with
    u_k = frac((k + 1 + first) / golden ratio) for stretch k -- a low-discrepancy walk over D = 7 / (rows - 1) decades (7 for one row; int16
    slots: 4 in place of 7), the gap to the next channel's level, so the rows together see every level from 100 down, in both directions.

    fm: the discriminator's output does not follow the input's amplitude, so there the plan's levels are the DEVIATION: a carrier of
    amplitude 0.5 at the LO's frequency (fs / 256: the NCO mixes it to 0 Hz) whose phase advances by 0.5 level audio[n] radians per sample
    -- the FM audio is then the synthetic audio at the plan's level (in half turns, wrapped above about 1), and a silent call is zeros."""
    assert len(lens) == 6 and all(n % block == 0 for n in lens)
    lv, out, at = levels(channels, q15), [], 0
    rows = channels if rows is None else rows
    sparse = rows < SPARSE_ROWS
    if envelopes is None:
        envelopes = SPARSE_ENVELOPES if sparse else 0
    rounds = max(1, -(-envelopes // (rows * (sum(lens) // block))))
    decades = (4.0 if q15 else 7.0) / max(rows - 1, 1)
    phase = np.zeros(channels)
    for i, n in enumerate(lens * rounds):
        i %= 6
        x = rc.synth_audio(0, channels, at, n) if audio or fm else rc.synth_iq(0, channels, at, n)
        s = (lv * f32(0.01) if i in QUIET else lv)[:, None]
        if sparse:
            u = ((at + np.arange(n)) // 256 + 1 + first) * 0.6180339887498949 % 1.0
            s = s * (10.0 ** (-decades * u)).astype(f32)[None, :]
        x = np.zeros_like(x) if i == SILENT else np.multiply(x, s.reshape(s.shape + (1,) * (x.ndim - 2)), dtype=f32)
        if fm:
            ph = phase[:, None] + np.cumsum(0.5 * x.astype(np.float64), axis=1)
            phase = ph[:, -1]
            ph = ph + 2.0 * np.pi / 256.0 * ((at + np.arange(n)) % 256)
            x = np.stack([0.5 * np.cos(ph), 0.5 * np.sin(ph)], axis=2) * (i != SILENT)
        out.append(to_q15(x) if q15 else np.ascontiguousarray(x, f32))
        at += n
    return out


def lens_for(block):
    """CALLS for a DSP block that divides them; the same plan in whole blocks for the others (10, 3, 20, 10, 10, 5 of them -- the second call
    is not a whole pass of any kernel; 2, 1, 4, 2, 2, 1 of a block longer than 256)"""
    if all(n % block == 0 for n in CALLS):
        return CALLS
    return tuple(block * k for k in ((2, 1, 4, 2, 2, 1) if block > 256 else (10, 3, 20, 10, 10, 5)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement on block maxima, and its mutants
# ---------------------------------------------------------------------------------------------------------------------------------------
def block_maxima(audio, na):
    a = np.abs(np.asarray(audio, f32))
    return a.reshape(a.shape[0], -1, na).max(axis=2)


def law_trace(env, params, variant="true"):
    """nr_oracle.Agc's statements on the block maxima env [channels][blocks] alone: (gain behind every block [channels][blocks], how often
    each branch was taken).  variant: "true"; "rcp" target * (1 / e) in place of the division; "fused" the update g + rate * diff in f64,
    rounded once (what one FMA gives)."""
    p = {k: f32(params[k]) for k in KEYS}
    env = np.asarray(env, f32)
    g = np.full(env.shape[0], p["gain_init"], f32)
    gains = np.empty_like(env)
    n = dict(floor=0, upper=0, lower=0, attack=0, decay=0, zero=0, blocks=env.size)
    for b in range(env.shape[1]):
        e = np.where(env[:, b] < p["env_floor"], p["env_floor"], env[:, b])
        with np.errstate(divide="ignore"):
            d = np.multiply(p["target"], np.divide(f32(1.0), e)) if variant == "rcp" else np.divide(p["target"], e)
        n["floor"] += int((env[:, b] < p["env_floor"]).sum())
        n["upper"] += int((d > p["gain_max"]).sum())
        d = np.where(d > p["gain_max"], p["gain_max"], d)
        n["lower"] += int((d < p["gain_min"]).sum())
        d = np.where(d < p["gain_min"], p["gain_min"], d)
        diff = np.subtract(d, g)
        n["attack"] += int((diff < 0).sum()); n["decay"] += int((diff > 0).sum()); n["zero"] += int((diff == 0).sum())
        rate = np.where(diff < f32(0), p["attack"], p["decay"])
        if variant == "fused":
            g = (g.astype(np.float64) + rate.astype(np.float64) * diff.astype(np.float64)).astype(f32)
        else:
            g = np.add(g, np.multiply(rate, diff))
        gains[:, b] = g
    return gains, n


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_defaults(name, env, defaults=RX_DEFAULTS, what=""):
    """the least a run must show: set `name` and the default parameters give different gains on its block maxima"""
    assert not same_bits(law_trace(env, defaults)[0], law_trace(env, SETS[name])[0]), "%s set %s: the default parameters give the same bits" % (what, name)


def check_conditions(name, env, defaults=RX_DEFAULTS, what=""):
    """The coverage and sensitivity conditions of set `name` on the block maxima of one run (every call, in order).  Conditions, not
    tolerances: a shape that misses one needs more blocks or levels, never a weaker condition."""
    gains, n = law_trace(env, SETS[name])
    msg = "%s set %s: %r" % (what, name, n)
    if name == "odd":
        assert min(n["floor"], n["upper"], n["lower"], n["attack"], n["decay"]) >= 1, msg
    if name == "fast":
        assert n["zero"] >= 1, msg
    if name == "slow":
        assert min(n["attack"], n["decay"], n["upper"]) >= 1, msg
    assert not same_bits(law_trace(env, SETS[name], "rcp")[0], gains), msg + ": target * (1 / e) gives the same bits"
    if name != "fast":      # rate 1.0: the product is exact, fused or not
        assert not same_bits(law_trace(env, SETS[name], "fused")[0], gains), msg + ": a fused update gives the same bits"
    assert not same_bits(law_trace(env, defaults)[0], gains), msg + ": the default parameters give the same bits"
    return gains, n


# ---------------------------------------------------------------------------------------------------------------------------------------
# the kernel forms: one RX chain per call site of the law (tests/test_gpu_gain_law.py maps sites to cases)
# ---------------------------------------------------------------------------------------------------------------------------------------
C, F, S, A = rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO
ARITH_NAME = {C: "cmsis", F: "fma", S: "split16", A: "auto"}
_LO = dict(nco=True, nco_step_all=0x01000000)
RERUN = "+exact rerun of guarded channels"


def _shape(block, decim, nd, nh, nbiq=0, mode=rc.MODE_USB, **kw):
    return lambda ch, arith, **more: rc.ChainSpec(ch, block, decim, nd, nh, nbiq, mode, arith, **dict(kw, **more))


# name -> (spec(channels, arith, **kw), {arith: kernel_name()})
RX_SHAPES = {
    # 16-lane DSP blocks (64 audio samples): demod_agc_store<16>, agc_pass<16>
    "cfg3": (_shape(256, 4, 256, 63, **_LO), {C: "k_ssb_fused<256,4,63>", F: "k_ssb_mfma<256,4,63>", S: "k_ssb_split16<256,4,63>",
                                               A: "k_ssb_split16<256,4,63>" + RERUN}),
    # 64-lane DSP blocks (256 audio samples): demod_agc_store<64>, agc_pass<64>
    "cfg2": (_shape(256, 1, 0, 127), {C: "k_ssb_fused<0,1,127>", F: "k_ssb_fused<0,1,127>", S: "k_hilb_split16<127>", A: "k_hilb_split16<127>" + RERUN}),
    # 32-lane DSP blocks (128 audio samples): demod_agc_store<32>, agc_pass<32>
    "cfg2_128": (_shape(128, 1, 0, 127), {C: "k_ssb_fused<0,1,127>", S: "k_hilb_split16<127>", A: "k_hilb_split16<127>" + RERUN}),
    # the firmware's 96-frame blocks by 4: 6-lane groups, not a power of two -- the run-time-group loops (demod_agc_store<0>, agc_pass<0>)
    "fw96": (_shape(96, 4, 256, 63, **_LO), {C: "k_ssb_fused<256,4,63>", F: "k_ssb_fused<256,4,63>", S: "k_ssb_split16<256,4,63>",
                                              A: "k_ssb_split16<256,4,63>" + RERUN}),
    # by 8: 8-lane groups on the by-4 product (agc_pass<0>, its DPP branch); by 2: 32-lane groups
    "by8": (_shape(256, 8, 256, 63, **_LO), {C: "k_ssb_fused<256,8,63>", S: "k_ssb_split16<256,8,63>", A: "k_ssb_split16<256,8,63>" + RERUN}),
    "by2": (_shape(256, 2, 256, 63, **_LO), {C: "k_ssb_fused<256,2,63>", F: "k_ssb_fused<256,2,63>", S: "k_ssb_split16<256,2,63>",
                                              A: "k_ssb_split16<256,2,63>" + RERUN}),
    # the cfg3 chain in DSP blocks of 64 frames (4-lane groups, 16 audio samples): four times the envelopes per sample
    "cfg3_64": (_shape(64, 4, 256, 63, **_LO), {C: "k_ssb_fused<256,4,63>", F: "k_ssb_mfma<256,4,63>", S: "k_ssb_split16<256,4,63>",
                                                 A: "k_ssb_split16<256,4,63>" + RERUN}),
    # ... and of 1024 frames: 64-lane groups on the decimating kernels (k_ssb_split16's agc_pass<64>)
    "cfg3_1024": (_shape(1024, 4, 256, 63, **_LO), {C: "k_ssb_fused<256,4,63>", S: "k_ssb_split16<256,4,63>", A: "k_ssb_split16<256,4,63>" + RERUN}),
    # CW: k_cw_fused
    "cfg4": (_shape(256, 1, 0, 0, 4, rc.MODE_CW, nco=True, nco_step_all=0x00800000), {C: "k_cw_fused<4,256>", F: "k_cw_fused<4,256>"}),
    # AM and FM on the cfg3 chain (raw SPLIT16 runs FM in the fma arithmetic: the matrix kernel k_ssb_mfma)
    "am": (_shape(256, 4, 256, 63, mode=rc.MODE_AM, **_LO), {C: "k_ssb_fused<256,4,63>", S: "k_ssb_split16<256,4,63>", A: "k_ssb_split16<256,4,63>" + RERUN}),
    # AM without a decimator: k_hilb_split16's agc_pass<64> behind arm_cmplx_mag_f32
    "cfg2_am": (_shape(256, 1, 0, 127, mode=rc.MODE_AM), {C: "k_ssb_fused<0,1,127>", S: "k_hilb_split16<127>", A: "k_hilb_split16<127>" + RERUN}),
    "fm": (_shape(256, 4, 256, 63, mode=rc.MODE_FM, **_LO), {C: "k_ssb_fused<256,4,63>", S: "k_ssb_mfma<256,4,63>", A: "k_ssb_split16<256,4,63>" + RERUN}),
    # the generic kernels' own shapes (no fused kernel serves them): 512 audio samples per DSP block (128 float4: more than a wavefront),
    # 14 audio samples per DSP block (not a multiple of four)
    "wide": (_shape(512, 1, 0, 15), {C: "generic", F: "generic"}),
    "na14": (_shape(56, 4, 17, 9, nco=True, nco_step_all=0x01234567), {C: "generic", F: "generic"}),
}


# the global gain's four apply forms (rx_generic.hip: launch_agc_apply_global), each with the run that carries the conditions for it:
# shape -> (channels, what the shape selects).  ONE envelope row, so these runs are sparse (plan()).
GLOBAL_RUNS = {
    # na = 16 divides 256: calls of whole 256-output rows (1024, 2048 samples) take k_agc_apply_global_rows, the calls of 256 and 512
    # samples (64 and 128 outputs) k_agc_apply_global's chunked form (na / 4 = 4 float4 per block: 16 channels per wavefront, so 17 channels are a full one and a ragged one)
    "cfg3_64": 17,
    # na = 512: 128 float4 per block, more than a wavefront -- k_agc_apply_global's strided form, one wavefront per channel
    "wide": 3,
    # na = 14, not a multiple of four: k_agc_apply_global's scalar form, one wavefront per channel
    "na14": 33,
}


# the runs with int16 slots (levels 1e-4 ... 1): (shape, channels).  An int16 output shows a one-ulp change of the gain only where it moves a
# sample across an integer, so these runs pin the parameters and the initial gain; the last bit of the law is pinned by the f32 runs of the
# same kernels.  cfg4 carries only check_defaults: at int16 levels the CW filter passes so little of the plan's signal that every envelope of
# `odd` is under its floor (2939 of 2990 blocks; the rest clamped); its f32 runs carry every condition.
Q15_RUNS = (("cfg3", 65), ("cfg3", 130), ("cfg2", 65), ("cfg2", 130), ("cfg2_128", 130), ("fw96", 130), ("cfg4", 65), ("cfg4", 130))


def rx_spec(shape, channels, arith, params, **kw):
    return RX_SHAPES[shape][0](channels, arith, agc_params=dict(params), **kw)


def rx_kernel(shape, arith):
    return RX_SHAPES[shape][1][arith]


def rx_lens(shape):
    return lens_for(RX_SHAPES[shape][0](1, C).block)


def rx_plan(shape, channels, q15=False, rows=None, plain=False):
    """the calls of `shape`'s run: rows = 1 for a global gain; plain: the six calls once, no level walk, whatever the rows"""
    rows = channels if rows is None else rows
    block = RX_SHAPES[shape][0](1, C).block
    if plain:
        return plan(channels, block, rx_lens(shape), q15, rows=SPARSE_ROWS, envelopes=0, fm=shape == "fm")
    return plan(channels, block, rx_lens(shape), q15, rows=rows, fm=shape == "fm", **run_kw(shape, rows, q15))


RX_RUNS = [(name, shape) for shape in RX_SHAPES for name in SET_NAMES]
RX_FORMS = [(name, shape, arith) for name, shape in RX_RUNS for arith in RX_SHAPES[shape][1]]
