"""The case generator of the RX stage fuzz (tests/test_gpu_rx_stage_fuzz.py): deterministic, free of GPU calls, never rejects a draw.

cases(seed, n, kind) yields plain descriptions -- numbers, strings, lists and dicts only, so that a failing case prints whole and can be
pasted into a directed test: the chain, the parameters of all nine stages, which of them are on at the start, and 3 .. 7 events.
build_spec(case) makes the rc.ChainSpec, signal(case, first, count) the input -- a pure function of (case, channel, absolute sample), so any
cut of the stream reproduces it.  Every case has a random stream of its own (seed, kind, index): case k of a kind is the same whatever n is.

Every draw is valid for selenite_rx_init and for the setter it goes to; the ranges restated here are the setters' own argument checks
(csrc/rx_*.hip: selenite_rx_set_*):
    spectrum  fft_len 64 or 512 (the pure radix-8 lengths; 128 is refused with LENGTH_ERROR), stride 1 .. 65535, average 0 / 1, alpha in (0, 1]
    iqc, nb   frame 32, 64 or 128 and a divisor of cfg.block; nb: guard 0 .. 8, max_hits 1 .. frame / 4, threshold >= 1, alpha in (0, 1], clamp >= 1;
              iqc: alpha, dc_alpha in [0, 1], p_max in (0, 1], g_max >= 1, |p_init| <= p_max, 1 / g_max <= g_init <= g_max
    tones     1 .. 64 tones, frame_blocks, confirm, release 1 .. 65535, ratio in [0, 1], min_power >= 0
    cwdec     rates in (0, 1], 0 < off_frac <= on_frac < 1, snr >= 1, debounce 1 .. 255, track 0 .. 8, 256 <= unit_min <= unit_init <= unit_max,
              ring a power of two from 16
    afilt     1 .. 8 sections, finite;  nr: 8 / 16 / 32 / 64 taps, delay 1 .. 64, mu in (0, 2);  meter: rates in (0, 1], close <= open (ABOVE)
    out       interp 1, 2, 4 or 8, ni_taps a multiple of it, 1 .. 64 taps per phase (0 taps: interp 1 only)
The first GPU run of the fuzz verifies this restatement: a refused setter raises.

walk(case) restates the HOST's rules for every planned call -- which kernel family serves it (csrc/rx_select.h: plan_shape; csrc/rx_cw.hip:
cw_fused_ok), whether it is cut in two launches (rx_select.h: Decision::first) and the facts route() (csrc/rx_route.h) is given for each of
its launches -- so that tests/test_rx_stage_fuzz_cases.py can assert on the CPU that the committed seed and counts reach every form.

Kinds: "ssb" (the cfg3 chain, by 4 and by 2, and in DSP blocks of 128: the only geometry whose calls rx_select.h cuts), "hilb" (no decimator,
63 or 127 taps), "cw" (cfg4 on k_cw_fused), "generic" (the firmware's 96-frame DSP blocks; the ssb and cw chains under OPT_FORCE_GENERIC).

TEST INFRASTRUCTURE.  Nothing here is imported by the product.
"""
import numpy as np

import rxcommon as rc
import tones_oracle as to
from selenite_rx.chain import design_lowpass

f32 = np.float32
SEED = 20261021
KINDS = ("ssb", "hilb", "cw", "generic")
COUNTS = {"ssb": 30, "hilb": 14, "cw": 12, "generic": 22}      # the default slices of the four GPU tests (profiles/rx_stage_fuzz/README.md: times)
STAGES = ("spectrum", "iqc", "nb", "tones", "cwdec", "afilt", "nr", "meter", "out")
UNSCALED = ("tones", "cwdec", "afilt", "nr", "meter")           # rx_route.h: StagesOn
CHANNELS = (1, 3, 17, 33, 65, 70)
LENGTHS = (1, 3, 4, 5, 16, 17, 20)                              # DSP blocks per call
ENTRIES = ("host_f32", "host_q15", "dev_f32", "dev_q15")
NLMS_MAX_AUDIO = 1536                                           # audio samples per call with NLMS on: its oracle is a Python loop over samples and taps
MAX_AUDIO = 2560                                                # ... and without: the filter's and the tone bank's are loops over samples
EXACT = (rc.ARITH_CMSIS, rc.ARITH_FMA)
AGC_ODD = dict(target=0.3, attack=0.37, decay=0.011, gain_min=0.7, gain_max=3.1, env_floor=0.05, gain_init=2.3)      # (tests/gain_law_cases.py: "odd")
LEVEL = 0.3


def scale_count(kind, env_value):
    """SELENITE_RX_STAGE_FUZZ_CASES=<n> scales the four slices: n cases in all in place of the default sum"""
    if not env_value:
        return COUNTS[kind]
    return max(1, int(env_value) * COUNTS[kind] // sum(COUNTS.values()))


def _pick(rng, items, weights=None):
    if weights is None:
        return items[int(rng.integers(len(items)))]
    w = np.asarray(weights, np.float64)
    return items[int(rng.choice(len(items), p=w / w.sum()))]


def _u32(rng):
    return int(rng.integers(0, 1 << 32, dtype=np.uint64))


def _fl(a):
    """float32 values as plain Python floats (exact, and JSON keeps them)"""
    return np.asarray(a, f32).astype(np.float64).tolist()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------------------------
def _draw_chain(rng, kind, idx):
    """(variant, shape dict, modes the family allows, arithmetics, force_generic)"""
    usual = (rc.MODE_USB, rc.MODE_LSB, rc.MODE_AM, rc.MODE_FM, rc.MODE_CW, rc.MODE_CWR)
    all4 = (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16, rc.ARITH_AUTO)
    if kind == "ssb":
        v = _pick(rng, ("by4", "by2", "by4_b128"), (0.5, 0.3, 0.2))
        if idx % 3 == 1:                                        # every third case: the geometry whose calls are cut, in the arithmetics that cut them
            v, all4 = "by4_b128", (rc.ARITH_SPLIT16, rc.ARITH_AUTO)
        shape = dict(block=128 if v == "by4_b128" else 256, decim=2 if v == "by2" else 4, nd_taps=256, nh_taps=63, n_biquad=0)
        return v, shape, usual, all4, False
    if kind == "hilb":
        nh = int(_pick(rng, (63, 127)))
        return "nh%d" % nh, dict(block=256, decim=1, nd_taps=0, nh_taps=nh, n_biquad=0), usual, all4, False
    if kind == "cw":
        return "cfg4", dict(block=256, decim=1, nd_taps=0, nh_taps=0, n_biquad=4), (rc.MODE_CW, rc.MODE_CWR), EXACT, False
    v = _pick(rng, ("b96_by4", "b96", "ssb_forced", "cw_forced"), (0.25, 0.2, 0.3, 0.25))
    if v == "b96_by4":                                          # tests/test_gpu_cwdec.py: generic_spec(ch, 24)
        return v, dict(block=96, decim=4, nd_taps=64, nh_taps=31, n_biquad=0), usual, EXACT, False
    if v == "b96":                                              # ... generic_spec(ch, 96)
        return v, dict(block=96, decim=1, nd_taps=0, nh_taps=31, n_biquad=0), usual, EXACT, False
    if v == "ssb_forced":                                       # (SELENITE_ARITH_AUTO is the CMSIS arithmetic on the generic kernels: it brings the per-channel words)
        return v, dict(block=256, decim=4, nd_taps=256, nh_taps=63, n_biquad=0), usual, EXACT + (rc.ARITH_AUTO,), True
    return v, dict(block=256, decim=1, nd_taps=0, nh_taps=0, n_biquad=4), (rc.MODE_CW, rc.MODE_CWR), EXACT, True


def _draw_nco(rng, channels, kind, arith):
    flavour = _pick(rng, ("off", "periodic", "table", "per"), (0.15, 0.3, 0.25, 0.3))
    if kind == "cw" and flavour == "off":
        flavour = "periodic"                                    # (the BFO: without it the CW chain's audio is the I rail)
    d = dict(nco=flavour != "off", nco_step_all=0x01000000, nco_steps=None, nco_flavour=flavour)
    if flavour == "periodic":
        d["nco_step_all"] = int(rng.integers(1, 3)) << 24
    elif flavour == "table":
        d["nco_step_all"] = (0x01000000 + int(rng.integers(-(1 << 20), 1 << 20))) | 1
    elif flavour == "per":
        # in band for most channels; a stop-band step on the others: under SELENITE_ARITH_AUTO their pass band is empty, the guard flags
        # them and the rerun pass serves part of the channels of every call
        stop = rng.random(channels) < (0.4 if arith == rc.ARITH_AUTO else 0.15)
        near = 0x01000000 + rng.integers(-(1 << 20), 1 << 20, channels)
        far = rng.integers(0x30000000, 0xD0000000, channels)
        d["nco_steps"] = [int(v) for v in np.where(stop, far, near)]
    return d


# ---------------------------------------------------------------------------------------------------------------------------------------
# the stages: parameters away from their defaults, fast enough that streams of a few dozen DSP blocks move every state
# ---------------------------------------------------------------------------------------------------------------------------------------
def _highpass(f0, q):
    """one RBJ high-pass section in CMSIS order and sign (float64, rounded once)"""
    w0 = 2.0 * np.pi * f0
    al, c = np.sin(w0) / (2.0 * q), np.cos(w0)
    a0 = 1.0 + al
    return [(1.0 + c) / 2.0 / a0, -(1.0 + c) / a0, (1.0 + c) / 2.0 / a0, 2.0 * c / a0, -(1.0 - al) / a0]


def _notch(f0, q):
    w0 = 2.0 * np.pi * f0
    al, c = np.sin(w0) / (2.0 * q), np.cos(w0)
    a0 = 1.0 + al
    return [1.0 / a0, -2.0 * c / a0, 1.0 / a0, 2.0 * c / a0, -(1.0 - al) / a0]


def _draw_stage(rng, name, shape, channels):
    block, na = shape["block"], shape["block"] // shape["decim"]
    if name == "spectrum":
        return dict(fft_len=int(_pick(rng, (64, 512), (0.7, 0.3))), stride=int(_pick(rng, (1, 2))), average=int(rng.integers(2)),
                    alpha=float(f32(_pick(rng, (0.25, 0.5, 1.0)))))
    frames = [f for f in (32, 64, 128) if block % f == 0]
    if name == "iqc":
        return dict(frame=int(_pick(rng, frames)), alpha=float(f32(_pick(rng, (0.25, 0.125)))), dc_alpha=float(f32(_pick(rng, (0.25, 0.0625)))),
                    p_max=0.5, g_max=2.0, min_power=1e-10, p_init=float(f32(rng.uniform(-0.05, 0.05))), g_init=float(f32(rng.uniform(0.95, 1.05))),
                    dc_i_init=float(f32(rng.uniform(-0.01, 0.01))), dc_q_init=0.0)
    if name == "nb":
        frame = int(_pick(rng, frames))
        return dict(frame=frame, guard=int(rng.integers(0, 4)), max_hits=int(rng.integers(2, frame // 4 + 1)), threshold=float(f32(rng.uniform(5.0, 9.0))),
                    alpha=float(f32(_pick(rng, (0.25, 0.5)))), clamp=float(f32(_pick(rng, (1.5, 2.0, 4.0)))))
    if name == "tones":
        k = int(rng.integers(2, 6))
        freq = sorted(float(v) for v in rng.uniform(0.02, 0.45, k))
        return dict(coeffs=[_fl(r) for r in to.design(freq)], frame_blocks=int(_pick(rng, (1, 2, 3))), confirm=int(_pick(rng, (1, 2))),
                    release=int(_pick(rng, (1, 2))), ratio=float(f32(_pick(rng, (0.0, 0.0, 0.25 / na)))), min_power=float(f32(_pick(rng, (0.0, 1e-9, 1e-4)))))
    if name == "cwdec":                                         # (tests/test_gpu_cwdec.py: PAR)
        return dict(peak_attack=0.5, peak_decay=float(f32(_pick(rng, (0.01, 0.05)))), floor_attack=0.25, floor_decay=0.01, on_frac=0.4, off_frac=0.25,
                    snr=4.0, min_power=1e-12, debounce=int(_pick(rng, (1, 1, 2))), adapt=1, track=int(_pick(rng, (1, 2))), unit_min=256,
                    unit_init=2 * 256, unit_max=16 * 256, ring=int(_pick(rng, (16, 64))))
    if name == "afilt":
        per = bool(rng.random() < 0.35)
        ns = int(_pick(rng, (1, 2, 3)))

        def cascade():
            return [_fl(_highpass(rng.uniform(0.01, 0.05), 0.7071) if s == 0 else _notch(rng.uniform(0.05, 0.3), rng.uniform(1.0, 8.0))) for s in range(ns)]
        return dict(coeffs=[cascade() for _ in range(channels)] if per else cascade(), per_channel=per)
    if name == "nr":
        taps = int(_pick(rng, (8, 16, 32)))
        d = dict(kind=int(_pick(rng, (1, 2))), num_taps=taps, delay=int(_pick(rng, (1, 4, 8, 13))), mu=float(f32(_pick(rng, (0.05, 0.2, 0.5)))))
        if rng.random() < 0.3:
            d["coeffs_init"] = _fl(rng.uniform(-0.1, 0.1, taps))
        return d
    if name == "meter":
        open_level = 10.0 ** rng.uniform(-4.5, -2.0)
        return dict(sense=0, gate=int(rng.random() < 0.8), hang=int(_pick(rng, (0, 1, 2))), attack=float(f32(_pick(rng, (0.5, 1.0)))),
                    decay=float(f32(_pick(rng, (0.5, 0.9375)))), open_level=float(f32(open_level)), close_level=float(f32(open_level * 0.2)),
                    level_init=float(f32(_pick(rng, (0.0, 1e-3)))))
    L = int(_pick(rng, (1, 2, 4)))
    P = int(_pick(rng, (0, 3) if L == 1 else (2, 8, 13)))
    coeffs = _fl(design_lowpass(P * L, 0.4 / max(L, 2)) * f32(L)) if P else None
    return dict(interp=L, coeffs=coeffs, frames=int(rng.integers(2)))


def _draw_on(rng, pos):
    """which stages are on at the start: each with probability about 1/2; every fourth case seven or more, cases 0, 4 and 8 of a kind all nine"""
    on = [s for s in STAGES if rng.random() < 0.5]
    if pos % 4 == 0:
        want = 9 if pos < 12 else int(rng.integers(7, 10))
        off = [s for s in STAGES if s not in on]
        while len(on) < want:
            on.append(off.pop(int(rng.integers(len(off)))))
    return [s for s in STAGES if s in on]


# ---------------------------------------------------------------------------------------------------------------------------------------
# events
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tolerance(case):
    return case["spec"]["arith"] not in EXACT and not case["force_generic"]


def _lengths(case, on):
    s = case["spec"]
    na = s["block"] // s["decim"]
    cap = NLMS_MAX_AUDIO if "nr" in on else MAX_AUDIO
    ok = [b for b in LENGTHS + ((9,) if case["variant"] == "by4_b128" else ()) if b * na <= cap]
    if _tolerance(case) and s["agc"] and s["agc_global"]:
        # the twin that stands for the chain has no global gain, and rx_select.h cuts only calls without one: keep to the lengths both
        # instances run in one launch, so that both run the same kernels
        ok = [b for b in ok if not is_cut(case, s["mode"], b, False)]
    return ok, [1.0 if b < 9 else (4.0 if case["variant"] == "by4_b128" and b in (9, 17) else 0.5) for b in ok]


def _draw_events(rng, case):
    s = case["spec"]
    on, mode = list(case["on"]), s["mode"]
    glob = s["agc"] and s["agc_global"]
    n = int(rng.integers(3, 8))
    events, calls = [], 0
    while len(events) < n:
        last = len(events) == n - 1
        ops, w = ["process", "set_mode", "reset", "checkpoint", "drop_stage", "add_stage"], [5.0, 1.7, 1.0, 1.2, 1.0, 1.4]
        if glob:
            ops += ["global_one_call", "global_split" if "out" not in on else "refused_split"]
            w += [2.0, 5.0 if "out" not in on else (6.0 if last else 0.0)]
        op = _pick(rng, ops, w)
        if last and glob and case["idx"] % 4 == 3 and "out" not in on:
            op = "global_split"
        if len(events) == 1 and case["idx"] % 2 == 1:           # every second case: one stage, taken in turn, is set mid-stream
            op = "add_stage"
        if (last or not events) and op in ("set_mode", "reset", "drop_stage", "add_stage"):
            op = "process"                                      # a case starts and ends with a call
        if op in ("set_mode", "reset", "drop_stage", "add_stage") and events and events[-1]["op"] in ("set_mode", "reset", "drop_stage", "add_stage"):
            op = "process"                                      # ... and a call follows every life-cycle event: what it did shows
        if op == "drop_stage" and not on:
            op = "add_stage"
        if op == "add_stage" and len(on) == len(STAGES):
            op = "drop_stage"
        ev = dict(op=op)
        if op in ("process", "global_one_call", "global_split", "refused_split", "checkpoint"):
            ok, lw = _lengths(case, on)
            ev["blocks"] = int(_pick(rng, ok, lw))
            calls += 1
        if op in ("process", "checkpoint"):
            entry = _pick(rng, ENTRIES)
            # SELENITE_ARITH_SPLIT16 / _AUTO: the twin's f32 audio stands for the chain's, so an int16 call must run as the f32 call it is
            # converted to -- behind the I/Q correction, in front of an output stage, or with un-scaled audio wanted (rx_route.h: convert_in)
            if _tolerance(case) and entry.endswith("q15") and not (glob or "iqc" in on or "out" in on or any(k in on for k in UNSCALED)):
                entry = entry[:-3] + "f32"
            ev["entry"] = entry
        elif op == "set_mode":
            ev["mode"] = int(_pick(rng, [m for m in case["modes"] if m != mode] or [mode]))
            mode = ev["mode"]
        elif op == "drop_stage":
            ev["stage"] = on.pop(int(rng.integers(len(on))))
        elif op == "add_stage":
            turn = _turn(case["kind"], case["idx"])
            ev["stage"] = turn if len(events) == 1 and turn not in on else _pick(rng, [k for k in STAGES if k not in on])
            on = [k for k in STAGES if k in on or k == ev["stage"]]
        events.append(ev)
    return events


def _turn(kind, idx):
    """the stage an odd case of a kind sets mid-stream: the nine in turn, the kinds starting at different stages"""
    return STAGES[(idx // 2 + {"ssb": 0, "hilb": 6, "cw": 4, "generic": 6}[kind]) % len(STAGES)]


def one_case(seed, kind, idx, channels=None):
    """case idx of a kind; channels: that many in place of the draw (the ragged channel chunks of a host call want hundreds)"""
    rng = np.random.default_rng([seed, KINDS.index(kind), idx])
    variant, shape, modes, ariths, force = _draw_chain(rng, kind, idx)
    channels = int(_pick(rng, CHANNELS)) if channels is None else (int(_pick(rng, CHANNELS)), channels)[1]
    arith = int(_pick(rng, ariths))
    front_only = idx % 4 == 2                                   # every fourth case: nothing in front of the AGC wants un-scaled audio at the start
    agc = _pick(rng, ("off", "channel", "global"), (0.2, 0.4, 0.0 if front_only or (kind == "ssb" and idx % 3 == 1) else 0.4))
    if idx % 4 == 3 and not (kind == "ssb" and idx % 3 == 1):   # every fourth case: a global gain without an output stage, split in its last call
        agc = "global"
    spec = dict(channels=channels, mode=int(_pick(rng, modes)), arith=arith, agc=agc != "off", agc_global=agc == "global",
                q15_rounding=bool(rng.integers(2)), agc_params=dict(AGC_ODD) if rng.random() < 0.35 else None, **shape)
    spec.update(_draw_nco(rng, channels, kind, arith))
    case = dict(kind=kind, idx=idx, variant=variant, force_generic=force, modes=[int(m) for m in modes], spec=spec,
                auto_launches=int(_pick(rng, (1, 3))), signal_seed=_u32(rng))
    case["params"] = {name: _draw_stage(rng, name, shape, channels) for name in STAGES}
    case["on"] = _draw_on(rng, idx)
    if front_only:
        case["on"] = [k for k in case["on"] if k not in UNSCALED]
    if idx % 2 == 1 and _turn(kind, idx) in case["on"] and len(case["on"]) < 9:
        case["on"].remove(_turn(kind, idx))                     # (the stage this case sets mid-stream)
    if idx % 4 == 3 and "out" in case["on"]:
        case["on"].remove("out")
    if len(case["on"]) < 3 and arith not in EXACT:              # _SPLIT16 / _AUTO: at least three stages
        fill = ("spectrum", "iqc", "nb", "out") if front_only else ("iqc", "afilt", "meter")
        case["on"] = [k for k in STAGES if k in case["on"] or k in fill][:max(3, len(case["on"]))] if front_only else [k for k in STAGES if k in case["on"] or k in fill]
    case["events"] = _draw_events(rng, case)
    return case


def cases(seed=SEED, n=None, kind=None):
    for k in KINDS if kind is None else (kind,):
        for idx in range(COUNTS[k] if n is None else n):
            yield one_case(seed, k, idx)


def chunk_cases(seed=SEED, channels=300):
    """two cases with all nine stages on (cases 0 and 4 of "ssb") at `channels` channels: one call of 2048 samples through the host entry is
    then cut into ragged channel chunks (tests/test_gpu_stage_chunks.py: the smallest such shape)"""
    out = [one_case(seed, "ssb", idx, channels) for idx in (0, 4)]
    assert all(len(c["on"]) == len(STAGES) for c in out)
    return out


def build_spec(case, **over):
    s = dict(case["spec"], **over)
    return rc.ChainSpec(s["channels"], s["block"], s["decim"], s["nd_taps"], s["nh_taps"], s["n_biquad"], s["mode"], s["arith"], nco=s["nco"],
                        nco_step_all=s["nco_step_all"], nco_steps=s["nco_steps"], agc=s["agc"], agc_global=s["agc_global"],
                        agc_params=s["agc_params"], q15_rounding=s["q15_rounding"])


def oracle_arith(case):
    """the arithmetic of the oracle chain: the instance's own; SELENITE_ARITH_AUTO on the generic kernels is the CMSIS arithmetic; None where
    the chain is tolerance-based and its audio comes from a twin instance"""
    if case["spec"]["arith"] in EXACT:
        return case["spec"]["arith"]
    return rc.ARITH_CMSIS if case["force_generic"] else None


def pipeline_of(case, on=None, mode=None):
    """the composed oracle of a case (tests/rx_pipeline_oracle.py) with the stages `on` (default: the case's own at its start)"""
    import rx_pipeline_oracle as po
    arith = oracle_arith(case)
    over = {} if arith is None else dict(arith=arith)
    if mode is not None:
        over["mode"] = mode
    return po.Pipeline(build_spec(case, **over), {k: case["params"][k] for k in (case["on"] if on is None else on)})


# ---------------------------------------------------------------------------------------------------------------------------------------
# the input
# ---------------------------------------------------------------------------------------------------------------------------------------
def envelope(seed, channels, first, count, block):
    """the keying of `count` input samples from sample `first` (tests/test_gpu_cwdec.py: envelope): per channel marks of about 2 or 6 DSP blocks
    and spaces of about 2, 6 or 14, each a few per cent off and so with its edges off the block grid; 0.03 up, 1 down"""
    env = np.empty((channels, count), f32)
    for c in range(channels):
        rng = np.random.default_rng([seed, 3, c])
        runs, total, down = [], 0, False
        while total < first + count:
            blocks = rng.choice([2, 6]) if down else rng.choice([2, 2, 6, 6, 14])
            n = max(1, int(blocks * block * rng.uniform(0.9, 1.1)))
            runs.append(np.full(n, 1.0 if down else 0.03, f32))
            total += n
            down = not down
        env[c] = np.concatenate(runs)[first:first + count]
    return env


IMPULSE_CHUNK = 2048


def signal(case, first, count, channels=None):
    """f32 [channels][count][2]: the suite's synthetic I/Q (rc.synth_iq) at LEVEL under the keying envelope (marks and spaces for the decoder,
    an open and a closed gate), with a fixed gain and phase imbalance and a DC offset per channel (the I/Q correction) and sparse large
    impulses (the blanker)"""
    ch = case["spec"]["channels"] if channels is None else channels
    seed = case["signal_seed"]
    x = rc.synth_iq(0, ch, first, count) * (envelope(seed, ch, first, count, case["spec"]["block"]) * f32(LEVEL))[:, :, None]
    rng = np.random.default_rng([seed, 5])
    gain, phase = rng.uniform(0.92, 1.08, ch), np.radians(rng.uniform(-4.0, 4.0, ch))
    dc = rng.uniform(-0.02, 0.02, (ch, 2))
    i, q = x[:, :, 0].astype(np.float64), x[:, :, 1].astype(np.float64)
    out = np.empty((ch, count, 2), f32)
    out[:, :, 0] = i + dc[:, :1]
    out[:, :, 1] = gain[:, None] * (q * np.cos(phase)[:, None] + i * np.sin(phase)[:, None]) + dc[:, 1:]
    for k in range(first // IMPULSE_CHUNK, (first + count + IMPULSE_CHUNK - 1) // IMPULSE_CHUNK):
        rng = np.random.default_rng([seed, 7, k])
        hit = rng.random((ch, IMPULSE_CHUNK)) < 1.0 / 400.0
        amp = np.where(rng.random((ch, IMPULSE_CHUNK, 2)) < 0.5, -2.5, 2.5).astype(f32)
        lo, hi = max(first, k * IMPULSE_CHUNK), min(first + count, (k + 1) * IMPULSE_CHUNK)
        m = hit[:, lo - k * IMPULSE_CHUNK:hi - k * IMPULSE_CHUNK]
        out[:, lo - first:hi - first][m] = amp[:, lo - k * IMPULSE_CHUNK:hi - k * IMPULSE_CHUNK][m]
    return out


def to_q15(iq):
    return np.clip(np.trunc(iq * 32768.0), -32768, 32767).astype(np.int16)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host's rules, restated
# ---------------------------------------------------------------------------------------------------------------------------------------
def kernel_family(case, mode):
    """"ssb_fused", "cw_fused" or "generic": what serves a call in front of the stages (rx_select.h: plan_shape with designed taps -- every mode
    of the fuzz runs on an SSB fused kernel where the chain has a FIR pair and DSP blocks of 4 .. 256 audio samples, a multiple of four;
    rx_cw.hip: cw_fused_ok)"""
    s = case["spec"]
    if case["force_generic"]:
        return "generic"
    na = s["block"] // s["decim"]
    cw = mode in (rc.MODE_CW, rc.MODE_CWR)
    if s["nh_taps"] and 4 <= na <= 256 and na % 4 == 0 and not (cw and s["n_biquad"]):
        return "ssb_fused"
    if cw and not s["nd_taps"] and s["decim"] == 1 and not s["nh_taps"] and s["n_biquad"] in (2, 4, 8):
        return "cw_fused"
    return "generic"


def is_cut(case, mode, blocks, glob_call):
    """rx_select.h: a split-precision call behind a decimator that ends in a partial pass shorter than a decimator history is two launches"""
    s = case["spec"]
    if not _tolerance(case) or kernel_family(case, mode) != "ssb_fused" or not s["nd_taps"] or glob_call:
        return False
    na = s["block"] // s["decim"]
    tq = (256 // na * na) * s["decim"]
    m = s["decim"]
    hs = (((s["nd_taps"] - 1 + m - 1) // m + 3) & ~3) * m
    bs = blocks * s["block"]
    return bs > tq and bs % tq != 0 and bs % tq < hs


def walk(case):
    """per planned call (events "process", "checkpoint", "global_one_call", "global_split", "refused_split"): (event index, facts)"""
    s = case["spec"]
    on, mode, prev = list(case["on"]), s["mode"], "init"
    glob = bool(s["agc"] and s["agc_global"])
    for i, ev in enumerate(case["events"]):
        op = ev["op"]
        if op == "set_mode":
            mode, prev = ev["mode"], "set_mode"
        elif op == "reset":
            prev = "reset"
        elif op == "drop_stage":
            on.remove(ev["stage"])
            prev = "drop_stage:" + ev["stage"]
        elif op == "add_stage":
            on = [k for k in STAGES if k in on or k == ev["stage"]]
            prev = "add_stage:" + ev["stage"]
        else:
            entry = ev.get("entry", "dev_f32")
            q15 = entry.endswith("q15")
            fam = kernel_family(case, mode)
            phase = {"global_one_call": "one_call", "global_split": "split", "refused_split": "refused"}.get(op, "all")
            # the launches of the call as route() sees them: the I/Q correction leaves f32, the output stage takes f32 and stores itself
            src_q15 = q15 and "iqc" not in on and "out" not in on
            dst_q15 = q15 and "out" not in on
            base = dict(src_q15=src_q15, dst_q15=dst_q15, agc=bool(s["agc"]), glob=glob, on={k: k in on for k in UNSCALED},
                        gate=bool("meter" in on and case["params"]["meter"]["gate"]), force=case["force_generic"], ssb=fam == "ssb_fused",
                        cw=fam == "cw_fused", cwbq=bool(mode in (rc.MODE_CW, rc.MODE_CWR) and s["n_biquad"]),
                        words=s["arith"] == rc.ARITH_AUTO)
            launches = [] if phase == "refused" else [dict(base, phase=p) for p in ((1, 2) if phase in ("one_call", "split") else (0,))]
            cut = phase == "all" and is_cut(case, mode, ev["blocks"], glob)
            if cut:
                launches = launches * 2
            yield i, dict(kernel=fam, arith=s["arith"], q15=q15, on=tuple(on), cut=cut, phase=phase, mode=mode,
                          gate_out=bool(base["gate"] and "out" in on), entry=entry, prev="checkpoint" if op == "checkpoint" else prev,
                          blocks=ev["blocks"], launches=launches)
            prev = "call"
