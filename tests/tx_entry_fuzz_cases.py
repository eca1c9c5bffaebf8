"""The case generator of the TX entry fuzz (tests/test_gpu_tx_fuzz.py: the KEY and IN slices): tests/tx_fuzz_cases.py's twin for instances
with a keyed CW path (selenite_tx_set_cw, k_tx_cw) and an audio input stage (selenite_tx_set_in, k_tx_in), on which one instance has three
kinds of entry -- audio calls, key calls, frame calls -- that all move nco_phase, interp_state, the host's phase_uniform / phase_host and
the cached LO table.  The conventions are tx_fuzz_cases's: plain dict cases, a random stream per (seed, kind, index), no rejected draws,
case k independent of n.  The shape, tap, NCO, FM and level draws are imported from there and not changed; the cases of kinds A, B and
FM stay what they were (tests/test_tx_entry_fuzz_cases.py pins their digest).

Kinds: "KEY" an instance with set_cw (set_fm in about a third), "IN" an instance with set_in (set_cw and set_fm in about half each); the
fused geometry (all tap variants) in half of the cases, generic shapes in the other half, all three arithmetics.

walk(case) restates the HOST's rules for the three entries (csrc/tx_select.h: tx_select; csrc/tx_api.hip: run(), reset_state,
selenite_tx_set_state; csrc/tx_cw.hip: run_key; csrc/tx_in.hip: run_frames, launch_in): with tx_fuzz_cases.walk the one restatement of
the rule outside tx_select.h (tests/test_tx_select.py holds the C++ rule against both).  cw_lds_bytes and in_lds_bytes restate cw_layout
and in_layout as tx_lds_bytes restates tx_layout.

A refused call latches the instance's status (tx_host.h: fail), so a refusal is the last event of its case.

TEST INFRASTRUCTURE.  Nothing here is imported by the product.
"""
import numpy as np

import gain_law_cases as gl
import rxcommon as rc
import tx_fuzz_cases as fz
from tx_fuzz_cases import FM, LDS_LIMIT, MAX_OUT, MODES, SEED, _pick, _u32, _up4

f32 = np.float32
KINDS = ("KEY", "IN")
COUNTS = {"KEY": 48, "IN": 64}                    # the default slices of the two GPU tests (profiles/tx_entry_fuzz/README.md: times)
STREAM = {"KEY": 3, "IN": 4}                      # the random streams behind those of tx_fuzz_cases.KINDS
CW, CWR = rc.MODE_CW, rc.MODE_CWR
MONO, LEFT, RIGHT, MIX = 0, 1, 2, 3
ENTRIES = ("f32_dev", "q15_dev", "q15f_dev", "f32_host", "q15_host")      # the five frame entries; q15f: int16 frames, f32 I/Q
NS_TAPS = (1, 2, 3, 63, 64, 65, 256)
ND_TAPS = (1, 2, 3, 63, 64, 65, 97, 255, 256)
MAX_IN = 400000                                   # input words of one frame call over all channels: MAX_OUT's analogue (the oracle's decimator)
BIG = ((136, 8), (200, 8), (264, 8), (264, 4), (520, 2), (1030, 1))      # (block, M) with block * M > 1024: more than one chunk per tile
FRAME_LEVEL = (1e-2, 10.0 ** -0.5)                # the frame levels: what a VOX threshold 60 dB under full scale tells apart (_draw_in)


def scale_count(kind, env_value):
    """SELENITE_FUZZ_CASES=<n> scales the two slices as it scales tx_fuzz_cases's: by n over the default sum of the three old slices"""
    if not env_value:
        return COUNTS[kind]
    return max(1, int(env_value) * COUNTS[kind] // sum(fz.COUNTS.values()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# LDS of k_tx_cw and k_tx_in, in bytes (csrc/tx_cw.hip: cw_layout, csrc/tx_in.hip: in_tile, in_layout), and launch_in's 16-byte rule
# ---------------------------------------------------------------------------------------------------------------------------------------
def cw_lds_bytes(block, L, ni, ns):
    P = ni // L if ni else 1
    return 4 * (516 + _up4(ni) + _up4(ns) + _up4((ns - 1) + block) + _up4((P - 1) + block))


def in_tile(block, M):
    want = 1024 // M
    return block if block >= want else block * (want // block)


def in_lds_bytes(block, M, nt):
    tile = in_tile(block, M)
    rs = tile + (max(nt - 1, 0) + M - 1) // M
    nblk = tile // block
    return 4 * (_up4(M * rs) + _up4(nblk * (block | 1)) + nblk)


def in_wide(block, M, fw, itemsize, bs):
    """16 bytes per lane: every row and every tile start on a 16-byte boundary (the source pointer is a buffer's start)"""
    return (bs * M * fw * itemsize) % 16 == 0 and (in_tile(block, M) * M * fw * itemsize) % 16 == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the draws
# ---------------------------------------------------------------------------------------------------------------------------------------
def _draw_cw(rng, channels, ns=None):
    if ns is None:
        ns = int(_pick(rng, NS_TAPS + (int(rng.integers(1, 301)),)))
    per = bool(rng.random() < 0.5)
    return dict(ns_taps=ns, shape_seed=_u32(rng), amplitude=float(f32(rng.uniform(0.2, 1.2) * (-1.0 if rng.random() < 0.25 else 1.0))),
                offset_step=int(_pick(rng, (0, int(rng.integers(1, 1 << 24)), _u32(rng)), (0.15, 0.6, 0.25))),
                side=_pick(rng, ("none", "store", "mix"), (0.3, 0.35, 0.35)), side_level=float(f32(rng.uniform(0.05, 0.9))),
                side_step_all=_u32(rng), side_steps=[_u32(rng) for _ in range(channels)] if per else None, hang_blocks=int(rng.integers(0, 4)))


def cw_args(cw):
    """the keyword arguments of sr.Tx.set_cw and TxCwOracle.set_cw"""
    return dict(shape=fz._dense(cw["shape_seed"], cw["ns_taps"]), amplitude=cw["amplitude"], offset_step=cw["offset_step"],
                side_level=cw["side_level"], side_step=np.array(cw["side_steps"], np.uint32) if cw["side_steps"] else cw["side_step_all"],
                side_mix=int(cw["side"] == "mix"), hang_blocks=cw["hang_blocks"])


def _draw_in(rng, M=None, nd=None):
    if M is None:
        M = int(_pick(rng, (1, 2, 4, 8)))
    if nd is None:
        nd = int(_pick(rng, ND_TAPS + (M, int(rng.integers(1, 257))) + ((0, 0) if M == 1 else ())))
    seed = _u32(rng)
    gain = float(f32(10.0 ** rng.uniform(-0.5, 0.5) * (-1.0 if rng.random() < 0.3 else 1.0)))
    vox = _pick(rng, ("none", "flag", "gate"), (0.2, 0.3, 0.5))
    # the threshold: the mean square of frames at 1e-3 of full scale behind gain and decimator (white frames: the taps' root sum of
    # squares); a frame level of FRAME_LEVEL is 20 ... 50 dB above it, a stretch 60 dB down at least 10 dB under it
    rss = float(np.sqrt((fz._dense(seed, nd).astype(np.float64) ** 2).sum())) if nd else 1.0
    open_level = float(f32((1e-3 * abs(gain) * rss) ** 2 / 3.0))
    return dict(M=M, nd_taps=nd, coeffs_seed=seed, pick=int(rng.integers(0, 4)), gain=gain, vox=vox, hang=int(rng.integers(0, 4)),
                attack=float(_pick(rng, (1.0, 0.75, 0.5))), decay=float(_pick(rng, (1.0, 0.875, 0.75))), open_level=open_level,
                close_level=float(f32(open_level * 0.25)))


def in_args(inp):
    """the keyword arguments of sr.Tx.set_in and TxInOracle.set_in"""
    vox = None
    if inp["vox"] != "none":
        vox = dict(gate=int(inp["vox"] == "gate"), hang=inp["hang"], attack=inp["attack"], decay=inp["decay"], open_level=inp["open_level"],
                   close_level=inp["close_level"], level_init=0.0)
    return dict(M=inp["M"], coeffs=fz._dense(inp["coeffs_seed"], inp["nd_taps"]) if inp["nd_taps"] else None, pick=inp["pick"],
                gain=inp["gain"], vox=vox)


def _fw(inp):
    return 1 if inp["pick"] == MONO else 2


def _clamp_channels(channels, per_channel_out, per_channel_in):
    """the largest channel count of CHANNELS, at most the drawn one, at which one DSP block stays within MAX_OUT and MAX_IN"""
    ok = [c for c in fz.CHANNELS if c <= channels and c * per_channel_out <= MAX_OUT and c * per_channel_in <= MAX_IN]
    return max(ok) if ok else 1


def _blocks(rng, case, frames_of=None, whole=0.5):
    s = case["spec"]
    if case["family"] == "A" and rng.random() < whole:             # whole passes of the matrix kernels
        blocks = int(_pick(rng, (4, 8)))
    else:
        blocks = int(rng.integers(1, 9))
    blocks = min(blocks, MAX_OUT // (s["channels"] * s["block"] * s["interp"]))
    if frames_of is not None:
        blocks = min(blocks, MAX_IN // (s["channels"] * s["block"] * frames_of["M"] * _fw(frames_of)))
    return max(1, blocks)


def _draw_key_call(rng, case, st, op, blocks=None):
    return dict(op=op, blocks=_blocks(rng, case, whole=0.0) if blocks is None else blocks, q15=bool(rng.random() < 0.4),
                device=bool(rng.random() < 0.5), seed=_u32(rng))


def _draw_frame_call(rng, case, st, op):
    blocks = _blocks(rng, case, st["inp"])
    level = 10.0 ** rng.uniform(np.log10(FRAME_LEVEL[0]), np.log10(FRAME_LEVEL[1]))
    if st["flevel"] is not None:                                   # (at most 80 dB from the call before: the range is 30 dB wide)
        level = min(max(level, st["flevel"] * 1e-4), st["flevel"] * 1e4)
    st["flevel"] = level
    a, b = sorted(int(v) for v in rng.integers(0, blocks + 1, 2))
    quiet = _pick(rng, (None, [0, blocks], [a, b], [a, blocks], [0, b]), (0.25, 0.1, 0.35, 0.15, 0.15))
    return dict(op=op, entry=_pick(rng, ENTRIES), blocks=blocks, level=float(f32(level)), quiet=quiet, seed=_u32(rng))


def _draw_entry_events(rng, case, script):
    s, kind = case["spec"], case["kind"]
    steps = s["nco_steps"]
    uniform_step = s["nco"] and (steps is None or len(set(steps)) == 1)
    st = dict(level=None, flevel=None, at=int(rng.integers(0, 4096)), mode=s["mode"], cw=case["cw"], inp=case["inp"])
    n = int(rng.integers(3, 8))
    events = []

    def audio_call():
        return fz._draw_call(rng, case, st, "process")

    for op in script:                                              # a scripted head (make_case), then random events up to n
        if op[0] == "audio":
            events.append(audio_call())
        elif op[0] == "audio_whole":                               # whole passes of the matrix kernels (MAX_OUT holds four blocks at 130 channels)
            events.append(dict(audio_call(), blocks=int(_pick(rng, (4, 4, 8) if s["channels"] <= 65 else (4,)))))
        elif op[0] == "set_mode":
            st["mode"] = op[1]
            events.append(dict(op="set_mode", mode=op[1]))
        else:
            events.append(_draw_key_call(rng, case, st, "key", blocks=op[1]))
    n = max(n, len(events) + 1)
    while len(events) < n:
        last, room = len(events) == n - 1, n - len(events)
        keyable = st["cw"] is not None and st["mode"] in (CW, CWR)
        o = {}
        if kind == "KEY":
            if keyable:
                o.update(key=0.45, key_checkpoint=0.1, audio=0.3)
            else:
                o.update(audio=0.35)
        else:
            o.update(frames=0.45, frames_checkpoint=0.08, audio=0.1)
            if keyable:
                o.update(key=0.2)
        if last:
            if len(events) >= 2:                                   # a refusal ends the case (module docstring)
                if st["cw"] is not None and not keyable:
                    o.update(refused_key=0.15)
        else:
            o.update(set_mode=0.1, reset=0.09)
            if case["fm"] is not None and st["mode"] != FM:
                o.update(to_fm=0.15)
            if st["cw"] is not None and not keyable:
                o.update(to_cw=0.4 if kind == "KEY" else 0.12)
            if st["cw"] is not None:
                o.update(set_cw_same=0.05, set_cw_new=0.05)
            if kind == "IN":
                o.update(set_in_same=0.04, set_in_new=0.04)
                if room == 2 and len(events) >= 1:
                    o.update(clear_in_refused=0.3)
            if uniform_step:
                o.update(set_phase=0.08)
        op = _pick(rng, tuple(o), tuple(o.values()))
        if op == "audio":
            events.append(audio_call())
        elif op in ("key", "key_checkpoint"):
            events.append(_draw_key_call(rng, case, st, op))
        elif op in ("frames", "frames_checkpoint"):
            events.append(_draw_frame_call(rng, case, st, op))
        elif op in ("set_mode", "to_cw", "to_fm"):
            modes = (CW, CWR) if op == "to_cw" else (FM,) if op == "to_fm" else MODES + ((FM,) if case["fm"] else ())
            st["mode"] = int(_pick(rng, modes))
            events.append(dict(op="set_mode", mode=st["mode"]))
        elif op == "reset":
            events.append(dict(op="reset"))
        elif op == "set_phase":
            events.append(dict(op="set_phase", phase=_u32(rng)))
        elif op in ("set_cw_same", "set_cw_new"):
            ns = st["cw"]["ns_taps"]
            st["cw"] = _draw_cw(rng, s["channels"], ns if op == "set_cw_same" else ns + int(rng.integers(1, 9)))
            events.append(dict(op="set_cw", cw=st["cw"]))
        elif op in ("set_in_same", "set_in_new"):
            nd = st["inp"]["nd_taps"]
            if op == "set_in_same":                                # a retune: gain, pick, taps and the VOX law change, M and nd_taps stay
                new = _draw_in(rng, st["inp"]["M"], nd)
            else:                                                  # (nd_taps = 0 goes with M = 1 alone)
                new = _draw_in(rng, st["inp"]["M"], nd + int(rng.integers(1, 9)) if nd < 248 else nd - int(rng.integers(1, 9)))
            new["pick"] = new["pick"] if _fw(new) == _fw(st["inp"]) else st["inp"]["pick"]      # the words of a DSP block stay: MAX_IN holds
            st["inp"] = new
            events.append(dict(op="set_in", inp=new))
        elif op == "refused_key":
            events.append(dict(op="refused_key", q15=bool(rng.random() < 0.5)))
        else:
            assert op == "clear_in_refused"
            events += [dict(op="clear_in"), dict(op="refused_frames", entry=_pick(rng, ENTRIES[:3]))]
    return events


def make_case(seed, kind, idx):
    rng = np.random.default_rng([seed, STREAM[kind], idx])
    family = "A" if rng.random() < 0.5 else "B"
    shape, taps = fz._draw_family_a(rng, "A") if family == "A" else fz._draw_family_b(rng)
    channels = int(_pick(rng, fz.CHANNELS, (1, 1, 1, 1, 0.5, 0.5, 0.5, 0.5)))
    arith = int(_pick(rng, (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16), (0.28, 0.28, 0.44) if family == "A" else (0.35, 0.35, 0.3)))
    alc = _pick(rng, ("off", "default") + gl.SET_NAMES, (0.15, 0.4, 0.15, 0.15, 0.15))
    has_cw = kind == "KEY" or rng.random() < 0.5
    has_fm = rng.random() < (1.0 / 3 if kind == "KEY" else 0.5)
    mode = int(_pick(rng, (CW, CWR))) if has_cw and rng.random() < 0.6 else int(_pick(rng, MODES))
    inp, script = None, []
    variant = rng.random()
    if kind == "IN":
        inp = _draw_in(rng)
        if family == "B" and variant < 0.3:                        # a DSP block of more than 1024 input samples
            shape["block"], inp["M"] = (int(rng.integers(129, 201)), 8) if rng.random() < 0.25 else _pick(rng, BIG)
            if inp["nd_taps"] == 0:
                inp["nd_taps"] = inp["M"]
    elif family == "B" and variant < 0.25:
        # a key call shorter than the interpolator history behind an audio call that left the Q rail something: P - 1 >= 19 samples of
        # history, DSP blocks of 1 ... 8, a first key call of 1 or 2 of them
        L, P = int(_pick(rng, (2, 3, 4, 5, 8))), int(rng.integers(20, 41))
        shape.update(block=int(_pick(rng, (1, 2, 3, 5, 8))), interp=L, ni_taps=P * L)
        if taps["ic"][0] == "designed" and rng.random() < 0.5:
            taps["ic"] = ["dense", _u32(rng)]
        mode = int(_pick(rng, (rc.MODE_USB, rc.MODE_LSB)))
        script = [("audio",), ("set_mode", int(_pick(rng, (CW, CWR)))), ("key", int(rng.integers(1, 3))), ("key", int(rng.integers(1, 6)))]
    elif family == "A" and variant < 0.4:                          # a key call, then whole passes of the matrix kernels on the phases it left
        mode = int(_pick(rng, (CW, CWR)))
        script = [("key", None), ("audio_whole",)]
    elif has_fm and variant < 0.7:                                 # from a key call into FM and back
        mode = int(_pick(rng, (CW, CWR)))
        script = [("key", None), ("set_mode", FM), ("audio",), ("set_mode", int(_pick(rng, (CW, CWR)))), ("key", None)]
    channels = _clamp_channels(channels, shape["block"] * shape["interp"], shape["block"] * inp["M"] * 2 if inp else 0)
    spec = dict(channels=channels, mode=mode, arith=arith, alc=alc != "off", alc_set=alc if alc in gl.SETS else None,
                q15_rounding=int(rng.integers(0, 2)), **shape)
    spec.update(fz._draw_nco(rng, channels, "B"))
    case = dict(kind=kind, idx=idx, seed=seed, family=family, spec=spec, taps=taps, fm=fz._draw_fm(rng, channels) if has_fm else None,
                cw=_draw_cw(rng, channels) if has_cw else None, inp=inp)
    case["events"] = _draw_entry_events(rng, case, script)
    return case


def cases(seed=SEED, n=None, kind=None):
    """kind: one of KINDS (n cases of it, COUNTS[kind] by default), or None: the two default slices one behind the other (n: of each)"""
    for k in (KINDS if kind is None else (kind,)):
        for idx in range(COUNTS[k] if n is None else n):
            yield make_case(seed, k, idx)


# ---------------------------------------------------------------------------------------------------------------------------------------
# from a description to the inputs of a call
# ---------------------------------------------------------------------------------------------------------------------------------------
build_spec, fm_args, audio, expected_kernel = fz.build_spec, fz.fm_args, fz.audio, fz.expected_kernel
PATTERNS = ("held", "up", "runs", "bytes")


def key_patterns(case, ev):
    r = np.random.default_rng([ev["seed"], 1])
    return [PATTERNS[int(v)] for v in r.choice(4, case["spec"]["channels"], p=(0.15, 0.1, 0.5, 0.25))]


def keys(case, ev):
    """[channels][blocks * block] uint8; per channel: held (all 1), up (all 0), runs (elements and gaps of random length, 1 and 0) or
    bytes (the same with any non-zero byte for key-down)"""
    s = case["spec"]
    n = ev["blocks"] * s["block"]
    r = np.random.default_rng([ev["seed"], 2])
    k = np.zeros((s["channels"], n), np.uint8)
    for c, pat in enumerate(key_patterns(case, ev)):
        if pat == "held":
            k[c] = 1
        elif pat != "up":
            run = int(_pick(r, (2, 7, 40, 200)))
            at, v = 0, int(r.integers(0, 2))
            while at < n:
                ln = int(r.integers(1, 2 * run))
                if v:
                    k[c, at:at + ln] = 1 if pat == "runs" else r.integers(1, 256, min(ln, n - at))
                at, v = at + ln, 1 - v
    return k


def side_in(case, ev):
    """what the sidetone buffer holds in front of a key call (a mix adds to it): f32, or int16 for a q15 call"""
    s = case["spec"]
    x = np.random.default_rng([ev["seed"], 3]).uniform(-0.5, 0.5, (s["channels"], ev["blocks"] * s["block"]))
    return np.round(x * 32768).astype(np.int16) if ev["q15"] else x.astype(f32)


def frames(case, ev, inp):
    """[channels][blocks * block * M * (1 or 2)] f32 or int16: white at the event's level, the quiet DSP blocks 60 dB down"""
    s = case["spec"]
    per = s["block"] * inp["M"] * _fw(inp)
    x = np.random.default_rng([ev["seed"], 4]).uniform(-1.0, 1.0, (s["channels"], ev["blocks"] * per)) * ev["level"]
    if ev["quiet"]:
        x[:, ev["quiet"][0] * per:ev["quiet"][1] * per] *= 1e-3
    if ev["entry"].startswith("f32"):
        return x.astype(f32)
    return np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host's rules for the three entries, restated
# ---------------------------------------------------------------------------------------------------------------------------------------
def walk(case):
    """(event index, record) for every planned call, a checkpoint's call twice; refused calls are not planned calls.  record, beyond
    tx_fuzz_cases.walk's: entry (audio / key / frames), kernel with the family "cw", prev_entry, next_entry (filled in behind the walk),
    tags with reset_behind_key, set_phase_behind_key and restore_behind_key, and what the coverage test counts: for a key call side, ns,
    block, L and short (shorter than the interpolator history while the Q rail holds what an audio call left there); for a frame call
    fentry, M, pick, nd, chunks (1024-sample chunks of the first tile), tiles, wide (launch_in's 16-byte path) and vox."""
    s = case["spec"]
    steps = s["nco_steps"] if s["nco_steps"] is not None else [s["nco_step_all"]] * s["channels"]
    steps_same = len(set(steps)) == 1
    inst = fz.FAMILY[fz.expected_kernel(case, rc.MODE_USB)]
    p1 = s["ni_taps"] // s["interp"] - 1 if s["ni_taps"] else 0
    fm, cw, inp = case["fm"], case["cw"], case["inp"]
    mode, prev, prev_entry = s["mode"], None, None
    uniform, equal, dirty, qlive = steps_same, True, frozenset(), False      # dirty: FM / key calls since the phases were repaired
    tags = set()
    out = []

    def call(ev, entry):
        nonlocal uniform, equal, dirty, qlive, prev, prev_entry, tags
        bs, was_uniform, was_qlive = ev["blocks"] * s["block"], uniform, qlive
        if entry == "key":
            fam, flavour = "cw", "perchan" if s["nco"] else "off"
            uniform, dirty = False, dirty | {"key"}                 # the offset went into every phase; equal phases stay equal
            qlive = False                                           # (counted directly behind the audio call only)
        elif mode == FM:
            fam, flavour = "fm", "nco" if s["nco"] else "zero_if"
            uniform, equal, dirty = False, s["channels"] == 1, dirty | {"fm"}
            qlive = False
        else:
            qlive = mode != rc.MODE_AM and p1 > 0
            if inst != "generic" and bs % 256 == 0:
                fam = inst
                if not s["nco"]:
                    flavour = "off"
                elif uniform:
                    flavour = "periodic" if inst == "split16" and steps[0] & 0x00FFFFFF == 0 else "table"
                else:
                    flavour = "perchan"
            else:
                fam, flavour = "generic", "off" if not s["nco"] else "perchan"
        rec = dict(entry=entry, kernel=fam, flavour=flavour, mode=mode, prev=prev, prev_entry=prev_entry, next_entry=None,
                   tags=frozenset(tags), bs=bs, uniform=was_uniform, steps_same=steps_same and s["nco"], arith=s["arith"], inst=inst)
        if entry == "key":
            rec.update(q15=ev["q15"], device=ev["device"], side=cw["side"], ns=cw["ns_taps"], block=s["block"], L=s["interp"],
                       short=was_qlive and bs < p1)
        elif entry == "frames":
            e, fw = ev["entry"], _fw(inp)
            tile = in_tile(s["block"], inp["M"])
            rec.update(q15=e.startswith("q15_"), device=e.endswith("_dev"), fentry=e, M=inp["M"], pick=inp["pick"], nd=inp["nd_taps"],
                       chunks=-(-min(bs, tile) * inp["M"] // 1024), tiles=-(-bs // tile), vox=inp["vox"],
                       wide=in_wide(s["block"], inp["M"], fw, 4 if e.startswith("f32") else 2, bs))
        else:
            rec.update(q15=ev["q15"], device=ev["device"])
        prev, prev_entry, tags = fam, entry, set()
        out.append(rec)
        return rec

    for i, ev in enumerate(case["events"]):
        op = ev["op"]
        if op == "set_mode":
            mode = ev["mode"]
        elif op == "set_cw":
            cw = ev["cw"]
        elif op == "set_in":
            inp = ev["inp"]
        elif op in ("reset", "set_phase"):
            tags |= {op + "_behind_" + d for d in dirty}
            uniform, equal, dirty = steps_same, True, frozenset()
            if op == "reset":
                qlive = False
        elif op in ("process", "key", "frames"):
            call(ev, {"process": "audio"}.get(op, op))
            yield i, out[-1]
        elif op in ("key_checkpoint", "frames_checkpoint"):
            entry = op.split("_")[0]
            before = (steps_same and equal, equal, dirty, qlive)
            call(ev, entry)
            yield i, out[-1]
            tags |= {"restore_behind_" + d for d in dirty}
            uniform, equal, dirty, qlive = before           # selenite_tx_set_state: uniform when the restored phases are all the same
            call(ev, entry)
            yield i, out[-1]
        else:
            assert op in ("refused_key", "clear_in", "refused_frames"), op
    for a, b in zip(out, out[1:]):                          # (for a caller that ran the generator to its end)
        a["next_entry"] = b["entry"]


def walked(case):
    """walk(case) run to its end: the records with next_entry filled in"""
    return list(walk(case))
