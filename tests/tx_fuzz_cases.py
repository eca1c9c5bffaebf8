"""The case generator of the TX fuzz (tests/test_gpu_tx_fuzz.py): deterministic, free of GPU calls, never rejects a draw.

cases(seed, n, kind) yields plain descriptions -- numbers, strings, lists and dicts only, so that a failing case prints whole and can be
pasted into a directed test: the spec arguments, how the taps were overwritten, the FM setting and a list of events.  build_spec(case)
makes the rc.TxSpec (taps overwritten as described), audio(case, event) the input of a call.  Every case has a random stream of its own
(seed, kind, index), so case k of a kind is the same whatever n is.

expected_kernel(case, mode) and walk(case) restate the HOST's rules (csrc/tx_select.h: tx_select; csrc/tx_api.hip: run(), reset_state,
selenite_tx_set_state): which kernel an instance reports, which kernel serves a call of a given length and from which phase source.  They
read the taps the way selenite_tx_init classifies them.  This is the one restatement of the rule outside tx_select.h, kept deliberately
as the independent check: tests/test_tx_select.py holds the C++ rule against it on every planned call of the committed cases.  tests/test_tx_fuzz_cases.py asserts on the CPU that the committed seed and counts
reach every form, so coverage is a checked property of the generator.

Kinds: "A" the fused geometry without FM events, "B" generic shapes without FM events, "FM" both families with an FM setting.

TEST INFRASTRUCTURE.  Nothing here is imported by the product.
"""
import numpy as np

import gain_law_cases as gl
import rxcommon as rc

f32 = np.float32
SEED = 20261020
KINDS = ("A", "B", "FM")
COUNTS = {"A": 40, "B": 40, "FM": 80}          # the default slices of the three GPU tests (profiles/tx_fuzz/README.md: times)
FM = rc.MODE_FM
MODES = (rc.MODE_LSB, rc.MODE_USB, rc.MODE_CW, rc.MODE_CWR, rc.MODE_AM, rc.MODE_DIG, rc.MODE_PKT)
GENERIC, FUSED, SPLIT16, KFM = "k_tx_generic", "k_tx_fused<4,256,63>", "k_tx_split16<4,256,63>", "k_tx_fm"
FAMILY = {GENERIC: "generic", FUSED: "fused", SPLIT16: "split16", KFM: "fm"}
CHANNELS = (1, 2, 3, 5, 63, 64, 65, 130)
B_INTERP = (1, 2, 3, 4, 5, 8)
B_NH = (0, 1, 2, 3, 15, 16, 63, 64, 129)
MAX_OUT = 160000                                # complex output samples of one call over all channels: the CPU oracle's time per call
LDS_LIMIT = 64 * 1024


def scale_count(kind, env_value):
    """SELENITE_FUZZ_CASES=<n> scales the three slices as the RX fuzz scales its own: n cases in all in place of the default sum"""
    if not env_value:
        return COUNTS[kind]
    return max(1, int(env_value) * COUNTS[kind] // sum(COUNTS.values()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# LDS of the two any-shape kernels, in bytes (csrc/tx_generic.hip: tx_layout, csrc/tx_fm.hip: fm_layout)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _up4(v):
    return (v + 3) & ~3


def tx_lds_bytes(block, L, ni, nh):
    P, nh1 = (ni // L if ni else 1), max(nh - 1, 0)
    return 4 * (516 + _up4(ni) + _up4(2 * nh) + _up4(2 * (nh1 + block)) + _up4(2 * ((P - 1) + block)))


def fm_lds_bytes(block, L, ni, nh):
    P, nh1 = (ni // L if ni else 1), max(nh - 1, 0)
    return 4 * (516 + _up4(ni) + _up4(nh) + _up4(nh1 + block) + _up4((P - 1) + block))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the draws
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pick(rng, items, weights=None):
    if weights is None:
        return items[int(rng.integers(len(items)))]
    w = np.asarray(weights, np.float64)
    return items[int(rng.choice(len(items), p=w / w.sum()))]


def _u32(rng):
    return int(rng.integers(0, 1 << 32, dtype=np.uint64))


def _draw_nco(rng, channels, kind):
    flavour = _pick(rng, ("off", "all_grid", "all_odd", "per", "per_equal"),
                    (0.1, 0.3, 0.3, 0.12, 0.18) if kind == "FM" else (0.2, 0.22, 0.22, 0.2, 0.16))
    d = dict(nco=flavour != "off", nco_step_all=0x01000000, nco_steps=None, nco_flavour=flavour)
    if flavour == "all_grid":
        d["nco_step_all"] = int(rng.integers(0, 256)) << 24
    elif flavour == "all_odd":
        d["nco_step_all"] = _u32(rng) | 1
    elif flavour == "per":
        d["nco_steps"] = [_u32(rng) for _ in range(channels)]
    elif flavour == "per_equal":
        d["nco_steps"] = [_u32(rng) if rng.random() < 0.5 else int(rng.integers(0, 256)) << 24] * channels
    return d


def _draw_fm(rng, channels):
    tone = _pick(rng, (None, "per", "all"), (0.35, 0.35, 0.3))
    return dict(deviation=float(f32(10.0 ** rng.uniform(-3.0, np.log10(4.0)))), amplitude=float(f32(rng.uniform(0.1, 1.5))),
                tone_level=float(f32(rng.uniform(0.0, 0.5))), tone=tone, tone_step_all=_u32(rng),
                tone_steps=[_u32(rng) for _ in range(channels)] if tone == "per" else None)


def _draw_family_a(rng, kind):
    shape = dict(block=64, interp=4, ni_taps=256, nh_taps=63)
    variant = _pick(rng, ("designed", "moved", "odd", "moved+odd", "dense", "negzero"),
                    (0.34, 0.22, 0.14, 0.14, 0.08, 0.08) if kind == "FM" else (0.3, 0.2, 0.12, 0.12, 0.13, 0.13))
    taps = dict(delay=["designed"], hilb=["designed"], ic=["designed"])
    if "moved" in variant:
        taps["delay"] = ["impulse", int(_pick(rng, (0, 1, 31, 61, 62, int(rng.integers(0, 63)), int(rng.integers(0, 63)))))]
    if "odd" in variant:
        taps["hilb"] = ["odd", _u32(rng)]
    if variant == "dense":
        taps[_pick(rng, ("delay", "hilb"))] = ["dense", _u32(rng)]
    if variant == "negzero":
        taps["hilb"] = ["negzero", 2 * int(rng.integers(0, 31)) + 1]          # centre 31: the odd indices sit at even distances
    return shape, taps


def _draw_family_b(rng):
    L = int(_pick(rng, B_INTERP))
    P = int(rng.integers(1, 41))
    nh = int(_pick(rng, B_NH))
    block = int(_pick(rng, (int(rng.integers(1, 201)), int(rng.integers(1, 201)), 1, 63, 64, 65, 127, 128, 200)))
    shape = dict(block=block, interp=L, ni_taps=0 if L == 1 else P * L, nh_taps=nh)
    designed = rng.random() < 0.5
    taps = dict(delay=["designed"] if designed and nh % 2 == 1 else ["dense", _u32(rng)],
                hilb=["designed"] if designed and nh % 2 == 1 else ["dense", _u32(rng)],
                ic=["designed"] if designed else ["dense", _u32(rng)])
    return shape, taps


def _draw_call(rng, case, st, op):
    s = case["spec"]
    if case["family"] == "A" and rng.random() < (0.7 if case["kind"] == "FM" else 0.5):       # whole passes of the matrix kernels
        blocks = int(_pick(rng, (4, 8)))
    else:
        blocks = int(rng.integers(1, 9))
    blocks = max(1, min(blocks, MAX_OUT // (s["channels"] * s["block"] * s["interp"])))
    q15 = bool(rng.random() < 0.4)
    level = 10.0 ** rng.uniform(-6.0, 1.0)
    if q15:
        level = min(max(level, 1e-2), 1.0)
    if st["level"] is not None:                                    # at most 80 dB from the call before
        level = min(max(level, st["level"] * 1e-4), st["level"] * 1e4)
    st["level"] = level
    ev = dict(op=op, blocks=blocks, q15=q15, device=bool(rng.random() < 0.4), level=float(f32(level)), at=st["at"])
    st["at"] += blocks * s["block"]
    return ev


def _draw_fm_events(rng, case, st, uniform_step):
    """An FM case goes round FM: [a call in the spec's mode,] FM, a call, [a retune and a call,] then out of FM again or not, a repair of
    the phases or not (reset, set_state with one phase for all), a last call.  What is in brackets goes first where six events are too few."""
    s = case["spec"]

    def a_call():
        return _draw_call(rng, case, st, "checkpoint" if rng.random() < 0.2 else "process")

    ops, w = [None, "reset"], [0.5, 0.25]
    if uniform_step:
        ops.append("set_phase"); w.append(0.25)
    head, retune, leave, repair = rng.random() < 0.75, rng.random() < 0.2, rng.random() < 0.8, _pick(rng, ops, w)
    tail = int(leave) + int(repair is not None) + 1
    if int(head) + 2 + 2 * int(retune) + tail > 6:
        retune = False
    if int(head) + 2 + tail > 6:
        head = False
    events = [a_call()] if head else []                              # the calls are drawn in the order they run: their levels chain
    events += [dict(op="set_mode", mode=FM), a_call()]
    if retune:
        events += [dict(op="set_fm", fm=_draw_fm(rng, s["channels"])), a_call()]
    if leave:
        events.append(dict(op="set_mode", mode=int(_pick(rng, MODES))))
    if repair is not None:
        events.append(dict(op="set_phase", phase=_u32(rng)) if repair == "set_phase" else dict(op="reset"))
    return events + [a_call()]


def _draw_events(rng, case):
    kind, s = case["kind"], case["spec"]
    steps = s["nco_steps"]
    uniform_step = s["nco"] and (steps is None or len(set(steps)) == 1)
    st = dict(level=None, at=int(rng.integers(0, 4096)))
    if kind == "FM":
        return _draw_fm_events(rng, case, st, uniform_step)
    n = int(rng.integers(2, 7))
    events, control_before = [], False
    for i in range(n):
        if i == n - 1 or control_before or rng.random() < 0.5:
            events.append(_draw_call(rng, case, st, "checkpoint" if rng.random() < 0.2 else "process"))
            control_before = False
            continue
        ops, w = ["set_mode", "reset", "refused_fm"], [0.55, 0.15, 0.15]
        if uniform_step:
            ops.append("set_phase"); w.append(0.2)
        op = _pick(rng, ops, w)
        if op == "set_mode":
            events.append(dict(op="set_mode", mode=int(_pick(rng, MODES))))
        elif op == "set_phase":
            events.append(dict(op="set_phase", phase=_u32(rng)))
        else:
            events.append(dict(op=op))
        control_before = True
    return events


def make_case(seed, kind, idx):
    rng = np.random.default_rng([seed, KINDS.index(kind), idx])
    family = kind if kind != "FM" else _pick(rng, ("A", "B"), (0.7, 0.3))
    shape, taps = _draw_family_a(rng, kind) if family == "A" else _draw_family_b(rng)
    channels = int(_pick(rng, CHANNELS, (1, 1, 1, 1, 0.5, 0.5, 0.5, 0.5)))       # the CPU oracle's time goes with the channels
    arith = int(_pick(rng, (rc.ARITH_CMSIS, rc.ARITH_FMA, rc.ARITH_SPLIT16), (0.28, 0.28, 0.44) if family == "A" else (0.4, 0.4, 0.2)))
    alc = _pick(rng, ("off", "default") + gl.SET_NAMES, (0.15, 0.4, 0.15, 0.15, 0.15))
    spec = dict(channels=channels, mode=int(_pick(rng, MODES)), arith=arith, alc=alc != "off", alc_set=alc if alc in gl.SETS else None,
                q15_rounding=int(rng.integers(0, 2)), **shape)
    spec.update(_draw_nco(rng, channels, kind))
    case = dict(kind=kind, idx=idx, seed=seed, family=family, spec=spec, taps=taps, fm=_draw_fm(rng, channels) if kind == "FM" else None)
    case["events"] = _draw_events(rng, case)
    assert tx_lds_bytes(shape["block"], shape["interp"], shape["ni_taps"], shape["nh_taps"]) <= LDS_LIMIT
    return case


def cases(seed=SEED, n=None, kind=None):
    """kind: one of KINDS (n cases of it, COUNTS[kind] by default), or None: the three default slices one behind the other (n: of each)"""
    for k in (KINDS if kind is None else (kind,)):
        for idx in range(COUNTS[k] if n is None else n):
            yield make_case(seed, k, idx)


# ---------------------------------------------------------------------------------------------------------------------------------------
# from a description to the spec and the audio
# ---------------------------------------------------------------------------------------------------------------------------------------
def _dense(seed, n):
    """n random taps, none of them 0 or 1, absolute sum about 1.5"""
    r = np.random.default_rng(seed)
    t = r.uniform(0.1, 1.0, n) * r.choice([-1.0, 1.0], n)
    return (t * (1.5 / np.abs(t).sum())).astype(f32)


def build_spec(case):
    s, taps = case["spec"], case["taps"]
    nh, ni = s["nh_taps"], s["ni_taps"]
    spec = rc.TxSpec(s["channels"], block=s["block"], interp=s["interp"], ni_taps=ni, nh_taps=nh if nh % 2 else 0, mode=s["mode"],
                     arith=s["arith"], nco=s["nco"], nco_step_all=s["nco_step_all"], nco_steps=s["nco_steps"], alc=s["alc"],
                     alc_params=gl.SETS[s["alc_set"]] if s["alc_set"] else None, q15_rounding=bool(s["q15_rounding"]))
    spec.nh_taps = nh
    if nh:
        d, h = taps["delay"], taps["hilb"]
        if d[0] == "impulse":
            spec.delay = np.zeros(nh, f32)
            spec.delay[d[1]] = 1.0
        elif d[0] == "dense":
            spec.delay = _dense(d[1], nh)
        if h[0] == "odd":                                          # type III with values of its own at the odd distances
            spec.hilb = np.zeros(nh, f32)
            k = np.arange(nh)
            odd = (k - (nh - 1) // 2) % 2 != 0
            spec.hilb[odd] = _dense(h[1], int(odd.sum()))
        elif h[0] == "dense":
            spec.hilb = _dense(h[1], nh)
        elif h[0] == "negzero":
            spec.hilb = spec.hilb.copy()
            assert spec.hilb[h[1]] == 0.0
            spec.hilb[h[1]] = f32(-0.0)
        assert spec.delay.shape == spec.hilb.shape == (nh,)
    if ni and taps["ic"][0] == "dense":
        spec.ic = _dense(taps["ic"][1], ni) * f32(s["interp"])
    return spec


def fm_args(fm):
    """(deviation, amplitude, tone_level, tone_steps) as sr.Tx.set_fm and TxFmOracle.set_fm take them"""
    steps = None
    if fm["tone"] == "per":
        steps = np.array(fm["tone_steps"], np.uint32)
    elif fm["tone"] == "all":
        steps = int(fm["tone_step_all"])
    return fm["deviation"], fm["amplitude"], fm["tone_level"], steps


def audio(case, ev):
    s = case["spec"]
    a = rc.synth_audio(case["idx"] % 7, s["channels"], ev["at"], ev["blocks"] * s["block"]) * f32(ev["level"])
    if ev["q15"]:
        return np.clip(np.trunc(a * f32(32768.0)), -32768, 32767).astype(np.int16)
    return np.ascontiguousarray(a, f32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host's rules, restated
# ---------------------------------------------------------------------------------------------------------------------------------------
def _plus_zero(v):
    return (v == 0) & ~np.signbit(v)


def matrix_shape(case):
    """tx_fused_ok without the call length: the fused geometry, a unit-impulse delay FIR (one 1.0f, the rest +0.0f) and a type-III
    Hilbert (+0.0f at every even distance from the centre), as selenite_tx_init classifies the taps it is given"""
    s = case["spec"]
    if (s["block"], s["interp"], s["ni_taps"], s["nh_taps"]) != (64, 4, 256, 63):
        return False
    spec = build_spec(case)
    d, h = spec.delay, spec.hilb
    impulse = int((d == 1.0).sum()) == 1 and bool(_plus_zero(d[d != 1.0]).all())
    k = np.arange(63)
    return impulse and bool(_plus_zero(h[(k - 31) % 2 == 0]).all())


def expected_kernel(case, mode=None):
    """selenite_tx_kernel_name: FM mode, then tx_fused_ok, then SPLIT16 with a table (built exactly where tx_fused_ok holds)"""
    mode = case["spec"]["mode"] if mode is None else mode
    if mode == FM:
        return KFM
    if not matrix_shape(case):
        return GENERIC
    return SPLIT16 if case["spec"]["arith"] == rc.ARITH_SPLIT16 else FUSED


def walk(case):
    """(event index, record) for every planned call, a checkpoint's call twice.  record: kernel family that serves the call, its NCO
    flavour (off / table / periodic / perchan; FM: nco / zero_if), q15, device, mode, prev (the family of the call before), tags (what
    the call is the first behind: reset_behind_fm, set_phase_behind_fm, restore_behind_fm), bs and uniform (the call's length and the
    host's phase_uniform in front of it), and the case's constants."""
    s = case["spec"]
    steps = s["nco_steps"] if s["nco_steps"] is not None else [s["nco_step_all"]] * s["channels"]
    steps_same = len(set(steps)) == 1
    inst = FAMILY[expected_kernel(case, rc.MODE_USB)]
    fm = case["fm"]
    mode, prev = s["mode"], None
    uniform, equal, dirty = steps_same, True, False          # phase_uniform; every channel at one phase; an FM call since they were
    tags = set()

    def call(ev):
        nonlocal uniform, equal, dirty, prev, tags
        bs, was_uniform = ev["blocks"] * s["block"], uniform
        if mode == FM:
            fam, flavour = "fm", "nco" if s["nco"] else "zero_if"
            uniform, equal, dirty = False, s["channels"] == 1, True
        elif inst != "generic" and bs % 256 == 0:
            fam = inst
            if not s["nco"]:
                flavour = "off"
            elif uniform:
                flavour = "periodic" if inst == "split16" and steps[0] & 0x00FFFFFF == 0 else "table"
            else:
                flavour = "perchan"
        else:
            fam, flavour = "generic", "off" if not s["nco"] else "perchan"
        rec = dict(kernel=fam, flavour=flavour, q15=ev["q15"], device=ev["device"], mode=mode, prev=prev, tags=frozenset(tags), bs=bs, uniform=was_uniform,
                   steps_same=steps_same and s["nco"], arith=s["arith"], alc_set=s["alc_set"], tone=fm["tone"] if fm and mode == FM else None,
                   moved=case["taps"]["delay"][0] == "impulse" and case["taps"]["delay"][1] != 31)
        prev, tags = fam, set()
        return rec

    for i, ev in enumerate(case["events"]):
        op = ev["op"]
        if op == "set_mode":
            mode = ev["mode"]
        elif op == "set_fm":
            fm = ev["fm"]
        elif op in ("reset", "set_phase"):
            if dirty:
                tags.add(op + "_behind_fm")
            uniform, equal, dirty = steps_same, True, False
        elif op == "process":
            yield i, call(ev)
        elif op == "checkpoint":
            before = (steps_same and equal, equal, dirty)
            yield i, call(ev)
            if dirty:
                tags.add("restore_behind_fm")
            uniform, equal, dirty = before              # selenite_tx_set_state: uniform when the restored phases are all the same
            yield i, call(ev)
        else:
            assert op == "refused_fm"
