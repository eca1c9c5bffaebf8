"""CPU: the generator of the TX entry fuzz (tests/tx_entry_fuzz_cases.py) -- the cases of the older kinds are what they were, the new kinds
are deterministic, every draw is valid for selenite_tx_init, selenite_tx_set_cw and selenite_tx_set_in and under the LDS bound of every
kernel that will serve it, and the committed seed with the default counts reaches every form the KEY and IN slices of the GPU fuzz
(tests/test_gpu_tx_fuzz.py) are there for."""
import collections
import hashlib
import json

import numpy as np

import rxcommon as rc
import tx_entry_fuzz_cases as ez
import tx_fuzz_cases as fz
import txin_oracle as tio

NEED = 3
# sha256 of json.dumps(list(tx_fuzz_cases.cases())) as the commit before the entry fuzz generated them
OLD_CASES_SHA256 = "cf40c5ca989ef921c4ff1353d63a0328031a1b4e69b85115a589807eff2f7331"


def test_the_cases_of_the_older_kinds_are_byte_identical():
    old = list(fz.cases())
    assert len(old) == 160 and [c["kind"] for c in old] == ["A"] * 40 + ["B"] * 40 + ["FM"] * 80
    assert hashlib.sha256(json.dumps(old).encode()).hexdigest() == OLD_CASES_SHA256


def _finite_f32(t, n):
    return t.shape == (n,) and t.dtype == np.float32 and bool(np.isfinite(t).all())


def _check_cw(case, cw):
    s = case["spec"]
    a = ez.cw_args(cw)
    assert 1 <= cw["ns_taps"] <= 308 and _finite_f32(a["shape"], cw["ns_taps"]) and a["side_mix"] in (0, 1) and 0 <= a["hang_blocks"] <= 3
    assert np.isfinite(a["amplitude"]) and np.isfinite(a["side_level"]) and 0 <= a["offset_step"] < 1 << 32
    assert np.ndim(a["side_step"]) == 0 or a["side_step"].shape == (s["channels"],)
    assert ez.cw_lds_bytes(s["block"], s["interp"], s["ni_taps"], cw["ns_taps"]) <= ez.LDS_LIMIT


def _check_in(case, inp):
    s = case["spec"]
    a = ez.in_args(inp)
    assert inp["M"] in (1, 2, 4, 8) and 0 <= inp["nd_taps"] <= 256 and (inp["nd_taps"] > 0 or inp["M"] == 1) and inp["pick"] in (0, 1, 2, 3)
    assert (a["coeffs"] is None and inp["nd_taps"] == 0) or _finite_f32(a["coeffs"], inp["nd_taps"])
    assert np.isfinite(a["gain"]) and a["gain"] != 0
    v = a["vox"]
    if v is not None:
        assert v["gate"] in (0, 1) and 0 <= v["hang"] <= 3 and 0 < v["attack"] <= 1 and 0 < v["decay"] <= 1
        assert 0 <= v["close_level"] <= v["open_level"] < np.inf and v["level_init"] == 0.0
    assert ez.in_lds_bytes(s["block"], inp["M"], inp["nd_taps"]) <= ez.LDS_LIMIT
    assert s["channels"] * s["block"] * inp["M"] * ez._fw(inp) <= ez.MAX_IN


def test_cases_are_plain_deterministic_and_valid():
    a, b = list(ez.cases()), list(ez.cases())
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True), "plain data, the same on every run"
    assert len(a) == sum(ez.COUNTS.values())
    assert json.dumps(list(ez.cases(ez.SEED, 5, "IN"))) == json.dumps(a[-ez.COUNTS["IN"]:][:5]), "case k of a kind does not depend on n"
    for case in a:
        s = case["spec"]
        shape = (s["block"], s["interp"], s["ni_taps"], s["nh_taps"])
        assert (s["interp"] > 1) == (s["ni_taps"] > 0) and s["ni_taps"] % s["interp"] == 0 and s["channels"] in fz.CHANNELS
        assert max(fz.tx_lds_bytes(*shape), fz.fm_lds_bytes(*shape)) <= fz.LDS_LIMIT
        assert s["channels"] * s["block"] * s["interp"] <= ez.MAX_OUT
        assert 3 <= len(case["events"]) <= 7
        assert case["events"][-1]["op"] in ("process", "key", "key_checkpoint", "frames", "frames_checkpoint", "refused_key", "refused_frames")
        assert (case["cw"] is not None) if case["kind"] == "KEY" else (case["inp"] is not None)
        spec = ez.build_spec(case)
        for taps, n in ((spec.delay, s["nh_taps"]), (spec.hilb, s["nh_taps"]), (spec.ic, s["ni_taps"])):
            assert (taps is None and n == 0) or _finite_f32(taps, n)
        mode, cw, inp, level, flevel = s["mode"], case["cw"], case["inp"], None, None
        if cw:
            _check_cw(case, cw)
        if inp:
            _check_in(case, inp)
        uniform_step = s["nco"] and (s["nco_steps"] is None or len(set(s["nco_steps"])) == 1)
        for i, ev in enumerate(case["events"]):
            op = ev["op"]
            assert op not in ("refused_key", "refused_frames") or i == len(case["events"]) - 1, "a refusal latches the status: it ends the case"
            if op == "process":
                x = ez.audio(case, ev)
                assert x.shape == (s["channels"], ev["blocks"] * s["block"]) and 1 <= ev["blocks"] <= 8 and np.isfinite(x).all()
                assert level is None or 1e-4 * 0.999 <= ev["level"] / level <= 1e4 * 1.001
                level = ev["level"]
            elif op in ("key", "key_checkpoint"):
                assert cw is not None and mode in (ez.CW, ez.CWR) and 1 <= ev["blocks"] <= 8
                k = ez.keys(case, ev)
                assert k.shape == (s["channels"], ev["blocks"] * s["block"]) and k.dtype == np.uint8
                assert ez.side_in(case, ev).dtype == (np.int16 if ev["q15"] else np.float32)
                assert s["channels"] * ev["blocks"] * s["block"] * s["interp"] <= ez.MAX_OUT
            elif op in ("frames", "frames_checkpoint"):
                assert inp is not None and 1 <= ev["blocks"] <= 8 and ev["entry"] in ez.ENTRIES
                x = ez.frames(case, ev, inp)
                assert x.shape == (s["channels"], ev["blocks"] * s["block"] * inp["M"] * ez._fw(inp)) and x.size <= ez.MAX_IN
                assert x.dtype == (np.float32 if ev["entry"].startswith("f32") else np.int16)
                assert ez.FRAME_LEVEL[0] * 0.999 <= ev["level"] <= ez.FRAME_LEVEL[1] * 1.001
                assert flevel is None or 1e-4 <= ev["level"] / flevel <= 1e4, "at most 80 dB from the call before"
                flevel = ev["level"]
                assert ev["quiet"] is None or 0 <= ev["quiet"][0] <= ev["quiet"][1] <= ev["blocks"]
            elif op == "set_mode":
                mode = ev["mode"]
                assert mode in fz.MODES or (mode == fz.FM and case["fm"] is not None)
            elif op == "set_cw":
                assert cw is not None
                cw = ev["cw"]
                _check_cw(case, cw)
            elif op == "set_in":
                assert inp is not None and ev["inp"]["M"] == inp["M"] and ez._fw(ev["inp"]) == ez._fw(inp)
                inp = ev["inp"]
                _check_in(case, inp)
            elif op == "set_phase":
                assert uniform_step
            elif op == "refused_key":
                assert cw is not None and mode not in (ez.CW, ez.CWR)
            elif op == "clear_in":
                assert inp is not None and case["events"][i + 1]["op"] == "refused_frames"
                inp = None
            elif op == "refused_frames":
                assert inp is None and case["kind"] == "IN"
            else:
                assert op == "reset", op


def test_the_layouts_restated():
    """the figures the directed tests rely on (tests/test_gpu_tx_entry_edges.py), from in_layout and cw_layout restated"""
    assert ez.in_lds_bytes(1700, 8, 64) == 61476 and ez.in_lds_bytes(1812, 8, 64) == 65508 and ez.in_lds_bytes(1813, 8, 64) == 65540
    assert ez.in_tile(64, 8) == 128 and ez.in_tile(12, 4) == 252 and ez.in_tile(136, 8) == 136 and ez.in_tile(1030, 1) == 1030
    assert ez.cw_lds_bytes(64, 2, 16, 6000) == 50672
    assert ez.in_wide(136, 8, 1, 4, 136) and not ez.in_wide(1030, 1, 1, 2, 1030)


def vox_edges(case):
    """per frame event: does some channel's VOX open and close within the call?  From txin_oracle.TxInStage followed through the case"""
    s, stage, inp, out = case["spec"], None, case["inp"], {}
    if inp is not None:
        stage = tio.TxInStage(s["channels"], s["block"], **ez.in_args(inp))
    for i, ev in enumerate(case["events"]):
        op = ev["op"]
        if op == "set_in":
            inp = ev["inp"]
            stage.configure(**ez.in_args(inp))
        elif op == "reset" and stage is not None:
            stage.reset()
        elif op == "clear_in":
            stage = None
        elif op in ("frames", "frames_checkpoint"):
            before = stage.state()["open"].copy() if stage.vox is not None else None
            r = stage.process(ez.frames(case, ev, inp), False)
            if r["bits"] is not None:
                b = np.concatenate([before[:, None], r["bits"]], axis=1).astype(np.int64)
                d = np.diff(b, axis=1)
                out[i] = bool(((d > 0).any(axis=1) & (d < 0).any(axis=1)).any())
    return out


def test_generator_covers_every_form():
    n = collections.Counter()
    for case in ez.cases():
        s = case["spec"]
        for _, r in ez.walked(case):
            k, e = r["kernel"], r["entry"]
            n[e, "served by " + k] += 1
            n["mode", r["mode"]] += 1
            if r["prev"] is not None and r["prev"] != k:
                n["from " + r["prev"], "to " + k] += 1
            for t in r["tags"]:
                n["first call", t] += 1
            if e == "key":
                n["key", "q15" if r["q15"] else "f32"] += 1
                n["key", "device" if r["device"] else "host"] += 1
                n["key", "side " + r["side"]] += 1
                n["key", "CW" if r["mode"] == ez.CW else "CWR"] += 1
                n["key", "block % 4 == 0" if r["block"] % 4 == 0 else "block % 4 != 0"] += 1
                n["key", "L even" if r["L"] % 2 == 0 else "L odd"] += 1
                n["key", "ns_taps > block"] += r["ns"] > r["block"]
                n["key", "split16 instance"] += r["arith"] == rc.ARITH_SPLIT16
                n["key", "shorter than the interpolator history behind an audio call"] += bool(r["short"])
            elif e == "frames":
                n["frames", r["fentry"]] += 1
                n["frames", "M %d" % r["M"]] += 1
                n["frames", "pick %d" % r["pick"]] += 1
                n["frames", "nd_taps 0"] += r["nd"] == 0
                n["frames", "nd_taps < M"] += 0 < r["nd"] < r["M"]
                n["frames", "more than one chunk in a tile"] += r["chunks"] > 1
                n["frames", "more than one tile"] += r["tiles"] > 1
                n["frames", "16-byte path" if r["wide"] else "element path"] += 1
                n["frames", "vox " + r["vox"]] += 1
                n["frames", "split16 instance"] += r["arith"] == rc.ARITH_SPLIT16
                n["frames", "behind a key call"] += r["prev_entry"] == "key"
                n["frames", "before a key call"] += r["next_entry"] == "key"
            elif k in ("fused", "split16") and r["flavour"] == "perchan" and r["steps_same"] and r["prev"] == "cw":
                n["audio", "per-channel LO on a uniform-step instance behind a key call"] += 1
        ns, nd = case["cw"] and case["cw"]["ns_taps"], case["inp"] and case["inp"]["nd_taps"]
        for ev in case["events"]:
            n["event", ev["op"]] += 1
            if ev["op"] == "set_in":
                n["event", "set_in with the same nd_taps" if ev["inp"]["nd_taps"] == nd else "set_in with a new nd_taps"] += 1
                nd = ev["inp"]["nd_taps"]
            if ev["op"] == "set_cw":
                n["event", "set_cw with the same ns_taps" if ev["cw"]["ns_taps"] == ns else "set_cw with a new ns_taps"] += 1
                ns = ev["cw"]["ns_taps"]
                n["event", "set_cw per-channel side_step" if ev["cw"]["side_steps"] else "set_cw shared side_step"] += 1
            if ev["op"] in ("key", "key_checkpoint"):
                for p in set(ez.key_patterns(case, ev)):
                    n["keys", p] += 1
        if case["cw"]:
            n["cw", "per-channel side_step" if case["cw"]["side_steps"] else "shared side_step"] += 1
            n["cw", "hang_blocks %d" % case["cw"]["hang_blocks"]] += 1
        n["frames", "VOX opens and closes within a call"] += sum(vox_edges(case).values())
    fams = ("fused", "split16", "generic", "fm")
    need = [("key", f) for f in ("f32", "q15", "device", "host", "side none", "side store", "side mix", "CW", "CWR", "block % 4 == 0",
                                 "block % 4 != 0", "L even", "L odd", "ns_taps > block", "split16 instance",
                                 "shorter than the interpolator history behind an audio call")]
    need += [("from cw", "to " + x) for x in fams] + [("from " + x, "to cw") for x in fams]
    need += [("first call", t + "_behind_key") for t in ("reset", "set_phase", "restore")]
    need += [("audio", "per-channel LO on a uniform-step instance behind a key call")]
    need += [("frames", f) for f in ez.ENTRIES + ("M 1", "M 2", "M 4", "M 8", "pick 0", "pick 1", "pick 2", "pick 3", "nd_taps 0", "nd_taps < M",
                                                  "more than one chunk in a tile", "more than one tile", "16-byte path", "element path",
                                                  "vox none", "vox flag", "vox gate", "split16 instance", "behind a key call", "before a key call",
                                                  "VOX opens and closes within a call")]
    need += [("frames", "served by " + x) for x in fams] + [("audio", "served by " + x) for x in fams]
    need += [("mode", m) for m in fz.MODES + (fz.FM,)]
    need += [("event", op) for op in ("process", "key", "key_checkpoint", "frames", "frames_checkpoint", "set_mode", "set_cw", "set_in", "reset",
                                      "set_phase", "refused_key", "clear_in", "refused_frames", "set_cw per-channel side_step",
                                      "set_cw shared side_step", "set_cw with the same ns_taps", "set_cw with a new ns_taps",
                                      "set_in with the same nd_taps", "set_in with a new nd_taps")]
    need += [("keys", p) for p in ez.PATTERNS] + [("cw", "per-channel side_step"), ("cw", "shared side_step")]
    need += [("cw", "hang_blocks %d" % h) for h in range(4)]
    short = {k: n[k] for k in need if n[k] < NEED}
    print(sorted(n.items(), key=str))
    assert not short, "planned calls, at least %d each: %r" % (NEED, short)
