"""CPU: the generator of the RX stage fuzz (tests/rx_stage_fuzz_cases.py) -- plain and deterministic, every draw inside the setters' ranges,
and the committed seed with the default counts reaches every form the GPU fuzz (tests/test_gpu_rx_stage_fuzz.py) is there for: every stage
on every kernel family, in both slot formats, in a cut call, under a global gain in one call and split, directly behind reset, checkpoint,
set_mode and its own add_stage; the ordered pairs whose order the dispatcher decides; every field of the route (csrc/rx_route.h) true and
false; and a signal that moves every stage's state (the composed oracle run alone over the bit-exact cases).  The floors are conditions of
the generator, not measurements: NEED planned calls (or cases) each."""
import collections
import json

import numpy as np
import pytest

import rx_stage_fuzz_cases as fz
import rxcommon as rc

NEED = 3
CALL_EVENTS = ("process", "checkpoint", "global_one_call", "global_split", "refused_split")


def test_cases_are_plain_deterministic_and_valid():
    a, b = list(fz.cases()), list(fz.cases())
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True), "plain data, the same on every run"
    assert len(a) == sum(fz.COUNTS.values())
    assert json.dumps(list(fz.cases(fz.SEED, 5, "cw"))) == json.dumps([c for c in a if c["kind"] == "cw"][:5]), "case k of a kind does not depend on n"
    for kind in fz.KINDS:
        mine = [c for c in a if c["kind"] == kind]
        assert 4 * sum(len(c["on"]) >= 7 for c in mine) >= len(mine), kind + ": a quarter of the cases with seven or more stages on"
        assert sum(len(c["on"]) == 9 for c in mine) >= 3, kind + ": three cases with all nine"
    for case in a:
        s, par = case["spec"], case["params"]
        assert s["channels"] in fz.CHANNELS and s["block"] % s["decim"] == 0 and (s["nd_taps"] > 0) == (s["decim"] > 1)
        assert s["mode"] in case["modes"] and (s["mode"] != rc.MODE_FM or s["nh_taps"] >= 2)
        assert (s["arith"] in fz.EXACT) or case["kind"] in ("ssb", "hilb") or case["variant"] == "ssb_forced"
        na = s["block"] // s["decim"]
        # the setters' ranges
        sp, iqc, nb, t, cw, nr, m, out = (par[k] for k in ("spectrum", "iqc", "nb", "tones", "cwdec", "nr", "meter", "out"))
        assert sp["fft_len"] in (64, 512) and 1 <= sp["stride"] <= 65535 and sp["average"] in (0, 1) and 0 < sp["alpha"] <= 1
        for g in (iqc, nb):
            assert g["frame"] in (32, 64, 128) and s["block"] % g["frame"] == 0
        assert 0 <= iqc["alpha"] <= 1 and 0 <= iqc["dc_alpha"] <= 1 and 0 < iqc["p_max"] <= 1 and iqc["g_max"] >= 1 and iqc["min_power"] >= 0
        assert abs(iqc["p_init"]) <= iqc["p_max"] and 1 / iqc["g_max"] <= iqc["g_init"] <= iqc["g_max"]
        assert nb["guard"] <= 8 and 1 <= nb["max_hits"] <= nb["frame"] // 4 and nb["threshold"] >= 1 and 0 < nb["alpha"] <= 1 and nb["clamp"] >= 1
        assert 1 <= len(t["coeffs"]) <= 64 and all(len(r) == 3 for r in t["coeffs"]) and 1 <= t["frame_blocks"] <= 65535
        assert 1 <= t["confirm"] <= 65535 and 1 <= t["release"] <= 65535 and 0 <= t["ratio"] <= 1 and t["min_power"] >= 0
        assert all(0 < cw[k] <= 1 for k in ("peak_attack", "peak_decay", "floor_attack", "floor_decay")) and 0 < cw["off_frac"] <= cw["on_frac"] < 1
        assert cw["snr"] >= 1 and 1 <= cw["debounce"] <= 255 and 0 <= cw["track"] <= 8 and 256 <= cw["unit_min"] <= cw["unit_init"] <= cw["unit_max"] <= 8192 * 256
        assert cw["ring"] >= 16 and cw["ring"] & (cw["ring"] - 1) == 0
        c = np.array(par["afilt"]["coeffs"], np.float32)
        assert c.shape[-1] == 5 and 1 <= c.shape[-2] <= 8 and np.isfinite(c).all() and (c.ndim == 3) == par["afilt"]["per_channel"]
        assert c.ndim == 2 or c.shape[0] == s["channels"]
        assert nr["kind"] in (1, 2) and nr["num_taps"] in (8, 16, 32) and 1 <= nr["delay"] <= 64 and 0 < nr["mu"] < 2
        assert "coeffs_init" not in nr or len(nr["coeffs_init"]) == nr["num_taps"]
        assert 0 < m["attack"] <= 1 and 0 < m["decay"] <= 1 and 0 <= m["close_level"] <= m["open_level"] and m["sense"] == 0 and m["hang"] <= 65535
        ntaps = len(out["coeffs"] or [])
        assert out["interp"] in (1, 2, 4) and ntaps % out["interp"] == 0 and ntaps // out["interp"] <= 64 and (ntaps or out["interp"] == 1)
        # the events
        ev = case["events"]
        assert 3 <= len(ev) <= 7 and ev[0]["op"] in CALL_EVENTS and ev[-1]["op"] in CALL_EVENTS
        on, glob = set(case["on"]), s["agc"] and s["agc_global"]
        for i, e in enumerate(ev):
            if e["op"] in CALL_EVENTS:
                assert e["blocks"] in fz.LENGTHS + (9,)
                assert "nr" not in on or e["blocks"] * na <= fz.NLMS_MAX_AUDIO, "the NLMS oracle's time"
            else:
                assert ev[i + 1]["op"] in CALL_EVENTS, "a call follows every life-cycle event"
            if e["op"] in ("global_one_call", "global_split", "refused_split"):
                assert glob
            if e["op"] == "global_split":
                assert "out" not in on
            if e["op"] == "refused_split":
                assert "out" in on and i == len(ev) - 1
            if e["op"] == "set_mode":
                assert e["mode"] in case["modes"]
            if e["op"] == "drop_stage":
                on.remove(e["stage"])
            if e["op"] == "add_stage":
                assert e["stage"] not in on
                on.add(e["stage"])
        x = fz.signal(case, 1000, 700)
        assert x.shape == (s["channels"], 700, 2) and x.dtype == np.float32 and np.isfinite(x).all()
        np.testing.assert_array_equal(fz.signal(case, 0, 2500)[:, 1000:1700], x, "a pure function of (case, channel, absolute sample)")


def route_fields(f):
    """csrc/rx_route.h restated from the facts of a launch, as tests/test_route.py restates it"""
    front = f["phase"] != 2
    w = {k: f["on"][k] and front for k in fz.UNSCALED}
    w["gate"] = f["gate"] and f["phase"] != 1
    w["mixed"] = not f["src_q15"] and f["dst_q15"]
    w["ssb_fused"] = front and not f["force"] and f["ssb"]
    w["cw_fused"] = front and not f["force"] and f["cw"]
    w["fused"] = w["ssb_fused"] or w["cw_fused"]
    w["unscaled"] = f["glob"] or any(w[k] for k in fz.UNSCALED) or w["mixed"]
    w["convert_in"] = w["unscaled"] and f["src_q15"] and w["fused"]
    w["audio_in_scratch"] = f["dst_q15"] and (w["unscaled"] or not w["fused"])
    w["fused_agc_off"] = w["fused"] and w["unscaled"]
    w["done_after_fused"] = w["fused"] and not w["unscaled"]
    w["clear_words"] = front and f["words"] and not w["ssb_fused"]
    w["generic_front"] = front and not w["fused"]
    w["biquad"] = w["generic_front"] and f["cwbq"]
    w["env"] = f["glob"] and front
    w["apply"] = f["glob"] and f["phase"] != 1
    w["agc_generic"] = not f["glob"] and (f["agc"] or f["dst_q15"])
    return w


def coverage():
    n = collections.Counter()
    for case in fz.cases():
        for _, r in fz.walk(case):
            on = set(r["on"])
            fmt = "int16" if r["q15"] else "f32"
            for s in on:
                n[s, r["kernel"]] += 1
                n[s, fmt] += 1
                n[s, "host" if r["entry"].startswith("host") else "device"] += 1
                if r["cut"]:
                    n[s, "cut"] += 1
                if r["phase"] != "all":
                    n[s, r["phase"]] += 1
                if r["prev"] in ("reset", "checkpoint", "set_mode"):
                    n[s, "behind " + r["prev"]] += 1
                if r["prev"] == "add_stage:" + s:
                    n[s, "behind its add_stage"] += 1
            for a, b in (("afilt", "nr"), ("tones", "afilt"), ("cwdec", "afilt"), ("iqc", "nb"), ("spectrum", "iqc")):
                if a in on and b in on:
                    n["pair", a + " with " + b] += 1
            if r["gate_out"]:
                n["pair", "meter-gate with out"] += 1
            if "iqc" in on and r["q15"] and "out" not in on:
                n["pair", "iqc with int16 out (mixed)"] += 1
            if "nb" in on and "iqc" not in on and r["q15"] and "out" not in on:
                n["pair", "nb alone with int16 in"] += 1
            if len(on) >= 3 and r["kernel"] == "ssb_fused":
                n["arith", {rc.ARITH_SPLIT16: "SPLIT16", rc.ARITH_AUTO: "AUTO"}.get(r["arith"], "exact") + " with three stages or more"] += 1
            for f in r["launches"]:
                for k, v in route_fields(f).items():
                    n["route", "%s=%d" % (k, v)] += 1
    return n


def needed():
    need = []
    for s in fz.STAGES:
        need += [(s, k) for k in ("ssb_fused", "cw_fused", "generic", "f32", "int16", "host", "device", "cut", "one_call",
                                  "behind reset", "behind checkpoint", "behind set_mode", "behind its add_stage")]
        need.append((s, "refused" if s == "out" else "split"))      # (the split call refuses an instance with an output stage: that refusal instead)
    need += [("pair", p) for p in ("afilt with nr", "tones with afilt", "cwdec with afilt", "meter-gate with out", "iqc with nb",
                                   "iqc with int16 out (mixed)", "nb alone with int16 in", "spectrum with iqc")]
    need += [("arith", a + " with three stages or more") for a in ("SPLIT16", "AUTO")]
    fields = list(fz.UNSCALED) + ("gate mixed ssb_fused cw_fused fused unscaled convert_in audio_in_scratch fused_agc_off done_after_fused "
                                  "clear_words generic_front biquad env apply agc_generic").split()
    need += [("route", "%s=%d" % (k, v)) for k in fields for v in (0, 1)]
    return need


def test_generator_covers_every_form():
    n = coverage()
    rows = collections.defaultdict(dict)
    for (a, b), v in n.items():
        rows[a][b] = v
    for a in list(fz.STAGES) + ["pair", "arith", "route"]:
        print("%-9s %s" % (a, "  ".join("%s %d" % kv for kv in sorted(rows[a].items()))))
    short = {k: n[k] for k in needed() if n[k] < NEED}
    assert not short, "planned calls, at least %d each: %r" % (NEED, short)


# ---- the signal moves every stage: the composed oracle alone, over the bit-exact cases ----------------------------------------------------------
def run_oracle(case):
    """walks the events on the oracle alone; returns {stage: its state was non-trivial behind some call}"""
    p = fz.pipeline_of(case)
    at, moved = 0, collections.Counter()
    for ev in case["events"]:
        op = ev["op"]
        if op == "set_mode":
            p.set_mode(ev["mode"])
        elif op == "reset":
            p.reset()
        elif op == "drop_stage":
            p.set_stage(ev["stage"], None)
        elif op == "add_stage":
            p.set_stage(ev["stage"], case["params"][ev["stage"]])
        elif op == "refused_split":
            pass
        else:
            if op == "checkpoint":
                q = fz.pipeline_of(case, on=list(p.par), mode=p.mode)
                q.set_state(p.state())
                p = q
            data = fz.signal(case, at, ev["blocks"] * case["spec"]["block"])
            at += data.shape[1]
            if op == "global_split":
                p.phase1(data)
                p.phase2()
            else:
                p.process_audio(None, fz.to_q15(data) if ev.get("entry", "").endswith("q15") else data)
            st, par = p.st, p.par
            if "nb" in st:
                moved["nb"] |= bool(st["nb"].blanked.any() and (st["nb"].blanked < np.uint64(at)).all())
            if "meter" in st:
                t = st["meter"].trace["open"]
                moved["meter open"] |= bool(t.any())
                moved["meter closed"] |= bool(not t.all())
            if "tones" in st:
                moved["tones"] |= bool(st["tones"].changes.any())
            if "cwdec" in st:
                moved["cwdec"] |= bool(st["cwdec"].count.any())
            if "nr" in st:
                moved["nlms overflow"] |= not bool(np.isfinite(st["nr"].coeffs).all() and np.isfinite(st["nr"].energy).all())
                init = np.zeros(par["nr"]["num_taps"], np.float32) if "coeffs_init" not in par["nr"] else np.array(par["nr"]["coeffs_init"], np.float32)
                moved["nr"] |= bool((st["nr"].coeffs != init).any())
            if "iqc" in st:
                moved["iqc"] |= bool((st["iqc"].p != np.float32(par["iqc"]["p_init"])).any() and (st["iqc"].g != np.float32(par["iqc"]["g_init"])).any())
            if "afilt" in st:
                moved["afilt"] |= bool(st["afilt"].state.any())
            if "spectrum" in st:
                moved["spectrum"] |= bool(st["spectrum"].rows.any())
            if "out" in st and st["out"].P >= 2:
                moved["out"] |= bool(st["out"].state.any())
    moved["meter"] = moved["meter open"] and moved["meter closed"]
    return moved


@pytest.fixture(scope="module")
def moved():
    n = collections.Counter()
    for case in fz.cases():
        if fz.oracle_arith(case) is not None:
            for k, v in run_oracle(case).items():
                n[k] += int(bool(v))
    return n


def test_the_signal_moves_every_stage(moved):
    """over the SELENITE_ARITH_CMSIS and _FMA cases: the blanker blanked samples and left others, the gate was open on some blocks and closed
    on others, a tone decision changed, the decoder's count advanced, the NLMS weights moved, the correction's p and g left their inits"""
    print(dict(moved))
    assert not moved["nlms overflow"], "a default case in which arm_lms_norm_f32's running energy passes zero and the weights overflow (the GPU fuzz ends such a case early)"
    short = {k: moved[k] for k in ("nb", "meter", "tones", "cwdec", "nr", "iqc", "afilt", "spectrum", "out") if moved[k] < NEED}
    assert not short, "cases in which the stage's state is non-trivial, at least %d each: %r" % (NEED, short)
