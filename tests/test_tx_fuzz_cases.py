"""CPU: the TX fuzz generator (tests/tx_fuzz_cases.py) -- deterministic, every draw valid for selenite_tx_init and under the LDS bound, and
the committed seed with the default counts reaches every form the GPU fuzz (tests/test_gpu_tx_fuzz.py) is there for."""
import collections
import json

import numpy as np

import rxcommon as rc
import tx_fuzz_cases as fz

NEED = 3


def test_cases_are_plain_deterministic_and_valid():
    a, b = list(fz.cases()), list(fz.cases())
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True), "plain data, the same on every run"
    assert len(a) == sum(fz.COUNTS.values())
    assert json.dumps(list(fz.cases(fz.SEED, 5, "FM"))) == json.dumps(a[-fz.COUNTS["FM"]:][:5]), "case k of a kind does not depend on n"
    for case in a:
        s = case["spec"]
        assert (s["interp"] > 1) == (s["ni_taps"] > 0) and s["ni_taps"] % s["interp"] == 0 and s["channels"] in fz.CHANNELS
        assert max(fz.tx_lds_bytes(s["block"], s["interp"], s["ni_taps"], s["nh_taps"]),
                   fz.fm_lds_bytes(s["block"], s["interp"], s["ni_taps"], s["nh_taps"])) <= fz.LDS_LIMIT
        assert 2 <= len(case["events"]) <= 6 and case["events"][-1]["op"] in ("process", "checkpoint")
        assert (case["fm"] is not None) == (case["kind"] == "FM")
        spec = fz.build_spec(case)
        for taps, n in ((spec.delay, s["nh_taps"]), (spec.hilb, s["nh_taps"]), (spec.ic, s["ni_taps"])):
            assert (taps is None and n == 0) or (taps.shape == (n,) and taps.dtype == np.float32 and np.isfinite(taps).all())
        level, mode, fm_set = None, s["mode"], case["fm"] is not None
        for ev in case["events"]:
            if ev["op"] in ("process", "checkpoint"):
                x = fz.audio(case, ev)
                assert x.shape == (s["channels"], ev["blocks"] * s["block"]) and 1 <= ev["blocks"] <= 8 and np.isfinite(x).all()
                assert level is None or 1e-4 * 0.999 <= ev["level"] / level <= 1e4 * 1.001, "at most 80 dB from the call before"
                level = ev["level"]
            if ev["op"] == "set_mode":
                assert ev["mode"] in fz.MODES or (ev["mode"] == fz.FM and fm_set)
            if ev["op"] == "set_phase":
                assert s["nco"] and (s["nco_steps"] is None or len(set(s["nco_steps"])) == 1)
            if ev["op"] == "refused_fm":
                assert not fm_set


def test_expected_kernel_restates_the_host_rule():
    by_variant = collections.defaultdict(set)
    for case in fz.cases():
        t = case["taps"]
        name = fz.expected_kernel(case, rc.MODE_USB)
        assert fz.expected_kernel(case, fz.FM) == fz.KFM
        if case["family"] == "B":
            assert name == fz.GENERIC
            continue
        falls = t["delay"][0] == "dense" or t["hilb"][0] in ("dense", "negzero")
        assert name == (fz.GENERIC if falls else fz.SPLIT16 if case["spec"]["arith"] == rc.ARITH_SPLIT16 else fz.FUSED), case
        by_variant[(t["delay"][0], t["hilb"][0])].add(name)
    assert {k[0] for k in by_variant} == {"designed", "impulse", "dense"} and {k[1] for k in by_variant} == {"designed", "odd", "dense", "negzero"}


def test_generator_covers_every_form():
    n = collections.Counter()
    for case in fz.cases():
        for _, r in fz.walk(case):
            k, fmt = r["kernel"], "q15" if r["q15"] else "f32"
            n[k, fmt] += 1
            n[k, "device" if r["device"] else "host"] += 1
            n["mode", r["mode"]] += 1
            if k in ("fused", "split16"):
                n[k, r["flavour"]] += 1
                if r["flavour"] == "perchan" and r["steps_same"]:
                    n[k, "perchan on a uniform-step instance"] += 1
                if r["moved"]:
                    n[k, "moved impulse"] += 1
            if k == "fm":
                n["fm", r["flavour"]] += 1
                n["fm", "tone on" if r["tone"] else "tone off"] += 1
                if r["tone"]:
                    n["fm", "tone " + r["tone"]] += 1
                if r["arith"] == rc.ARITH_SPLIT16:
                    n["fm", "split16 instance"] += 1
                if r["alc_set"]:
                    n["fm", "alc away from its defaults"] += 1
            if r["prev"] is not None and r["prev"] != k:
                n["from " + r["prev"], "to " + k] += 1
            for t in r["tags"]:
                n["first call", t] += 1
    need = [(k, f) for k in ("generic", "fused", "split16", "fm") for f in ("f32", "q15", "device", "host")]
    need += [("fused", f) for f in ("off", "table", "perchan")] + [("split16", f) for f in ("off", "periodic", "table", "perchan")]
    need += [(k, f) for k in ("fused", "split16") for f in ("perchan on a uniform-step instance", "moved impulse")]
    need += [("fm", f) for f in ("nco", "zero_if", "tone on", "tone off", "tone per", "tone all", "split16 instance", "alc away from its defaults")]
    need += [("mode", m) for m in fz.MODES + (fz.FM,)]
    need += [("from " + x, "to fm") for x in ("generic", "fused", "split16")] + [("from fm", "to " + x) for x in ("generic", "fused", "split16")]
    need += [("from fused", "to generic"), ("from generic", "to fused")]
    need += [("first call", t + "_behind_fm") for t in ("reset", "restore", "set_phase")]
    short = {k: n[k] for k in need if n[k] < NEED}
    print(sorted(n.items(), key=str))
    assert not short, "planned calls, at least %d each: %r" % (NEED, short)
