"""The route of a launch through the RX stages (csrc/rx_route.h: route) on a CPU: a stand-alone program (tests/route_cases.cpp, g++, no HIP)
prints the route for the full product of the facts of a launch; this module recomputes every field from the rules the dispatcher followed
before the route was one function -- written out here, not read from the code under test -- compares all rows, counts them against the
product, and asserts the invariants a wrong edit of the route would break (a stage skipped, an AGC applied twice, a wrong buffer)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL, PHASE1, PHASE2 = range(3)
NEITHER, SSB, CW = range(3)
FACTS = "phase src_q15 dst_q15 glob agc on_tones on_afilt on_nr on_meter on_gate force kernel cwbq words".split()
FIELDS = ("tones afilt nr meter gate mixed ssb_fused cw_fused fused unscaled convert_in audio_in_scratch fused_agc_off done_after_fused "
          "clear_words generic_front biquad env apply agc_generic").split()
COLS = FACTS + FIELDS


@pytest.fixture(scope="module")
def t(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("route") / "route_cases")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "route_cases.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    a = np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.int64)
    assert a.shape[1] == len(COLS)
    return {k: a[:, i] for i, k in enumerate(COLS)}


def _none(mask, t, what):
    bad = np.flatnonzero(mask)
    assert bad.size == 0, "%s: %d cases, first: %s" % (what, bad.size, {k: int(t[k][bad[0]]) for k in COLS})


def test_every_case_of_the_product_is_routed(t):
    # phases 1 and 2 only with a global gain; the gate only with the meter
    phase_global = 3 + 1
    slots, agc, stages_gate, force, kernel, cwbq, words = 3, 2, 8 + 8 * 2, 2, 3, 2, 2
    want = phase_global * slots * agc * stages_gate * force * kernel * cwbq * words
    assert len(t["phase"]) == want == 13824
    facts = np.stack([t[k] for k in FACTS], axis=1)
    assert len(np.unique(facts, axis=0)) == want, "a case printed twice"
    _none((t["phase"] != ALL) & (t["glob"] == 0), t, "a split call without a global gain")
    _none((t["on_gate"] == 1) & (t["on_meter"] == 0), t, "a gate without its meter")
    for k, n in (("phase", 3), ("glob", 2), ("agc", 2), ("force", 2), ("kernel", 3), ("cwbq", 2), ("words", 2), ("on_gate", 2)):
        assert set(t[k].tolist()) == set(range(n)), k
    assert {(int(s), int(d)) for s, d in zip(t["src_q15"], t["dst_q15"])} == {(0, 0), (1, 1), (0, 1)}
    assert len({tuple(r) for r in np.stack([t["on_tones"], t["on_afilt"], t["on_nr"], t["on_meter"]], axis=1).tolist()}) == 16


def test_every_field_is_what_the_dispatcher_computed(t):
    b = {k: v.astype(bool) for k, v in t.items()}
    phase, src_q15, dst_q15, glob, agc = t["phase"], b["src_q15"], b["dst_q15"], b["glob"], b["agc"]
    want = {}
    for s in ("tones", "afilt", "nr", "meter"):
        want[s] = b["on_" + s] & (phase != PHASE2)
    want["gate"] = b["on_meter"] & b["on_gate"] & (phase != PHASE1)
    want["mixed"] = ~src_q15 & dst_q15
    want["ssb_fused"] = (phase != PHASE2) & ~b["force"] & (t["kernel"] == SSB)
    want["cw_fused"] = (phase != PHASE2) & ~b["force"] & (t["kernel"] == CW)
    want["fused"] = want["ssb_fused"] | want["cw_fused"]
    want["unscaled"] = glob | want["nr"] | want["meter"] | want["afilt"] | want["tones"] | want["mixed"]
    want["convert_in"] = want["unscaled"] & src_q15 & want["fused"]
    want["audio_in_scratch"] = dst_q15 & (want["unscaled"] | ~want["fused"])
    want["fused_agc_off"] = want["fused"] & want["unscaled"]
    want["done_after_fused"] = want["fused"] & ~want["unscaled"]
    want["clear_words"] = (phase != PHASE2) & b["words"] & ~want["ssb_fused"]
    want["generic_front"] = (phase != PHASE2) & ~want["fused"]
    want["biquad"] = want["generic_front"] & b["cwbq"]
    want["env"] = glob & (phase != PHASE2)
    want["apply"] = glob & (phase != PHASE1)
    want["agc_generic"] = ~glob & (agc | dst_q15)
    assert sorted(want) == sorted(FIELDS)
    for k in FIELDS:
        _none(b[k] != want[k], t, k)


def test_the_invariants_of_a_route(t):
    b = {k: v.astype(bool) for k, v in t.items()}
    done, off, fused = b["done_after_fused"], b["fused_agc_off"], b["fused"]
    stage = b["tones"] | b["afilt"] | b["nr"] | b["meter"]
    _none(done & (stage | b["glob"] | b["mixed"]), t, "the fused kernel finishes a call that a stage, the global gain or the int16 store still works on")
    _none(done & b["on_meter"] & ~b["on_gate"] & (t["phase"] != PHASE2), t, "the fused kernel finishes a call whose meter has not read it")
    _none(done & b["gate"], t, "the fused kernel finishes a call whose gate is still to come")
    _none((done | off) != fused, t, "AGC off / done do not cover the fused launches")
    _none(done & off, t, "AGC off and done at once")
    _none(~fused & (done | off), t, "a fused kernel's flags without a fused kernel")
    _none(b["audio_in_scratch"] & ~b["dst_q15"], t, "f32 dst, audio in the scratch")
    _none(b["dst_q15"] & ~b["audio_in_scratch"] & ~done, t, "int16 dst holds the un-scaled f32 audio")
    p2 = t["phase"] == PHASE2
    _none(p2 & (stage | fused | b["generic_front"] | b["biquad"] | b["clear_words"] | b["convert_in"] | b["env"]), t, "phase 2 runs a stage or a front kernel")
    _none(p2 & ~b["apply"], t, "phase 2 without its gain pass")
    # exactly one thing applies the AGC / stores dst: the fused kernel itself, the global gain's pass, or k_agc_generic where there is an
    # AGC or an int16 store (phase 1 leaves un-scaled audio on purpose)
    _none(b["glob"] & b["agc_generic"], t, "both tails")
    _none(b["apply"] != (b["glob"] & (t["phase"] != PHASE1)), t, "the gain pass")
    _none(off & ~(b["glob"] | b["agc_generic"]) & (b["agc"] | b["dst_q15"]), t, "AGC off in the fused kernel and no tail that applies it")
    _none(b["convert_in"] & ~(b["src_q15"] & fused), t, "an up-front conversion nothing needs")
    _none(b["ssb_fused"] & b["cw_fused"], t, "two fused kernels")
    _none(b["biquad"] & ~b["generic_front"], t, "the generic biquad kernel behind a fused kernel")
    _none(b["clear_words"] & b["ssb_fused"], t, "the words cleared in front of the kernel that reads them")
