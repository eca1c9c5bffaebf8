"""The FSK decoder's flag in the route of a launch (csrc/rx_route.h: StagesOn::fskdec) on a CPU.  tests/route_fskdec_cases.cpp (g++, no HIP)
prints the route over the product of tests/route_cases.cpp twice, the flag off and on.  With the flag off every field is what the route was
before the flag existed: the rules are written out here, as tests/test_route.py does, not read from the code under test, and the rows are
also the rows tests/route_cases.cpp prints, line by line.  With the flag on, run.fskdec follows phase != phase 2 and counts in `unscaled`
like any other stage in front of the AGC; everything behind `unscaled` follows from it by the same rules."""
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
COLS = FACTS + FIELDS + ["on_fskdec", "fskdec"]


def _run(tmp, name):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    return np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.int64)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("route_fskdec")
    a, old = _run(tmp, "route_fskdec_cases"), _run(tmp, "route_cases")
    assert a.shape[1] == len(COLS)
    return {k: a[:, i] for i, k in enumerate(COLS)}, a, old


def _none(mask, t, what):
    bad = np.flatnonzero(mask)
    assert bad.size == 0, "%s: %d cases, first: %s" % (what, bad.size, {k: int(t[k][bad[0]]) for k in COLS})


def rules(t, fskdec):
    """every field of the route from the facts; `fskdec`: the flag, per row"""
    b = {k: v.astype(bool) for k, v in t.items()}
    phase, src_q15, dst_q15, glob, agc = t["phase"], b["src_q15"], b["dst_q15"], b["glob"], b["agc"]
    want = {}
    for s in ("tones", "afilt", "nr", "meter"):
        want[s] = b["on_" + s] & (phase != PHASE2)
    want["fskdec"] = fskdec & (phase != PHASE2)
    want["gate"] = b["on_meter"] & b["on_gate"] & (phase != PHASE1)
    want["mixed"] = ~src_q15 & dst_q15
    want["ssb_fused"] = (phase != PHASE2) & ~b["force"] & (t["kernel"] == SSB)
    want["cw_fused"] = (phase != PHASE2) & ~b["force"] & (t["kernel"] == CW)
    want["fused"] = want["ssb_fused"] | want["cw_fused"]
    want["unscaled"] = glob | want["nr"] | want["meter"] | want["afilt"] | want["tones"] | want["mixed"] | want["fskdec"]
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
    return want


def test_flag_off_is_the_route_as_it_was_field_by_field(rows):
    t, a, old = rows
    off = t["on_fskdec"] == 0
    assert off.sum() == 13824 == len(old) and (~off).sum() == 13824
    # line by line the rows of tests/route_cases.cpp, which never sets the flag ...
    assert np.array_equal(a[off][:, :len(FACTS) + len(FIELDS)], old)
    # ... and field by field the rules as they stood before the flag
    want = rules(t, np.zeros(len(off), bool))
    b = {k: v.astype(bool) for k, v in t.items()}
    for k in FIELDS + ["fskdec"]:
        _none(off & (b[k] != want[k]), t, k)
    _none(off & b["fskdec"], t, "the decoder runs with its flag off")


def test_flag_on_runs_in_front_and_wants_unscaled_audio(rows):
    t, a, _ = rows
    on = t["on_fskdec"] == 1
    b = {k: v.astype(bool) for k, v in t.items()}
    _none(on & (b["fskdec"] != (t["phase"] != PHASE2)), t, "run.fskdec does not follow phase != phase 2")
    want = rules(t, on)
    for k in FIELDS + ["fskdec"]:
        _none(on & (b[k] != want[k]), t, k)
    # the decoder alone: nothing else asks for un-scaled audio
    alone = on & ~(b["on_tones"] | b["on_afilt"] | b["on_nr"] | b["on_meter"] | b["glob"] | b["mixed"])
    assert alone.sum() > 0 and (t["phase"][alone] == ALL).all()              # (phases 1 and 2 exist only with a global gain)
    _none(alone & ~b["unscaled"], t, "fskdec alone does not make the launch un-scaled")
    _none(alone & b["fused"] & ~b["fused_agc_off"], t, "fskdec alone: a fused kernel keeps its own AGC")
    _none(alone & b["done_after_fused"], t, "fskdec alone: the fused kernel finishes the call")
    # the same facts without the flag: not un-scaled -- the flag is what made it so
    facts = len(FACTS) + len(FIELDS)
    i_uns = COLS.index("unscaled")
    twin = a[t["on_fskdec"] == 0]
    assert np.array_equal(twin[:, :len(FACTS)], a[on][:, :len(FACTS)]) and facts == 34
    alone_rows = alone[on]
    assert not twin[alone_rows, i_uns].any()
    # phase 2 runs none of it, and the flag changes nothing there
    p2 = t["phase"][on] == PHASE2
    assert p2.any() and np.array_equal(a[on][p2][:, :facts], twin[p2][:, :facts])
