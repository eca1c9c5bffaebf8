"""The decision function of the TX direction (csrc/tx_select.h: tx_select) on a CPU: a stand-alone program (tests/tx_select_cases.cpp, g++, no
HIP) prints the decision for the full product of geometries, tap classes, arithmetics, modes, LO situations, plan options, call lengths,
key calls and LDS byte counts; this module checks every line against what the kernels and their launchers admit, and then holds the rule
against the one restatement of it that is kept on purpose (tests/tx_fuzz_cases.py: expected_kernel, walk) on every planned call of the
committed fuzz cases.

"phase_uniform holds" is read as the instance keeps it: selenite_tx_reset and selenite_tx_set_state never set it unless every channel has
the same step, so the product's (phase_uniform, not steps_same) corner is a state no instance reaches; the rule shares no LO there either.
Arithmetic 3 (AUTO) is an RX mode that selenite_tx_init refuses; the rule runs it as FMA, which the product records.  fm_set is not an
input of the rule (selenite_tx_set_mode guards the way into FM): the two FM entries of the mode list must decide alike."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rxcommon as rc
import tx_entry_fuzz_cases as ez
import tx_fuzz_cases as fz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, FUSED, SPLIT16, KFM, KCW = range(5)
NAMES = {GENERIC: "k_tx_generic", FUSED: "k_tx_fused<4,256,63>", SPLIT16: "k_tx_split16<4,256,63>", KFM: "k_tx_fm", KCW: "k_tx_cw"}
GEOS = ((64, 4, 256, 63), (65, 4, 256, 63), (64, 2, 256, 63), (64, 4, 252, 63), (64, 4, 256, 65))      # (block, interp, ni_taps, nh_taps)
MODES = (rc.MODE_LSB, rc.MODE_USB, rc.MODE_CW, rc.MODE_CWR, rc.MODE_AM, rc.MODE_DIG, rc.MODE_PKT, rc.MODE_FM, rc.MODE_FM)
COLS = "geo imp odd arith mode fg table nco same uni grid npl blocks key lds kernel flavour".split()      # one character each, then
TAIL = "clears refused".split()                                                                          # lo_n (five digits) and these


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("tx_select") / "tx_select_cases")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "tx_select_cases.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def t(prog):
    out = subprocess.run([prog], check=True, stdout=subprocess.PIPE).stdout
    width = len(COLS) + 5 + len(TAIL) + 1
    a = np.frombuffer(out, np.uint8).reshape(-1, width)
    assert (a[:, -1] == ord("\n")).all()
    d = a[:, :-1] - ord("0")
    assert (d <= 9).all()
    t = {k: d[:, i] for i, k in enumerate(COLS)}
    t["lo_n"] = d[:, len(COLS):len(COLS) + 5].astype(np.int32) @ np.array([10000, 1000, 100, 10, 1], np.int32)
    t.update({k: d[:, len(COLS) + 5 + i] for i, k in enumerate(TAIL)})
    t["bs"] = t["blocks"] * np.array([g[0] for g in GEOS], np.int32)[t["geo"]]
    t["interp"] = np.array([g[1] for g in GEOS], np.int32)[t["geo"]]
    t["fm"] = t["mode"] >= 7
    t["matrix"] = (t["kernel"] == FUSED) | (t["kernel"] == SPLIT16)
    t["shared"] = (t["nco"] == 1) & (t["same"] == 1) & (t["uni"] == 1)
    return t


def _none(mask, t, what):
    bad = np.flatnonzero(mask)
    assert bad.size == 0, "%s: %d cases, first: %s" % (what, bad.size, {k: int(t[k][bad[0]]) for k in COLS + ["lo_n"] + TAIL})


def test_every_case_of_the_product_is_decided(t):
    n = len(GEOS) * 2 * 2 * 4 * len(MODES) * 2 * 2 * 2 * 2 * 2 * 2 * 2 * 4 * 2 * 8
    assert len(t["geo"]) == n
    for k, vals in dict(geo=range(5), imp=(0, 1), odd=(0, 1), arith=range(4), mode=range(9), fg=(0, 1), table=(0, 1), nco=(0, 1), same=(0, 1),
                        uni=(0, 1), grid=(0, 1), npl=(0, 1), blocks=(1, 3, 4, 8), key=(0, 1), lds=range(8)).items():
        assert sorted(set(t[k].tolist())) == list(vals), k
        assert all((t[k] == v).sum() * len(vals) == n for v in vals), k
    _none(t["kernel"] > KCW, t, "no kernel named")
    _none(t["flavour"] > 3, t, "no flavour the templates number")
    _none((t["key"] == 1) != (t["kernel"] == KCW), t, "k_tx_cw serves the key calls and nothing else")
    _none((t["key"] == 0) & (t["fm"] != (t["kernel"] == KFM)), t, "k_tx_fm serves the audio calls of FM and nothing else")
    for k in ("kernel", "flavour", "lo_n", "clears", "refused"):      # fm_set is no input of the rule
        assert (t[k][t["mode"] == 7] == t[k][t["mode"] == 8]).all(), k


def test_matrix_kernels_only_where_they_are_written_for(t):
    ok = (t["geo"] == 0) & (t["imp"] == 1) & (t["odd"] == 1) & (t["bs"] % 256 == 0) & ~t["fm"] & (t["fg"] == 0) & (t["key"] == 0)
    _none(t["matrix"] != ok, t, "k_tx_fused / k_tx_split16: the fused geometry with both tap classes, whole passes, outside FM, without force_generic")
    _none(t["matrix"] & ((t["kernel"] == SPLIT16) != ((t["arith"] == rc.ARITH_SPLIT16) & (t["table"] == 1))), t, "k_tx_split16: SPLIT16 with a table")
    assert (t["kernel"] == SPLIT16).any() and (t["kernel"] == FUSED).any() and (t["kernel"] == GENERIC).any()


def test_the_nco_flavour(t):
    f = t["flavour"]
    three = t["shared"] & (t["kernel"] == SPLIT16) & (t["grid"] == 1) & (t["npl"] == 0)
    _none((f == 3) != three, t, "flavour 3: k_tx_split16, a shared LO on the fs / 256 grid, periodic LO not switched off")
    _none((f == 2) != (t["matrix"] & t["shared"] & ~three), t, "flavour 2: NCO on, phase_uniform, a matrix kernel")
    _none((f >= 2) & ~t["matrix"], t, "a shared table on k_tx_generic, k_tx_fm or k_tx_cw")
    _none((f == 0) != (t["nco"] == 0), t, "flavour 0 is NCO off")
    _none(t["lo_n"] != np.where(f >= 2, t["bs"] * t["interp"], 0), t, "the table's length: block_size * interp, or none")
    assert (f == 3).any() and (f == 2).any() and ((f == 1) & t["matrix"]).any()


def test_phase_uniform_is_lost_behind_fm_and_key_calls_only(t):
    _none((t["clears"] == 1) != (t["fm"] | (t["key"] == 1)), t, "clears phase_uniform")


def test_refusals_are_the_serving_kernels_lds(t):
    above = np.select([t["kernel"] == GENERIC, t["kernel"] == KFM, t["kernel"] == KCW], [t["lds"] & 1, (t["lds"] >> 1) & 1, (t["lds"] >> 2) & 1], 0)
    _none(t["refused"] != above, t, "refused exactly when the serving any-shape kernel's layout exceeds 64 KiB; never on the matrix kernels")
    assert (t["refused"] == 1).any() and (t["matrix"] & (t["lds"] == 7)).any()


def test_the_name_is_the_whole_pass_decision(prog):
    lines = subprocess.run([prog, "names"], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    assert len(lines) == len(GEOS) * 2 * 2 * 4 * len(MODES) * 2 * 2
    for line in lines:
        geo, imp, odd, arith, mode, fg, table, kernel, name = line.split(" ", 8)
        want = KFM if int(mode) >= 7 else GENERIC
        if want == GENERIC and (geo, imp, odd, fg) == ("0", "1", "1", "0"):
            want = SPLIT16 if (int(arith), table) == (rc.ARITH_SPLIT16, "1") else FUSED
        assert (int(kernel), name) == (want, NAMES[want]), line


def _lds(s):
    shape = (s["block"], s["interp"], s["ni_taps"], s["nh_taps"])
    return fz.tx_lds_bytes(*shape), fz.fm_lds_bytes(*shape)


def test_the_rule_agrees_with_the_fuzz_generators_restatement(prog):
    """every planned call of the committed cases, through `eval`: kernel family and flavour as walk() expects them, the instance's name as
    expected_kernel() does; the inputs are the case's own (taps classified by matrix_shape as selenite_tx_init does, the table where
    selenite_tx_init builds it) and walk's phase_uniform in front of the call.  The cases of the entry fuzz (tests/tx_entry_fuzz_cases.py)
    go the same way: a key call with key = 1 and k_tx_cw's LDS as cw_lds_bytes restates it, a frame call as the audio call it ends in;
    phase_uniform behind a key call is walk's, which a key call clears as an FM call does."""
    flavours = {"off": 0, "perchan": 1, "table": 2, "periodic": 3, "zero_if": 0, "nco": 1}
    families = {"generic": GENERIC, "fused": FUSED, "split16": SPLIT16, "fm": KFM, "cw": KCW}
    asked, want = [], []
    for gen, kinds in ((fz, fz.KINDS), (ez, ez.KINDS)):
        for kind in kinds:
            for case in gen.cases(gen.SEED, gen.COUNTS[kind], kind):
                s = case["spec"]
                classed = int(fz.matrix_shape(case))            # both tap classes or neither: what matrix_shape tells apart
                steps = s["nco_steps"] if s["nco_steps"] is not None else [s["nco_step_all"]] * s["channels"]
                table = int(classed and s["arith"] == rc.ARITH_SPLIT16)
                lg, lf = _lds(s)
                cw = case.get("cw")
                for i, r in gen.walk(case):
                    key = int(r.get("entry") == "key")
                    if key:                                      # (the setting of the call: a retune in front of it counts)
                        ns = [ev["cw"] for ev in case["events"][:i] if ev["op"] == "set_cw"][-1:] or [cw]
                        assert ns[0]["ns_taps"] == r["ns"]
                    lc = ez.cw_lds_bytes(s["block"], s["interp"], s["ni_taps"], r["ns"]) if key else 0
                    asked.append("%d %d %d %d %d %d %d %d %d %d %d %d 0 0 %d %d %d %d %d %d" % (
                        s["block"], s["interp"], s["ni_taps"], s["nh_taps"], classed, classed, s["arith"], r["mode"], int(bool(s["nco"])),
                        int(len(set(steps)) == 1), int(bool(r["uniform"])), steps[0], table, r["bs"], key, lg, lf, lc))
                    name = fz.expected_kernel(case, r["mode"])      # (the instance's name: a key call does not change it)
                    want.append((families[r["kernel"]], flavours[r["flavour"]], name, int(key or r["mode"] == fz.FM), case["kind"], case["idx"]))
    out = subprocess.run([prog, "eval"], input="\n".join(asked) + "\n", check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    assert len(out) == len(want) > 800
    seen = set()
    for line, (kernel, flavour, name, clears, kind, idx) in zip(out, want):
        k, f, _, got_clears, refused, got_name = line.split(" ", 5)
        assert (int(k), int(f), int(got_clears), int(refused), got_name) == (kernel, flavour, clears, 0, name), (kind, idx, line)
        seen.add((kernel, flavour))
    assert {(SPLIT16, 3), (SPLIT16, 2), (FUSED, 2), (FUSED, 1), (GENERIC, 1), (GENERIC, 0), (KFM, 1), (KFM, 0), (KCW, 1), (KCW, 0)} <= seen
