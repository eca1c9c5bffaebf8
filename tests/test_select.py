"""The decision function of the SSB fused path (csrc/rx_select.h: select) on a CPU: a stand-alone program (tests/select_cases.cpp, g++, no HIP)
prints the decision for the full product of shapes, arithmetics, modes, slot formats, DSP blocks, call lengths, LO situations and call facts;
this module checks every line against what the kernels' instantiation lists and launchers admit -- several of these conditions are otherwise
enforced only by a hipErrorNotSupported at run time on a GPU.  The lists are read from the header's text, the arithmetic over them is redone here.

One condition differs from the issue that asked for this test: it wanted NCO flavour 3 never on k_ssb_mfma, but rx_fused.hip instantiates
k_ssb_mfma<3, ...> (the shared periodic LO in registers) and launches it, so flavour 3 is admitted there on whole 256-output passes; 4 never."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "selenite-lite_amd", "csrc", "rx_select.h")
SPLIT16, HILB16, MFMA, FUSED_FMA, FUSED_EXACT, DENSE_FMA, DENSE_EXACT = range(1, 8)
USB, AM, FM = 0x01, 0x04, 0x08
CMSIS, FMA, SPLIT, AUTO = range(4)
COLS = ("nd m nh plain arith mode block bs q15 lo unscaled rows launches tnd nds btab16 mfma ext_len family dq15 pass_out dec2 nco_rx lo_period nco "
        "nco_rerun lo_n env_part auto_form repair_all first family1 first1").split()


def _list(name):
    text = open(HEADER).read()
    body = re.search(r"#define %s\(X\)((?:.*\\\n)*.*)\n" % name, text).group(1)
    return [tuple(int(v) for v in m.split(",")) for m in re.findall(r"X\(([^)]*)\)", body)]


SHAPES = [s[:3] for s in _list("SRX_SHAPES")]
DENSE = [s[:3] for s in _list("SRX_DENSE_SHAPES")]
S16 = _list("SRX_SPLIT16_SHAPES")
H16 = [s[0] for s in _list("SRX_HILB16_SHAPES")]


def _shortest(shapes, nd, m, nh):
    fit = [s[0] for s in shapes if s[1] == m and (nh is None or s[2] == nh) and (s[0] == 0 if nd == 0 else (s[0] >= nd >= 2))]
    return min(fit) if fit else -1


def _nds(nd, m, nh):
    return -1 if nd < 2 or nd % 2 else _shortest(S16, nd, 4 if m == 8 else m, nh)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("select") / "select_cases")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "select_cases.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def t(prog):
    out = subprocess.run([prog], check=True, stdout=subprocess.PIPE).stdout
    a = np.fromstring(out, dtype=np.int64, sep=" ").reshape(-1, len(COLS))
    t = {k: a[:, i] for i, k in enumerate(COLS)}
    # per-row arithmetic over the lists, redone here
    packed, inv = np.unique(((a[:, 0] * 16 + a[:, 1]) * 256 + a[:, 2]) * 2 + a[:, 3], return_inverse=True)
    key = np.stack([packed // 8192, packed // 512 % 16, packed // 2 % 256, packed % 2], axis=1)
    t["shapes"] = key
    per = []
    for k in key.tolist():
        tnd = _shortest(SHAPES, k[0], k[1], k[2]) if k[3] else -1      # a shape of its own; else the dense flavour, any pair of up to 127 taps
        per.append((_nds(*k[:3]), tnd, 0) if tnd >= 0 else (-1, _shortest(DENSE, k[0], k[1], None), 1))
    per = np.array(per)[inv]
    t["py_nds"] = per[:, 0]
    t["py_tnd"] = per[:, 1]
    t["py_dense"] = per[:, 2]
    mk = np.where(t["m"] == 8, 4, t["m"])
    t["py_hs"] = np.where(t["py_nds"] > 0, (-(-(t["py_nds"] - 1) // mk) + 3) // 4 * 4 * mk, 0)      # whole groups of four phase-samples
    t["na"] = t["block"] // t["m"]
    t["py_p16"] = np.where(t["m"] == 8, 128, 256) // t["na"] * t["na"]
    t["bs_eff"] = np.where(t["first"] > 0, t["first"], t["bs"])        # what the first (or only) launch takes
    t["py_ext"] = np.where((t["arith"] == AUTO) & (t["py_nds"] > 0), t["m"] * ((t["nh"] - 1 + 3) // 4 * 4), 0)
    return t


def _none(mask, t, what):
    bad = np.flatnonzero(mask)
    assert bad.size == 0, "%s: %d cases, first: %s" % (what, bad.size, {k: int(t[k][bad[0]]) for k in COLS})


def test_every_case_of_the_product_is_decided(t):
    shapes = set(map(tuple, t["shapes"].tolist()))
    want = {s + (1,) for s in SHAPES} | {s + (0,) for s in DENSE} | {s + (1,) for s in S16} | {(0, 1, nh, 1) for nh in H16} | {(100, 4, 63, 1), (256, 4, 65, 1)}
    assert shapes == want
    admitted = sum(1 for s in want for b in (64, 96, 128, 192, 256) if 4 <= b // s[1] <= 256 and b // s[1] % 4 == 0)
    assert len(t["nd"]) == admitted * 4 * 3 * 8 * 2 * 5 * 2 * 2 * 2
    _none((t["family"] < SPLIT16) | (t["family"] > DENSE_EXACT), t, "no kernel family named")
    _none(t["dq15"] != (t["q15"] & (1 - t["unscaled"])), t, "slot format of the launch")


def test_every_decision_names_an_instantiation_that_exists(t):
    f, mk = t["family"], np.where(t["m"] == 8, 4, t["m"])
    in_s16 = np.zeros(len(f), bool)
    for n, m, h in S16:
        in_s16 |= (t["py_nds"] == n) & (mk == m) & (t["nh"] == h)
    _none((f == SPLIT16) & ~(in_s16 & (t["nds"] == t["py_nds"]) & (t["py_dense"] == 0)), t, "k_ssb_split16 without a shape of SRX_SPLIT16_SHAPES")
    _none((f == SPLIT16) & ((t["dec2"] == 1) != (t["m"] == 8)), t, "by 8: the by-4 entry with dec2, and only by 8")
    _none((f != SPLIT16) & (t["dec2"] == 1), t, "dec2 off k_ssb_split16")
    _none((f == SPLIT16) & ((t["pass_out"] != t["py_p16"]) | (t["pass_out"] % 16 != 0) | (t["pass_out"] == 0)), t, "k_ssb_split16: passes of whole 16-output tiles")
    _none((f == HILB16) & ~((t["nd"] == 0) & (t["m"] == 1) & np.isin(t["nh"], H16) & (t["py_dense"] == 0)), t, "k_hilb_split16 without a shape of SRX_HILB16_SHAPES")
    _none((f == MFMA) & ~((t["m"] == 4) & (t["nd"] > 0) & (t["pass_out"] == 256) & (t["bs_eff"] // 4 % 256 == 0) & (t["py_dense"] == 0)), t, "k_ssb_mfma: by 4, whole 256-output passes")
    plain = (f == FUSED_FMA) | (f == FUSED_EXACT) | (f <= MFMA)
    _none(plain & ~((t["py_dense"] == 0) & (t["tnd"] == t["py_tnd"]) & (t["py_tnd"] >= 0)), t, "a shape of SRX_SHAPES")
    _none((f >= DENSE_FMA) & ~((t["py_dense"] == 1) & (t["tnd"] == t["py_tnd"]) & (t["py_tnd"] >= 0)), t, "a shape of SRX_DENSE_SHAPES")
    _none((f != SPLIT16) & (f != HILB16) & (f != MFMA) & (t["pass_out"] != 256 // t["na"] * t["na"]), t, "k_ssb_fused: passes of the largest whole number of DSP blocks in 256")
    # block maxima: only the by-4, 16-lane-block, f32, NCO-on, neither AM nor FM, whole-pass launch of k_ssb_split16
    _none((t["env_part"] == 1) & ~((f == SPLIT16) & (t["m"] == 4) & (t["na"] == 64) & (t["dq15"] == 0) & (t["nco"] != 0) & (t["mode"] == USB)
                                   & (t["bs_eff"] // 4 % 256 == 0) & (t["dec2"] == 0)), t, "block maxima from a launch that has none")
    # the NCO flavour the kernel template understands
    lo_rx = np.array([0, 2, 2, 1, 1])[t["lo"]]
    _none(t["nco_rx"] != lo_rx, t, "RxParams::nco against the LO situation")
    _none(np.array([0, 1, 2, 2, 1])[t["nco"]] != t["nco_rx"], t, "flavour against RxParams::nco")
    _none(np.array([0, 1, 2, 2, 1])[t["nco_rerun"]] != t["nco_rx"], t, "the rerun pass's flavour against RxParams::nco")
    _none((t["nco"] >= 3) & ~np.isin(t["lo"], (2, 3)), t, "a register-held LO off the fs / 256 grid")
    _none((t["nco"] >= 3) & (f == SPLIT16) & (t["pass_out"] != np.where(t["m"] == 8, 128, 256)), t, "flavour 3 / 4 on k_ssb_split16 whose pass is no whole number of periods")
    fused = f >= FUSED_FMA
    _none(fused & ((t["nco"] == 3) | ((t["nco"] == 4) & (t["pass_out"] != 256))), t, "k_ssb_fused: flavour 4 only with 256-output passes, never 3")
    _none((t["nco_rerun"] == 3) | ((t["nco_rerun"] == 4) & (256 % t["na"] != 0)), t, "the rerun pass: k_ssb_fused's flavours")
    _none((f == MFMA) & (t["nco"] == 4), t, "flavour 4 on k_ssb_mfma")
    _none((f == HILB16) & (t["nco"] >= 3), t, "flavour 3 / 4 on k_hilb_split16")
    _none(t["lo_n"] != np.where(t["nco_rx"] == 2, np.maximum(t["bs_eff"], 256), 0), t, "the shared table's length")


def test_the_cut(t):
    cut, tail = t["first"] > 0, t["bs"] - t["first"]
    unit = t["py_p16"] * t["m"]
    _none(cut & ~((t["first"] < t["bs"]) & (t["first"] % np.maximum(unit, 1) == 0) & (unit > 0)), t, "first part: a positive whole number of passes, tail left")
    _none(cut & ~(tail < t["py_hs"]), t, "tail not shorter than HS")
    _none(cut & ~(np.isin(t["arith"], (SPLIT, AUTO)) & (t["btab16"] == 1) & (t["nd"] > 0) & (t["unscaled"] == 0)), t, "a cut without split tables, a decimator, or with a global gain")
    _none(cut & ~((t["family1"] == t["family"]) & (t["first1"] == 0)), t, "the first part decided as a call of its own")
    could = np.isin(t["arith"], (SPLIT, AUTO)) & (t["btab16"] == 1) & (t["nd"] > 0) & (t["unscaled"] == 0) & (t["py_p16"] % 16 == 0) & (t["py_p16"] > 0)
    short = could & (t["bs"] > unit) & (t["bs"] % np.maximum(unit, 1) != 0) & (t["bs"] % np.maximum(unit, 1) < t["py_hs"])
    _none(short & ~cut, t, "a partial last pass shorter than HS left on the call")
    assert cut.any() and (short & (t["arith"] == AUTO)).any()


def test_auto(t):
    f, auto = t["family"], t["arith"] == AUTO
    matrix = (f == SPLIT16) | (f == HILB16) | (f == MFMA)
    need = np.where(t["nd"] > 0, t["nd"] - 1, 0) + t["py_ext"]
    _none(auto & (t["rows"] == 1) & matrix & ~(t["bs_eff"] + 1 >= need), t, "a matrix kernel on a call too short to leave the repair rows")
    _none(auto & ((f == MFMA) | (f == FUSED_FMA) | (f == DENSE_FMA)), t, "AUTO in fma arithmetic")
    _none((t["auto_form"] != 0) != (auto & matrix), t, "the rerun (inline or as a pass) follows exactly the matrix kernels of AUTO")
    _none(~np.isin(t["auto_form"], (0, 1, 3)), t, "form")
    _none((t["auto_form"] == 1) & ~((f == HILB16) & (t["mode"] != AM) & (t["launches"] == 1)), t, "inline off k_hilb_split16, in AM, or with three launches asked")
    _none((t["repair_all"] == 1) & ~auto, t, "a history repair outside AUTO")
    assert (t["auto_form"] == 1).any() and (t["auto_form"] == 3).any() and (auto & (f == FUSED_EXACT) & (t["repair_all"] == 1)).any()


def test_the_name_is_the_whole_pass_decision(prog):
    heads = {SPLIT16: "k_ssb_split16<", HILB16: "k_hilb_split16<", MFMA: "k_ssb_mfma<", FUSED_FMA: "k_ssb_fused<", FUSED_EXACT: "k_ssb_fused<",
             DENSE_FMA: "k_ssb_fused<", DENSE_EXACT: "k_ssb_fused<"}
    lines = subprocess.run([prog, "names"], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    assert len(lines) > 500
    for line in lines:
        nd, m, nh, plain, arith, mode, block, fam, name = line.split(" ", 8)
        fam = int(fam)
        assert name.startswith(heads[fam]), line
        assert [h for h in set(heads.values()) if name.startswith(h)] == [heads[fam]], line
        assert name.endswith("(dense FIR pair)") == (fam >= DENSE_FMA), line
        assert ("+exact rerun" in name) == (int(arith) == AUTO and fam in (SPLIT16, HILB16)), line
        shape = "<%s>" % nh if fam == HILB16 else "<%s,%s,%s>" % (nd, m, nh)
        assert name[len(heads[fam]) - 1:].startswith(shape), line
