"""GPU: random configurations and call sequences of the TX chain (csrc/tx_api.hip: run(), as csrc/tx_select.h decides -- k_tx_generic, k_tx_fused, k_tx_split16, k_tx_fm)
against the oracle (tests/txfm_oracle.py: TxFmOracle over oracle/tx_oracle.c), the counterpart of tests/test_gpu_fuzz.py for the RX side.

tests/tx_fuzz_cases.py draws the cases: shapes (the fused geometry with designed, moved-impulse, odd-distance, dense and -0.0f taps; generic
shapes with odd blocks, L 1 ... 8, 0 ... 129 Hilbert taps), the three arithmetics, channel counts, NCO flavours, ALC off / default / away
from its defaults, both q15 roundings, an FM setting, and 2 ... 6 events: calls of 1 ... 8 ALC blocks in f32 or int16 slots through the host or
the device entry at levels from 1e-6 to 10, set_mode, an FM retune, reset, checkpoint / restore, set_state with one phase for all channels.
tests/test_tx_fuzz_cases.py asserts on the CPU that the committed seed and counts reach every kernel form and hand-over.
tests/tx_fuzz_runner.py holds what is asserted on every event: kernel_name() behind every set_mode, the output and every state array on
bits (k_tx_split16's output: the 1e-5 bar of tests/test_gpu_tx.py per 256 complex outputs, 1 LSB in int16), sync() == 0, no sticky status.

Three tests, a slice of the cases each (tx_fuzz_cases.COUNTS; SELENITE_FUZZ_CASES=<n> scales them, 160 in all by default;
SELENITE_FUZZ_ONLY=<index> runs one case of a slice).  A failure prints the whole case and the event index.

Two more tests, a slice each, for the instances on which a call can come in through three kinds of entry (tests/tx_entry_fuzz_cases.py):
KEY with a keyed CW path (k_tx_cw: key calls in f32 and int16 through the host and the device entry, the sidetone stored or mixed, audio
calls between them, retunes, checkpoints over a key call, a refused key call) and IN with an audio input stage (k_tx_in: frame calls
through all five entries into k_tx_fused, k_tx_split16, k_tx_generic and k_tx_fm, with key and audio calls between them, VOX, retunes,
checkpoints over a frame call, clear_in and a refused frame call).  tests/test_tx_entry_fuzz_cases.py asserts their coverage on the CPU;
tx_fuzz_runner.EntryPair holds what is asserted: on top of the above, the stage's audio, the sidetone buffer, cw_state, in_state and
fm_state on bits against tests/txin_oracle.py's TxInOracle.  The two environment variables work on them as on the three."""
import os

import pytest

import tx_entry_fuzz_cases as ez
import tx_fuzz_cases as fz
import tx_fuzz_runner as fr

pytestmark = pytest.mark.gpu


def run_slice(kind):
    n = fz.scale_count(kind, os.environ.get("SELENITE_FUZZ_CASES"))
    only = os.environ.get("SELENITE_FUZZ_ONLY")
    for case in fz.cases(fz.SEED, n, kind):
        if only is None or case["idx"] == int(only):
            fr.run_case(case)
    print("tx fuzz %s: %d cases; worst k_tx_split16 per-block error so far %.3g of the block maximum (bar %g)" % (kind, n, fr.WORST[0], fr.TOL))


def test_fused_geometry_without_fm():
    run_slice("A")


def test_generic_shapes_without_fm():
    run_slice("B")


def test_both_families_through_fm():
    run_slice("FM")


def run_entry_slice(kind):
    n = ez.scale_count(kind, os.environ.get("SELENITE_FUZZ_CASES"))
    only = os.environ.get("SELENITE_FUZZ_ONLY")
    for case in ez.cases(ez.SEED, n, kind):
        if only is None or case["idx"] == int(only):
            fr.run_entry_case(case)
    print("tx entry fuzz %s: %d cases; worst k_tx_split16 per-block error so far %.3g of the block maximum (bar %g)" % (kind, n, fr.WORST[0], fr.TOL))


def test_key_calls_between_audio_calls():
    run_entry_slice("KEY")


def test_frame_calls_between_key_and_audio_calls():
    run_entry_slice("IN")
